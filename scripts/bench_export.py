#!/usr/bin/env python
"""Time the gaze-map export: extract_map.py's avg_pool on the host against rgp_mapexport.

Workload: 1024 softmax maps of 49 x 49 fp32 (9.8 MB) -> 7 x 7 float64, bilinear: the maps of about ten LSMDC clips.

  host    the reference's loop per map -- bytescale (tests/export_ref.py, numpy), Image.fromarray(u).resize((7, 7),
          Image.BILINEAR), the division by the sum -- wall clock on this box's CPU; where Pillow does not import the
          resample is the numpy oracle's and `host.resample` says so
  device  the C call with the maps already on the device (events around the one launch; pooled alone, and all three
          outputs), and the whole Python call on a device tensor (wall clock: table lookup, allocation of the output,
          launch, status read)

Times are medians over --repeats timed runs after --warmup untimed ones.  Bytes moved = maps read once + outputs written
once; the floor is that over the 6.29 TB/s a float4 copy reaches on this chip -- a launch this small is nowhere near
it, the figure says how far.  `equal_to_host` compares every output of all maps with the host's, float64 through its
bits.  Writes one JSON document (--out) and prints it.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

HBM_COPY = 6.29e12
MAP_HW, OUT_HW, FILTER = (49, 49), (7, 7), 'bilinear'


def host_avg_pool(maps, ref, Image):
    """extract_map.py:35-41 with the oracle's bytescale; -> (pooled, resized bytes, bytes)."""
    pooled = np.zeros((len(maps),) + OUT_HW, np.float64)
    small = np.zeros((len(maps),) + OUT_HW, np.uint8)
    u8 = np.zeros(maps.shape, np.uint8)
    for i in range(len(maps)):
        u8[i] = ref.bytescale(maps[i])
        if Image is not None:
            small[i] = np.asarray(Image.fromarray(u8[i]).resize((OUT_HW[1], OUT_HW[0]), Image.BILINEAR))
        else:
            small[i] = ref.imresize(u8[i:i + 1], OUT_HW, FILTER)[0]
        p = small[i].astype(np.float64)
        with np.errstate(invalid='ignore', divide='ignore'):
            pooled[i] = p / p.sum()
    return pooled, small, u8


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--maps', type=int, default=1024)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--out', default=os.path.join('profiles', 'export_bench.json'))
    a = ap.parse_args()

    import torch
    import export_ref as ref
    from recurrent_gaze_prediction_amd import _lib
    from recurrent_gaze_prediction_amd import frames as fr
    from recurrent_gaze_prediction_amd.models import extract_map as em
    if not torch.cuda.is_available():
        raise SystemExit('bench_export.py needs a GPU: timings taken elsewhere say nothing about it')
    try:
        from PIL import Image
    except ImportError:
        Image = None
    dev = torch.device('cuda:0')
    lib = _lib.load()

    N, (H, W), (oh, ow) = a.maps, MAP_HW, OUT_HW
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    d_maps = torch.softmax(torch.randn((N, H * W), device=dev, generator=gen), dim=1).reshape(N, H, W).contiguous()
    kh, bh, ksh = fr._device_tables(dev, W, ow, FILTER)
    kv, bv, ksv = fr._device_tables(dev, H, oh, FILTER)
    pooled = torch.empty((N, oh, ow), dtype=torch.float64, device=dev)
    small = torch.empty((N, oh, ow), dtype=torch.uint8, device=dev)
    u8 = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    ws = torch.empty(max(int(lib.rgp_mapexport_workspace_bytes()), 64), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    result = {'maps': N, 'map_hw': list(MAP_HW), 'out_hw': list(OUT_HW), 'filter': FILTER, 'ksize_h': ksh, 'ksize_v': ksv,
              'warmup': a.warmup, 'repeats': a.repeats, 'device_name': torch.cuda.get_device_name(0), 'threads': torch.get_num_threads(),
              'hbm_copy_bytes_per_s': HBM_COPY}

    def run(all_three):
        args = _lib.MapExportArgs(maps=d_maps.data_ptr(), n=N, h=H, w=W, out_h=oh, out_w=ow, kh=kh.data_ptr(), bh=bh.data_ptr(),
                                  ksize_h=ksh, kv=kv.data_ptr(), bv=bv.data_ptr(), ksize_v=ksv, pooled=pooled.data_ptr(),
                                  pooled_u8=small.data_ptr() if all_three else None, bytes=u8.data_ptr() if all_three else None,
                                  workspace=ws.data_ptr(), workspace_bytes=ws.numel())
        _lib.check(lib.rgp_mapexport(ctypes.byref(args), stream))

    def timed(all_three):
        moved = N * H * W * 4 + N * oh * ow * 8 + (N * oh * ow + N * H * W if all_three else 0)
        times = []
        for i in range(a.warmup + a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(all_three)
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                times.append(e0.elapsed_time(e1))
        _lib.check(lib.rgp_mapexport_status(ws.data_ptr(), None, stream))
        ms = float(np.median(times))
        return {'ms_median': ms, 'ms_min': float(np.min(times)), 'ms_max': float(np.max(times)), 'bytes_moved': moved,
                'floor_ms': moved / HBM_COPY * 1e3, 'fraction_of_floor': moved / HBM_COPY * 1e3 / ms, 'us_per_map': ms * 1e3 / N}

    result['device'] = timed(False)
    result['device_all_three_outputs'] = timed(True)          # last: the three tensors now hold this launch's outputs

    h_maps = d_maps.cpu().numpy()
    host_avg_pool(h_maps[:8], ref, Image)
    t0 = time.perf_counter()
    h_pooled, h_small, h_u8 = host_avg_pool(h_maps, ref, Image)
    host_ms = (time.perf_counter() - t0) * 1e3
    result['host'] = {'maps': N, 'ms': host_ms, 'us_per_map': host_ms * 1e3 / N, 'resample': 'Pillow' if Image is not None else 'numpy oracle'}
    result['equal_to_host'] = {'maps_compared': N, 'pooled': ref.same_float64(pooled.cpu().numpy(), h_pooled),
                               'pooled_u8': bool(np.array_equal(small.cpu().numpy(), h_small)),
                               'bytes': bool(np.array_equal(u8.cpu().numpy(), h_u8)),
                               'nan_maps': int(np.isnan(h_pooled).any(axis=(1, 2)).sum())}
    result['speedup_host_over_device_launch'] = host_ms / result['device']['ms_median']

    walls = []
    for i in range(a.warmup + a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = em.avg_pool(d_maps)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
        del out
    result['device']['python_call_ms_median'] = float(np.median(walls[a.warmup:]))
    result['speedup_host_over_device_python_call'] = host_ms / result['device']['python_call_ms_median']
    # the path predict_long_clip(pool_to_7x7=True) takes today: every 49 x 49 map to the host, then the block mean
    walls = []
    for i in range(a.warmup + a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = d_maps.cpu().numpy().reshape(N, 7, 7, 7, 7).mean(axis=(2, 4))
        walls.append((time.perf_counter() - t0) * 1e3)
        del out
    result['block_mean_on_the_host_after_copy_ms_median'] = float(np.median(walls[a.warmup:]))

    text = json.dumps(result, indent=1, sort_keys=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fp:
        fp.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
