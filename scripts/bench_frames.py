#!/usr/bin/env python
"""Time the loader's frame images: Pillow's Image.resize(..., LANCZOS) per frame on the host against rgp_frame_images.

Workload: 1024 uint8 frames of 405 x 720 x 3 (0.9 GB, more than the Infinity Cache holds) -> 98 x 98 fp32 images, Lanczos.

  host    Image.fromarray(frame).resize((98, 98), Image.LANCZOS) and the scale by 1 / 255 per frame (wall clock, this
          box's CPU), timed on --host-frames frames and stated per frame; null where Pillow does not import
  device  the C call with the frames already on the device (events around the one launch), per --bands request (0 = the
          library's choice, which is the figure reported as `device`), and the whole Python call on a device tensor
          (wall clock: table lookup, allocation of the output, launch, status read)

Times are medians over --repeats timed runs after --warmup untimed ones.  The kernel's own time comes from a separate
run under `rocprofv3 --kernel-trace --stats` (--profile-only makes the calls and nothing else); --merge-kernel-stats CSV
adds it to the JSON.  Bytes moved = frames read once + images written once; the floor is that over the 6.29 TB/s a
float4 copy reaches on this chip.  Writes one JSON document (--out) and prints it.
"""
import argparse
import csv
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_COPY = 6.29e12
FRAME_HW, OUT_HW, FILTER = (405, 720), (98, 98), 'lanczos'


def pillow_images(frames, out_hw):
    from PIL import Image
    oh, ow = out_hw
    images = np.stack([np.array(Image.fromarray(f).resize((ow, oh), Image.LANCZOS)) for f in frames])
    return np.multiply(images.astype(np.float32), 1.0 / 255.0)


def merge_kernel_stats(result, path, profiled_calls):
    for row in csv.DictReader(open(path)):
        if 'frame_images_kernel' in row['Name']:
            ms = float(row['TotalDurationNs']) * 1e-6 / int(row['Calls'])
            result['kernel_trace'] = {'calls': int(row['Calls']), 'ms_per_call': ms, 'profiled_calls': profiled_calls,
                                      'fraction_of_floor': result['floor_ms'] / ms, 'source': os.path.basename(path)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--frames', type=int, default=1024)
    ap.add_argument('--host-frames', type=int, default=32)
    ap.add_argument('--bands', type=int, nargs='*', default=[0], help='band requests to time (0 = the library\'s choice)')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--profile-only', type=int, default=0, metavar='CALLS',
                    help='make CALLS calls and nothing else (for a run under rocprofv3 --kernel-trace --stats)')
    ap.add_argument('--merge-kernel-stats', nargs=2, metavar=('CSV', 'CALLS'),
                    help='add the kernel time of a kernel_stats.csv that covers CALLS calls to --out; needs no GPU')
    ap.add_argument('--out', default=os.path.join('profiles', 'frames_bench.json'))
    a = ap.parse_args()

    if a.merge_kernel_stats:
        with open(a.out) as fp:
            result = json.load(fp)
        merge_kernel_stats(result, a.merge_kernel_stats[0], int(a.merge_kernel_stats[1]))
        text = json.dumps(result, indent=1, sort_keys=True)
        with open(a.out, 'w') as fp:
            fp.write(text + '\n')
        print(text)
        return

    import torch
    from recurrent_gaze_prediction_amd import _lib
    from recurrent_gaze_prediction_amd import frames as fr
    if not torch.cuda.is_available():
        raise SystemExit('bench_frames.py needs a GPU: timings taken elsewhere say nothing about it')
    dev = torch.device('cuda:0')
    lib = _lib.load()

    N, (H, W), (oh, ow) = a.frames, FRAME_HW, OUT_HW
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    d_frames = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, device=dev, generator=gen)
    kh, bh, ksh = fr._device_tables(dev, W, ow, FILTER)
    kv, bv, ksv = fr._device_tables(dev, H, oh, FILTER)
    images = torch.empty((N, oh, ow, 3), dtype=torch.float32, device=dev)
    ws = torch.empty(max(int(lib.rgp_frames_workspace_bytes()), 64), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    moved = N * H * W * 3 + N * oh * ow * 3 * 4
    result = {'frames': N, 'frame_hw': list(FRAME_HW), 'out_hw': list(OUT_HW), 'filter': FILTER, 'ksize_h': ksh, 'ksize_v': ksv,
              'warmup': a.warmup, 'repeats': a.repeats, 'device_name': torch.cuda.get_device_name(0), 'threads': torch.get_num_threads(),
              'bytes_read': N * H * W * 3, 'bytes_written': N * oh * ow * 3 * 4, 'bytes_moved': moved,
              'hbm_copy_bytes_per_s': HBM_COPY, 'floor_ms': moved / HBM_COPY * 1e3}

    def run(bands):
        args = _lib.FramesArgs(frames=d_frames.data_ptr(), n_frames=N, fh=H, fw=W, frame_index=None, n_out=N, out_h=oh, out_w=ow,
                               kh=kh.data_ptr(), bh=bh.data_ptr(), ksize_h=ksh, kv=kv.data_ptr(), bv=bv.data_ptr(), ksize_v=ksv,
                               bands=bands, images=images.data_ptr(), images_u8=None, workspace=ws.data_ptr(),
                               workspace_bytes=ws.numel())
        _lib.check(lib.rgp_frame_images(ctypes.byref(args), stream))

    if a.profile_only:
        for _ in range(a.profile_only):
            run(0)
        torch.cuda.synchronize()
        print(json.dumps({'profiled_calls': a.profile_only}))
        return

    def timed(bands):
        times = []
        for i in range(a.warmup + a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(bands)
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                times.append(e0.elapsed_time(e1))
        _lib.check(lib.rgp_frames_status(ws.data_ptr(), None, stream))
        plan, lds, _ = fr.band_plan((H, W), (oh, ow), (ksh, ksv), N, bands or None)
        ms = float(np.median(times))
        return {'ms_median': ms, 'ms_min': float(np.min(times)), 'ms_max': float(np.max(times)), 'bands': len(plan),
                'lds_bytes_per_workgroup': lds, 'fraction_of_floor': result['floor_ms'] / ms, 'bytes_per_s': moved / (ms * 1e-3)}

    result['by_band_request'] = {str(b): timed(b) for b in a.bands if b != 0}
    result['device'] = timed(0)                         # last: `images` now holds the default banding's output
    result['device']['ms_per_frame'] = result['device']['ms_median'] / N

    Nh = min(a.host_frames, N)
    head = d_frames[:Nh].cpu().numpy()
    try:
        pillow_images(head[:1], OUT_HW)
        t0 = time.perf_counter()
        h_images = pillow_images(head, OUT_HW)
        host_ms = (time.perf_counter() - t0) * 1e3
        result['host'] = {'frames': Nh, 'ms': host_ms, 'ms_per_frame': host_ms / Nh, 'ms_for_all_frames': host_ms / Nh * N}
        result['equal_to_host'] = {'frames_compared': Nh, 'images': bool(np.array_equal(images[:Nh].cpu().numpy(), h_images))}
        result['speedup_host_over_device_launch'] = result['host']['ms_for_all_frames'] / result['device']['ms_median']
    except ImportError:
        result['host'] = result['equal_to_host'] = result['speedup_host_over_device_launch'] = None

    walls = []
    for i in range(a.warmup + a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fr.frame_images(d_frames, OUT_HW)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
        del out
    result['device']['python_call_ms_median'] = float(np.median(walls[a.warmup:]))
    if result['host']:
        result['speedup_host_over_device_python_call'] = result['host']['ms_for_all_frames'] / result['device']['python_call_ms_median']

    text = json.dumps(result, indent=1, sort_keys=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fp:
        fp.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
