#!/usr/bin/env python
"""Time the frame overlay: rgp_overlay against the host pipeline and against a plain copy of the same bytes.

Workload: 1024 softmax maps of 49 x 49 fp32 drawn over 1024 RGB frames of 405 x 720 uint8 that are in device memory,
alpha 0.4, jet.

  device  the C call with everything on the device, events around the whole call: the whole overlay (first launch: min /
          max per band; second launch: render), the same with the caller's limits (the first launch is skipped: the
          difference is what the first launch costs), and with heat_u8 as well.  The events enclose everything the call
          puts on the stream: besides the kernels the 64-byte memset of the status word and the two host-to-device
          copies of the spline tables (36 KB from pageable memory), so `times_the_copy` contains their latency too;
          no kernel trace was taken.  Then the whole Python call on device tensors (wall clock: colour table upload,
          both launches, the status read)
  copy    a device-to-device copy of the frames' bytes (as many bytes read and written as the overlay's frame traffic),
          timed in this script with the same events, alternating with the overlay: the floor the launches are judged by
  host    evaluation_metrics.resize (scipy) + bytescale + the colour table + PIL.Image.blend on a sample of --host-frames
          frames, wall clock; the figure for all frames is that times frames / sample: SCALED, not measured

Times are medians over --repeats timed runs after --warmup untimed ones, with min, max and the 10th / 90th percentile.
`first_frames_equal_oracle` compares the first three overlays and heat planes with tests/overlay_ref.py, byte for byte.
Writes one JSON document (--out) and prints it.
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

MAP_HW, FRAME_HW, ALPHA, CMAP = (49, 49), (405, 720), 0.4, 'jet'


def spread(times):
    t = np.asarray(times, np.float64)
    return {'ms_median': float(np.median(t)), 'ms_min': float(t.min()), 'ms_max': float(t.max()),
            'ms_p10': float(np.percentile(t, 10)), 'ms_p90': float(np.percentile(t, 90))}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--maps', type=int, default=1024)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=50)
    ap.add_argument('--host-frames', type=int, default=4)
    ap.add_argument('--out', default=os.path.join('profiles', 'overlay_bench.json'))
    a = ap.parse_args()

    import torch
    import overlay_ref as ref
    from recurrent_gaze_prediction_amd import _lib
    from recurrent_gaze_prediction_amd import overlay as ov
    if not torch.cuda.is_available():
        raise SystemExit('bench_overlay.py needs a GPU: timings taken elsewhere say nothing about it')
    dev = torch.device('cuda:0')
    lib = _lib.load()

    N, (h, w), (H, W) = a.maps, MAP_HW, FRAME_HW
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    d_maps = torch.softmax(torch.randn((N, h * w), device=dev, generator=gen), dim=1).reshape(N, h, w).contiguous()
    d_frames = torch.randint(0, 256, (N, H, W, 3), device=dev, generator=gen, dtype=torch.uint8)
    d_out = torch.empty_like(d_frames)
    d_copy = torch.empty_like(d_frames)
    d_heat = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    d_lut = torch.from_numpy(ov.colormap_lut(CMAP)).to(dev)
    d_limits = torch.tensor([[0.0, 0.01]] * N, dtype=torch.float32, device=dev)
    ws = torch.empty(max(int(lib.rgp_overlay_workspace_bytes(N, h, w, H, W)), 64), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    pix = N * H * W
    result = {'maps': N, 'map_hw': list(MAP_HW), 'frame_hw': list(FRAME_HW), 'alpha': ALPHA, 'colormap': CMAP, 'warmup': a.warmup,
              'repeats': a.repeats, 'device_name': torch.cuda.get_device_name(0), 'threads': torch.get_num_threads(),
              'frame_bytes_read_plus_written': 6 * pix,
              'device_times_enclose': 'the kernels, the memset of the status word and two host-to-device copies of the spline tables'}

    def run(limits, heat):
        args = _lib.OverlayArgs(frames=d_frames.data_ptr(), frame_idx=None, maps=d_maps.data_ptr(),
                                limits=d_limits.data_ptr() if limits else None, lut=d_lut.data_ptr(), alpha=ALPHA, flags=0,
                                out=d_out.data_ptr(), heat_u8=d_heat.data_ptr() if heat else None, n=N, n_src=N, h=h, w=w, H=H, W=W)
        _lib.check(lib.rgp_overlay(ctypes.byref(args), ws.data_ptr(), ws.numel(), stream))

    variants = {'overlay': lambda: run(False, False), 'overlay_with_limits_one_launch': lambda: run(True, False),
                'overlay_and_heat': lambda: run(False, True), 'copy_of_the_frames': lambda: d_copy.copy_(d_frames)}
    times = {k: [] for k in variants}
    for i in range(a.warmup + a.repeats):            # alternating: every variant sees the same neighbours on the machine
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
    _lib.check(lib.rgp_overlay_status(ws.data_ptr(), None, stream))
    result['device'] = {k: spread(v) for k, v in times.items()}
    copy_ms = result['device']['copy_of_the_frames']['ms_median']
    result['device']['copy_of_the_frames']['bytes_per_s'] = 6 * pix / (copy_ms * 1e-3)
    for k in ('overlay', 'overlay_with_limits_one_launch', 'overlay_and_heat'):
        d = result['device'][k]
        d['times_the_copy'] = d['ms_median'] / copy_ms
        d['us_per_frame'] = d['ms_median'] * 1e3 / N
    result['device']['first_launch_ms_by_difference'] = (result['device']['overlay']['ms_median']
                                                         - result['device']['overlay_with_limits_one_launch']['ms_median'])

    run(False, True)                                  # the tensors now hold the data-limits overlay and its heat
    torch.cuda.synchronize()
    k = min(3, N)
    h_frames, h_maps = d_frames[:max(k, a.host_frames)].cpu().numpy(), d_maps[:max(k, a.host_frames)].cpu().numpy()
    lut = ov.colormap_lut(CMAP)
    want_out, want_heat, _ = ref.overlay(h_frames[:k], h_maps[:k], lut, ALPHA)
    result['first_frames_equal_oracle'] = {'frames_compared': k, 'out': bool(np.array_equal(d_out[:k].cpu().numpy(), want_out)),
                                           'heat_u8': bool(np.array_equal(d_heat[:k].cpu().numpy(), want_heat))}

    walls = []
    for i in range(a.warmup + a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = ov.overlay_maps(d_frames, d_maps, alpha=ALPHA, colormap=CMAP, out=d_out)
        torch.cuda.synchronize()
        if i >= a.warmup:
            walls.append((time.perf_counter() - t0) * 1e3)
        del out
    result['python_call'] = spread(walls)

    try:
        from PIL import Image
        from recurrent_gaze_prediction_amd.evaluation_metrics import resize
        from recurrent_gaze_prediction_amd.models.extract_map import bytescale

        def host_one(frame, m):
            u = bytescale(np.asarray(resize(m, (H, W), order=3, mode='reflect')).astype(np.float32))
            return np.asarray(Image.blend(Image.fromarray(frame), Image.fromarray(lut[u]), ALPHA))
        host_one(h_frames[0], h_maps[0])
        t0 = time.perf_counter()
        for i in range(a.host_frames):
            host_one(h_frames[i], h_maps[i])
        host_ms = (time.perf_counter() - t0) * 1e3
        result['host'] = {'frames_measured': a.host_frames, 'ms_measured': host_ms, 'ms_per_frame': host_ms / a.host_frames,
                          'ms_all_frames_SCALED_not_measured': host_ms / a.host_frames * N}
    except ImportError as e:
        result['host'] = {'not_measured': 'scipy or Pillow does not import here: %s' % e}

    text = json.dumps(result, indent=1, sort_keys=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fp:
        fp.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
