#!/usr/bin/env python
"""Time the ground-truth gaze maps: host path (numpy scatter + scipy.ndimage.gaussian_filter) against the HIP kernel.

Workload: 1024 frames of 49x49 (what one end-to-end step of the driver consumes), 16 observers, one sample per
observer per frame, raw frame 405 x 720.

  host    per observer a boolean map per frame from the rescaled points, the sum over observers, the division, then per
          frame scipy's gaussian_filter and the min-max normalisation (wall clock, this box's CPU)
  device  rgp_gazemaps_from_fixations with the samples already on the device: the launch alone (events), gazemaps and
          fixationmaps requested; and the whole Python call, upload of the samples included (wall clock)

Launch times are medians over --repeats timed launches after --warmup untimed ones, from device events around the C
call.  Writes one JSON document (--out) and prints it.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def host_maps(packed, out_shape, sigma):
    import scipy.ndimage
    (D1, D2), (S1, S2) = packed.raw_shape, out_shape
    N, n_obs = len(packed.frame_ptr) - 1, packed.n_observers
    frame = np.repeat(np.arange(N), np.diff(packed.frame_ptr))
    u, a, b = packed.samples.T
    a_ = (np.round(a * (S1 - 1.0) / (D1 - 1.0)) + 1e-9).astype(np.int64)
    b_ = (np.round(b * (S2 - 1.0) / (D2 - 1.0)) + 1e-9).astype(np.int64)
    hit = np.zeros((n_obs, N, S2, S1), bool)
    hit[u, frame, b_, a_] = True
    fix = hit.sum(0)
    gaze = fix.astype(np.float32) / n_obs
    for t in range(N):
        g = scipy.ndimage.gaussian_filter(gaze[t], sigma)
        if g.sum() == 0:
            continue
        g -= np.min(g)
        g /= np.max(g)
        gaze[t] = g
    return gaze, fix.astype(np.float32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--frames', type=int, default=1024)
    ap.add_argument('--observers', type=int, default=16)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=50)
    ap.add_argument('--out', default=os.path.join('profiles', 'gtmaps_bench.json'))
    a = ap.parse_args()

    import torch
    from recurrent_gaze_prediction_amd import _lib
    from recurrent_gaze_prediction_amd import gazemaps as gm
    if not torch.cuda.is_available():
        raise SystemExit('bench_gtmaps.py needs a GPU: timings taken elsewhere say nothing about it')
    dev = torch.device('cuda:0')
    lib = _lib.load()

    N, n_obs, raw, shape, sigma = a.frames, a.observers, (405, 720), (49, 49), 2.0
    rs = np.random.RandomState(0)
    observers = [(np.arange(N), rs.randint(0, raw[0], N), rs.randint(0, raw[1], N), N) for _ in range(n_obs)]
    packed = gm.pack_fixations(observers, raw, frames=np.arange(N))
    w, r = gm.gaussian_weights(sigma)
    result = {'frames': N, 'map': list(shape), 'observers': n_obs, 'samples': int(len(packed.samples)), 'raw': list(raw),
              'sigma': sigma, 'radius': r, 'warmup': a.warmup, 'repeats': a.repeats, 'device': torch.cuda.get_device_name(0),
              'threads': torch.get_num_threads()}

    host_ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        h_gaze, h_fix = host_maps(packed, shape, sigma)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    result['host'] = {'ms_median': float(np.median(host_ms)), 'ms_min': float(np.min(host_ms)), 'runs': len(host_ms)}

    d_ptr, d_samples, d_w = (torch.from_numpy(x).to(dev) for x in (packed.frame_ptr, packed.samples, w))
    gaze = torch.empty((N, shape[1], shape[0]), dtype=torch.float32, device=dev)
    fix = torch.empty_like(gaze)
    ws = torch.empty(int(lib.rgp_gtmaps_workspace_bytes()), dtype=torch.uint8, device=dev)
    args = _lib.GtmapsArgs(frame_ptr=d_ptr.data_ptr(), samples=d_samples.data_ptr(), weights=d_w.data_ptr(), n_frames=N,
                           n_observers=n_obs, raw_d1=raw[0], raw_d2=raw[1], out_s1=shape[0], out_s2=shape[1], radius=r,
                           gazemaps=gaze.data_ptr(), fixationmaps=fix.data_ptr(), labels=None, workspace=ws.data_ptr(),
                           workspace_bytes=ws.numel())
    stream = torch.cuda.current_stream(dev).cuda_stream
    times = []
    for i in range(a.warmup + a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(lib.rgp_gazemaps_from_fixations(ctypes.byref(args), stream))
        e1.record()
        e1.synchronize()
        if i >= a.warmup:
            times.append(e0.elapsed_time(e1))
    _lib.check(lib.rgp_gtmaps_status(ws.data_ptr(), stream))
    result['device'] = {'ms_median': float(np.median(times)), 'ms_min': float(np.min(times)), 'ms_max': float(np.max(times))}
    result['equal_to_host'] = {'gazemaps': bool(np.array_equal(gaze.cpu().numpy(), h_gaze)),
                               'fixationmaps': bool(np.array_equal(fix.cpu().numpy(), h_fix))}

    walls = []
    for i in range(a.warmup + a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gm.gazemaps_from_fixations(packed, out_shape=shape, sigma=sigma, device=dev)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    result['device']['python_call_ms_median'] = float(np.median(walls[a.warmup:]))
    result['speedup_host_over_device_launch'] = result['host']['ms_median'] / result['device']['ms_median']
    result['speedup_host_over_device_python_call'] = result['host']['ms_median'] / result['device']['python_call_ms_median']

    text = json.dumps(result, indent=1, sort_keys=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fp:
        fp.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
