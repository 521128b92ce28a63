#!/usr/bin/env python
"""Time the original-scale ground-truth gaze maps: host path (numpy scatter + scipy.ndimage.gaussian_filter, sigma = 19)
against rgp_gazemaps_full_from_fixations.

Workload: 1024 frames of 405 x 720 (raw (720, 405)), 16 observers, one sample per observer per frame; gazemaps and
fixationmaps requested: 2.4 GB of output.

  host    per frame the boolean map per observer, the sum, the division, scipy's gaussian_filter and the min-max
          normalisation (wall clock, this box's CPU), timed on --host-frames frames and stated per frame
  device  the C calls for all frames with the samples already on the device and one workspace reused (events around the
          chunk calls of gazemaps_original_scale's default frames_per_call), and the whole Python call, upload of the
          samples and allocation of the outputs included (wall clock)
  dense   the same calls on frames with a sample in every column, where the zero skipping of pass 1 finds nothing to
          skip: what the skipping buys is the difference (timed on --dense-frames frames, stated per frame)

Times are medians over --repeats timed runs after --warmup untimed ones.  Per-launch times come from a separate run
under `rocprofv3 --kernel-trace --stats` (--profile-only makes the calls and nothing else); --merge-kernel-stats CSV
adds them to the JSON with the bytes each launch must move and the share of the HBM figure DESIGN.md uses (8.0 TB/s
spec; 6.29 TB/s measured copy).  Writes one JSON document (--out) and prints it.
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

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12
RAW, SIGMA = (720, 405), 19


def host_maps(packed, sigma):
    import scipy.ndimage
    D1, D2 = packed.raw_shape
    N, n_obs = len(packed.frame_ptr) - 1, packed.n_observers
    frame = np.repeat(np.arange(N), np.diff(packed.frame_ptr))
    u, a, b = packed.samples.T
    gaze = np.zeros((N, D2, D1), np.float32)
    fix = np.zeros((N, D2, D1), np.float32)
    for t in range(N):
        rows = frame == t
        hit = np.zeros((n_obs, D2, D1), bool)
        hit[u[rows], b[rows], a[rows]] = True
        fix[t] = hit.sum(0)
        g = scipy.ndimage.gaussian_filter(fix[t] / np.float32(n_obs), sigma)
        if g.sum() != 0:
            g -= np.min(g)
            g /= np.max(g)
        gaze[t] = g
    return gaze, fix


def launch_bytes(n_pix):
    """Bytes per frame each launch must move: outputs written once, the intermediate plane written and read, the masks
    cleared and read (the head of the workspace and the samples are noise next to these)."""
    return {'memset': 4 * n_pix, 'scatter': 0, 'pass1': 4 * n_pix + 4 * n_pix + 4 * n_pix,      # masks read, fixationmaps and the plane written
            'pass2': 4 * n_pix + 4 * n_pix,                                                      # the plane read, gazemaps written
            'normalise': 4 * n_pix + 4 * n_pix}                                                  # gazemaps read and written


def launch_of(kernel_name):
    for key in ('scatter', 'pass1', 'pass2', 'normalise'):
        if 'gtmaps_full_' + key in kernel_name:
            return key
    return 'memset' if 'fillBuffer' in kernel_name else None


def merge_kernel_stats(result, path, profiled_frames):
    n_pix = RAW[0] * RAW[1]
    per_launch = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            key = launch_of(row['Name'])
            if key is None:
                continue
            e = per_launch.setdefault(key, {'calls': 0, 'total_ns': 0.0})
            e['calls'] += int(row['Calls'])
            e['total_ns'] += float(row['TotalDurationNs'])
    need = launch_bytes(n_pix)
    total_ms = total_bytes = 0.0
    for key, e in per_launch.items():
        ms = e['total_ns'] * 1e-6 / profiled_frames * result['frames']
        e['ms_per_%d_frames' % result['frames']] = ms
        e['bytes_per_frame'] = need[key]
        e['fraction_of_hbm_spec'] = need[key] * result['frames'] / (ms * 1e-3) / HBM_SPEC if ms > 0 else None
        total_ms += ms
        total_bytes += need[key] * result['frames']
    result['per_launch'] = per_launch
    result['per_launch_total'] = {'ms': total_ms, 'bytes': total_bytes, 'fraction_of_hbm_spec': total_bytes / (total_ms * 1e-3) / HBM_SPEC,
                                  'fraction_of_hbm_copy': total_bytes / (total_ms * 1e-3) / HBM_COPY,
                                  'profiled_frames': profiled_frames, 'source': os.path.basename(path)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--frames', type=int, default=1024)
    ap.add_argument('--observers', type=int, default=16)
    ap.add_argument('--host-frames', type=int, default=32)
    ap.add_argument('--dense-frames', type=int, default=128)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--profile-only', type=int, default=0, metavar='RUNS',
                    help='make RUNS sets of calls and nothing else (for a run under rocprofv3 --kernel-trace --stats)')
    ap.add_argument('--merge-kernel-stats', nargs=2, metavar=('CSV', 'FRAMES'),
                    help='add the per-launch times of a kernel_stats.csv that covers FRAMES frames to --out; needs no GPU')
    ap.add_argument('--out', default=os.path.join('profiles', 'gtmaps_full_bench.json'))
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
    from recurrent_gaze_prediction_amd import gazemaps as gm
    if not torch.cuda.is_available():
        raise SystemExit('bench_gtmaps_full.py needs a GPU: timings taken elsewhere say nothing about it')
    dev = torch.device('cuda:0')
    lib = _lib.load()

    N, n_obs, (D1, D2) = a.frames, a.observers, RAW
    rs = np.random.RandomState(0)
    observers = [(np.arange(N), rs.randint(0, D1, N), rs.randint(0, D2, N), N) for _ in range(n_obs)]
    packed = gm.pack_fixations(observers, RAW, frames=np.arange(N))
    # a sample in every column of every frame, the observers taking turns
    Nd = min(a.dense_frames, N)
    cols = np.tile(np.arange(D1), Nd)
    dense = gm.PackedFixations((np.arange(Nd + 1) * D1).astype(np.int32),
                               np.stack([cols % n_obs, cols, rs.randint(0, D2, Nd * D1)], 1).astype(np.int32), n_obs, RAW)
    w, r = gm.gaussian_weights(SIGMA)
    per_call = max(1, gm.FULL_WORKSPACE_TARGET // (8 * D1 * D2 + 4 * (3 + (D1 + 31) // 32)))
    result = {'frames': N, 'observers': n_obs, 'samples': int(len(packed.samples)), 'raw': list(RAW), 'sigma': SIGMA, 'radius': r,
              'warmup': a.warmup, 'repeats': a.repeats, 'device_name': torch.cuda.get_device_name(0), 'threads': torch.get_num_threads(),
              'frames_per_call': per_call, 'output_bytes': 2 * 4 * N * D1 * D2,
              'workspace_bytes': int(lib.rgp_gtmaps_full_workspace_bytes(min(per_call, N), D1, D2))}

    gaze = torch.empty((N, D2, D1), dtype=torch.float32, device=dev)
    fix = torch.empty_like(gaze)
    ws = torch.empty(result['workspace_bytes'], dtype=torch.uint8, device=dev)
    d_w = torch.from_numpy(w).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def calls(p):
        n_all = len(p.frame_ptr) - 1
        d_ptr, d_samples = torch.from_numpy(p.frame_ptr).to(dev), torch.from_numpy(p.samples).to(dev)

        def run():
            for lo in range(0, n_all, per_call):
                args = _lib.GtmapsFullArgs(frame_ptr=d_ptr[lo:].data_ptr(), samples=d_samples.data_ptr(), weights=d_w.data_ptr(),
                                           n_frames=min(per_call, n_all - lo), n_observers=n_obs, raw_d1=D1, raw_d2=D2, radius=r,
                                           gazemaps=gaze[lo:].data_ptr(), fixationmaps=fix[lo:].data_ptr(), workspace=ws.data_ptr(),
                                           workspace_bytes=ws.numel())
                _lib.check(lib.rgp_gazemaps_full_from_fixations(ctypes.byref(args), stream))
        return run, (d_ptr, d_samples)

    def timed(run, warmup, repeats):
        times = []
        for i in range(warmup + repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            if i >= warmup:
                times.append(e0.elapsed_time(e1))
        _lib.check(lib.rgp_gtmaps_full_status(ws.data_ptr(), None, stream))
        return {'ms_median': float(np.median(times)), 'ms_min': float(np.min(times)), 'ms_max': float(np.max(times))}

    run_sparse, keep_sparse = calls(packed)
    if a.profile_only:
        for _ in range(a.profile_only):
            run_sparse()
        torch.cuda.synchronize()
        print(json.dumps({'profiled_frames': a.profile_only * N}))
        return

    run_dense, keep_dense = calls(dense)
    d = timed(run_dense, a.warmup, a.repeats)
    result['dense_columns'] = dict(d, frames=Nd, ms_per_frame=d['ms_median'] / Nd)
    result['device'] = timed(run_sparse, a.warmup, a.repeats)            # last: gaze and fix now hold the timed workload's maps
    result['device']['ms_per_frame'] = result['device']['ms_median'] / N

    Nh = min(a.host_frames, N)
    head = gm.PackedFixations(packed.frame_ptr[:Nh + 1], packed.samples[:packed.frame_ptr[Nh]], n_obs, RAW)
    t0 = time.perf_counter()
    h_gaze, h_fix = host_maps(head, SIGMA)
    host_ms = (time.perf_counter() - t0) * 1e3
    result['host'] = {'frames': Nh, 'ms': host_ms, 'ms_per_frame': host_ms / Nh}
    result['equal_to_host'] = {'frames_compared': Nh, 'gazemaps': bool(np.array_equal(gaze[:Nh].cpu().numpy(), h_gaze)),
                               'fixationmaps': bool(np.array_equal(fix[:Nh].cpu().numpy(), h_fix))}
    del gaze, fix, ws
    torch.cuda.empty_cache()

    walls = []
    for i in range(a.warmup + a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = gm.gazemaps_original_scale(packed, device=dev)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
        del out
    result['device']['python_call_ms_median'] = float(np.median(walls[a.warmup:]))
    result['speedup_host_over_device_calls_per_frame'] = result['host']['ms_per_frame'] / result['device']['ms_per_frame']
    result['speedup_host_over_device_python_call_per_frame'] = result['host']['ms_per_frame'] / (result['device']['python_call_ms_median'] / N)
    result['speedup_skipped_over_dense_columns_per_frame'] = result['dense_columns']['ms_per_frame'] / result['device']['ms_per_frame']

    text = json.dumps(result, indent=1, sort_keys=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fp:
        fp.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
