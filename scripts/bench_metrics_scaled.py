#!/usr/bin/env python
"""Time the saliency metrics at frame resolution: host module against the HIP kernel that resizes on the fly.

Workload: 1024 frames of 49x49 scored against 405x720 fixation maps (what the reference's evaluate_gaze.py runs),
at most 16 fixations per frame, six metrics, 100 repetitions of the sampled AUCs.

  host     evaluation_metrics.saliency_score_single on a SAMPLE of frames (--host-frames), wall clock, scaled to all
           frames and labelled as such: the whole set takes minutes
  device   rgp_saliency_scores_scaled with its own Philox draws, maps and points already on the device: the launch
           alone (device events around the C call, median of --repeats after --warmup) and the whole Python call
           (wall clock up to the scores on the host)
  resize   rgp_spline_resize alone at the same shape (fp64 output), and whether its values equal the numpy oracle
           of tests/spline_ref.py bit for bit on the first frames

Writes one JSON document (--out) and prints it.  ``--table JSON`` prints DESIGN section 20's table from such a document
(no GPU needed).
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


def table(r):
    """DESIGN section 20's table from the JSON document of a run."""
    h, d, z = r['host'], r['device'], r['resize']
    rows = [
        ('host module (scipy resize + numpy), %d frames timed' % h['frames_timed'], '%.1f ms = %.1f ms per frame' % (h['ms_on_the_sample'], h['ms_per_frame']),
         'wall clock, six metrics'),
        ('host module, SCALED to %d frames' % r['frames'], '%.0f ms' % h['ms_scaled_to_all_frames'], 'the sample times frames / frames timed: not measured'),
        ('device, launch', '%.2f ms (min %.2f, max %.2f)' % (d['ms_median'], d['ms_min'], d['ms_max']),
         'maps and points already on the device; device draws; median of %d after %d warm-ups' % (r['repeats'], r['warmup'])),
        ('device, whole Python call', '%.2f ms' % d['python_call_ms_median'], 'allocation, table upload, launch, status read, scores to the host'),
        ('`rgp_spline_resize` alone, fp64 output', '%.2f ms (min %.2f, max %.2f)' % (z['ms_median'], z['ms_min'], z['ms_max']),
         '%.2f GB written; equal to the numpy oracle on the first %d frames: %s' % (z['output_bytes'] / 1e9, z['oracle_frames'], z['equal_to_oracle'])),
    ]
    out = ['| path | time | notes |', '|---|---|---|'] + ['| %s | %s | %s |' % row for row in rows]
    return '\n'.join(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--frames', type=int, default=1024)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=50)
    ap.add_argument('--host-frames', type=int, default=4, help='frames the host path is timed on')
    ap.add_argument('--out', default=os.path.join('profiles', 'metrics_scaled_bench.json'))
    ap.add_argument('--table', metavar='JSON', help='print the DESIGN table of an earlier run and exit')
    a = ap.parse_args()
    if a.table:
        with open(a.table) as fp:
            print(table(json.load(fp)))
        return

    import torch
    from recurrent_gaze_prediction_amd import _lib
    from recurrent_gaze_prediction_amd import evaluation_metrics as em
    from recurrent_gaze_prediction_amd import evaluation_metrics_gpu as emg
    from recurrent_gaze_prediction_amd import synthetic as syn
    import spline_ref
    if not torch.cuda.is_available():
        raise SystemExit('bench_metrics_scaled.py needs a GPU: timings taken elsewhere say nothing about it')
    dev = torch.device('cuda:0')
    lib = _lib.load()

    N, n_rep, (h, w), (H, W) = a.frames, 100, (49, 49), (405, 720)
    gt = syn.gaze_maps(0, N, 1)[0][:, 0]
    pred = (gt + 0.3 * np.random.RandomState(2).rand(*gt.shape)).astype(np.float32)
    rs = np.random.RandomState(1)
    points = [np.sort(rs.choice(H * W, rs.randint(4, 17), replace=False)) for _ in range(N)]
    ptr = np.concatenate([[0], np.cumsum([len(p) for p in points])]).astype(np.int32)
    idx = np.concatenate(points).astype(np.int32)
    union = np.unique(np.concatenate([points[i] for i in np.random.RandomState(3).choice(N, 10, replace=False)]))
    other = (np.array([0, len(union)], np.int32), union.astype(np.int32))
    n_fix = np.diff(ptr)
    result = {'frames': N, 'map': [h, w], 'fixation_map': [H, W], 'metrics': list(emg.METRICS), 'n_rep': n_rep, 'warmup': a.warmup,
              'repeats': a.repeats, 'fixations_per_frame': [int(n_fix.min()), int(n_fix.max())], 'negative_set': int(len(union)),
              'device': torch.cuda.get_device_name(0), 'threads': torch.get_num_threads()}

    # ---- host, a sample of frames
    nh = min(a.host_frames, N)
    other_map = np.zeros(H * W)
    other_map[union] = 1
    other_map = other_map.reshape(H, W)
    per_metric, host = {}, {}
    np.random.seed(0)
    for m in emg.METRICS:
        t0 = time.perf_counter()
        vals = []
        for i in range(nh):
            f = np.zeros(H * W, np.float32)
            f[points[i]] = 1
            vals.append(em.saliency_score_single(m, pred[i], gt[i], f.reshape(H, W), other_map))
        host[m] = np.array(vals)
        per_metric[m] = (time.perf_counter() - t0) * 1e3
    host_ms = sum(per_metric.values())
    result['host'] = {'frames_timed': nh, 'ms_per_metric_on_the_sample': per_metric, 'ms_on_the_sample': host_ms,
                      'ms_per_frame': host_ms / nh, 'ms_scaled_to_all_frames': host_ms / nh * N,
                      'note': 'measured on frames_timed frames and scaled linearly to `frames`; not a measurement of all frames'}

    # ---- device, device draws
    d_pred, d_gt = torch.tensor(pred, device=dev), torch.tensor(gt, device=dev)
    d_ptr, d_idx, d_optr, d_oidx = (torch.tensor(x, device=dev) for x in (ptr, idx, other[0], other[1]))
    stream = torch.cuda.current_stream(dev).cuda_stream
    flags = _lib.RGP_METRICS_DEVICE_DRAWS | _lib.RGP_METRICS_SCALED_OTHER_SHARED
    stride = int(n_fix.max())
    ws = torch.empty(lib.rgp_metrics_scaled_workspace_bytes(N, n_rep, stride, H, W, flags), dtype=torch.uint8, device=dev)
    scores = torch.zeros(6, N, dtype=torch.float64, device=dev)
    args = _lib.MetricsScaledArgs(pred=d_pred.data_ptr(), gt=d_gt.data_ptr(), fix_ptr=d_ptr.data_ptr(), fix_idx=d_idx.data_ptr(),
                                  other_ptr=d_optr.data_ptr(), other_idx=d_oidx.data_ptr(), fix_len=len(idx), other_len=len(union),
                                  n_frames=N, height=h, width=w, target_height=H, target_width=W, metrics=63, flags=flags, n_rep=n_rep,
                                  neg_stride=stride, step_size=0.1, seed=0, offset=0, workspace=ws.data_ptr(),
                                  workspace_bytes=ws.numel(), scores=scores.data_ptr())

    def time_calls(call):
        times = []
        for i in range(a.warmup + a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(call())
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                times.append(e0.elapsed_time(e1))
        return {'ms_median': float(np.median(times)), 'ms_min': float(np.min(times)), 'ms_max': float(np.max(times))}

    result['device'] = time_calls(lambda: lib.rgp_saliency_scores_scaled(ctypes.byref(args), stream))
    _lib.check(lib.rgp_metrics_status(ws.data_ptr(), stream))
    result['device']['workspace_bytes'] = int(ws.numel())
    walls = []
    for i in range(a.warmup + min(a.repeats, 10)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = emg.saliency_scores_resized(d_pred, d_gt, (d_ptr, d_idx), (d_optr, d_oidx), emg.METRICS, draws='device', seed=i,
                                          shape=(H, W), max_fix=stride)
        walls.append((time.perf_counter() - t0) * 1e3)
    result['device']['python_call_ms_median'] = float(np.median(walls[a.warmup:]))
    result['device']['means'] = {m: float(np.nanmean(out[m])) for m in emg.METRICS}
    result['host']['means_on_the_sample'] = {m: float(np.nanmean(host[m])) for m in emg.METRICS}
    s = scores.cpu().numpy()
    result['max_abs_diff_to_host_sim_cc_nss'] = {m: float(np.nanmax(np.abs(s[_lib.METRIC_ROWS[m], :nh] - host[m])))
                                                 for m in ('sim', 'cc', 'NSS')}
    result['speedup_scaled_host_over_device_launch'] = result['host']['ms_scaled_to_all_frames'] / result['device']['ms_median']
    result['speedup_scaled_host_over_device_python_call'] = (result['host']['ms_scaled_to_all_frames'] /
                                                             result['device']['python_call_ms_median'])

    # ---- the resize alone
    dst = torch.empty((N, H, W), dtype=torch.float64, device=dev)
    rws = torch.empty(lib.rgp_spline_resize_workspace_bytes(H, W), dtype=torch.uint8, device=dev)
    result['resize'] = time_calls(lambda: lib.rgp_spline_resize(d_pred.data_ptr(), 0, N, h, w, dst.data_ptr(), 1, H, W, rws.data_ptr(),
                                                                 rws.numel(), stream))
    result['resize']['output_bytes'] = int(dst.numel() * 8)
    k = min(N, 3)
    want = np.stack([spline_ref.resize(pred[i], (H, W)) for i in range(k)])
    result['resize']['equal_to_oracle'] = bool(np.array_equal(dst[:k].cpu().numpy(), want))
    result['resize']['oracle_frames'] = k

    text = json.dumps(result, indent=1, sort_keys=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fp:
        fp.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
