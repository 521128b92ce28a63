#!/usr/bin/env python
"""Time the saliency metrics: host module against the HIP metrics kernel.

Workload: 1024 frames of 49x49 (what one end-to-end step of the driver produces), six metrics, 100 repetitions
of the sampled AUCs.  Three ways to score them:

  host              evaluation_metrics, one frame and one metric at a time (wall clock)
  device-reference  the kernel fed with the host's own draws: the host draw time (draw_reference_samples, dominated
                    by n_frames * n_rep numpy permutation calls), the upload of the draws, and the launch are
                    reported separately
  device            the kernel with its own Philox draws, maps already on the device: the launch alone (events),
                    and the whole Python call (wall clock up to the scores on the host)

Launch times are medians over --repeats timed launches after --warmup untimed ones, from device events around
the C call; wall-clock figures end in a device synchronise.  Writes one JSON document (--out) and prints it.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--frames', type=int, default=1024)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=50)
    ap.add_argument('--host-frames', type=int, default=None, help='frames the host path is timed on (default: all)')
    ap.add_argument('--skip-host', action='store_true')
    ap.add_argument('--out', default=os.path.join('profiles', 'metrics_bench.json'))
    a = ap.parse_args()

    import torch
    from recurrent_gaze_prediction_amd import _lib
    from recurrent_gaze_prediction_amd import evaluation_metrics as em
    from recurrent_gaze_prediction_amd import evaluation_metrics_gpu as emg
    from recurrent_gaze_prediction_amd import synthetic as syn
    if not torch.cuda.is_available():
        raise SystemExit('bench_metrics.py needs a GPU: timings taken elsewhere say nothing about it')
    dev = torch.device('cuda:0')
    lib = _lib.load()

    N, n_rep = a.frames, 100
    gt, centres = syn.gaze_maps(0, N, 1)
    fix = syn.fixation_maps(1, centres)[:, 0]
    gt = gt[:, 0]
    pred = (np.random.RandomState(2).rand(*gt.shape) + 0.05).astype(np.float32)       # random positive maps
    other = (fix[np.random.RandomState(3).choice(N, 10, replace=False)] > 0).sum(0).astype(np.float32)
    n_fix = (fix > 0.5).reshape(N, -1).sum(1)
    result = {'frames': N, 'map': [49, 49], 'metrics': list(emg.METRICS), 'n_rep': n_rep, 'warmup': a.warmup, 'repeats': a.repeats,
              'fixations_per_frame': [int(n_fix.min()), int(n_fix.max())], 'negative_set': int((other > 0.5).sum()),
              'device': torch.cuda.get_device_name(0), 'threads': torch.get_num_threads()}

    # ---- host
    host = None
    if not a.skip_host:
        nh = a.host_frames or N
        per_metric, host = {}, {}
        np.random.seed(0)
        for m in emg.METRICS:
            t0 = time.perf_counter()
            host[m] = np.array([em.saliency_score_single(m, p, g, f, other) for p, g, f in zip(pred[:nh], gt[:nh], fix[:nh])])
            per_metric[m] = (time.perf_counter() - t0) * 1e3
        result['host'] = {'frames': nh, 'ms_per_metric': per_metric, 'ms': sum(per_metric.values())}

    d_pred, d_gt, d_fix, d_other = (torch.tensor(x, device=dev) for x in (pred, gt, fix, other))
    stream = torch.cuda.current_stream(dev).cuda_stream

    def time_launches(args):
        times = []
        for i in range(a.warmup + a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(lib.rgp_saliency_scores(ctypes.byref(args), stream))
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                times.append(e0.elapsed_time(e1))
        _lib.check(lib.rgp_metrics_status(args.workspace, stream))
        return {'ms_median': float(np.median(times)), 'ms_min': float(np.min(times)), 'ms_max': float(np.max(times))}

    def make_args(flags, stride, ws, scores, **draws):
        return _lib.MetricsArgs(pred=d_pred.data_ptr(), gt=d_gt.data_ptr(), fix=d_fix.data_ptr(), other=d_other.data_ptr(),
                                other_stride=0, n_frames=N, height=49, width=49, metrics=63, flags=flags, n_rep=n_rep,
                                neg_stride=stride, step_size=0.1, seed=0, offset=0, workspace=ws.data_ptr(),
                                workspace_bytes=ws.numel(), scores=scores.data_ptr(), **draws)

    # ---- device, the host's draws
    np.random.seed(0)
    t0 = time.perf_counter()
    packed = emg.draw_reference_samples(fix, other, emg.METRICS, n_rep=n_rep)
    draw_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    up = {k: torch.from_numpy(packed[k]).to(dev) for k in ('judd_jitter', 'borji_neg', 'shuf_neg', 'shuf_cnt')}
    torch.cuda.synchronize()
    upload_ms = (time.perf_counter() - t0) * 1e3
    stride = int(packed['neg_stride'])
    ws = torch.empty(lib.rgp_metrics_workspace_bytes(N, n_rep, stride, 0), dtype=torch.uint8, device=dev)
    scores = torch.zeros(6, N, dtype=torch.float64, device=dev)
    ref = time_launches(make_args(0, stride, ws, scores, **{k: v.data_ptr() for k, v in up.items()}))
    ref.update(host_draws_ms=draw_ms, upload_draws_ms=upload_ms, upload_bytes=int(sum(v.numel() * v.element_size() for v in up.values())))
    result['device_reference'] = ref
    if host is not None:
        s = scores.cpu().numpy()
        result['max_abs_diff_to_host'] = {m: float(np.nanmax(np.abs(s[_lib.METRIC_ROWS[m], :len(host[m])] - host[m])))
                                          for m in emg.METRICS}

    # ---- device, device draws
    flags = _lib.RGP_METRICS_DEVICE_DRAWS
    ws = torch.empty(lib.rgp_metrics_workspace_bytes(N, n_rep, stride, flags), dtype=torch.uint8, device=dev)
    result['device'] = time_launches(make_args(flags, stride, ws, scores))
    walls = []
    for i in range(a.warmup + a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = emg.saliency_scores_single(d_pred, d_gt, d_fix, d_other, emg.METRICS, draws='device', seed=i)
        walls.append((time.perf_counter() - t0) * 1e3)
    result['device']['python_call_ms_median'] = float(np.median(walls[a.warmup:]))
    result['device']['means'] = {m: float(np.mean(out[m])) for m in emg.METRICS}
    if host is not None:
        result['host']['means'] = {m: float(np.mean(host[m])) for m in emg.METRICS}
        scale = N / float(result['host']['frames'])
        result['speedup_host_over_device_launch'] = result['host']['ms'] * scale / result['device']['ms_median']
        result['speedup_host_over_device_python_call'] = result['host']['ms'] * scale / result['device']['python_call_ms_median']

    text = json.dumps(result, indent=1, sort_keys=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fp:
        fp.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
