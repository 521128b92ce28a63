#!/usr/bin/env python
"""Time gaze_lstm: the persistent ConvLSTM kernel against the per-step path, the training step, and gaze_grcn beside them.

Shapes: B 64 x T 16 and B 8 x T 35.  For each shape a bf16 'persistent' plan (RGP_LSTM_PERSISTENT) and a bf16 'per_step' plan
(RGP_LSTM_PER_STEP) are built in ONE process on one device, both shapes are warmed first, and the two paths ALTERNATE: a
window is --calls calls of one path between two device synchronisations (host clock), --windows windows per path; the
figure is the median window divided by the calls, the spread is (max - min) / median of the windows.  The forward is timed
on the placeholder layout (fp32 [B,T,1024,7,7]).  gaze_grcn's inference forward (GrcnEngine, bf16, its persistent ConvGRU
kernel) is timed in the same alternation at the same shapes.  The training step (forward + backward + clipped Adam +
re-pack) is timed the same way on two bf16 training plans per shape that alternate: 'train_step' with the flags of today
(BPTT per step) and 'train_step_bptt_persistent' (RGP_LSTM_BPTT_PERSISTENT); 'backward' / 'backward_bptt_persistent' are
windows of backward calls alone on the same two plans, so the BPTT's share is visible.

The rule for the default of eligible plans (bf16, <= 64 clips): the persistent kernel only if it is faster than the
per-step path at both shapes (every window, not just the medians); the JSON records the verdict next to what the library
does, for the forward (persistent_faster_at_both_shapes) and for the BPTT (bptt_persistent_faster_at_both_shapes, on the
training step).
--trace-only: a short run of every path for a profiler (rocprofv3 --kernel-trace --stats); no timing, no file.
Writes one JSON document (--out) and prints it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((64, 16), (8, 35))
PATHS = ('persistent', 'per_step', 'gaze_grcn')


def window(fn, calls, sync):
    sync()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    sync()
    return (time.perf_counter() - t0) * 1e3 / calls


def summarise(ms):
    med = float(np.median(ms))
    return {'ms_median': med, 'ms_min': float(np.min(ms)), 'ms_max': float(np.max(ms)),
            'spread': float((np.max(ms) - np.min(ms)) / med), 'windows': len(ms)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--calls', type=int, default=100, help='calls per timed window')
    ap.add_argument('--windows', type=int, default=7, help='windows per path (>= 7)')
    ap.add_argument('--train-calls', type=int, default=10)
    ap.add_argument('--trace', default=None, help='kernel-stats CSV of a separate rocprofv3 run to attach')
    ap.add_argument('--trace-only', action='store_true')
    ap.add_argument('--out', default=os.path.join('profiles', 'lstm_bench.json'))
    a = ap.parse_args()

    import torch
    from recurrent_gaze_prediction_amd import synthetic as syn
    from recurrent_gaze_prediction_amd.engine import GrcnEngine, LstmEngine
    if not torch.cuda.is_available():
        raise SystemExit('bench_lstm.py needs a GPU: timings taken elsewhere say nothing about it')
    dev = torch.device('cuda:0')
    sync = torch.cuda.synchronize
    params = syn.lstm_params(0)

    plans = {}
    for B, T in SHAPES:
        x = torch.tensor(syn.c3d_features(1, B, T), device=dev)
        out = (torch.empty(B, T, 49, 49, device=dev), torch.empty(B, T, 49, 49, device=dev))
        engs = {'persistent': LstmEngine(B, T, dtype='bf16', device=dev, persistent=True),
                'per_step': LstmEngine(B, T, dtype='bf16', device=dev, per_step=True)}
        assert engs['persistent'].persistent and not engs['per_step'].persistent
        for e in engs.values():
            e.set_weights(params)
        engs['gaze_grcn'] = GrcnEngine(B, T, dtype='bf16', device=dev)
        engs['gaze_grcn'].set_weights(syn.grcn_params(0, T))
        plans[(B, T)] = (x, out, engs)
    for (B, T), (x, out, engs) in plans.items():
        for e in engs.values():
            for _ in range(3):
                e.forward(x, out_logits=out[0], out_probs=out[1])
    sync()
    for (B, T), (x, out, engs) in plans.items():
        engs['persistent'].status()

    result = {'device': torch.cuda.get_device_name(0), 'calls_per_window': a.calls, 'windows': a.windows, 'dtype': 'bf16',
              'method': 'host clock around windows of calls between device synchronisations; paths alternate; median window / calls',
              'shapes': {}}
    for (B, T), (x, out, engs) in plans.items():
        if a.trace_only:
            break
        ms = {p: [] for p in PATHS}
        for _ in range(a.windows):
            for path in PATHS:
                ms[path].append(window(lambda: engs[path].forward(x, out_logits=out[0], out_probs=out[1]), a.calls, sync))
        entry = {'frames': B * T, 'forward': {p: summarise(v) for p, v in ms.items()}}
        f, s = entry['forward']['persistent'], entry['forward']['per_step']
        entry['forward']['persistent_over_per_step'] = f['ms_median'] / s['ms_median']
        entry['forward']['persistent_faster'] = bool(f['ms_max'] < s['ms_min'])      # every window, not just the medians
        result['shapes']['%dx%d' % (B, T)] = entry
    del plans
    for B, T in SHAPES:
        engs = {'': LstmEngine(B, T, dtype='bf16', save_for_backward=True, device=dev),
                '_bptt_persistent': LstmEngine(B, T, dtype='bf16', save_for_backward=True, device=dev, bptt_persistent=True)}
        assert engs['_bptt_persistent'].bptt_persistent and not engs[''].bptt_persistent
        x = torch.tensor(syn.c3d_features(1, B, T), device=dev)
        g = syn.gaze_maps(2, B, T)[0]
        labels = torch.tensor(g / g.reshape(B, T, -1).sum(-1)[..., None, None], device=dev).contiguous()
        step = [0]
        fwd = {}

        def train(eng):
            logits, probs = eng.forward(x)
            eng.backward(logits, probs, labels)
            eng.adam_step(step[0], 1e-4)
            step[0] += 1
        for k, eng in engs.items():
            eng.set_weights(params)
            for _ in range(3):
                train(eng)
            fwd[k] = eng.forward(x)
            eng.backward(fwd[k][0], fwd[k][1], labels)
        sync()
        for eng in engs.values():
            eng.status()
        if a.trace_only:
            continue
        ms = {kind + k: [] for kind in ('train_step', 'backward') for k in engs}
        for _ in range(a.windows):
            for k, eng in engs.items():
                ms['train_step' + k].append(window(lambda: train(eng), a.train_calls, sync))
            for k, eng in engs.items():
                eng.forward(x, out_logits=fwd[k][0], out_probs=fwd[k][1])
                ms['backward' + k].append(window(lambda: eng.backward(fwd[k][0], fwd[k][1], labels), a.train_calls, sync))
        entry = result['shapes']['%dx%d' % (B, T)]
        entry.update({k: summarise(v) for k, v in ms.items()})
        entry['bptt_persistent_faster'] = bool(entry['train_step_bptt_persistent']['ms_max'] < entry['train_step']['ms_min'])
        del engs
    if a.trace_only:
        return
    result['persistent_faster_at_both_shapes'] = all(e['forward']['persistent_faster'] for e in result['shapes'].values())
    result['bptt_persistent_faster_at_both_shapes'] = all(e['bptt_persistent_faster'] for e in result['shapes'].values())
    result['default_of_eligible_plans'] = 'persistent' if LstmEngine(2, 2, dtype='bf16', device=dev).persistent else 'per_step'
    result['default_bptt_of_eligible_plans'] = 'persistent' if LstmEngine(2, 2, dtype='bf16', save_for_backward=True,
                                                                          device=dev).bptt_persistent else 'per_step'
    if a.trace and os.path.exists(a.trace):
        rows_ = [l.rstrip('\n') for l in open(a.trace)]
        result['kernel_trace_stats'] = {'header': rows_[0], 'rows': [r for r in rows_[1:] if 'lstm' in r.lower() or 'igemm' in r or 'wgrad' in r or
                                                                     'col2im' in r or 'softmax' in r or 'nchw_to_rows' in r]}
    text = json.dumps(result, indent=1, sort_keys=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fp:
        fp.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
