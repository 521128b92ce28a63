#!/usr/bin/env python
"""Time gaze_grcn77: its inference forward on the persistent ConvGRU kernel and on the per-step path, gaze_grcn's forward
beside them, the read-out kernel alone, and the training step.

Shapes: B 64 x T 16 and B 8 x T 35.  The method is scripts/bench_lstm.py's: for each shape a bf16 'persistent' plan, a bf16
'per_step' plan (RGP_GRCN77_PER_STEP) and gaze_grcn's bf16 plan (GrcnEngine, its persistent kernel and folded up-sampling
head) are built in ONE process on one device, both shapes are warmed first, and the paths ALTERNATE: a window is --calls
calls of one path between two device synchronisations (host clock), --windows windows per path; the figure is the median
window divided by the calls, the spread is (max - min) / median of the windows.  The forward is timed on the placeholder
layout (fp32 [B,T,1024,7,7]).  'head' is windows of the read-out stage alone (rgp_grcn77_head_fwd on the plan's states:
one launch of head_point_fwd_kernel per call); its achieved bytes/s is (F*49*128*4 state bytes + 2*F*49*4 output bytes) /
time, next to the HBM figure of the micro-architecture guide (6.29 TB/s measured float4 copy, 8.0 TB/s spec) -- from the
host-clock windows, which include the launch, and, with --trace, from the kernel times of a separate rocprofv3 run.  The
training step (forward + backward + clipped Adam + re-pack) is timed the same way on a bf16 training plan per shape.

The sanity relation: at both shapes grcn77's forward median should not exceed gaze_grcn's in the same alternation (the same
graph with a far lighter head); the JSON records it per shape (grcn77_not_slower_than_gaze_grcn).
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
HBM_TBS = {'measured_float4_copy': 6.29, 'spec': 8.0}          # MI355X micro-architecture guide


def head_bytes(frames):
    """What the read-out has to move: the fp32 states in, logits and probs out."""
    return frames * 49 * 128 * 4 + 2 * frames * 49 * 4


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
    ap.add_argument('--out', default=os.path.join('profiles', 'grcn77_bench.json'))
    a = ap.parse_args()

    import torch
    from recurrent_gaze_prediction_amd import synthetic as syn
    from recurrent_gaze_prediction_amd.engine import Grcn77Engine, GrcnEngine
    if not torch.cuda.is_available():
        raise SystemExit('bench_grcn77.py needs a GPU: timings taken elsewhere say nothing about it')
    dev = torch.device('cuda:0')
    sync = torch.cuda.synchronize
    params = syn.grcn77_params(0)

    plans = {}
    for B, T in SHAPES:
        x = torch.tensor(syn.c3d_features(1, B, T), device=dev)
        out7 = (torch.empty(B, T, 7, 7, device=dev), torch.empty(B, T, 7, 7, device=dev))
        out49 = (torch.empty(B, T, 49, 49, device=dev), torch.empty(B, T, 49, 49, device=dev))
        engs = {'persistent': Grcn77Engine(B, T, dtype='bf16', device=dev),
                'per_step': Grcn77Engine(B, T, dtype='bf16', device=dev, per_step=True)}
        assert engs['persistent'].persistent and not engs['per_step'].persistent
        for e in engs.values():
            e.set_weights(params)
        engs['gaze_grcn'] = GrcnEngine(B, T, dtype='bf16', device=dev)
        engs['gaze_grcn'].set_weights(syn.grcn_params(0, T))
        plans[(B, T)] = (x, {'persistent': out7, 'per_step': out7, 'gaze_grcn': out49}, engs)
    for (B, T), (x, outs, engs) in plans.items():
        for k, e in engs.items():
            for _ in range(3):
                e.forward(x, out_logits=outs[k][0], out_probs=outs[k][1])
        for _ in range(3):
            engs['persistent'].head_forward()
    sync()
    for (B, T), (x, outs, engs) in plans.items():
        engs['persistent'].status()
        engs['gaze_grcn'].status()

    result = {'device': torch.cuda.get_device_name(0), 'calls_per_window': a.calls, 'windows': a.windows, 'dtype': 'bf16',
              'method': 'host clock around windows of calls between device synchronisations; paths alternate; median window / calls',
              'hbm_tb_per_s': HBM_TBS, 'shapes': {}}
    for (B, T), (x, outs, engs) in plans.items():
        if a.trace_only:
            break
        ms = {p: [] for p in PATHS + ('head',)}
        for _ in range(a.windows):
            for path in PATHS:
                ms[path].append(window(lambda: engs[path].forward(x, out_logits=outs[path][0], out_probs=outs[path][1]), a.calls, sync))
            ms['head'].append(window(engs['persistent'].head_forward, a.calls, sync))
        entry = {'frames': B * T, 'forward': {p: summarise(ms[p]) for p in PATHS}, 'head': summarise(ms['head'])}
        f = entry['forward']
        f['persistent_over_per_step'] = f['persistent']['ms_median'] / f['per_step']['ms_median']
        f['grcn77_over_gaze_grcn'] = f['persistent']['ms_median'] / f['gaze_grcn']['ms_median']
        f['grcn77_not_slower_than_gaze_grcn'] = bool(f['persistent']['ms_median'] <= f['gaze_grcn']['ms_median'])
        entry['head']['bytes'] = head_bytes(B * T)
        entry['head']['tb_per_s_host_window'] = head_bytes(B * T) / (entry['head']['ms_median'] * 1e-3) / 1e12
        entry['head']['note'] = 'host-clock window of launches of head_point_fwd_kernel (plus two torch.empty): an upper bound of the kernel time'
        result['shapes']['%dx%d' % (B, T)] = entry
    del plans
    for B, T in SHAPES:
        eng = Grcn77Engine(B, T, dtype='bf16', save_for_backward=True, device=dev)
        x = torch.tensor(syn.c3d_features(1, B, T), device=dev)
        g = syn.gaze_maps(2, B, T, hw=7)[0]
        labels = torch.tensor(g / g.reshape(B, T, -1).sum(-1)[..., None, None], device=dev).contiguous()
        step = [0]

        def train():
            logits, probs = eng.forward(x)
            eng.backward(logits, probs, labels)
            eng.adam_step(step[0], 1e-4)
            step[0] += 1
        eng.set_weights(params)
        for _ in range(3):
            train()
        fwd = eng.forward(x)
        eng.backward(fwd[0], fwd[1], labels)
        sync()
        eng.status()
        if a.trace_only:
            continue
        ms = {'train_step': [], 'backward': []}
        for _ in range(a.windows):
            ms['train_step'].append(window(train, a.train_calls, sync))
            eng.forward(x, out_logits=fwd[0], out_probs=fwd[1])
            ms['backward'].append(window(lambda: eng.backward(fwd[0], fwd[1], labels), a.train_calls, sync))
        result['shapes']['%dx%d' % (B, T)].update({k: summarise(v) for k, v in ms.items()})
        del eng
    if a.trace_only:
        return
    result['grcn77_not_slower_than_gaze_grcn_at_both_shapes'] = all(
        e['forward']['grcn77_not_slower_than_gaze_grcn'] for e in result['shapes'].values())
    if a.trace and os.path.exists(a.trace):
        rows_ = [l.rstrip('\n') for l in open(a.trace)]
        result['kernel_trace_stats'] = {'header': rows_[0], 'rows': [r for r in rows_[1:] if 'head_point' in r]}
    text = json.dumps(result, indent=1, sort_keys=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fp:
        fp.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
