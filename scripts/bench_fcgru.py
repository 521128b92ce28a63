#!/usr/bin/env python
"""Time the fc-GRU (gaze_rnn, gaze_rnn77): the persistent recurrence (RGP_FCGRU_PERSISTENT, csrc/fcgru_seq.hip.h) against the
per-step path, forward and training step.

Shapes (B x T, map side): 64x16 (BASELINE config 2, 7x7), 8x35 (49x49) and 7x35 (gaze_rnn77's, 7x7), bf16.  For each shape
one 'per_step' and one 'persistent' plan with the same weights are built in ONE process on one device, all are warmed
first, and the two paths ALTERNATE: a window is --calls calls of one path between two device synchronisations (host
clock), --windows windows per path; the figure is the median window divided by the calls, the spread is (max - min) /
median of the windows (the protocol of bench_stream.py).  The training step is forward + backward + clipped Adam + re-pack
on two training plans per shape, alternating the same way.

--forward-only: the inference forward alone, and of the per-step path alone on a build whose engine has no `persistent`
argument: for build-to-build A/Bs of the default path (run it on both builds, alternating).
--bptt: the persistent BPTT (RGP_FCGRU_BPTT_PERSISTENT, csrc/fcgru_bptt.hip.h) against the per-step BPTT, each behind both
forwards: four training plans per shape in one process, alternating as above; the backward alone (backward() called again and
again behind one forward: it reads what the forward kept) and the training step.  Then the backward alone at T = 16 and T = 32
on 7x7 plans of 8 and 64 clips behind the per-step forward: the difference over 16 is what one more step costs each BPTT path.
Writes profiles/fcgru_bptt_bench.json unless --out names another file.  --train-only (with a build that has no `persistent`
argument too): the training step of per-step plans alone, for build-to-build A/Bs of the default path.
--dtype f32: the same protocol on f32 plans, the f32 persistent recurrence (RGP_FCGRU_PERSISTENT_F32, csrc/fcgru_seq_f32.hip.h)
against the per-step f32 path; then the inference forward at T = 16 and T = 32 on 7x7 plans of 8 and 64 clips: the difference
over 16 is what one more step costs each path.  Writes profiles/fcgru_f32_bench.json unless --out names another file.
--dtype f32 --bptt: the --bptt protocol on f32 plans, the f32 persistent BPTT (RGP_FCGRU_BPTT_PERSISTENT_F32,
csrc/fcgru_bptt_f32.hip.h) against the per-step f32 BPTT behind both f32 forwards.  Writes profiles/fcgru_f32_bptt_bench.json
unless --out names another file.
--per-step-only: the per-step path alone, whatever the build offers (build-to-build A/Bs of the default path in either dtype).
Writes one JSON document (--out) and prints it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((64, 16, 7), (8, 35, 49), (7, 35, 7))


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


def compare(entry, a, b):
    entry['persistent_over_per_step'] = entry[a]['ms_median'] / entry[b]['ms_median']
    entry['persistent_faster'] = bool(entry[a]['ms_max'] < entry[b]['ms_min'])       # every window, not just the medians


def bptt_mode(a, torch, syn, FcGruEngine, dev, sync):
    combos = [(f, b) for f in ('per_step', 'persistent') for b in ('per_step', 'persistent')]      # (forward, BPTT)
    name = lambda c: 'fwd_%s__bptt_%s' % c

    def make(B, T, GH, fwd, bptt):
        kw = {'bptt_persistent_f32' if a.dtype == 'f32' else 'bptt_persistent': True} if bptt == 'persistent' else {}
        eng = FcGruEngine(B, T, (GH, GH), dtype=a.dtype, device=dev, save_for_backward=True, **dict(kw, **{fwd: True}))
        eng.set_weights(syn.fcgru_params(0, GH, GH))
        assert eng.persistent == (fwd == 'persistent') and eng.bptt_persistent == (bptt == 'persistent')
        return eng

    def inputs(B, T, GH):
        x = torch.tensor(syn.c3d_features(1, B, T), device=dev)
        g = syn.gaze_maps(2, B, T, hw=GH)[0]
        return x, torch.tensor(g / g.reshape(B, T, -1).sum(-1)[..., None, None], device=dev).contiguous()

    def time_backward(engs, x, labels):
        """{key: windows} of backward() alone, the plans alternating; every plan has run one forward on x."""
        outs = {k: e.forward(x) for k, e in engs.items()}
        for k, e in engs.items():
            for _ in range(3):
                e.backward(outs[k][0], outs[k][1], labels)
        sync()
        ms = {k: [] for k in engs}
        for _ in range(a.windows):
            for k, e in engs.items():
                ms[k].append(window(lambda: e.backward(outs[k][0], outs[k][1], labels), a.calls, sync))
        for e in engs.values():
            e.status()
        return ms

    def ratios(entry):
        for f in ('per_step', 'persistent'):
            p, q = entry[name((f, 'persistent'))], entry[name((f, 'per_step'))]
            entry['persistent_bptt_over_per_step__fwd_' + f] = p['ms_median'] / q['ms_median']
            entry['persistent_bptt_faster__fwd_' + f] = bool(p['ms_max'] < q['ms_min'])            # every window
            entry['persistent_bptt_slower__fwd_' + f] = bool(p['ms_min'] > q['ms_max'])

    result = {'device': torch.cuda.get_device_name(0), 'calls_per_window': a.calls, 'windows': a.windows, 'dtype': a.dtype,
              'method': 'host clock around windows of calls between device synchronisations; plans alternate; median window / calls',
              'plans': [name(c) for c in combos], 'shapes': {}, 'per_step_of_T': {}}
    for B, T, GH in SHAPES:
        x, labels = inputs(B, T, GH)
        engs = {name(c): make(B, T, GH, *c) for c in combos}
        entry = {'frames': B * T, 'map': GH}
        entry['backward'] = {k: summarise(v) for k, v in time_backward(engs, x, labels).items()}
        ratios(entry['backward'])
        step = [0]

        def train(eng):
            logits, probs = eng.forward(x)
            eng.backward(logits, probs, labels)
            eng.adam_step(step[0], 1e-4)
            step[0] += 1
        for e in engs.values():
            for _ in range(3):
                train(e)
        sync()
        ms = {k: [] for k in engs}
        for _ in range(a.windows):
            for k, e in engs.items():
                ms[k].append(window(lambda: train(e), max(a.calls // 5, 1), sync))
        for e in engs.values():
            e.status()
        entry['train_step'] = {k: summarise(v) for k, v in ms.items()}
        ratios(entry['train_step'])
        result['shapes']['%dx%d' % (B, T)] = entry
        del engs
    # what one more step costs the backward: T = 16 against T = 32, 7x7 plans behind the per-step forward
    for B in (8, 64):
        med = {}
        for T in (16, 32):
            x, labels = inputs(B, T, 7)
            engs = {b: make(B, T, 7, 'per_step', b) for b in ('per_step', 'persistent')}
            med[T] = {k: summarise(v) for k, v in time_backward(engs, x, labels).items()}
            del engs
        result['per_step_of_T'][str(B)] = {
            'backward_T16': med[16], 'backward_T32': med[32],
            'us_per_step': {k: (med[32][k]['ms_median'] - med[16][k]['ms_median']) * 1e3 / 16 for k in ('per_step', 'persistent')}}
    result['default_bptt_of_eligible_plans'] = \
        'persistent' if FcGruEngine(2, 2, (7, 7), dtype=a.dtype, device=dev, save_for_backward=True).bptt_persistent else 'per_step'
    return result


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--calls', type=int, default=50, help='calls per timed window')
    ap.add_argument('--windows', type=int, default=7, help='windows per path')
    ap.add_argument('--forward-only', action='store_true')
    ap.add_argument('--train-only', action='store_true', help='the training step of per-step plans alone (build-to-build A/Bs)')
    ap.add_argument('--bptt', action='store_true', help='per-step against persistent BPTT, behind both forwards')
    ap.add_argument('--dtype', default='bf16', choices=('bf16', 'f32'), help='operand dtype of the plans')
    ap.add_argument('--per-step-only', action='store_true', help='the per-step path alone (build-to-build A/Bs)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join('profiles', ('fcgru_f32_bptt_bench.json' if a.dtype == 'f32' else 'fcgru_bptt_bench.json') if a.bptt else 'fcgru_f32_bench.json' if a.dtype == 'f32' else 'fcgru_bench.json')

    import inspect
    import torch
    from recurrent_gaze_prediction_amd import synthetic as syn
    from recurrent_gaze_prediction_amd.engine import FcGruEngine
    if not torch.cuda.is_available():
        raise SystemExit('bench_fcgru.py needs a GPU: timings taken elsewhere say nothing about it')
    dev = torch.device('cuda:0')
    sync = torch.cuda.synchronize
    has_paths = 'persistent' in inspect.signature(FcGruEngine.__init__).parameters
    paths = ('per_step', 'persistent') if has_paths and not a.train_only and not a.per_step_only else ('per_step',)
    if a.bptt:
        result = bptt_mode(a, torch, syn, FcGruEngine, dev, sync)
        text = json.dumps(result, indent=1, sort_keys=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fp:
            fp.write(text + '\n')
        print(text)
        return

    def make(B, T, GH, path, train):
        kw = {path: True} if has_paths else {}
        eng = FcGruEngine(B, T, (GH, GH), dtype=a.dtype, device=dev, save_for_backward=train, **kw)
        eng.set_weights(syn.fcgru_params(0, GH, GH))
        assert not has_paths or eng.persistent == (path == 'persistent')
        return eng

    result = {'device': torch.cuda.get_device_name(0), 'calls_per_window': a.calls, 'windows': a.windows, 'dtype': a.dtype,
              'method': 'host clock around windows of calls between device synchronisations; paths alternate; median window / calls',
              'forward_only': bool(a.forward_only), 'paths': list(paths), 'shapes': {}}
    for B, T, GH in SHAPES:
        x = torch.tensor(syn.c3d_features(1, B, T), device=dev)
        entry = {'frames': B * T, 'map': GH}
        result['shapes']['%dx%d' % (B, T)] = entry
        if not a.train_only:
            engs = {p: make(B, T, GH, p, False) for p in paths}
            for e in engs.values():
                for _ in range(3):
                    e.forward(x)
            sync()
            ms = {p: [] for p in paths}
            for _ in range(a.windows):
                for p in paths:
                    ms[p].append(window(lambda: engs[p].forward(x), a.calls, sync))
            entry['forward'] = {p: summarise(v) for p, v in ms.items()}
            if 'persistent' in paths:
                engs['persistent'].status()
                compare(entry['forward'], 'persistent', 'per_step')
            del engs
        if a.forward_only:
            continue
        g = syn.gaze_maps(2, B, T, hw=GH)[0]
        labels = torch.tensor(g / g.reshape(B, T, -1).sum(-1)[..., None, None], device=dev).contiguous()
        engs = {p: make(B, T, GH, p, True) for p in paths}
        step = [0]

        def train(eng):
            logits, probs = eng.forward(x)
            eng.backward(logits, probs, labels)
            eng.adam_step(step[0], 1e-4)
            step[0] += 1
        for e in engs.values():
            for _ in range(3):
                train(e)
        sync()
        ms = {p: [] for p in paths}
        for _ in range(a.windows):
            for p in paths:
                ms[p].append(window(lambda: train(engs[p]), max(a.calls // 5, 1), sync))
        entry['train_step'] = {p: summarise(v) for p, v in ms.items()}
        if 'persistent' in paths:
            engs['persistent'].status()
            compare(entry['train_step'], 'persistent', 'per_step')
        del engs
    if a.dtype == 'f32' and 'persistent' in paths and not a.train_only:
        # what one more step costs the forward: T = 16 against T = 32, 7x7 inference plans
        result['per_step_of_T'] = {}
        for B in (8, 64):
            med = {}
            for T in (16, 32):
                x = torch.tensor(syn.c3d_features(1, B, T), device=dev)
                engs = {p: make(B, T, 7, p, False) for p in paths}
                for e in engs.values():
                    for _ in range(3):
                        e.forward(x)
                sync()
                ms = {p: [] for p in paths}
                for _ in range(a.windows):
                    for p in paths:
                        ms[p].append(window(lambda: engs[p].forward(x), a.calls, sync))
                engs['persistent'].status()
                med[T] = {p: summarise(v) for p, v in ms.items()}
                del engs
            result['per_step_of_T'][str(B)] = {
                'forward_T16': med[16], 'forward_T32': med[32],
                'us_per_step': {p: (med[32][p]['ms_median'] - med[16][p]['ms_median']) * 1e3 / 16 for p in paths}}
    if has_paths and not a.train_only and not a.per_step_only:
        result['default_of_eligible_plans'] = 'persistent' if FcGruEngine(2, 2, (7, 7), dtype=a.dtype, device=dev).persistent else 'per_step'
    text = json.dumps(result, indent=1, sort_keys=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fp:
        fp.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
