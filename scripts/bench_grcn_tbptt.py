#!/usr/bin/env python
"""Time gaze_grcn's streaming backward (GrcnEngine.backward_stream) next to its plain backward.

Shapes (B x T): 8x35 (BASELINE config 4 per GPU) and 64x16 (bench.py's default); one training plan per shape and path: bf16 with
the persistent recurrence and BPTT kernels (csrc/convgru_seq.hip.h, csrc/convgru_bptt.hip.h) and f32 with per-step launches.
Per plan, in one process:
  (a) step / step_stream     forward + backward against forward_stream(state) + backward_stream(d_state, d_state_in wanted): what
                             the seed, the way out and -- persistent plans -- the STREAM = true instantiations add to a step
  (b) tail_T / tail_1        backward_stream alone behind a forward_stream with n_valid = T and with n_valid = 1 (a film's one-
                             step tail): the steps behind n_valid are skipped, their rows zeroed
  (c) film / plain_steps     an 'exact' film of 4 T + 1 steps (five forward_stream calls, then five recomputations with
                             backward_stream and the gradient sum) against the same frames as five unrelated forward + backward
Each pair ALTERNATES: a window is --calls calls of one between two device synchronisations (host clock), --windows windows
each; the figure is the median window divided by the calls, the spread (max - min) / median of the windows
(scripts/bench_fcgru_tbptt.py's method).  Inputs are resident on the device.
Writes one JSON document (--out) and prints it.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts.bench_fcgru_tbptt import pair                      # noqa: E402

SHAPES = ((8, 35), (64, 16))
PLANS = (('bf16', 'persistent', {}), ('f32', 'per_step', {}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--calls', type=int, default=20, help='calls per timed window')
    ap.add_argument('--windows', type=int, default=5, help='windows per call kind')
    ap.add_argument('--out', default=os.path.join('profiles', 'grcn_tbptt_bench.json'))
    a = ap.parse_args()

    import torch
    from recurrent_gaze_prediction_amd import synthetic as syn
    from recurrent_gaze_prediction_amd.engine import GrcnEngine
    if not torch.cuda.is_available():
        raise SystemExit('bench_grcn_tbptt.py needs a GPU: timings taken elsewhere say nothing about it')
    dev = torch.device('cuda:0')
    sync = torch.cuda.synchronize

    result = {'device': torch.cuda.get_device_name(0), 'calls_per_window': a.calls, 'windows': a.windows,
              'method': 'host clock around windows of calls between device synchronisations; the two call kinds of a pair alternate '
                        'on one plan; median window / calls', 'shapes': {}}
    for B, T in SHAPES:
        x = torch.tensor(syn.c3d_features(1, B, T), device=dev)
        g = torch.rand(B, T, 49, 49, device=dev)
        g /= g.sum((2, 3), keepdim=True)
        entry = {'frames': B * T}
        for dtype, path, kw in PLANS:
            eng = GrcnEngine(B, T, dtype=dtype, device=dev, save_for_backward=True, **kw)
            eng.set_weights(syn.grcn_params(0, T, gru_std=0.05, random_bn=True))
            assert eng.persistent == (path == 'persistent')
            e = {}
            state = [eng.forward_stream(x)[2]]
            d_state = [torch.zeros(B, 7, 7, 128, device=dev)]

            def step():
                z, p = eng.forward(x)
                eng.backward(z, p, g)

            def step_stream():
                z, p, state[0] = eng.forward_stream(x, state=state[0])
                d_state[0] = eng.backward_stream(z, p, g, d_state=d_state[0])[1]
            pair(e, 'step', step, 'step_stream', step_stream, a.calls, a.windows, sync)

            held = {}

            def tail(n):
                if held.get('n') != n:                      # (the forward of the window's first call; the others differentiate it again)
                    held['n'], (held['z'], held['p'], _) = n, eng.forward_stream(x, state=state[0], n_valid=n)
                eng.backward_stream(held['z'], held['p'], g, d_state=None, loss_frames=B * n, want_d_state=False)
            pair(e, 'tail_T', lambda: tail(T), 'tail_1', lambda: tail(1), a.calls, a.windows, sync)

            def film():
                states = [None]
                for _ in range(5):
                    states.append(eng.forward_stream(x, state=states[-1], n_valid=T if len(states) < 5 else 1, want_probs=False)[2])
                acc, d = None, None
                for i in reversed(range(5)):
                    z, p, _ = eng.forward_stream(x, state=states[i], n_valid=T if i < 4 else 1)
                    d = eng.backward_stream(z, p, g, d_state=d, loss_frames=B * (4 * T + 1), want_d_state=i > 0)[1]
                    acc = eng.flat_grads.clone() if acc is None else acc.add_(eng.flat_grads)

            def plain_steps():
                for _ in range(5):
                    step()
            pair(e, 'plain_steps', plain_steps, 'film', film, max(1, a.calls // 5), a.windows, sync)
            eng.status()
            assert torch.isfinite(eng.flat_grads).all() and torch.isfinite(d_state[0]).all()
            entry['%s-%s' % (dtype, path)] = e
            del eng
        result['shapes']['%dx%d' % (B, T)] = entry

    text = json.dumps(result, indent=1, sort_keys=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fp:
        fp.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
