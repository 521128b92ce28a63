#!/usr/bin/env python
"""Time the fc-GRU's streaming call (FcGruEngine.forward_stream) next to its plain forward, on both recurrence paths.

Shapes (B x T, map side): 64x16 (BASELINE config 2, 7x7) and 8x35 (49x49), bf16, one inference plan per shape and path
('per_step', 'persistent': csrc/fcgru_seq.hip.h).  Per plan, in one process:
  (a) forward          the zero-state call
  (b) forward_stream   with a carried state (the state of the previous call): what the seed launch (instead of two memsets),
                       the state's copy-out and the new state's allocation cost on top of (a); on the persistent path also
                       the STREAM = true instantiation, whose step 0 multiplies the seeded rows where (a) skips
The two ALTERNATE: a window is --calls calls of one between two device synchronisations (host clock), --windows windows each;
the figure is the median window divided by the calls, the spread (max - min) / median of the windows (scripts/bench_stream.py's
method).  Inputs are resident on the device.  The seed's cost is reported as the difference (b) - (a).
Writes one JSON document (--out) and prints it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((64, 16, 7), (8, 35, 49))
PATHS = ('per_step', 'persistent')


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
    ap.add_argument('--calls', type=int, default=50, help='calls per timed window')
    ap.add_argument('--windows', type=int, default=7, help='windows per call kind')
    ap.add_argument('--out', default=os.path.join('profiles', 'fcgru_stream_bench.json'))
    a = ap.parse_args()

    import torch
    from recurrent_gaze_prediction_amd import synthetic as syn
    from recurrent_gaze_prediction_amd.engine import FcGruEngine
    if not torch.cuda.is_available():
        raise SystemExit('bench_fcgru_stream.py needs a GPU: timings taken elsewhere say nothing about it')
    dev = torch.device('cuda:0')
    sync = torch.cuda.synchronize

    result = {'device': torch.cuda.get_device_name(0), 'calls_per_window': a.calls, 'windows': a.windows, 'dtype': 'bf16',
              'method': 'host clock around windows of calls between device synchronisations; forward and forward_stream alternate '
                        'on one plan; median window / calls', 'shapes': {}}
    for B, T, GH in SHAPES:
        x = torch.tensor(syn.c3d_features(1, B, T), device=dev)
        entry = {'frames': B * T, 'map': GH}
        for path in PATHS:
            eng = FcGruEngine(B, T, (GH, GH), dtype='bf16', device=dev, **{path: True})
            eng.set_weights(syn.fcgru_params(0, GH, GH))
            assert eng.persistent == (path == 'persistent')
            state = [eng.forward_stream(x)[2]]

            def stream():
                state[0] = eng.forward_stream(x, state=state[0])[2]
            for _ in range(3):
                eng.forward(x)
                stream()
            ms = {'forward': [], 'forward_stream': []}
            for _ in range(a.windows):
                ms['forward'].append(window(lambda: eng.forward(x), a.calls, sync))
                ms['forward_stream'].append(window(stream, a.calls, sync))
            eng.status()
            assert torch.isfinite(state[0]).all()
            e = {k: summarise(v) for k, v in ms.items()}
            e['stream_over_forward'] = e['forward_stream']['ms_median'] / e['forward']['ms_median']
            e['stream_minus_forward_ms'] = e['forward_stream']['ms_median'] - e['forward']['ms_median']
            e['stream_minus_forward_percent'] = 100.0 * (e['stream_over_forward'] - 1.0)
            entry[path] = e
            del eng
        result['shapes']['%dx%d' % (B, T)] = entry

    text = json.dumps(result, indent=1, sort_keys=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fp:
        fp.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
