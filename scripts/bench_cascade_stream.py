#!/usr/bin/env python
"""Time the cascade's streaming call (CascadeEngine.forward_stream) next to its plain forward.

Shapes: B 16 x T 35 and B 5 x T 35, bf16, one inference plan each (the shapes of scripts/time_cascade.py).  Per shape, on ONE
plan in one process:
  (a) forward          the zero-state call
  (b) forward_stream   with a carried state (the state of the previous call) -- what the top seed launch, the bottom seed
                       launch, the two state copy-outs and the new state's allocation cost on top of (a)
The two ALTERNATE: a window is --calls calls of one between two device synchronisations (host clock), --windows windows each;
the figure is the median window divided by the calls, the spread (max - min) / median of the windows (scripts/bench_stream.py's
method).  Inputs are resident on the device.
Then, on a cascade model per shape, end to end from host arrays (one warm-up, then --clip-runs runs, the median):
  (c) a 1024-step clip through predict_long_clip, chunked: every chunk from the zero state, B chunks per call
  (d) the same clip with carry_state=True: one recurrence, T steps per call in lane 0 (the other lanes idle)
(c) and (d) include building each call's host batch, frames included, and its copy to the device.
--forward-only: (a) alone, and nothing that needs the streaming symbols -- the same script then runs on a build without them
(one process per figure when two builds are compared).
Writes one JSON document (--out) and prints it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((16, 35), (5, 35))
CLIP_STEPS = 1024


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
    ap.add_argument('--calls', type=int, default=20, help='calls per timed window')
    ap.add_argument('--windows', type=int, default=7, help='windows per path')
    ap.add_argument('--clip-runs', type=int, default=3)
    ap.add_argument('--no-clips', action='store_true', help='skip (c) and (d)')
    ap.add_argument('--forward-only', action='store_true', help='(a) alone: needs no streaming symbol')
    ap.add_argument('--out', default=os.path.join('profiles', 'cascade_stream_bench.json'))
    a = ap.parse_args()

    import torch
    from recurrent_gaze_prediction_amd import synthetic as syn
    from recurrent_gaze_prediction_amd.engine import CascadeEngine
    if not torch.cuda.is_available():
        raise SystemExit('bench_cascade_stream.py needs a GPU: timings taken elsewhere say nothing about it')
    dev = torch.device('cuda:0')
    sync = torch.cuda.synchronize

    result = {'device': torch.cuda.get_device_name(0), 'calls_per_window': a.calls, 'windows': a.windows, 'dtype': 'bf16',
              'forward_only': bool(a.forward_only),
              'method': 'host clock around windows of calls between device synchronisations; forward and forward_stream alternate '
                        'on one plan; median window / calls', 'shapes': {}}
    params = syn.cascade_params(0)
    for B, T in SHAPES:
        eng = CascadeEngine(B, T, 98, dtype='bf16', device=dev)
        eng.set_weights(params)
        frames = torch.rand(B, T, 98, 98, 3, device=dev)
        x = torch.tensor(syn.c3d_features(1, B, T), device=dev)
        entry = {'frames': B * T}
        ms = {'forward': []}
        if a.forward_only:
            for _ in range(3):
                eng.forward(frames, x)
            for _ in range(a.windows):
                ms['forward'].append(window(lambda: eng.forward(frames, x), a.calls, sync))
        else:
            state = [eng.forward_stream(frames, x)[1]]

            def stream():
                state[0] = eng.forward_stream(frames, x, state=state[0])[1]
            for _ in range(3):
                eng.forward(frames, x)
                stream()
            ms['forward_stream'] = []
            for _ in range(a.windows):
                ms['forward'].append(window(lambda: eng.forward(frames, x), a.calls, sync))
                ms['forward_stream'].append(window(stream, a.calls, sync))
            assert torch.isfinite(state[0]).all()
        e = {k: summarise(v) for k, v in ms.items()}
        if not a.forward_only:
            e['stream_over_forward'] = e['forward_stream']['ms_median'] / e['forward']['ms_median']
            e['stream_minus_forward_ms'] = e['forward_stream']['ms_median'] - e['forward']['ms_median']
            e['stream_minus_forward_percent'] = 100.0 * (e['stream_over_forward'] - 1.0)
        entry['engine'] = e
        result['shapes']['%dx%d' % (B, T)] = entry
        del eng

    if not a.no_clips and not a.forward_only:
        from recurrent_gaze_prediction_amd.models.base import Session
        from recurrent_gaze_prediction_amd.models.evaluate_gaze import predict_long_clip
        from recurrent_gaze_prediction_amd.models.gaze_grcn_cascade import GazePredictionGRCN, GRUModelConfig
        clip = syn.c3d_features(2, 1, CLIP_STEPS)[0]
        clip_frames = np.random.RandomState(3).rand(CLIP_STEPS, 98, 98, 3).astype(np.float32)
        for B, T in SHAPES:
            cfg = GRUModelConfig()
            cfg.batch_size, cfg.n_lstm_steps, cfg.compute_dtype, cfg.trainable = B, T, 'bf16', False
            model = GazePredictionGRCN(Session(dev), None, cfg)
            # (the chunked path hands the same [B,T,hw,hw,3] images to every call: same work, one host array)
            call_frames = np.ascontiguousarray(clip_frames[:B * T].reshape(B, T, 98, 98, 3))

            def timed(fn):
                fn()
                ts = []
                for _ in range(a.clip_runs):
                    sync()
                    t0 = time.perf_counter()
                    fn()
                    sync()
                    ts.append(time.perf_counter() - t0)
                return float(np.median(ts)), [float(t) for t in ts]
            c_s, c_all = timed(lambda: predict_long_clip(model, clip, frames=call_frames))
            d_s, d_all = timed(lambda: predict_long_clip(model, clip, frames=clip_frames, carry_state=True))
            result['shapes']['%dx%d' % (B, T)]['long_clip'] = {
                'clip_steps': CLIP_STEPS,
                'c_chunked_s': c_s, 'c_runs_s': c_all, 'c_steps_per_s': CLIP_STEPS / c_s, 'c_calls': -(-(-(-CLIP_STEPS // T)) // B),
                'd_carried_s': d_s, 'd_runs_s': d_all, 'd_steps_per_s': CLIP_STEPS / d_s, 'd_calls': -(-CLIP_STEPS // T),
                'note': 'end to end from host arrays: includes building every call\'s fp32 batch (features and frames) on the host and '
                        'its copy to the device; the carried clip occupies one of the B lanes, the chunked one all of them'}
            del model

    text = json.dumps(result, indent=1, sort_keys=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fp:
        fp.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
