#!/usr/bin/env python
"""Time streaming inference (engine.forward_stream, stream.predict_long_clips) next to the plain forward.

Shapes: B 64 x T 16 and B 8 x T 35, bf16 (the persistent recurrence kernels).  Per shape and family (gaze_grcn, gaze_grcn77,
gaze_lstm), on ONE plan in one process:
  (a) forward          the zero-state call
  (b) forward_stream   with a carried state (the state of the previous call; gaze_grcn: bn_phase 0) -- what the seed launch,
                       the kernel's image load and the state copy-out cost on top of (a)
The two ALTERNATE: a window is --calls calls of one between two device synchronisations (host clock), --windows windows each;
the figure is the median window divided by the calls, the spread (max - min) / median of the windows (scripts/bench_lstm.py's
method).  Both are fed the placeholder layout (fp32 [B,T,1024,7,7], resident on the device).
Then, on a gaze_grcn model per shape, end to end from host arrays (one warm-up, then --clip-runs runs, the median):
  (c) a 1024-step clip through predict_long_clip, chunked, every chunk from the zero state (the reference's evaluation)
  (d) 64 such clips through stream.predict_long_clips: B lanes, the state carried, 64 * 1024 steps
(c) and (d) include building each call's host batch and its copy to the device; (d) reports steps per second next to (c).
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
FAMILIES = ('gaze_grcn', 'gaze_grcn77', 'gaze_lstm')
CLIP_STEPS, N_CLIPS = 1024, 64


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
    ap.add_argument('--windows', type=int, default=7, help='windows per path')
    ap.add_argument('--clip-runs', type=int, default=3)
    ap.add_argument('--no-clips', action='store_true', help='skip (c) and (d)')
    ap.add_argument('--out', default=os.path.join('profiles', 'stream_bench.json'))
    a = ap.parse_args()

    import torch
    from recurrent_gaze_prediction_amd import synthetic as syn
    from recurrent_gaze_prediction_amd.engine import Grcn77Engine, GrcnEngine, LstmEngine
    if not torch.cuda.is_available():
        raise SystemExit('bench_stream.py needs a GPU: timings taken elsewhere say nothing about it')
    dev = torch.device('cuda:0')
    sync = torch.cuda.synchronize

    result = {'device': torch.cuda.get_device_name(0), 'calls_per_window': a.calls, 'windows': a.windows, 'dtype': 'bf16',
              'method': 'host clock around windows of calls between device synchronisations; forward and forward_stream alternate '
                        'on one plan; median window / calls', 'shapes': {}}
    for B, T in SHAPES:
        x = torch.tensor(syn.c3d_features(1, B, T), device=dev)
        entry = {'frames': B * T}
        for fam in FAMILIES:
            if fam == 'gaze_grcn':
                eng = GrcnEngine(B, T, dtype='bf16', device=dev)
                eng.set_weights(syn.grcn_params(0, T, random_bn=True))
            elif fam == 'gaze_grcn77':
                eng = Grcn77Engine(B, T, dtype='bf16', device=dev)
                eng.set_weights(syn.grcn77_params(0))
            else:
                eng = LstmEngine(B, T, dtype='bf16', device=dev)
                eng.set_weights(syn.lstm_params(0))
            assert eng.persistent
            state = [eng.forward_stream(x)[2]]

            def stream():
                state[0] = eng.forward_stream(x, state=state[0])[2]
            for _ in range(3):
                eng.forward(x)
                stream()
            sync()
            eng.status()
            ms = {'forward': [], 'forward_stream': []}
            for _ in range(a.windows):
                ms['forward'].append(window(lambda: eng.forward(x), a.calls, sync))
                ms['forward_stream'].append(window(stream, a.calls, sync))
            eng.status()
            assert torch.isfinite(state[0]).all()
            e = {k: summarise(v) for k, v in ms.items()}
            e['stream_over_forward'] = e['forward_stream']['ms_median'] / e['forward']['ms_median']
            e['stream_minus_forward_us'] = (e['forward_stream']['ms_median'] - e['forward']['ms_median']) * 1e3
            entry[fam] = e
            del eng
        result['shapes']['%dx%d' % (B, T)] = entry

    if not a.no_clips:
        from recurrent_gaze_prediction_amd.models.base import Session
        from recurrent_gaze_prediction_amd.models.evaluate_gaze import predict_long_clip
        from recurrent_gaze_prediction_amd.models.gaze_grcn import GazePredictionGRCN, GRUModelConfig
        from recurrent_gaze_prediction_amd.stream import predict_long_clips
        clip = syn.c3d_features(2, 1, CLIP_STEPS)[0]
        for B, T in SHAPES:
            cfg = GRUModelConfig()
            cfg.batch_size, cfg.n_lstm_steps, cfg.compute_dtype, cfg.trainable = B, T, 'bf16', False
            model = GazePredictionGRCN(Session(dev), None, cfg)
            model.load_state_dict(syn.grcn_params(0, T, random_bn=True))

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
            c_s, c_all = timed(lambda: predict_long_clip(model, clip))
            d_s, d_all = timed(lambda: predict_long_clips(model, [clip] * N_CLIPS))
            result['shapes']['%dx%d' % (B, T)]['long_clips_gaze_grcn'] = {
                'clip_steps': CLIP_STEPS,
                'c_chunked_one_clip_s': c_s, 'c_runs_s': c_all, 'c_steps_per_s': CLIP_STEPS / c_s,
                'd_streamed_64_clips_s': d_s, 'd_runs_s': d_all, 'd_steps_per_s': N_CLIPS * CLIP_STEPS / d_s,
                'note': 'end to end from host arrays: includes building every call\'s fp32 batch on the host and its copy to the device'}
            del model

    text = json.dumps(result, indent=1, sort_keys=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fp:
        fp.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
