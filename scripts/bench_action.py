#!/usr/bin/env python
"""Times the action classifier (csrc/rgp_action.hip) on one GPU: the forward and the training step at B = 10 and B = 64,
C = 1024 -- NN with and without the gaze map, SVM, the fused and the unfused plan -- next to a PyTorch eager restatement of
the same step (addmm, Adam written out) on the same device, and records beside each time the bytes the step has to move.

    python scripts/bench_action.py [--out profiles/action_bench.json] [--iters 50] [--warmup 10] [--dtype bf16]

Times are device-event times over `iters` back-to-back calls after `warmup` calls of the same shape.  The floor of a row is
its bytes over 6.29 TB/s (the measured copy rate of the chip)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from recurrent_gaze_prediction_amd import synthetic as syn          # noqa: E402
from recurrent_gaze_prediction_amd.engine import ActionEngine, action_learning_rate      # noqa: E402

COPY_RATE = 6.29e12
C = 1024
K = 49 * C


def step_bytes(B, mode, use_gazemap, dtype, fused, train):
    """Bytes the algorithm has to move through HBM: W1 in the operand dtype (+ c3d) for the forward; for the training step
    also W1 (and Adam's m, v) read and written once and the operand copy written; the unfused plan adds dW1 (written, read)
    and, with the gaze map, one more read of W1 for dx."""
    N = 256 if mode == 'NN' else 13
    es = 2 if dtype == 'bf16' else 4
    w = K * N * 4
    fwd = K * (N if mode == 'NN' else 16) * es + B * K * 4
    if not train:
        return fwd
    total = fwd + (3 if mode == 'NN' else 1) * 2 * w + K * (N if mode == 'NN' else 16) * es + B * K * 4
    if not fused:
        total += 2 * w + (w if use_gazemap else 0) + (2 * B * K * 4 if use_gazemap else 0)
    return total


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters          # microseconds


class EagerNN(object):
    """The NN step in PyTorch eager, fp32: the op sequence of action_classification.py:210-292 with its gradients and
    tf.train.AdamOptimizer written out (no autograd, no torch.optim: the same arithmetic as the library's step)."""

    def __init__(self, p, use_gazemap, dev):
        self.p = {k: torch.tensor(v, device=dev) for k, v in p.items()}
        self.m = {k: torch.zeros_like(v) for k, v in self.p.items()}
        self.v = {k: torch.zeros_like(v) for k, v in self.p.items()}
        self.use_gazemap = use_gazemap

    def forward(self, c3d, gm):
        p, B = self.p, c3d.shape[0]
        self.a = gm.reshape(B, 2401) @ p['Wg'] if self.use_gazemap else None
        self.x = (c3d * self.a[:, None, :]).reshape(B, -1) if self.use_gazemap else c3d.reshape(B, -1)
        self.h1 = torch.addmm(p['b1'], self.x, p['W1'])
        self.h2 = torch.addmm(p['b2'], self.h1, p['W2'])
        self.z = torch.addmm(p['b3'], self.h2, p['W3'])
        return torch.sigmoid(self.z)

    def step(self, c3d, gm, labels, step, lr):
        p, B = self.p, c3d.shape[0]
        y = self.forward(c3d, gm)
        g = {}
        dz = (y - labels) / (B * 13)
        g['W3'], g['b3'] = self.h2.t() @ dz, dz.sum(0)
        dh2 = dz @ p['W3'].t()
        g['W2'], g['b2'] = self.h1.t() @ dh2, dh2.sum(0)
        dh1 = dh2 @ p['W2'].t()
        g['W1'], g['b1'] = self.x.t() @ dh1, dh1.sum(0)
        if self.use_gazemap:
            dx = dh1 @ p['W1'].t()
            da = (c3d * dx.reshape(c3d.shape)).sum(1)
            g['Wg'] = gm.reshape(B, 2401).t() @ da
        t = step + 1
        lr_t = lr * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        for k in p:
            self.m[k].mul_(0.9).add_(g[k], alpha=0.1)
            self.v[k].mul_(0.999).addcmul_(g[k], g[k], value=0.001)
            p[k].addcdiv_(self.m[k], self.v[k].sqrt().add_(1e-8), value=-lr_t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'action_bench.json'))
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--dtype', default='bf16')
    ap.add_argument('--batches', default='10,64')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_action.py measures on the GPU: no HIP device visible')
    dev = torch.device('cuda:0')
    rows = []
    for B in [int(b) for b in args.batches.split(',')]:
        rs = np.random.RandomState(B)
        c3d = torch.tensor(np.maximum(rs.randn(B, C, 49), 0).astype(np.float32), device=dev)
        gm = torch.tensor(rs.rand(B, 49, 49).astype(np.float32), device=dev)
        gm /= gm.sum((1, 2), keepdim=True)
        labels = torch.tensor((rs.rand(B, 13) < 0.3).astype(np.float32), device=dev)
        for mode, use_gazemap in (('NN', True), ('NN', False), ('SVM', True)):
            p = syn.action_params(1, mode, use_gazemap, dim_feat=C)
            # (NN: the f32 plan too, the like-for-like row beside the f32 eager baseline)
            for dtype, fused in [(args.dtype, True), (args.dtype, False)] + ([('f32', True)] if mode == 'NN' and args.dtype != 'f32' else []):
                e = ActionEngine(B, C, mode, use_gazemap, dtype, save_for_backward=True, device=dev, unfused=not fused)
                e.set_weights(p)
                state = {'step': 0}

                def train():
                    e.train_step(c3d, gm, labels, state['step'], action_learning_rate(state['step']) if mode == 'NN' else 1e-6)
                    state['step'] += 1
                for what, fn in (('forward', lambda: e.forward(c3d, gm)), ('train_step', train)):
                    us = timed(fn, args.iters, args.warmup)
                    nbytes = step_bytes(B, mode, use_gazemap, dtype, fused, what == 'train_step')
                    rows.append({'impl': 'fused' if fused else 'unfused', 'mode': mode, 'use_gazemap': use_gazemap, 'batch': B,
                                 'dtype': dtype, 'what': what, 'us': round(us, 2), 'bytes': nbytes,
                                 'floor_us': round(nbytes / COPY_RATE * 1e6, 2)})
                    print(json.dumps(rows[-1]))
                del e
            if mode == 'NN':
                eager = EagerNN(p, use_gazemap, dev)
                state = {'step': 0}

                def etrain():
                    eager.step(c3d, gm, labels, state['step'], action_learning_rate(state['step']))
                    state['step'] += 1
                for what, fn in (('forward', lambda: eager.forward(c3d, gm)), ('train_step', etrain)):
                    us = timed(fn, args.iters, args.warmup)
                    rows.append({'impl': 'torch_eager_f32', 'mode': mode, 'use_gazemap': use_gazemap, 'batch': B, 'dtype': 'f32',
                                 'what': what, 'us': round(us, 2)})
                    print(json.dumps(rows[-1]))
                del eager
    out = {'device': torch.cuda.get_device_name(0), 'dim_feat': C, 'iters': args.iters, 'warmup': args.warmup,
           'copy_rate_bytes_per_s': COPY_RATE, 'rows': rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print('wrote %s' % args.out)


if __name__ == '__main__':
    main()
