#!/usr/bin/env python
"""Time the ShallowNet pre-training step (SaliencyModel) with its two feeds, the batch kernel alone, and evaluate().

Workload: an image set of --samples synthetic samples (uint8 images 98 x 98 x 3, maps 49 x 49), batch --batch, the
reference's configuration (keep 0.4, l2_reg 1e-7, Adam, clip 10), per operand dtype (bf16, f32).

  host_feed    what a port without the new entries does: numpy gather of the float32 arrays and flip of half the batch on
               the host, upload, forward, the loss and its gradient as torch element-wise ops, engine.backward, the
               regulariser as torch ops on the flat buffers, clip_step_multi
  device_feed  rgp_salicon_batch from the resident uint8 set, forward, rgp_euclid_loss_fwd_bwd, engine.backward,
               rgp_l2_reg, clip_step_multi
Both run on ONE engine (same plan, same weights, dropout drawn per step), alternating step by step in one process after
--warmup steps of each; a step is timed on the host clock from before the feed to after a device synchronise.  Reported:
median, min, max and the 10th / 90th percentiles of --steps steps each.

  batch_kernel rgp_salicon_batch alone (events around the C call into preallocated outputs, and around the whole Python
               call) against a device-to-device copy of as many bytes as it writes, alternating in the same run, with
               the bytes it reads and writes
  evaluate     images per second of SaliencyModel.evaluate(scorer='device') and, on fewer images, scorer='host'

Writes one JSON document (--out) and prints it.  No GPU: the script stops."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def spread(ms):
    ms = np.asarray(ms, np.float64)
    return {'ms_median': float(np.median(ms)), 'ms_min': float(ms.min()), 'ms_max': float(ms.max()),
            'ms_p10': float(np.percentile(ms, 10)), 'ms_p90': float(np.percentile(ms, 90)), 'steps': int(ms.size)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--samples', type=int, default=4096)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--hw', type=int, default=98)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--eval-images', type=int, default=1024)
    ap.add_argument('--eval-host-images', type=int, default=128)
    ap.add_argument('--dtypes', nargs='*', default=['bf16', 'f32'])
    ap.add_argument('--out', default=os.path.join('profiles', 'salicon_bench.json'))
    a = ap.parse_args()

    import scipy.sparse
    import torch
    from recurrent_gaze_prediction_amd import _lib
    from recurrent_gaze_prediction_amd import salicon_input_data as sid
    from recurrent_gaze_prediction_amd.engine import (ShallowNetEngine, SaliconBatcher, clip_step_multi, euclid_loss_fwd_bwd,
                                                      l2_reg)
    from recurrent_gaze_prediction_amd import synthetic as syn
    if not torch.cuda.is_available():
        raise SystemExit('bench_salicon.py needs a GPU: timings taken elsewhere say nothing about it')
    dev = torch.device('cuda:0')
    N, B, hw = a.samples, a.batch, a.hw
    rs = np.random.RandomState(0)
    images_u8 = rs.randint(0, 256, size=(N, hw, hw, 3)).astype(np.uint8)
    maps_u8 = rs.randint(0, 64, size=(N, 49, 49)).astype(np.uint8)
    fix = np.empty(N, dtype=object)
    for i in range(N):
        dense = np.zeros((60, 80), np.float32)
        dense[rs.randint(0, 60, 12), rs.randint(0, 80, 12)] = 1.0
        fix[i] = scipy.sparse.csr_matrix(dense)
    images_f, maps_f = np.multiply(images_u8.astype(np.float32), 1.0 / 255.0), np.multiply(maps_u8.astype(np.float32), 1.0 / 255.0)
    host_set = sid.SaliconDataset(images_f, maps_f, fix)
    dev_set = sid.SaliconDataset(images_f, maps_f, fix).to_device(dev, images_u8, maps_u8)
    result = {'samples': N, 'batch': B, 'image_hw': hw, 'warmup': a.warmup, 'device_name': torch.cuda.get_device_name(0),
              'threads': torch.get_num_threads(), 'keep_prob': 0.4, 'l2_reg': 1e-7, 'train_step': {}}
    coeff, lr, scale = 1e-7, 3e-5, 2.0 / (2401.0 * B)
    flip_rng = np.random.RandomState(1)

    def flips():
        f = np.zeros(B, np.uint8)
        f[flip_rng.choice(B, B // 2, replace=False)] = 1
        return f

    for dtype in a.dtypes:
        eng = ShallowNetEngine(B, hw, dtype=dtype, device=dev, save_for_backward=True, dropout=True)
        eng.set_weights(syn.shallownet_params(0, hw))
        eng.dropout.configure(0.4, seed=7)
        step = [0]

        def host_feed_step():
            images, maps = host_set.next_batch(B)[:2]
            images, maps = np.array(images), np.array(maps)
            sel = np.flatnonzero(flips())
            images[sel] = images[sel][:, :, ::-1, :]
            maps[sel] = maps[sel][:, :, ::-1]
            x, y = torch.from_numpy(images).to(dev), torch.from_numpy(maps).to(dev)
            sal, _ = eng.forward(x, train=True)
            diff = sal - y
            target = (diff * diff).sum() * (0.5 * scale)
            eng.backward((diff * scale).contiguous())
            reg = (eng.flat_params * eng.flat_params).sum() * (0.5 * coeff)
            eng.flat_grads.add_(eng.flat_params, alpha=coeff)
            clip_step_multi([eng], step[0], lr, 10.0, 'adam')
            step[0] += 1
            return target, reg

        def device_feed_step():
            x, y, _ = dev_set.next_batch_device(B, flips())
            sal, _ = eng.forward(x, train=True)
            target, d = euclid_loss_fwd_bwd(sal, y, B)
            eng.backward(d)
            reg = l2_reg(eng.flat_params, eng.flat_grads, coeff)
            clip_step_multi([eng], step[0], lr, 10.0, 'adam')
            step[0] += 1
            return target, reg

        times = {'host_feed': [], 'device_feed': []}
        last = {}
        for i in range(a.warmup + a.steps):
            for name, fn in (('host_feed', host_feed_step), ('device_feed', device_feed_step)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                target, reg = fn()
                torch.cuda.synchronize()
                if i >= a.warmup:
                    times[name].append((time.perf_counter() - t0) * 1e3)
                last[name] = (float(target.item()), float(reg.item()))
        r = {k: spread(v) for k, v in times.items()}
        r['device_over_host_median'] = r['device_feed']['ms_median'] / r['host_feed']['ms_median']
        r['last_losses'] = {k: {'target': v[0], 'reg': v[1]} for k, v in last.items()}
        result['train_step'][dtype] = r
        del eng
        torch.cuda.empty_cache()

    # ---- the batch kernel alone against a copy of its output bytes
    batcher = SaliconBatcher(dev_set.images_u8, dev_set.maps_u8)
    index = torch.from_numpy(np.asarray(dev_set.batch_perm[:B], np.int32)).to(dev)
    flip = torch.from_numpy(flips()).to(dev)
    out_bytes = B * (hw * hw * 3 + 2401) * 4
    src = torch.empty(out_bytes // 4, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    out_i = torch.empty(B, hw, hw, 3, dtype=torch.float32, device=dev)
    out_m = torch.empty(B, 49, 49, dtype=torch.float32, device=dev)
    args = _lib.SaliconBatchArgs(images_u8=dev_set.images_u8.data_ptr(), maps_u8=dev_set.maps_u8.data_ptr(), n=N, h=hw, w=hw, map_h=49,
                                 map_w=49, index=index.data_ptr(), flip=flip.data_ptr(), batch=B, images=out_i.data_ptr(),
                                 maps=out_m.data_ptr(), workspace=batcher.workspace.data_ptr(),
                                 workspace_bytes=batcher.workspace.numel())
    stream = torch.cuda.current_stream(dev).cuda_stream
    lib = _lib.load()
    runs = {'c_call': lambda: _lib.check(lib.rgp_salicon_batch(ctypes.byref(args), stream)),
            'python_call': lambda: batcher.batch(index, flip, check=False), 'copy_of_output_bytes': lambda: dst.copy_(src)}
    ms = {k: [] for k in runs}
    for i in range(a.warmup + a.steps):
        for which, fn in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                ms[which].append(e0.elapsed_time(e1))
    batcher.status()
    want = batcher.batch(index, flip)
    moved = B * (hw * hw * 3 + 2401) + 5 * B + out_bytes
    result['batch_kernel'] = {k: spread(v) for k, v in ms.items()}
    result['batch_kernel'].update({
        'bytes_read': B * (hw * hw * 3 + 2401) + 5 * B, 'bytes_written': out_bytes,
        'c_call_bytes_per_s': moved / (result['batch_kernel']['c_call']['ms_median'] * 1e-3),
        'c_call_equals_python_call': bool(torch.equal(out_i, want[0]) and torch.equal(out_m, want[1])),
        'note': 'events around the C call (the 8-byte memset of the status word and the launch) into preallocated outputs / around '
                'the whole Python call (two output allocations, index and flip conversion, the C call) / around dst.copy_(src)'})

    # ---- evaluate
    from recurrent_gaze_prediction_amd.models.base import Session
    from recurrent_gaze_prediction_amd.models.saliency_shallownet import SaliencyModel, SaliencyModelConfig
    import tempfile
    cfg = SaliencyModelConfig()
    cfg.batch_size, cfg.image_hw, cfg.train_dir, cfg.trainable = B, hw, tempfile.mkdtemp(prefix='bench-salicon-'), False
    model = SaliencyModel(Session(dev), None, cfg)
    ev = {}
    for scorer, n in (('device', a.eval_images), ('host', a.eval_host_images)):
        n = min(n, N) // B * B
        if n == 0:
            continue
        sub = sid.SaliconDataset(images_f[:n], maps_f[:n], fix[:n])
        if scorer == 'device':
            model.evaluate(sid.SaliconDataset(images_f[:B], maps_f[:B], fix[:B]), scorer=scorer)      # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        scores = model.evaluate(sub, scorer=scorer)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        ev[scorer] = {'images': n, 'seconds': dt, 'images_per_s': n / dt, 'scores': {k: float(v) for k, v in scores.items()}}
    result['evaluate'] = ev

    text = json.dumps(result, indent=1, sort_keys=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fp:
        fp.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
