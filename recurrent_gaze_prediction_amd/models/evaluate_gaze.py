"""Mirror of /root/reference/models/evaluate_gaze.py: per-frame scoring of a
model's generate() output, per-frame dumps and ``overall.txt``; plus the long-clip inference of
models/extract_map.py:148-229.  The two ``pdb.set_trace()`` calls of the reference (:100, :189)
are not reproduced.  The frames are scored by the host module or, on request, on the GPU -- at the maps' own shape or
at the fixation maps' (frame resolution, the reference's setting) with the spline resize fused into the kernel."""
import logging
import os
from collections import OrderedDict, defaultdict

import numpy as np
import scipy.sparse
import torch

from ..evaluation_metrics import resize_onehot_tensor_sparse, saliency_score_single

log = logging.getLogger('rgp')
FRAME_METRICS = ('sim', 'cc', 'AUC_Borji', 'AUC_Judd', 'AUC_shuffled')       # evaluate_gaze.py:135
DUMP_SCALES = ('minmax', 'bytescale')


def _dense(m):
    return m.toarray() if scipy.sparse.issparse(m) else np.asarray(m)


def _write_frame(i, n_images, image, pred_gazemap, gt_gazemap, scores, out_dir, dump_images, dump_scale='minmax',
                 pred_bytes=None):
    """evaluate_gaze.py:137-158: the per-frame dumps.  ``dump_scale='minmax'`` (default) scales in float64 and truncates
    a * 255; ``'bytescale'`` writes the bytes scipy.misc.imsave encodes (models/extract_map.py: ``bytescale``, which
    rounds).  ``pred_bytes``: the predicted map's bytes where the caller has them already (``bytescale_maps``)."""
    if dump_scale not in DUMP_SCALES:
        raise ValueError('dump_scale must be one of %s, got %r' % (DUMP_SCALES, dump_scale))
    if dump_images:
        try:
            from PIL import Image

            def save(name, arr, ready=None):
                if dump_scale == 'bytescale':
                    from .extract_map import bytescale
                    u8 = np.asarray(ready, np.uint8) if ready is not None else bytescale(np.asarray(arr, np.float32))
                    Image.fromarray(u8).save(os.path.join(out_dir, name))
                    return
                a = np.asarray(arr, np.float64)
                a = (a - a.min()) / max(a.max() - a.min(), 1e-12)
                Image.fromarray((a * 255).astype(np.uint8)).save(os.path.join(out_dir, name))
            save('%05d.frame.jpg' % i, image)
            save('%05d.gaze_pred.jpg' % i, pred_gazemap, pred_bytes)
            save('%05d.gaze_gt.jpg' % i, gt_gazemap)
        except ImportError:
            pass
    with open(os.path.join(out_dir, '%05d.scores.txt' % i), 'w') as fp:
        fp.write('%d / %d\n' % (i, n_images))
        for k, v in scores.items():
            fp.write('%s : %.4f\n' % (k, v))


def handle_frame(i, n_images, image, pred_gazemap, gt_gazemap, fixationmap, out_dir, fixationmaps_all, rng,
                 dump_images=True, dump_scale='minmax'):
    """evaluate_gaze.py:116-158: union of 10 random other fixation maps, 5 metrics, dumps."""
    fixationmap = _dense(fixationmap)
    other_map_union = np.zeros(fixationmap.shape, np.uint8)
    for oth in rng.choice(range(len(fixationmaps_all)), 10, replace=False):
        other_map = _dense(fixationmaps_all[oth])
        if other_map.shape != fixationmap.shape:
            other_map = resize_onehot_tensor_sparse(other_map, fixationmap.shape)
        other_map_union += (other_map > 0).astype(np.uint8)
    scores = OrderedDict()
    for metric in FRAME_METRICS:
        scores[metric] = saliency_score_single(metric, pred_map=pred_gazemap, gt_map=gt_gazemap,
                                               fixation_map=fixationmap, other_map_union=other_map_union)
    if out_dir is not None:
        _write_frame(i, n_images, image, pred_gazemap, gt_gazemap, scores, out_dir, dump_images, dump_scale)
    return scores


def _device_frame_scores(pred, gt, fix, rng, scorer, seed):
    """All frames in one launch of the HIP metrics kernels (evaluation_metrics_gpu): per frame the union of 10 random
    other fixation maps drawn from ``rng`` as handle_frame draws them, then the five FRAME_METRICS.  'device-reference'
    feeds the kernel the draws the host loop would take from numpy's global RNG (frame after frame, FRAME_METRICS
    order); 'device' lets the kernel draw from ``seed``.  Fixation maps of the maps' shape go to the equal-shape kernel;
    of another shape -- the reference's evaluation, fixations at frame resolution, usually sparse -- to the kernel that
    resizes on the fly, as point lists: no dense [N,H,W] array is built."""
    from .. import evaluation_metrics_gpu as emg
    shape = emg._maps_shape(fix)
    if shape != tuple(pred.shape[1:]):
        ptr, idx = emg.pack_points(fix, shape)
        points = [idx[a:b] for a, b in zip(ptr[:-1], ptr[1:])]
        unions = [emg.union_of_ten_points(points, rng) for _ in range(len(points))]
        other_ptr = np.zeros(len(unions) + 1, np.int64)
        other_ptr[1:] = np.cumsum([len(u) for u in unions])
        other = (other_ptr.astype(np.int32), np.concatenate(unions).astype(np.int32))
        draws = 'device'
        if scorer == 'device-reference':
            draws = emg.draw_reference_samples_points((ptr, idx), other, shape, FRAME_METRICS, order='frame')
        return emg.saliency_scores_resized(pred, gt, (ptr, idx), other, FRAME_METRICS, draws=draws, seed=seed, shape=shape)
    fix = np.asarray(emg.stack_maps(fix, 'fixationmap_list'))
    positive = (fix > 0).astype(np.uint8)
    unions = np.stack([positive[rng.choice(range(len(fix)), 10, replace=False)].sum(0, dtype=np.uint8) for _ in range(len(fix))])
    draws = 'device'
    if scorer == 'device-reference':
        draws = emg.draw_reference_samples(fix, unions, FRAME_METRICS, order='frame')
    return emg.saliency_scores_single(pred, gt, fix, unions, FRAME_METRICS, draws=draws, seed=seed)


def _write_overlays(images, pred, gt, out_dir, device, alpha=0.4, colormap='jet'):
    """%05d.overlay_pred.jpg and %05d.overlay_gt.jpg: every frame's maps drawn over it (overlay.overlay_maps, one call for
    all predictions and one for all ground-truth maps).  The loader's float images go back to bytes with rint(img * 255)."""
    from PIL import Image
    from ..overlay import overlay_maps
    frames = np.stack([np.asarray(im) for im in images])
    if frames.dtype != np.uint8:
        frames = np.rint(frames.astype(np.float32) * np.float32(255.0)).clip(0, 255).astype(np.uint8)
    for name, maps in (('overlay_pred', pred), ('overlay_gt', gt)):
        drawn = overlay_maps(frames, np.ascontiguousarray(maps, np.float32), alpha=alpha, colormap=colormap, device=device).cpu().numpy()
        for i in range(len(drawn)):
            Image.fromarray(drawn[i]).save(os.path.join(out_dir, '%05d.%s.jpg' % (i, name)))


def run_evaluation(model, data_sets, out_dir, num_frames=1000, seed=0, dump_images=False, scorer='host', dump_scale='minmax',
                   dump_overlays=False):
    """evaluate_gaze.py:172-227 -> {metric: mean}; writes <out_dir>/overall.txt in the reference's format.

    ``scorer``: 'host' (default) scores frame by frame with evaluation_metrics; 'device-reference' and 'device' score all
    frames in one launch on the GPU (see _device_frame_scores), the former with the host's own draws -- same numbers, same
    files -- the latter with draws made on the device from ``seed``.  Fixation maps of the maps' shape or, as in the reference's
    evaluation, of the video frame's (dense or scipy.sparse; the maps are then upsized on the device, inside the scoring
    kernel) are both scored on the device; frames of different shapes are the host scorer's.

    ``dump_scale``: how the per-frame images are scaled to 8 bits (``dump_images=True``): 'minmax' (default), or
    'bytescale', the bytes the reference's scipy.misc.imsave encodes; with the device scorers the predicted maps' bytes
    then come from one ``extract_map.bytescale_maps`` launch for all frames.

    ``dump_overlays=True`` also writes ``%05d.overlay_pred.jpg`` and ``%05d.overlay_gt.jpg`` beside the dumps: the maps drawn
    over their frames on the device (overlay.overlay_maps; jet, alpha 0.4).  The default writes exactly the files above."""
    assert out_dir is not None
    if dump_scale not in DUMP_SCALES:
        raise ValueError('dump_scale must be one of %s, got %r' % (DUMP_SCALES, dump_scale))
    if scorer not in ('host', 'device', 'device-reference'):
        raise ValueError("scorer must be 'host', 'device' or 'device-reference', got %r" % (scorer,))
    os.makedirs(out_dir, exist_ok=True)
    T = model.n_lstm_steps
    ret = model.generate(data_sets.valid, max_instances=int(np.divide(num_frames, T, dtype=float) + 1))
    pred, gt = np.asarray(ret['pred_gazemap_list']), np.asarray(ret['gt_gazemap_list'])
    images, fix = ret['images_list'], ret['fixationmap_list']
    n_images = len(pred)
    assert n_images == len(gt) == len(images) == len(fix)
    rng = np.random.RandomState(seed)
    state = np.random.get_state()
    np.random.seed(seed)                       # AUC_Judd / AUC_Borji draw from the global RNG (9-Q11)
    try:
        aggregated = defaultdict(list)
        if scorer == 'host':
            for i in range(n_images):
                scores = handle_frame(i, n_images, images[i], pred[i], gt[i], fix[i], out_dir, fix, rng, dump_images, dump_scale)
                for metric, score in scores.items():
                    aggregated[metric].append(score)
        else:
            per_frame = _device_frame_scores(pred, gt, fix, rng, scorer, seed)
            for metric in FRAME_METRICS:
                aggregated[metric] = [float(v) for v in per_frame[metric]]
            pred_bytes = None
            if dump_images and dump_scale == 'bytescale' and n_images:
                from .extract_map import bytescale_maps
                pred_bytes = bytescale_maps(np.ascontiguousarray(pred, np.float32), device=model.session.device)
            for i in range(n_images):
                scores = OrderedDict((metric, aggregated[metric][i]) for metric in FRAME_METRICS)
                _write_frame(i, n_images, images[i], pred[i], gt[i], scores, out_dir, dump_images, dump_scale,
                             None if pred_bytes is None else pred_bytes[i])
    finally:
        np.random.set_state(state)
    if dump_overlays and n_images:
        _write_overlays(images, pred, gt, out_dir, model.session.device)
    overall = OrderedDict()
    with open(os.path.join(out_dir, 'overall.txt'), 'w') as fp:
        for metric, score_list in aggregated.items():
            overall[metric] = float(np.mean(score_list))
            fp.write("Average %s : %.4f\n" % (metric, overall[metric]))
            fp.write(''.join('%.3f ' % s for s in score_list) + '\n')
    return overall


def predict_long_clip(model, c3d, frames=None, pool_to_7x7=False, carry_state=False):
    """extract_map.py:148-229: a clip of any length through a fixed-T model.  c3d [N,1024,7,7]
    (or [N,512,2,7,7]) is cut into T-chunks, the tail zero-padded, B chunks per call; returns
    [N,GH,GW] of the model (49x49; 7x7 for gaze_grcn77 / gaze_rnn77), or [N,7,7] with a 7x7 average re-pool of each 49x49 map
    (a 7x7 model's maps are at that resolution already).  pool_to_7x7='imresize' returns instead what the reference's export
    writes to <clip>.gazemap.npy: extract_map.avg_pool of every map (scipy's imresize to 7x7 over its sum, float64, NaN
    where the resized bytes sum to 0), made on the device from the maps predict() left there.
    carry_state=False is the reference's evaluation: every chunk starts from the zero state (extract_map.py:65).
    carry_state=True runs the clip as ONE recurrence (stream.predict_long_clips; every recurrent model of the family, the
    fc-GRU models gaze_rnn / gaze_rnn77 included; gaze_c3d_conv has no state and refuses).
    frames means a different array on the two branches, and only the cascade reads it (every other model ignores it on both):
      carry_state=False  one batch [B,T,hw,hw,3], handed to every predict() call as it is (the chunks' own images are not cut
                         out of a clip here);
      carry_state=True   the clip's images [N,hw,hw,3], one per step, cut, padded and trimmed beside the features; for the
                         cascade any other shape is a ValueError."""
    if isinstance(pool_to_7x7, str) and pool_to_7x7 != 'imresize':
        raise ValueError("pool_to_7x7 must be False, True or 'imresize', got %r" % (pool_to_7x7,))
    imresize = isinstance(pool_to_7x7, str)
    c3d = np.asarray(c3d, np.float32).reshape(len(c3d), 1024, 7, 7)
    n, T, B = len(c3d), model.n_lstm_steps, model.batch_size
    if carry_state:
        from ..stream import predict_long_clips
        if frames is not None and getattr(model, 'NEEDS_FRAMES', False):
            shape = tuple(frames.shape) if hasattr(frames, 'shape') else np.shape(frames)
            if len(shape) != 4 or shape[0] != n:
                raise ValueError('predict_long_clip(carry_state=True): frames must be the clip\'s images [N = %d, hw, hw, 3], one per '
                                 'step, got %s (the [B,T,hw,hw,3] batch belongs to carry_state=False)' % (n, shape))
        maps = predict_long_clips(model, [c3d], frames=None if frames is None else [frames])[0]
        if imresize:
            from .extract_map import avg_pool
            return avg_pool(np.ascontiguousarray(maps, np.float32), device=model.session.device)
        if pool_to_7x7 and maps.shape[-1] == 49:
            maps = maps.reshape(n, 7, 7, 7, 7).mean(axis=(2, 4))
        return maps
    n_chunks = -(-n // T)
    padded = np.zeros((n_chunks * T, 1024, 7, 7), np.float32)
    padded[:n] = c3d
    chunks = padded.reshape(n_chunks, T, 1024, 7, 7)
    outs = []
    for i in range(0, n_chunks, B):
        batch = chunks[i:i + B]
        if len(batch) < B:
            batch = np.concatenate([batch, np.zeros((B - len(batch),) + batch.shape[1:], np.float32)])
        maps = model.predict(batch, frames)
        if imresize:
            from .extract_map import avg_pool
            k = min(B, n_chunks - i) * T
            pooled = avg_pool(maps.reshape((B * T,) + tuple(maps.shape[-2:]))[:k].to(torch.float32).contiguous())
            outs.append(pooled.cpu().numpy() if torch.is_tensor(pooled) else pooled)
            continue
        maps = maps.cpu().numpy()
        outs.append(maps[:min(B, n_chunks - i)])
    if imresize:
        return np.concatenate(outs)[:n]
    maps = np.concatenate(outs).reshape(n_chunks * T, model.gazemap_height, model.gazemap_width)[:n]
    if pool_to_7x7 and maps.shape[-1] == 49:
        maps = maps.reshape(n, 7, 7, 7, 7).mean(axis=(2, 4))
    return maps
