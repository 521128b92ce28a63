"""Saliency metrics scored on the GPU: all frames and all requested metrics in one launch.

Device-side counterpart of ``evaluation_metrics`` (the host module, pinned to the reference's
evaluation_metrics.py by tests/golden/metrics_ref.npz) for prediction, ground truth and
fixation maps of one common shape of at most 4096 pixels (:func:`saliency_scores_single`).  The kernel
(csrc/rgp_metrics.hip, ``rgp_saliency_scores`` in include/rgp.h) follows the host module statement for
statement in fp64, so with the host's own random draws it returns the host's scores to summation order
(about 1e-12); the averaging over frames stays here (``np.mean``).

Random draws come in two forms:

* ``draws='reference'``: :func:`draw_reference_samples` consumes numpy's global RNG exactly as the host
  functions do and hands the draws to the kernel -- same seed, same scores as the host module;
* ``draws='device'``: the kernel draws with Philox-4x32-10 keyed by ``seed`` -- nothing but the launch.

Fixation maps of another shape than the maps -- what the reference's evaluation runs, fixations at the video
frame's resolution -- go through :func:`saliency_scores_resized`: the kernel of csrc/rgp_metrics_scaled.hip
(``rgp_saliency_scores_scaled``) upsizes prediction and ground truth with the host's cubic-spline ``resize`` on the
fly, inside the metric sweeps, and takes the fixations as point lists (:func:`pack_points`).  :func:`saliency_score`
dispatches on the shapes; :func:`resize_maps` returns the resized maps themselves (overlays, dumps).

What the kernels do not cover -- equal shapes of more than 4096 pixels, source maps of more than 4096 pixels, more
than 256 fixations in a frame, frames of different shapes -- raises ``ValueError``; there is no silent fallback: use
``evaluation_metrics`` for those.
"""
import ctypes

import numpy as np
import numpy.random as random
import scipy.sparse
import torch

from . import _lib

METRICS = ('sim', 'cc', 'AUC_Judd', 'AUC_Borji', 'AUC_shuffled', 'NSS')       # rows of the kernel's score table
FRAME_METRICS = ('sim', 'cc', 'AUC_Borji', 'AUC_Judd', 'AUC_shuffled')        # evaluate_gaze.py:135
MAX_PIX, MAX_FIX = _lib.RGP_METRICS_MAX_PIX, _lib.RGP_METRICS_MAX_FIX
SCALED_MAX_PIX, SCALED_MAX_OTHER = _lib.RGP_METRICS_SCALED_MAX_PIX, _lib.RGP_METRICS_SCALED_MAX_OTHER
_HOST = 'recurrent_gaze_prediction_amd.evaluation_metrics (the host module) scores such input'


def _dense(m):
    return m.toarray() if scipy.sparse.issparse(m) else m


def _is_tensor(x):
    return isinstance(x, torch.Tensor)


def stack_maps(maps, what):
    """A [N,H,W] array (or the tensor itself) from an array, a tensor or a list of (sparse) maps."""
    if _is_tensor(maps):
        out = maps
    elif isinstance(maps, np.ndarray) and maps.dtype != object:
        out = maps
    else:
        maps = [np.asarray(_dense(m)) for m in maps]
        if len({m.shape for m in maps}) > 1:
            raise ValueError('%s: frames of different shapes; %s' % (what, _HOST))
        out = np.stack(maps)
    if out.ndim != 3:
        raise ValueError('%s: expected [N,H,W], got shape %s' % (what, tuple(out.shape)))
    return out


def _check_metrics(metrics):
    metrics = (metrics,) if isinstance(metrics, str) else tuple(metrics)
    for m in metrics:
        if m not in _lib.METRIC_BITS:
            raise ValueError(m)
    if not metrics:
        raise ValueError('no metric requested')
    return metrics


def draw_reference_samples(fixation_maps, other_union, metrics, n_rep=100, order='metric', jitter=True):
    """The random draws of the host metrics, taken from numpy's GLOBAL RNG in the host's order, packed for the kernel.

    Per frame that has a fixation (the host functions return NaN before drawing otherwise) AUC_Judd consumes
    ``rand(H, W)``, AUC_Borji ``randint(0, n_pix, [n_fix, n_rep])`` and AUC_shuffled ``n_rep`` calls of
    ``permutation(M)`` (M = size of the negative set), of which the first n_fix entries are used.
    ``order='metric'``: all frames of the first metric of ``metrics``, then the next -- what ``saliency_score`` called
    once per metric consumes.  ``order='frame'``: per frame the requested metrics in ``FRAME_METRICS`` order -- what
    ``evaluate_gaze.handle_frame`` consumes.  ``other_union``: one [H,W] map for all frames or [N,H,W], one per frame;
    only AUC_shuffled reads it.

    Returns a dict: ``judd_jitter`` f64 [N, n_pix] (None when AUC_Judd is not requested or ``jitter`` is off),
    ``borji_neg`` / ``shuf_neg`` int32 [N, n_rep, neg_stride] pixel indices (None when not requested), ``shuf_cnt``
    int32 [N] = min(n_fix, M), ``n_fix`` int32 [N] and ``neg_stride`` = the largest n_fix (at least 1)."""
    fix = np.asarray(stack_maps(fixation_maps, 'fixation_maps')) > 0.5
    N, H, W = fix.shape
    n_fix = fix.reshape(N, H * W).sum(1).astype(np.int32)
    negatives = None
    if 'AUC_shuffled' in _check_metrics(metrics):
        if other_union is None:
            raise ValueError('other_map_union required')
        other = np.asarray(_dense(other_union)) > 0.5
        if other.shape not in ((H, W), (N, H, W)):
            raise ValueError('other_map.shape != fixation_map.shape')
        negatives = [np.nonzero(o)[0] for o in other.reshape(-1, H * W)]
    return _draw_reference(n_fix, negatives, H, W, metrics, n_rep, order, jitter)


def draw_reference_samples_points(fix_points, other_points, shape, metrics, n_rep=100, order='metric', jitter=True):
    """:func:`draw_reference_samples` for fixations given as points (:func:`pack_points` on the host): the same draws
    in the same order without a dense [N,H,W] array.  ``other_points``: (ptr, idx) with N + 1 (one set per frame) or 2
    (one set for all frames) entries in ptr; None unless AUC_shuffled is requested."""
    H, W = (int(v) for v in shape)
    ptr = np.asarray(fix_points[0], np.int64)
    negatives = None
    if 'AUC_shuffled' in _check_metrics(metrics):
        if other_points is None:
            raise ValueError('other_map_union required')
        optr, oidx = np.asarray(other_points[0], np.int64), np.asarray(other_points[1], np.int64)
        if len(optr) not in (2, len(ptr)):
            raise ValueError('other_map.shape != fixation_map.shape')
        negatives = [oidx[a:b] for a, b in zip(optr[:-1], optr[1:])]
    return _draw_reference(np.diff(ptr).astype(np.int32), negatives, H, W, metrics, n_rep, order, jitter)


def _draw_reference(n_fix, negatives, H, W, metrics, n_rep, order, jitter):
    """The draws of :func:`draw_reference_samples` from the fixation counts and the members of the negative sets."""
    metrics = _check_metrics(metrics)
    if order not in ('metric', 'frame'):
        raise ValueError(order)
    N, n_pix = len(n_fix), H * W
    if n_fix.max(initial=0) > MAX_FIX:
        raise ValueError('a frame has %d fixations, more than RGP_METRICS_MAX_FIX = %d; %s' % (n_fix.max(), MAX_FIX, _HOST))
    stride = max(1, int(n_fix.max(initial=0)))
    out = {'judd_jitter': None, 'borji_neg': None, 'shuf_neg': None, 'shuf_cnt': None, 'n_fix': n_fix, 'neg_stride': stride}
    if 'AUC_Judd' in metrics and jitter:
        out['judd_jitter'] = np.zeros((N, n_pix), np.float64)
    if 'AUC_Borji' in metrics:
        out['borji_neg'] = np.zeros((N, n_rep, stride), np.int32)
    if 'AUC_shuffled' in metrics:
        out['shuf_neg'] = np.zeros((N, n_rep, stride), np.int32)
        out['shuf_cnt'] = np.zeros(N, np.int32)

    def draw(metric, i):
        k = int(n_fix[i])
        if k == 0:
            return
        if metric == 'AUC_Judd' and jitter:
            out['judd_jitter'][i] = random.rand(H, W).ravel()
        elif metric == 'AUC_Borji':
            out['borji_neg'][i, :, :k] = random.randint(0, n_pix, [k, n_rep]).T
        elif metric == 'AUC_shuffled':
            members = negatives[i if len(negatives) > 1 else 0]
            idx = np.stack([random.permutation(len(members))[:k] for _ in range(n_rep)])      # [n_rep, min(k, M)]
            out['shuf_cnt'][i] = idx.shape[1]
            out['shuf_neg'][i, :, :idx.shape[1]] = members[idx]

    if order == 'metric':
        for metric in metrics:
            for i in range(N):
                draw(metric, i)
    else:
        for i in range(N):
            for metric in FRAME_METRICS:
                if metric in metrics:
                    draw(metric, i)
    return out


def _device_maps(x, what, dev, binary=False):
    """-> contiguous device tensor the kernel reads: fp32 / fp64 maps as they are, anything else as numpy would treat
    it (fp64); ``binary`` maps as fp32 0 / 1 of ``x > 0.5`` unless already fp32 on the device."""
    if _is_tensor(x):
        t = x.to(dev)
    else:
        a = np.asarray(x)
        if binary:
            a = (a > 0.5).astype(np.float32)
        elif a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if binary:
        if t.dtype != torch.float32:
            t = (t > 0.5).to(torch.float32)
    elif t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float64)
    return t.contiguous()


def _resolve_draws(draws, metrics, other, jitter, reference):
    """-> (flags, packed) of the ``draws`` argument of the scorers: the host's draws (the dict given, or ``reference()``
    for ``'reference'``), or None and the flags of device draws."""
    if isinstance(draws, dict):
        return 0, draws
    if draws == 'reference':
        return 0, reference()
    if draws == 'device':
        if 'AUC_shuffled' in metrics and other is None:
            raise ValueError('other_map_union required')
        return _lib.RGP_METRICS_DEVICE_DRAWS | (0 if jitter else _lib.RGP_METRICS_NO_JITTER), None
    raise ValueError("draws must be 'device', 'reference' or the result of draw_reference_samples")


def _ptr(t):
    return None if t is None else t.data_ptr()


def _upload_draws(packed, dev):
    """The caller's draws as device tensors, by the argument structs' field names (None: not given, or device draws)."""
    def up(key, dtype):
        a = packed.get(key) if packed is not None else None
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)
    return {'judd_jitter': up('judd_jitter', np.float64), 'borji_neg': up('borji_neg', np.int32),
            'shuf_neg': up('shuf_neg', np.int32), 'shuf_cnt': up('shuf_cnt', np.int32)}


def _metric_bits(metrics):
    return sum({_lib.METRIC_BITS[m] for m in metrics})       # one bit each: the sum over the set is their OR


def _score_buffers(ws_bytes, N, dev):
    """-> the workspace and the [6, N] score table of one launch."""
    ws = torch.empty(max(int(ws_bytes), 64), dtype=torch.uint8, device=dev)
    return ws, torch.full((_lib.RGP_METRICS_COUNT, N), float('nan'), dtype=torch.float64, device=dev)


def _launch_scores(lib_fn, args, ws, scores, metrics, dev):
    """The launch, the count of refused frames (rgp_metrics_status), ValueError for what the kernel refuses (naming the
    host module), and the rows of the score table as {metric: f64 [N]}."""
    lib = _lib.load()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        rc = lib_fn(ctypes.byref(args), stream)
        if rc == 0:
            rc = lib.rgp_metrics_status(ws.data_ptr(), stream)
    if rc == -1:
        raise ValueError('%s; %s' % (lib.rgp_last_error().decode(), _HOST))
    _lib.check(rc)
    host_scores = scores.cpu().numpy()
    return {m: host_scores[_lib.METRIC_ROWS[m]].copy() for m in metrics}


def _device_draws_from(ws, N, n_rep, stride):
    """The indices the kernel drew, read back from the head of its workspace (behind the 64-byte status block)."""
    e = N * int(n_rep) * stride
    ints = ws[64:64 + (2 * e + N) * 4].view(torch.int32).cpu().numpy()
    return {'borji_neg': ints[:e].reshape(N, n_rep, stride), 'shuf_neg': ints[e:2 * e].reshape(N, n_rep, stride),
            'shuf_cnt': ints[2 * e:], 'neg_stride': stride}


def saliency_scores_single(pred, gt, fix, other, metrics, draws='device', seed=0, offset=0, n_rep=100, step_size=0.1,
                           jitter=True, max_fix=None, device=None, return_draws=False):
    """Per-frame scores {metric: f64 [N]} of N frames in one launch (``evaluation_metrics.saliency_score_single`` for
    every frame and every metric of ``metrics``).

    pred, gt, fix: [N,H,W], torch device tensors (fp32 / fp64 ones are read in place) or numpy arrays / lists of maps
    (uploaded).  other: the AUC_shuffled negative set, [H,W] (one for all frames) or [N,H,W]; None if AUC_shuffled is
    not requested.  ``draws='reference'`` takes the draws from numpy's global RNG as the host does, metric after
    metric in the order of ``metrics`` (:func:`draw_reference_samples`, or pass its result as ``draws``);
    ``draws='device'`` draws on the device from (seed, offset + frame): frames a..b of one call equal a call on those
    frames alone with ``offset=a``.  ``max_fix``: upper bound of the fixations per frame if known (device draws size
    their index buffers by it; by default it is counted).  ``return_draws`` adds the indices the kernel used under
    the key ``'draws'``.  Raises ValueError for what the kernel does not cover, naming the host module."""
    metrics = _check_metrics(metrics)
    pred, gt, fix = stack_maps(pred, 'pred'), stack_maps(gt, 'gt'), stack_maps(fix, 'fix')
    if not (tuple(pred.shape) == tuple(gt.shape) == tuple(fix.shape)):
        raise ValueError('pred %s, gt %s and fixation maps %s differ in shape; %s'
                         % (tuple(pred.shape), tuple(gt.shape), tuple(fix.shape), _HOST))
    N, H, W = (int(v) for v in pred.shape)
    if N < 1:
        raise ValueError('no frames')
    if H * W > MAX_PIX:
        raise ValueError('maps of %d x %d pixels, more than RGP_METRICS_MAX_PIX = %d; %s' % (H, W, MAX_PIX, _HOST))
    if device is None:
        device = next((t.device for t in (pred, gt, fix) if _is_tensor(t) and t.is_cuda), torch.device('cuda:0'))
    dev = torch.device(device)

    def reference():
        host_fix = fix.cpu().numpy() if _is_tensor(fix) else fix
        host_other = other.cpu().numpy() if _is_tensor(other) else other
        return draw_reference_samples(host_fix, host_other, metrics, n_rep=n_rep, jitter=jitter)
    flags, packed = _resolve_draws(draws, metrics, other, jitter, reference)
    if packed is not None:
        stride = int(packed['neg_stride'])

    if packed is None and max_fix is None and not _is_tensor(fix):
        max_fix = int((np.asarray(fix) > 0.5).reshape(N, -1).sum(1).max())
    if max_fix is not None and max_fix > MAX_FIX:
        raise ValueError('a frame has %d fixations, more than RGP_METRICS_MAX_FIX = %d; %s' % (max_fix, MAX_FIX, _HOST))
    d_pred, d_gt = _device_maps(pred, 'pred', dev), _device_maps(gt, 'gt', dev)
    d_fix = _device_maps(fix, 'fix', dev, binary=True)
    flags |= _lib.RGP_METRICS_PRED_F64 if d_pred.dtype == torch.float64 else 0
    flags |= _lib.RGP_METRICS_GT_F64 if d_gt.dtype == torch.float64 else 0
    d_other, other_stride = None, 0
    if packed is None:
        if max_fix is None:
            max_fix = int((d_fix > 0.5).reshape(N, -1).sum(1).max().item())
        if max_fix > MAX_FIX:
            raise ValueError('a frame has %d fixations, more than RGP_METRICS_MAX_FIX = %d; %s' % (max_fix, MAX_FIX, _HOST))
        stride = max(1, int(max_fix))
        if 'AUC_shuffled' in metrics:
            d_other = _device_maps(_dense(other), 'other', dev, binary=True)
            if tuple(d_other.shape) == (N, H, W):
                other_stride = H * W
            elif tuple(d_other.shape) != (H, W):
                raise ValueError('other_map.shape != fixation_map.shape')

    d_draws = _upload_draws(packed, dev)
    lib = _lib.load()
    ws, scores = _score_buffers(lib.rgp_metrics_workspace_bytes(N, n_rep, stride, flags), N, dev)
    args = _lib.MetricsArgs(pred=_ptr(d_pred), gt=_ptr(d_gt), fix=_ptr(d_fix), other=_ptr(d_other), other_stride=other_stride,
                            n_frames=N, height=H, width=W, metrics=_metric_bits(metrics), flags=flags, n_rep=int(n_rep),
                            neg_stride=stride, step_size=float(step_size), seed=int(seed) & (2 ** 64 - 1), offset=int(offset),
                            workspace=ws.data_ptr(), workspace_bytes=ws.numel(), scores=scores.data_ptr(),
                            **{k: _ptr(t) for k, t in d_draws.items()})
    out = _launch_scores(lib.rgp_saliency_scores, args, ws, scores, metrics, dev)
    if return_draws:
        out['draws'] = packed if packed is not None else dict(
            _device_draws_from(ws, N, n_rep, stride), n_fix=(d_fix > 0.5).reshape(N, -1).sum(1).to(torch.int32).cpu().numpy())
    return out


def _maps_shape(maps):
    """(H, W) of a [N,H,W] array / tensor or of a list of (sparse) maps (the first one's)."""
    if _is_tensor(maps) or (isinstance(maps, np.ndarray) and maps.dtype != object):
        return tuple(int(v) for v in maps.shape[-2:])
    first = maps[0]
    return tuple(int(v) for v in (first.shape if scipy.sparse.issparse(first) else np.asarray(first).shape))


def _is_packed(x):
    return isinstance(x, tuple) and len(x) == 2 and (_is_tensor(x[0]) or isinstance(x[0], np.ndarray)) and x[0].ndim == 1


def pack_points(maps_or_points, shape):
    """Fixation (or negative-set) maps as the point lists the frame-resolution scorer takes: ``(ptr, idx)``, int32, frame
    n owning ``idx[ptr[n]:ptr[n + 1]]``, the flat indices ``row * W + col`` of its pixels ``> 0.5`` on the ``shape`` =
    (H, W) grid, unique and increasing -- the order of ``np.nonzero(F.ravel())``.

    Accepted: a dense [N,H,W] array; a [N,H,W] device tensor (``torch.nonzero`` on the device, no host round trip:
    the result is a pair of device tensors); a list of ``scipy.sparse`` matrices or dense maps; a list of per-frame
    ``(rows, cols)`` pairs.  Frames of another shape than ``shape`` raise ValueError naming the host module."""
    H, W = (int(v) for v in shape)
    if _is_tensor(maps_or_points):
        t = maps_or_points
        if t.ndim != 3 or tuple(t.shape[1:]) != (H, W):
            raise ValueError('maps of shape %s on a grid of %s; %s' % (tuple(t.shape), (H, W), _HOST))
        nz = torch.nonzero(t.reshape(t.shape[0], H * W) > 0.5)                      # sorted by frame, then pixel
        ptr = torch.zeros(t.shape[0] + 1, dtype=torch.int64, device=t.device)
        ptr[1:] = torch.cumsum(torch.bincount(nz[:, 0], minlength=t.shape[0]), 0)
        return ptr.to(torch.int32), nz[:, 1].to(torch.int32).contiguous()
    if isinstance(maps_or_points, np.ndarray) and maps_or_points.dtype != object:
        a = maps_or_points
        if a.ndim != 3 or a.shape[1:] != (H, W):
            raise ValueError('maps of shape %s on a grid of %s; %s' % (a.shape, (H, W), _HOST))
        frames, pix = np.nonzero(a.reshape(len(a), H * W) > 0.5)
        ptr = np.zeros(len(a) + 1, np.int64)
        ptr[1:] = np.cumsum(np.bincount(frames, minlength=len(a)))
        return ptr.astype(np.int32), pix.astype(np.int32)
    per_frame = []
    for m in maps_or_points:
        if isinstance(m, (tuple, list)) and len(m) == 2 and np.ndim(m[0]) == 1:
            rows, cols = (np.asarray(v).astype(np.int64).reshape(-1) for v in m)
            if len(rows) != len(cols) or (len(rows) and (rows.min() < 0 or rows.max() >= H or cols.min() < 0 or cols.max() >= W)):
                raise ValueError('a point lies outside the grid of %s' % ((H, W),))
        else:
            if tuple(m.shape) != (H, W):
                raise ValueError('a map of shape %s among maps of %s: frames of different shapes; %s' % (tuple(m.shape), (H, W), _HOST))
            if scipy.sparse.issparse(m):
                c = m.tocoo()
                keep = c.data > 0.5
                rows, cols = c.row[keep].astype(np.int64), c.col[keep].astype(np.int64)
            else:
                rows, cols = np.nonzero(np.asarray(m) > 0.5)
        per_frame.append(np.unique(rows * W + cols))
    ptr = np.zeros(len(per_frame) + 1, np.int64)
    ptr[1:] = np.cumsum([len(v) for v in per_frame])
    if ptr[-1] >= 2 ** 31:
        raise ValueError('more than 2^31 points')
    idx = np.concatenate(per_frame) if per_frame else np.zeros(0, np.int64)
    return ptr.astype(np.int32), idx.astype(np.int32)


def _host_points(points):
    return tuple(v.cpu().numpy() if _is_tensor(v) else np.asarray(v) for v in points)


def _device_points(points, dev):
    """(ptr, idx) -> int32 device tensors (idx never empty: the kernel is handed a valid pointer) and len(idx)."""
    ptr, idx = (v.to(dev, torch.int32) if _is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v, np.int32)).to(dev)
                for v in points)
    n = int(idx.numel())
    if n == 0:
        idx = torch.zeros(1, dtype=torch.int32, device=dev)
    return ptr.contiguous(), idx.contiguous(), n


def saliency_scores_resized(pred, gt, fix, other, metrics, draws='device', seed=0, offset=0, n_rep=100, step_size=0.1,
                            jitter=True, max_fix=None, device=None, return_draws=False, shape=None):
    """:func:`saliency_scores_single` for fixation maps of ANOTHER shape than the maps: per-frame scores
    {metric: f64 [N]} of ``evaluation_metrics.saliency_score_single``, which upsizes prediction and ground truth to the
    fixation map's shape with a cubic spline and scores there.  One launch; the upsized maps are never stored.

    pred, gt: [N,h,w] as for saliency_scores_single.  fix: fixation maps of shape (H, W) in any form
    :func:`pack_points` takes, or its result ``(ptr, idx)`` together with ``shape=(H, W)``.  other: the AUC_shuffled
    negative set likewise -- one map / ``ptr`` of two entries for all frames, or N of them; None if AUC_shuffled is not
    requested.  Draws, seed, offset, n_rep, step_size, jitter, max_fix, return_draws and the return value as in
    saliency_scores_single; ``draws='reference'`` takes the host's draws on the full-size grid
    (:func:`draw_reference_samples_points`).  Raises ValueError for what the kernel does not cover."""
    metrics = _check_metrics(metrics)
    pred, gt = stack_maps(pred, 'pred'), stack_maps(gt, 'gt')
    if tuple(pred.shape) != tuple(gt.shape):
        raise ValueError('pred %s and gt %s differ in shape; %s' % (tuple(pred.shape), tuple(gt.shape), _HOST))
    N, h, w = (int(v) for v in pred.shape)
    if N < 1:
        raise ValueError('no frames')
    if _is_packed(fix):
        if shape is None:
            raise ValueError('fixations given as (ptr, idx) need shape=(H, W)')
    else:
        shape = _maps_shape(fix) if shape is None else shape
        fix = pack_points(fix, shape)
    H, W = (int(v) for v in shape)
    if (H, W) == (h, w):
        raise ValueError('maps and fixation maps share the shape %s: saliency_scores_single scores those' % ((H, W),))
    if h < 2 or w < 2 or h * w > MAX_PIX:
        raise ValueError('maps of %d x %d pixels: sides of at least 2 and at most RGP_METRICS_MAX_PIX = %d pixels; %s' % (h, w, MAX_PIX, _HOST))
    if H < 1 or W < 1 or H * W > SCALED_MAX_PIX:
        raise ValueError('fixation maps of %d x %d pixels, more than RGP_METRICS_SCALED_MAX_PIX = %d; %s' % (H, W, SCALED_MAX_PIX, _HOST))
    if len(fix[0]) != N + 1:
        raise ValueError('%d frames of fixations for %d maps' % (len(fix[0]) - 1, N))
    if device is None:
        device = next((t.device for t in (pred, gt, fix[0]) if _is_tensor(t) and t.is_cuda), torch.device('cuda:0'))
    dev = torch.device(device)
    shared = False
    if other is not None:
        if not _is_packed(other):
            if scipy.sparse.issparse(other) or (not isinstance(other, (list, tuple)) and other.ndim == 2):
                other = _dense(other)[None]
            other = pack_points(other, (H, W))
        if len(other[0]) not in (2, N + 1):
            raise ValueError('other_map.shape != fixation_map.shape')
        shared = len(other[0]) == 2 and N != 1

    def reference():
        return draw_reference_samples_points(_host_points(fix), None if other is None else _host_points(other), (H, W),
                                             metrics, n_rep=n_rep, jitter=jitter)
    flags, packed = _resolve_draws(draws, metrics, other, jitter, reference)
    flags |= _lib.RGP_METRICS_SCALED_OTHER_SHARED if shared else 0
    if packed is not None:
        stride = int(packed['neg_stride'])
        for key, want in (('judd_jitter', (N, H * W)), ('borji_neg', (N, int(n_rep), stride)), ('shuf_neg', (N, int(n_rep), stride)),
                          ('shuf_cnt', (N,))):                       # the kernel reads them by these extents
            if packed.get(key) is not None and tuple(np.shape(packed[key])) != want:
                raise ValueError('draws[%r] has shape %s, expected %s' % (key, tuple(np.shape(packed[key])), want))
    else:
        if max_fix is None:
            counts = fix[0][1:] - fix[0][:-1]
            max_fix = int(counts.max().item() if _is_tensor(counts) else counts.max(initial=0))
        stride = max(1, int(max_fix))
    if stride > MAX_FIX:
        raise ValueError('a frame has %d fixations, more than RGP_METRICS_MAX_FIX = %d; %s' % (stride, MAX_FIX, _HOST))

    d_pred, d_gt = _device_maps(pred, 'pred', dev), _device_maps(gt, 'gt', dev)
    flags |= _lib.RGP_METRICS_PRED_F64 if d_pred.dtype == torch.float64 else 0
    flags |= _lib.RGP_METRICS_GT_F64 if d_gt.dtype == torch.float64 else 0
    d_fptr, d_fidx, fix_len = _device_points(fix, dev)
    d_optr, d_oidx, other_len = (None, None, 0) if other is None else _device_points(other, dev)

    d_draws = _upload_draws(packed, dev)
    lib = _lib.load()
    ws, scores = _score_buffers(lib.rgp_metrics_scaled_workspace_bytes(N, n_rep, stride, H, W, flags), N, dev)
    args = _lib.MetricsScaledArgs(pred=_ptr(d_pred), gt=_ptr(d_gt), fix_ptr=_ptr(d_fptr), fix_idx=_ptr(d_fidx), other_ptr=_ptr(d_optr),
                                  other_idx=_ptr(d_oidx), fix_len=fix_len, other_len=other_len, n_frames=N, height=h, width=w,
                                  target_height=H, target_width=W, metrics=_metric_bits(metrics), flags=flags, n_rep=int(n_rep),
                                  neg_stride=stride, step_size=float(step_size), seed=int(seed) & (2 ** 64 - 1), offset=int(offset),
                                  workspace=ws.data_ptr(), workspace_bytes=ws.numel(), scores=scores.data_ptr(),
                                  **{k: _ptr(t) for k, t in d_draws.items()})
    out = _launch_scores(lib.rgp_saliency_scores_scaled, args, ws, scores, metrics, dev)
    if return_draws:
        out['draws'] = packed if packed is not None else dict(
            _device_draws_from(ws, N, n_rep, stride), n_fix=np.diff(_host_points(fix)[0]).astype(np.int32))
    return out


def resize_maps(maps, out_shape, out_dtype=torch.float64, device=None):
    """[N,h,w] maps (array, list or device tensor; fp32 / fp64 read in place, anything else as fp64) -> device tensor
    [N,H,W] of ``out_dtype`` (float64 or float32): ``evaluation_metrics.resize`` -- scipy's order-3 spline, mode
    'reflect' -- of every map, in one launch.  The frame-size map for overlays and dumps; the spline is applied at
    equal shapes too (there the host's ``resize`` is the identity).  fp32 output is the fp64 value rounded once."""
    maps = stack_maps(maps, 'maps')
    N, h, w = (int(v) for v in maps.shape)
    H, W = (int(v) for v in out_shape)
    if out_dtype not in (torch.float64, torch.float32):
        raise ValueError('out_dtype must be torch.float64 or torch.float32')
    if N < 1:
        raise ValueError('no frames')
    if h < 2 or w < 2 or h * w > MAX_PIX:
        raise ValueError('maps of %d x %d pixels: sides of at least 2 and at most RGP_METRICS_MAX_PIX = %d pixels; %s' % (h, w, MAX_PIX, _HOST))
    if H < 1 or W < 1 or H * W > SCALED_MAX_PIX:
        raise ValueError('target of %d x %d pixels, more than RGP_METRICS_SCALED_MAX_PIX = %d; %s' % (H, W, SCALED_MAX_PIX, _HOST))
    if device is None:
        device = maps.device if _is_tensor(maps) and maps.is_cuda else torch.device('cuda:0')
    dev = torch.device(device)
    src = _device_maps(maps, 'maps', dev)
    dst = torch.empty((N, H, W), dtype=out_dtype, device=dev)
    lib = _lib.load()
    ws = torch.empty(max(int(lib.rgp_spline_resize_workspace_bytes(H, W)), 64), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.rgp_spline_resize(src.data_ptr(), int(src.dtype == torch.float64), N, h, w, dst.data_ptr(),
                                         int(out_dtype == torch.float64), H, W, ws.data_ptr(), ws.numel(), stream))
        torch.cuda.current_stream(dev).synchronize()          # the workspace is released on return
    return dst


def union_of_ten_points(point_lists, rng=random):
    """:func:`union_of_ten` on per-frame arrays of flat pixel indices: the sorted union of ten of them drawn without
    replacement from ``rng`` -- the same ``choice`` -- without a dense map."""
    n = len(point_lists)
    assert n >= 10
    return np.unique(np.concatenate([point_lists[int(i)] for i in rng.choice(range(n), 10, replace=False)]))


def union_of_ten(fixation_maps, rng=random):
    """The AUC_shuffled negative set of ``saliency_score`` (evaluation_metrics.py:275-295): the sum of ``> 0`` of ten
    fixation maps drawn without replacement from ``rng`` (numpy's global RNG by default)."""
    n = len(fixation_maps)
    assert n >= 10
    union = None
    for i in rng.choice(range(n), 10, replace=False):
        fm = fixation_maps[int(i)]
        fm = (fm > 0).to(torch.float32) if _is_tensor(fm) else (np.asarray(_dense(fm)) > 0).astype(np.float32)
        union = fm if union is None else union + fm
    return union


def saliency_score(metric, pred_maps, gt_maps, fixation_maps, draws='device', seed=0):
    """``evaluation_metrics.saliency_score`` with the frames scored on the device: the mean over the frames of
    ``metric``, AUC_shuffled's negatives from the union of ten fixation maps chosen with numpy's global RNG (both
    forms of ``draws`` consume that ``choice``).  With ``draws='reference'`` the result is the host function's for the
    same global RNG state.  Fixation maps of the maps' shape go to :func:`saliency_scores_single`, of another shape
    (sparse ones included) to :func:`saliency_scores_resized`."""
    assert len(gt_maps) == len(pred_maps) == len(fixation_maps)
    union = union_of_ten(fixation_maps)
    if _maps_shape(fixation_maps) != _maps_shape(pred_maps):       # the reference's case: fixations at frame resolution
        score = saliency_scores_resized
    else:
        score = saliency_scores_single
    scores = score(pred_maps, gt_maps, fixation_maps, union, (metric,), draws=draws, seed=seed)
    return np.mean(scores[metric])


__all__ = ['METRICS', 'FRAME_METRICS', 'stack_maps', 'draw_reference_samples', 'draw_reference_samples_points', 'pack_points',
           'saliency_scores_single', 'saliency_scores_resized', 'resize_maps', 'saliency_score', 'union_of_ten', 'union_of_ten_points']
