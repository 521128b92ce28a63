"""Ground-truth gaze maps from fixation points, built on the GPU in one launch.

The arithmetic of the reference's loader, for someone who brings eye-tracking data as fixation lists (the
reference's ``.mat`` files keep exactly those: ``fixation_t/_r/_c`` per observer): the rescale of raw gaze points to
the map grid (process_gazemap.py:35-58), the per-observer de-duplication, the sum over observers and the swap of the
axes (crc_input_data_seq.py:261-288), scipy's Gaussian filter and the min-max normalisation (:41-53).  The kernel
(csrc/rgp_gtmaps.hip, ``rgp_gazemaps_from_fixations`` in include/rgp.h) reproduces the host arithmetic bit for bit and
leaves ``gazemaps`` / ``fixationmaps`` (and, if asked, the xentropy ``labels``) on the device, where the scorer
(``evaluation_metrics_gpu``) and the action classifier read them.

Host side (numpy): :func:`pack_fixations` selects the frames and packs the observers' samples per frame;
:func:`gaussian_weights` makes scipy's kernel in float64 (the device's ``exp`` is not numpy's).

:func:`fixation_points` gives the same fixations at the raw resolution as point lists, the form the frame-resolution
scorer takes.

The loader's original-scale path (``gazemap_height is None``: sigma = 19 on the raw frame, 405 x 720 cells) is
:func:`gazemaps_original_scale` (csrc/rgp_gtmaps_full.hip, ``rgp_gazemaps_full_from_fixations``): the same arithmetic
with the planes in HBM and the filter tiled over them, the same bits as the host; it has no ``labels``.

Not covered by :func:`gazemaps_from_fixations`: maps of more than 4096 cells, more than 32 observers, a filter radius
above 32; by :func:`gazemaps_original_scale`: frames of more than 2^22 cells, more than 32 observers, a radius above
256.  Those raise ``ValueError``; there is no host fallback.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _image, _lib

# (S1, S2) -> sigma (crc_input_data_seq.py:225-236)
SIGMA_FOR_SHAPE = {(49, 49): 2.0, (48, 48): 2.0, (14, 14): 0.6, (7, 7): 0.3}
OUTPUTS = ('gazemaps', 'fixationmaps', 'labels')
MAX_PIX, MAX_OBSERVERS, MAX_RADIUS = _lib.RGP_GTMAPS_MAX_PIX, _lib.RGP_GTMAPS_MAX_OBSERVERS, _lib.RGP_GTMAPS_MAX_RADIUS
# the original-scale path: the loader's sigma on the raw frame (crc_input_data_seq.py:237-240), its outputs and caps
SIGMA_ORIGINAL_SCALE = 19
OUTPUTS_ORIGINAL_SCALE = ('gazemaps', 'fixationmaps')
FULL_MAX_PIX, FULL_MAX_RADIUS = _lib.RGP_GTMAPS_FULL_MAX_PIX, _lib.RGP_GTMAPS_FULL_MAX_RADIUS
FULL_WORKSPACE_TARGET = 256 << 20      # frames_per_call by default: as many frames as keep the workspace under this

# frame_ptr int32 [N + 1], samples int32 [n_samples, 3] = (observer, a, b), rows frame_ptr[n] .. frame_ptr[n + 1] being
# frame n's; n_observers = the divisor; raw_shape = (D1, D2), the extents a and b live in
PackedFixations = collections.namedtuple('PackedFixations', 'frame_ptr samples n_observers raw_shape')


def gaussian_weights(sigma):
    """-> (w float64 [2 r + 1], r): the kernel scipy.ndimage.gaussian_filter builds for ``sigma`` (truncate = 4)."""
    sigma = float(sigma)
    if not sigma > 0.0:
        raise ValueError('sigma = %r must be positive' % sigma)
    r = int(4.0 * sigma + 0.5)
    x = np.arange(-r, r + 1)
    w = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return w / w.sum(), r


def reference_frames(lengths):
    """The loader's frame selection (crc_input_data_seq.py:261-269) from the observers' recording lengths:
    -> (gazelen, indices of the observers kept, frame indices).  gazelen = max(len_0, len_1) - 10 (a single observer:
    len_0 - 10), observers shorter than gazelen are dropped, frames are range(15, gazelen, 5)."""
    lengths = [int(v) for v in lengths]
    if not lengths:
        raise ValueError('no observers')
    gazelen = max(lengths[:2]) - 10
    keep = [k for k, n in enumerate(lengths) if n > gazelen - 1]
    return gazelen, keep, np.arange(15, max(gazelen, 15), 5, dtype=np.int64)


def _ranges(start, count):
    """Concatenation of arange(start[i], start[i] + count[i])."""
    total = int(count.sum())
    if total == 0:
        return np.zeros(0, np.int64)
    ends = np.cumsum(count)
    return np.repeat(start - (ends - count), count) + np.arange(total, dtype=np.int64)


def pack_fixations(observers, raw_shape, frames='reference', fill_missing=False):
    """Per-frame sample lists of several observers -> :class:`PackedFixations`.

    observers: a list of ``(t, a, b, length)``: the frame index and the raw coordinates of each gaze sample of one
    observer (``a`` in [0, raw_shape[0]), ``b`` in [0, raw_shape[1])) and the number of frames of that recording.
    frames: ``'reference'`` (:func:`reference_frames`: the divisor is the number of observers kept) or an explicit
    array of frame indices (every observer kept; a frame past an observer's recording has no sample of theirs).
    fill_missing: per observer, before the selection, a frame without a sample takes the samples of the nearest
    earlier frame that has one, and the frames ahead of the first such frame take that one's (add_gazemap.py:57-74);
    filled frames duplicate their source's rows.  An observer without any sample stays empty."""
    D1, D2 = (int(v) for v in raw_shape)
    obs = []
    for k, (t, a, b, length) in enumerate(observers):
        t, a, b = (np.asarray(v).astype(np.int64).reshape(-1) for v in (t, a, b))
        length = int(length)
        if not (len(t) == len(a) == len(b)):
            raise ValueError('observer %d: t, a and b differ in length' % k)
        if len(t) and (t.min() < 0 or t.max() >= length):
            raise ValueError('observer %d: a sample lies outside the recording of %d frames' % (k, length))
        if len(t) and (a.min() < 0 or a.max() >= D1 or b.min() < 0 or b.max() >= D2):
            raise ValueError('observer %d: a sample lies outside the raw frame %s' % (k, (D1, D2)))
        obs.append((t, a, b, length))
    if isinstance(frames, str):
        if frames != 'reference':
            raise ValueError("frames must be 'reference' or an array of frame indices")
        _, keep, sel = reference_frames([o[3] for o in obs])
        obs = [obs[k] for k in keep]
    else:
        sel = np.asarray(frames).astype(np.int64).reshape(-1)
        if len(sel) and sel.min() < 0:
            raise ValueError('negative frame index')
    N = len(sel)
    starts, counts, sorted_ab = [], [], []
    for t, a, b, length in obs:
        order = np.argsort(t, kind='stable')
        ts = t[order]
        src = sel.copy()
        if fill_missing and len(ts):
            have = np.unique(ts)
            inside = sel < length
            prev = np.searchsorted(have, sel, side='right') - 1          # the last frame <= sel that has a sample
            src = np.where(inside, have[np.maximum(prev, 0)], sel)
        lo, hi = np.searchsorted(ts, src, side='left'), np.searchsorted(ts, src, side='right')
        starts.append(lo)
        counts.append(hi - lo)
        sorted_ab.append((a[order], b[order]))
    per_frame = np.sum(counts, axis=0) if obs else np.zeros(N, np.int64)
    frame_ptr = np.zeros(N + 1, np.int64)
    frame_ptr[1:] = np.cumsum(per_frame)
    if frame_ptr[-1] >= 2 ** 31:
        raise ValueError('more than 2^31 samples')
    samples = np.zeros((int(frame_ptr[-1]), 3), np.int32)
    offset = frame_ptr[:-1].copy()                                       # frame-major, observer after observer within a frame
    for k, ((a, b), lo, cnt) in enumerate(zip(sorted_ab, starts, counts)):
        src_rows, dst_rows = _ranges(lo, cnt), _ranges(offset, cnt)
        samples[dst_rows, 0] = k
        samples[dst_rows, 1] = a[src_rows]
        samples[dst_rows, 2] = b[src_rows]
        offset += cnt
    return PackedFixations(frame_ptr.astype(np.int32), samples, len(obs), (D1, D2))


def _check_packed(packed):
    """-> (frame_ptr int32 [N + 1], samples int32 [n, 3], n_observers, (D1, D2), N) of packed fixations; the refusals
    the host can make about them, which both fixation entries share."""
    frame_ptr, samples, n_observers, raw_shape = packed
    D1, D2 = (int(v) for v in raw_shape)
    if D1 < 2 or D2 < 2:
        raise ValueError('raw_shape %s: both extents must be at least 2' % ((D1, D2),))
    n_observers = int(n_observers)
    if not 1 <= n_observers <= MAX_OBSERVERS:
        raise ValueError('%d observers: must be in [1, RGP_GTMAPS_MAX_OBSERVERS = %d]' % (n_observers, MAX_OBSERVERS))
    frame_ptr = np.ascontiguousarray(frame_ptr, np.int32).reshape(-1)
    samples = np.ascontiguousarray(samples, np.int32).reshape(-1, 3)
    N = len(frame_ptr) - 1
    if N < 0 or frame_ptr[0] != 0 or np.any(np.diff(frame_ptr) < 0) or frame_ptr[-1] != len(samples):
        raise ValueError('frame_ptr must start at 0, not decrease and end at len(samples)')
    return frame_ptr, samples, n_observers, (D1, D2), N


def _upload(frame_ptr, samples, w, dev):
    """-> the three inputs of a fixation entry on the device (a row of zeros stands in for no samples at all)."""
    return (torch.from_numpy(frame_ptr).to(dev), torch.from_numpy(samples if len(samples) else np.zeros((1, 3), np.int32)).to(dev),
            torch.from_numpy(np.ascontiguousarray(w, np.float64)).to(dev))


def gazemaps_from_fixations(packed, out_shape=(49, 49), sigma=None, want=('gazemaps', 'fixationmaps'), device=None):
    """Packed fixations -> {name: device tensor fp32 [N, S2, S1]} for the names in ``want`` (of ``OUTPUTS``), one launch.

    out_shape = (S1, S2), the extents ``a`` and ``b`` are scaled to; the frames come out as the loader hands them out,
    row ``b_``, column ``a_``.  sigma: by default the loader's value for the shape (``SIGMA_FOR_SHAPE``).
    ``fixationmaps``: observers per cell; ``gazemaps``: the filtered, min-max normalised mean; ``labels``:
    ``normalize_probability_map`` of the gaze maps (what the xentropy / KLD models train on).
    Raises ValueError for what the kernel does not cover and ``_lib.RgpError`` if the device refused a frame (a sample
    out of range: that frame is NaN; the error carries the tensors as ``.outputs``)."""
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(w not in OUTPUTS for w in want):
        raise ValueError('want = %r: choose from %s' % (want, OUTPUTS))
    S1, S2 = (int(v) for v in out_shape)
    frame_ptr, samples, n_observers, (D1, D2), N = _check_packed(packed)
    if sigma is None:
        if (S1, S2) not in SIGMA_FOR_SHAPE:
            raise ValueError('no default sigma for maps of %s; pass sigma' % ((S1, S2),))
        sigma = SIGMA_FOR_SHAPE[(S1, S2)]
    w, r = gaussian_weights(sigma)
    if S1 < 1 or S2 < 1 or S1 * S2 > MAX_PIX:
        raise ValueError('maps of %d x %d cells: more than RGP_GTMAPS_MAX_PIX = %d (the original-scale path is gazemaps_original_scale)'
                         % (S1, S2, MAX_PIX))
    if r > MAX_RADIUS:
        raise ValueError('sigma = %g: filter radius %d above RGP_GTMAPS_MAX_RADIUS = %d' % (sigma, r, MAX_RADIUS))
    dev = torch.device('cuda:0' if device is None else device)
    out = {name: torch.empty((N, S2, S1), dtype=torch.float32, device=dev) for name in want}
    if N == 0:
        return out
    d_ptr, d_samples, d_w = _upload(frame_ptr, samples, w, dev)
    lib = _lib.load()
    ws = _image.workspace(lib.rgp_gtmaps_workspace_bytes(), dev)

    def ptr(name):
        return _image.ptr(out.get(name))
    args = _lib.GtmapsArgs(frame_ptr=d_ptr.data_ptr(), samples=d_samples.data_ptr(), weights=d_w.data_ptr(), n_frames=N,
                           n_observers=n_observers, raw_d1=D1, raw_d2=D2, out_s1=S1, out_s2=S2, radius=r,
                           gazemaps=ptr('gazemaps'), fixationmaps=ptr('fixationmaps'), labels=ptr('labels'),
                           workspace=ws.data_ptr(), workspace_bytes=ws.numel())
    _image.launch(dev, lambda s: lib.rgp_gazemaps_from_fixations(ctypes.byref(args), s),
                  lambda s: lib.rgp_gtmaps_status(ws.data_ptr(), s), out)
    return out


def gazemaps_original_scale(packed, sigma=SIGMA_ORIGINAL_SCALE, want=OUTPUTS_ORIGINAL_SCALE, device=None, frames_per_call=None):
    """Packed fixations -> {name: device tensor fp32 [N, D2, D1]} at the raw frame's own resolution (row ``b``, column
    ``a``): the loader's original-scale maps.  ``fixationmaps``: observers per cell; ``gazemaps``: their mean filtered
    with ``sigma`` (the loader's 19) and min-max normalised per frame.  Bit for bit what
    ``gazemaps_from_fixations(out_shape=raw_shape)`` would give if it reached this size.

    The kernels keep two 4-byte planes per frame in a workspace, so the frames go through in calls of at most
    ``frames_per_call`` (default: what keeps the workspace under 256 MB) that reuse one workspace; frames are
    independent, so the split changes no bit.  Raises ValueError for what the entry does not cover (``labels`` among
    it) and ``_lib.RgpError`` if the device refused a frame (a sample out of range: that frame is NaN; the error carries
    the tensors as ``.outputs``)."""
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(w not in OUTPUTS_ORIGINAL_SCALE for w in want):
        raise ValueError('want = %r: choose from %s (the original-scale path has no labels)' % (want, OUTPUTS_ORIGINAL_SCALE))
    frame_ptr, samples, n_observers, (D1, D2), N = _check_packed(packed)
    w, r = gaussian_weights(sigma)
    if D1 * D2 > FULL_MAX_PIX:
        raise ValueError('frames of %d x %d cells: more than RGP_GTMAPS_FULL_MAX_PIX = %d' % (D1, D2, FULL_MAX_PIX))
    if r > FULL_MAX_RADIUS:
        raise ValueError('sigma = %g: filter radius %d above RGP_GTMAPS_FULL_MAX_RADIUS = %d' % (sigma, r, FULL_MAX_RADIUS))
    if frames_per_call is None:
        frames_per_call = max(1, FULL_WORKSPACE_TARGET // (8 * D1 * D2 + 4 * (3 + (D1 + 31) // 32)))
    frames_per_call = int(frames_per_call)
    if frames_per_call < 1:
        raise ValueError('frames_per_call = %d must be at least 1' % frames_per_call)
    dev = torch.device('cuda:0' if device is None else device)
    out = {name: torch.empty((N, D2, D1), dtype=torch.float32, device=dev) for name in want}
    if N == 0:
        return out
    d_ptr, d_samples, d_w = _upload(frame_ptr, samples, w, dev)
    lib = _lib.load()
    per_call = min(frames_per_call, N)
    ws = torch.empty(int(lib.rgp_gtmaps_full_workspace_bytes(per_call, D1, D2)), dtype=torch.uint8, device=dev)
    refused_total, rc = 0, 0
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        for lo in range(0, N, per_call):
            n = min(per_call, N - lo)

            def ptr(name):
                return _image.ptr(out[name][lo:] if name in out else None)
            # frame_ptr holds absolute rows of `samples`: a later chunk takes the same samples and a shifted frame_ptr
            args = _lib.GtmapsFullArgs(frame_ptr=d_ptr[lo:].data_ptr(), samples=d_samples.data_ptr(), weights=d_w.data_ptr(),
                                       n_frames=n, n_observers=n_observers, raw_d1=D1, raw_d2=D2, radius=r,
                                       gazemaps=ptr('gazemaps'), fixationmaps=ptr('fixationmaps'),
                                       workspace=ws.data_ptr(), workspace_bytes=ws.numel())
            rc = lib.rgp_gazemaps_full_from_fixations(ctypes.byref(args), stream)
            if rc != 0:
                break
            refused = ctypes.c_int(0)
            rc = lib.rgp_gtmaps_full_status(ws.data_ptr(), ctypes.byref(refused), stream)
            if rc != 0 and refused.value == 0:
                break
            refused_total, rc = refused_total + refused.value, 0
    if rc == 0 and refused_total:
        err = _lib.RgpError('librgp_hip error -1: rgp_gazemaps_full_from_fixations: %d frame(s) refused (a sample\'s observer, a or '
                            'b out of range, or a bad frame_ptr pair): their outputs are NaN' % refused_total)
        err.code, err.outputs = -1, out
        raise err
    _image.check(rc, out)
    return out


def fixation_points(packed):
    """Packed fixations -> ``(ptr, idx)`` int32: per frame the union over the observers of its samples at the RAW
    resolution, as sorted flat indices ``b * D1 + a`` on the (D2, D1) grid -- row ``b``, column ``a``, the axes of
    ``gazemaps_from_fixations``' ``fixationmaps``.  What ``evaluation_metrics_gpu.saliency_scores_resized`` takes
    as ``fix`` (with ``shape=(D2, D1)``) when the targets came from fixation lists."""
    frame_ptr, samples, _, raw_shape = packed
    D1, D2 = (int(v) for v in raw_shape)
    frame_ptr = np.asarray(frame_ptr, np.int64).reshape(-1)
    samples = np.asarray(samples, np.int64).reshape(-1, 3)
    N = len(frame_ptr) - 1
    if len(samples) and (samples[:, 1].min() < 0 or samples[:, 1].max() >= D1 or samples[:, 2].min() < 0 or samples[:, 2].max() >= D2):
        raise ValueError('a sample lies outside the raw frame %s' % ((D1, D2),))
    frame = np.repeat(np.arange(N, dtype=np.int64), np.diff(frame_ptr))
    key = np.unique(frame * (D1 * D2) + samples[:, 2] * D1 + samples[:, 1])
    ptr = np.searchsorted(key, np.arange(N + 1, dtype=np.int64) * (D1 * D2))
    return ptr.astype(np.int32), (key % (D1 * D2)).astype(np.int32)


__all__ = ['SIGMA_FOR_SHAPE', 'SIGMA_ORIGINAL_SCALE', 'OUTPUTS', 'OUTPUTS_ORIGINAL_SCALE', 'PackedFixations', 'gaussian_weights',
           'reference_frames', 'pack_fixations', 'gazemaps_from_fixations', 'gazemaps_original_scale', 'fixation_points']
