"""Numpy restatement of the frame overlay (csrc/rgp_overlay.hip, recurrent_gaze_prediction_amd/overlay.py): the oracle of
the overlay tests, every step with an explicit cast.

Per map [h, w] fp32 and frame [H, W, 3] uint8:
  resize     spline_ref.resize in float64, rounded once to fp32 (the identity at equal shapes)
  bytescale  export_ref.bytescale on the resized map, or -- with limits -- the same statements with the given cmin, cmax
  colour     lut[u], lut uint8 [256, 3]
  blend      PIL.Image.blend: alpha 0 the frame, alpha 1 the colour, else uint8(trunc(fp32(f) + fp32(alpha) * fp32(c - f))),
             the product rounded to fp32 before the add (not fused)
A refused map (NaN / Inf in it, limits not finite or descending, a frame index outside the clip) leaves its frame as it
is (zeros for a bad index) and heat 0."""
import numpy as np

import export_ref
import spline_ref


def resize32(m, HW):
    """One fp32 map -> fp32 [H, W], the value rgp_spline_resize writes."""
    m = np.asarray(m, np.float32)
    HW = tuple(int(v) for v in HW)
    if m.shape == HW:
        return m.copy()
    with np.errstate(all='ignore'):
        return spline_ref.resize(m.astype(np.float64), HW).astype(np.float32)


def bytescale_limits(v, cmin, cmax):
    """export_ref.bytescale with the caller's fp32 cmin and cmax (scipy's bytescale(data, cmin=, cmax=))."""
    v = np.asarray(v, np.float32)
    cmin, cmax = np.float32(cmin), np.float32(cmax)
    with np.errstate(all='ignore'):
        cscale = np.float32(cmax - cmin)
        if float(cscale) == 0.0:
            cscale = np.float32(1.0)
        scale = np.float32(255.0 / float(cscale))
        b = np.multiply(np.subtract(v, cmin, dtype=np.float32), scale, dtype=np.float32)
        nan = np.isnan(b)
        c = np.minimum(np.maximum(np.where(nan, np.float32(0.0), b), np.float32(0.0)), np.float32(255.0)).astype(np.float32)
        t = np.add(c, np.float32(0.5), dtype=np.float32)
    out = np.floor(t).astype(np.int64)
    out[nan] = 0
    return out.astype(np.uint8)


def blend(f, c, alpha):
    """PIL.Image.blend(f, c, alpha) on uint8 arrays of one shape, alpha in [0, 1]."""
    f, c = np.asarray(f, np.uint8), np.asarray(c, np.uint8)
    a = np.float32(alpha)
    if a == np.float32(0.0):
        return f.copy()
    if a == np.float32(1.0):
        return c.copy()
    d = (c.astype(np.int32) - f.astype(np.int32)).astype(np.float32)
    prod = np.multiply(a, d, dtype=np.float32)
    return np.trunc(np.add(f.astype(np.float32), prod, dtype=np.float32)).astype(np.uint8)


def blend_fused(f, c, alpha):
    """What a fused multiply-add would give: the product not rounded before the add (exact in float64, rounded once)."""
    f, c = np.asarray(f, np.uint8), np.asarray(c, np.uint8)
    d = c.astype(np.float64) - f.astype(np.float64)
    return np.trunc((f.astype(np.float64) + np.float64(np.float32(alpha)) * d).astype(np.float32)).astype(np.uint8)


def overlay(frames, maps, lut, alpha, frame_idx=None, limits=None):
    """-> (out uint8 [n, H, W, 3], heat uint8 [n, H, W], the list of refused maps).  limits: None, 'clip' or [n, 2]."""
    frames, maps, lut = np.asarray(frames), np.asarray(maps), np.asarray(lut)
    assert frames.dtype == np.uint8 and maps.dtype == np.float32 and lut.dtype == np.uint8 and lut.shape == (256, 3)
    n, (n_src, H, W, _) = len(maps), frames.shape
    idx = np.arange(n) if frame_idx is None else np.asarray(frame_idx).astype(np.int64)
    out, heat, refused = np.zeros((n, H, W, 3), np.uint8), np.zeros((n, H, W), np.uint8), []
    ok = [bool(np.isfinite(maps[i]).all()) and 0 <= idx[i] < n_src for i in range(n)]
    if limits is not None and not isinstance(limits, str):
        limits = np.broadcast_to(np.asarray(limits, np.float32), (n, 2))
        ok = [ok[i] and bool(np.isfinite(limits[i]).all()) and limits[i, 1] >= limits[i, 0] for i in range(n)]
    v = [resize32(maps[i], (H, W)) if ok[i] else None for i in range(n)]
    if isinstance(limits, str):
        assert limits == 'clip'
        good = [x for x in v if x is not None]
        lo = np.float32(min(x.min() for x in good)) if good else np.float32(0)
        hi = np.float32(max(x.max() for x in good)) if good else np.float32(0)
        limits = np.broadcast_to(np.array([lo, hi], np.float32), (n, 2))
    for i in range(n):
        if not ok[i]:
            refused.append(i)
            if 0 <= idx[i] < n_src:
                out[i] = frames[idx[i]]
            continue
        heat[i] = export_ref.bytescale(v[i]) if limits is None else bytescale_limits(v[i], limits[i, 0], limits[i, 1])
        out[i] = blend(frames[idx[i]], lut[heat[i]], alpha)
    return out, heat, refused


def grid_shape(N, height=None, width=None):
    """Rows and columns of the contact sheet: a near-square grid, or the rows that `width` columns need."""
    if height is None:
        height = int(np.ceil(np.sqrt(N))) if width is None else -(-N // int(width))
    if width is None:
        width = -(-N // int(height))
    assert height * width >= N
    return int(height), int(width)


def tile_grid(data, height=None, width=None, padsize=1, padval=0):
    """The array the reference's imshow_grid (evaluation/visualize_output.py:22-51) hands to imshow, written as a loop:
    image k sits at row k // width, column k % width of a sheet of cells (H + padsize) x (W + padsize) filled with padval."""
    data = np.asarray(data)
    N, H, W = data.shape[:3]
    rows, cols = grid_shape(N, height, width)
    ch, cw = H + padsize, W + padsize
    sheet = np.full((rows * ch, cols * cw) + data.shape[3:], padval, data.dtype)
    for k in range(N):
        r, c = divmod(k, cols)
        sheet[r * ch:r * ch + H, c * cw:c * cw + W] = data[k]
    return sheet
