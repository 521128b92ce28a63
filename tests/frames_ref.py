"""Numpy restatement of Pillow's 8-bit antialiased resize (Image.resize with LANCZOS / BILINEAR / BICUBIC on RGB frames)
and of the loader's frame step around it (crc_input_data_seq.py:186-209): the oracle of the frame-image tests.

Written from the recipe, in scalar Python where the tables are made (math.sin, one weight at a time, the sum accumulated
in order) and without a look at recurrent_gaze_prediction_amd/frames.py, whose tables the CPU test compares with these.
tests/test_frames_cpu.py pins :func:`resize` to Pillow bit for bit where Pillow is installed.

Per axis, in -> out, a filter of support s:  scale = in / out, fs = max(scale, 1), support = s fs,
ksize = 2 ceil(support) + 1; per output xx: center = (xx + 0.5) scale, xmin = max(int(center - support + 0.5), 0),
xmax = min(int(center + support + 0.5), in), n = xmax - xmin, w[x] = filter((x + xmin - center + 0.5) (1 / fs)), each
divided by their sum (accumulated in order) unless it is 0.  The argument is scaled by the reciprocal 1 / fs, as Pillow
does it; at these shapes x / fs gives the same tables.  22-bit fixed point: int(w 2^22 + 0.5) (- 0.5 for a negative w),
truncated toward zero.  A pass: acc = 2^21 + sum pixel k in integers, out = clamp(acc >> 22, 0, 255) with an
arithmetic shift.  Horizontal first, on the input rows the vertical tables touch, then vertical on the 8-bit
intermediate; a pass whose in == out is skipped.  The fp32 image is float32(u8) * float32(1 / 255)."""
import math

import numpy as np

PRECISION_BITS = 22
SUPPORT = {'lanczos': 3.0, 'bilinear': 1.0, 'bicubic': 2.0}


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    if -3.0 <= x < 3.0:
        return _sinc(x) * _sinc(x / 3)
    return 0.0


def _bilinear(x):
    if x < 0.0:
        x = -x
    if x < 1.0:
        return 1.0 - x
    return 0.0


def _bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


FILTERS = {'lanczos': _lanczos, 'bilinear': _bilinear, 'bicubic': _bicubic}


def tables(in_size, out_size, filt='lanczos'):
    """-> (k int64 [out, ksize], bounds int64 [out, 2] = (xmin, n), ksize); entries past n are 0."""
    f, s = FILTERS[filt], SUPPORT[filt]
    scale = float(in_size) / out_size
    fs = scale if scale >= 1.0 else 1.0
    support = s * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    k = np.zeros((out_size, ksize), np.int64)
    bounds = np.zeros((out_size, 2), np.int64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        n = xmax - xmin
        w, ww = [], 0.0
        for x in range(n):
            v = f((x + xmin - center + 0.5) * ss)
            w.append(v)
            ww += v
        for x in range(n):
            v = w[x] / ww if ww != 0.0 else w[x]
            k[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, n)
    return k, bounds, ksize


def _pass(img, k, bounds, presum=None):
    """img int64 [..., in, C] resampled along axis -2 -> uint8 [..., out, C]; presum (a list) receives the sums >> 22
    before the clamp."""
    out = np.empty(img.shape[:-2] + (len(bounds), img.shape[-1]), np.int64)
    for xx, (xmin, n) in enumerate(bounds):
        acc = np.tensordot(img[..., xmin:xmin + n, :], k[xx, :n], axes=([-2], [0]))
        out[..., xx, :] = (acc + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS
    if presum is not None:
        presum.append(out)
    return np.clip(out, 0, 255).astype(np.uint8)


def resize(frames, out_hw, filt='lanczos', presums=None):
    """frames uint8 [N, H, W, C] -> uint8 [N, out_h, out_w, C].  presums: a dict that receives 'h' / 'v', the sums of
    the pass before the clamp (absent for a skipped pass)."""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.ndim == 4
    N, H, W, C = frames.shape
    out_h, out_w = out_hw
    img = frames
    kv = bv = None
    y0, y1 = 0, H
    if out_h != H:
        kv, bv, _ = tables(H, out_h, filt)
        y0, y1 = int(bv[0, 0]), int(bv[-1, 0] + bv[-1, 1])
    if out_w != W:
        kh, bh, _ = tables(W, out_w, filt)
        store = [] if presums is not None else None
        img = _pass(img[:, y0:y1].astype(np.int64), kh, bh, store)           # [N, y1 - y0, out_w, C]
        if store:
            presums['h'] = store[0]
        if bv is not None:
            bv = bv - np.array([y0, 0])
    elif bv is not None:
        img = img[:, y0:y1]
        bv = bv - np.array([y0, 0])
    if bv is not None:
        store = [] if presums is not None else None
        img = _pass(np.swapaxes(img.astype(np.int64), 1, 2), kv, bv, store)  # along rows: [N, out_w, out_h, C]
        img = np.ascontiguousarray(np.swapaxes(img, 1, 2))
        if store:
            presums['v'] = np.swapaxes(store[0], 1, 2)
    return np.ascontiguousarray(img)


def scaled(images_u8):
    """The loader's np.multiply(images.astype(np.float32), 1.0 / 255.0) (crc_input_data_seq.py:209)."""
    return np.multiply(np.asarray(images_u8).astype(np.float32), 1.0 / 255.0)


def loader_frame_index(n_frames):
    """Every fifth frame from 15 on (crc_input_data_seq.py:186-190)."""
    return np.array([i for i in range(15, int(n_frames), 5)], np.int64)


def loader_images(frames, out_hw=(98, 98), frame_index=None, filt='lanczos'):
    """-> (uint8 [n, oh, ow, 3], float32 [n, oh, ow, 3]) of the selected frames."""
    frames = np.asarray(frames)
    sel = np.arange(len(frames)) if frame_index is None else np.asarray(frame_index, np.int64)
    u8 = resize(frames[sel], out_hw, filt) if len(sel) else np.zeros((0,) + tuple(out_hw) + (3,), np.uint8)
    return u8, scaled(u8)
