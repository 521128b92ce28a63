"""Numpy restatement of the reference's gaze-map export arithmetic (extract_map.py:35-41, evaluate_gaze.py:148-152): the
oracle of the export tests.  scipy.misc.bytescale / imresize / imsave left scipy in 1.3, so the recipe is written out,
every step with an explicit cast: nothing here depends on NumPy's promotion rules (the reference ran a NumPy before
NEP 50, where a float64 scalar does not promote an fp32 array).  Written without a look at
recurrent_gaze_prediction_amd/models/extract_map.py.

Per map a [H, W] fp32:
  bytescale  cmin = a.min(), cmax = a.max() (fp32); cscale = cmax - cmin in fp32, 1 if that is 0;
             scale = float32(255.0 / float64(cscale)); b = (a - cmin) * scale, an fp32 subtract and an fp32 multiply (the
             "+ low" that follows adds 0); u = uint8(trunc(clip(b, 0, 255) + 0.5f)), the add in fp32.
             Where 255 / cscale overflows fp32, scale is +inf and a cell equal to cmin is 0 * inf = NaN: clip keeps the
             NaN and the conversion to uint8 of a NaN is what the processor makes of it -- x86's cvttss2si gives
             0x80000000, whose low byte is 0.  The oracle writes that 0 explicitly; every other cell is +inf -> 255.
  imresize   mode 'L', Image.resize((out_w, out_h), filter): Pillow's 8-bit resample of one channel, tests/frames_ref.resize
             (test_export_cpu.py pins it to Pillow at the shapes the GPU test uses).
  normalise  p = float64(resized); p / p.sum(): the sum of integers is exact in any order, the division is IEEE float64;
             a zero sum gives 0 / 0 = NaN in every cell, as NumPy does."""
import numpy as np

import frames_ref


def bytescale(a):
    """One map (or any array scaled as a whole) -> uint8 of the same shape."""
    a = np.asarray(a).astype(np.float32)
    cmin, cmax = np.float32(a.min()), np.float32(a.max())
    with np.errstate(all='ignore'):
        cscale = np.float32(np.float32(cmax) - np.float32(cmin))
        if float(cscale) == 0.0:
            cscale = np.float32(1.0)
        scale = np.float32(255.0 / float(cscale))                       # float64 division, rounded once to fp32
        d = np.subtract(a, cmin, dtype=np.float32)
        b = np.multiply(d, scale, dtype=np.float32)
        nan = np.isnan(b)
        c = np.minimum(np.maximum(np.where(nan, np.float32(0.0), b), np.float32(0.0)), np.float32(255.0)).astype(np.float32)
        t = np.add(c, np.float32(0.5), dtype=np.float32)
    out = np.floor(t).astype(np.int64)                                   # t >= 0.5: floor is trunc
    out[nan] = 0
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def imresize(u8, out_hw, filt='bilinear'):
    """uint8 [n, H, W] -> uint8 [n, out_h, out_w]."""
    u8 = np.asarray(u8)
    if len(u8) == 0:
        return np.zeros((0,) + tuple(out_hw), np.uint8)
    return frames_ref.resize(np.ascontiguousarray(u8[..., None]), tuple(out_hw), filt)[..., 0]


def avg_pool(maps, out_hw=(7, 7), filt='bilinear'):
    """maps fp32 [n, H, W] -> (pooled float64 [n, oh, ow], the resized bytes uint8 [n, oh, ow], the bytescaled maps uint8
    [n, H, W])."""
    maps = np.asarray(maps)
    assert maps.dtype == np.float32 and maps.ndim == 3
    u8 = np.stack([bytescale(m) for m in maps]) if len(maps) else np.zeros(maps.shape, np.uint8)
    small = imresize(u8, out_hw, filt)
    pooled = np.zeros(small.shape, np.float64)
    for i in range(len(small)):
        p = small[i].astype(np.float64)
        s = float(int(small[i].astype(np.int64).sum()))
        with np.errstate(invalid='ignore', divide='ignore'):
            pooled[i] = np.divide(p, np.float64(s))
    return pooled, small, u8


def same_float64(a, b):
    """Bit for bit, NaN cells compared by position."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.int64)[~na], b.view(np.int64)[~nb]))
