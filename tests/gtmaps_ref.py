"""Oracle of the ground-truth gaze maps (include/rgp.h, "ground-truth maps from fixation points"): pure numpy, the
definition taken literally, float64 where the definition says float64.

Two evaluations that share only the filter:
  * packed: from (frame_ptr, samples) as the kernel reads them -- `fixation_counts`;
  * dense: the loader's own route -- a boolean [T, D1, D2] array per observer, np.where, the rescale into a boolean
    [T, S1, S2] array, the frame selection, the sum over observers, the swap of the axes -- `dense_counts`.
`gaussian_filter_f32` restates scipy.ndimage.gaussian_filter on an fp32 frame (tests/test_gtmaps_cpu.py holds it to
scipy bit for bit), `gazemaps_from_counts` is the loader's division, filter and min-max normalisation.
"""
import numpy as np


def gaussian_weights(sigma):
    r = int(4.0 * float(sigma) + 0.5)
    x = np.arange(-r, r + 1)
    w = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2)
    return w / w.sum(), r


def rescale(v, S, D):
    """process_gazemap.py:51-54 for an integer array: multiply, divide, round half to even, + 1e-9, truncate."""
    return (np.round(np.asarray(v).astype(np.float64) * (S - 1.0) / (D - 1.0)) + 1e-9).astype(np.int64)


def reflect_index(j, n):
    """d c b a | a b c d | d c b a, at any distance."""
    m = np.mod(j, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def filter_axis(x32, w, r, axis):
    """correlate1d with a symmetric kernel: fp32 widened to fp64, tmp = c w[r]; tmp += (line[l+i] + line[l-i]) w[i+r]
    for i = -r .. -1 in that order, rounded to fp32."""
    assert x32.dtype == np.float32
    x = np.moveaxis(x32.astype(np.float64), axis, 0)
    n = x.shape[0]
    l = np.arange(n)
    tmp = x * w[r]
    for i in range(-r, 0):
        tmp = tmp + (x[reflect_index(l + i, n)] + x[reflect_index(l - i, n)]) * w[i + r]
    return np.moveaxis(tmp.astype(np.float32), 0, axis)


def gaussian_filter_f32(frame, sigma):
    w, r = gaussian_weights(sigma)
    out = np.ascontiguousarray(frame, np.float32)
    for axis in range(out.ndim):
        out = filter_axis(out, w, r, axis)
    return out


def fixation_counts(frame_ptr, samples, n_observers, raw_shape, out_shape):
    """-> int64 [N, S2, S1]: observers per cell; an observer who hits a cell twice in a frame counts once."""
    (D1, D2), (S1, S2) = raw_shape, out_shape
    N = len(frame_ptr) - 1
    counts = np.zeros((N, S2, S1), np.int64)
    for n in range(N):
        hit = np.zeros((n_observers, S2, S1), bool)
        rows = np.asarray(samples[frame_ptr[n]:frame_ptr[n + 1]]).reshape(-1, 3)
        hit[rows[:, 0], rescale(rows[:, 2], S2, D2), rescale(rows[:, 1], S1, D1)] = True
        counts[n] = hit.sum(0)
    return counts


def dense_counts(observers, frames, raw_shape, out_shape):
    """The loader's route.  observers: (t, a, b, length) per observer kept; frames: the selected frame indices."""
    (D1, D2), (S1, S2) = raw_shape, out_shape
    per_observer = []
    for t, a, b, length in observers:
        raw = np.zeros((length, D1, D2), bool)
        raw[t, a, b] = True
        small = np.zeros((length, S1, S2), bool)
        for tt, x, y in zip(*np.where(raw > 0)):
            y_ = y * (S2 - 1.0) / (D2 - 1.0)
            x_ = x * (S1 - 1.0) / (D1 - 1.0)
            small[tt, int(np.round(x_) + 1e-9), int(np.round(y_) + 1e-9)] = 1
        per_observer.append(small[np.asarray(frames)])
    total = np.sum(np.asarray(per_observer), axis=0)
    return np.swapaxes(total, 1, 2).astype(np.int64)


def gazemaps_from_counts(counts, n_observers, sigma):
    """crc_input_data_seq.py:286-288 with :41-53: -> fp32 [N, S2, S1]."""
    maps = counts.astype(np.float32) / n_observers
    assert maps.dtype == np.float32
    for t in range(len(maps)):
        g = gaussian_filter_f32(maps[t], sigma)
        if g.sum() == 0:
            continue
        g -= np.min(g)
        with np.errstate(invalid='ignore', divide='ignore'):
            g /= np.max(g)
        maps[t] = g
    return maps


def labels64(gazemaps):
    """g / sum(g) per frame, evaluated in float64 (an all-zero frame: NaN)."""
    g = gazemaps.astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        return g / g.reshape(len(g), -1).sum(-1)[:, None, None]
