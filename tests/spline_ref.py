"""numpy oracle of the device's cubic-spline resize (csrc/rgp_metrics_scaled.hip), statement for statement.

``evaluation_metrics.resize`` is ``scipy.ndimage.map_coordinates(order=3, mode='reflect')`` on a pixel-centre grid.
Restated: scipy's recursive B-spline prefilter (pole sqrt(3) - 2, exact 'reflect' initialisation) along axis 0 and
then axis 1, then per target pixel a 16-term sum over the taps floor(x) - 1 .. floor(x) + 2 with reflected indices.
Everything here is an element-wise numpy multiply, add, subtract or divide in float64, in the kernel's order
(``filter_line`` / ``spline_at`` there), so kernel and oracle hold the same bits; against scipy the restatement
agrees to about 2e-15 (tests/test_metrics_scaled_cpu.py).  No ``**``, no dot products, nothing that could fuse.
"""
import numpy as np


def pole_constants(n):
    """(z, z^n, gain, z / (1 - z^n z^n), z / (z - 1)) for lines of n samples; z^n as n - 1 multiplies."""
    z = np.sqrt(np.float64(3.0)) - np.float64(2.0)
    zn = z
    for _ in range(1, n):
        zn = zn * z
    one = np.float64(1.0)
    return z, zn, (one - z) * (one - one / z), z / (one - zn * zn), z / (z - one)


def _filter_axis0(c):
    """The prefilter along axis 0 of a float64 array, all lines at once (the lines are independent)."""
    n = c.shape[0]
    z, zn, gain, k0, last = pole_constants(n)
    c = c * gain
    c0 = c[0].copy()
    acc = c0 + zn * c[n - 1]
    zi = z
    for i in range(1, n):
        mirrored = acc if i == n - 1 else c[n - 1 - i]         # scipy accumulates in c[0] itself
        acc = acc + zi * (c[i] + zn * mirrored)
        zi = zi * z
    acc = acc * k0
    acc = acc + c0
    c[0] = acc
    for i in range(1, n):
        c[i] = c[i] + z * c[i - 1]
    c[n - 1] = c[n - 1] * last
    for i in range(n - 2, -1, -1):
        c[i] = z * (c[i + 1] - c[i])
    return c


def spline_coefficients(img):
    """B-spline coefficients of a 2-D map (scipy.ndimage.spline_filter(img, 3, mode='reflect')): axis 0, then axis 1."""
    c = np.array(img, dtype=np.float64)
    assert c.ndim == 2 and min(c.shape) >= 2
    with np.errstate(all='ignore'):
        c = _filter_axis0(c)
        c = np.ascontiguousarray(_filter_axis0(np.ascontiguousarray(c.T)).T)
    return c


def resize_tables(n_in, n_out):
    """(weights float64 [n_out, 4], indices int64 [n_out, 4]) of one axis: the taps of every target coordinate."""
    x = (np.arange(n_out) + 0.5) * (float(n_in) / n_out) - 0.5
    f = np.floor(x)
    t = x - f
    u = 1.0 - t
    w = np.stack([u * u * u / 6.0, (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0, (u * u * (u - 2.0) * 3.0 + 4.0) / 6.0, t * t * t / 6.0],
                 axis=1)
    i = f.astype(np.int64)[:, None] + np.arange(-1, 3)[None, :]
    i = np.where(i < 0, -i - 1, i)
    i = i % (2 * n_in)
    i = np.where(i >= n_in, 2 * n_in - 1 - i, i)
    return w, i


def resize(img, out_shape):
    """The resized map, float64 [H, W]: rows outer, each row's four column taps summed left to right first."""
    c = spline_coefficients(img)
    H, W = (int(v) for v in out_shape)
    wy, iy = resize_tables(c.shape[0], H)
    wx, ix = resize_tables(c.shape[1], W)
    out = None
    with np.errstate(all='ignore'):
        for a in range(4):
            rows = c[iy[:, a]]                                   # [H, w]
            s = wx[None, :, 0] * rows[:, ix[:, 0]]
            for b in range(1, 4):
                s = s + wx[None, :, b] * rows[:, ix[:, b]]
            out = wy[:, a, None] * s if a == 0 else out + wy[:, a, None] * s
    return out


def resize_fn(image, output_shape, order=3, mode='reflect'):
    """Drop-in for ``evaluation_metrics.resize`` (identity at equal shapes included)."""
    assert order == 3 and mode == 'reflect'
    image = np.asarray(image, dtype=np.float64)
    output_shape = tuple(int(s) for s in output_shape)
    if image.shape == output_shape:
        return image.copy()
    return resize(image, output_shape)
