"""The cases of the gaze-map export tests (test_export_cpu.py, test_export_gpu.py): shapes, map counts and inputs, and
the oracle's results for them, computed once per process and handed out read-only.

Shapes: the maps in use (49 x 49, 48 x 48, 14 x 14, 7 x 7) to 7 x 7, one with both passes skipped, one to a single cell
and one non-square.  n in {1, 5, 67}: 67 is no multiple of the 4 maps a workgroup takes, so the last one is part-filled.
Map i of a case is of kind KINDS[i % len(KINDS)], so 67 maps hold every kind about six times with different draws."""
import functools

import numpy as np

import export_ref as ref

SHAPES = [((49, 49), (7, 7)), ((48, 48), (7, 7)), ((14, 14), (7, 7)), ((7, 7), (7, 7)), ((49, 49), (1, 1)), ((49, 48), (7, 3))]
COUNTS = (1, 5, 67)
FILTERS = ('bilinear', 'lanczos', 'bicubic')
TEMPERATURES = (0.25, 1.0, 2.0)
KINDS = ('softmax0', 'softmax1', 'softmax2', 'half_integers', 'negative', 'constant', 'one_hot', 'span_1e30', 'subnormal_entries',
         'subnormal_range')
RANDOM_KINDS = ('softmax0', 'softmax1', 'softmax2')      # test_export_cpu.py asserts a non-zero pooled sum for these
NAN_KINDS = ('constant',)                                # the resized bytes sum to 0 at every shape: NaN in every cell

CASES = [(hw, out, n) for hw, out in SHAPES for n in COUNTS]
IDS = ['%dx%d-%dx%d-n%d' % (hw + out + (n,)) for hw, out, n in CASES]


def kind_of(i):
    return KINDS[i % len(KINDS)]


def one_map(kind, h, w, rs):
    hw = h * w
    if kind.startswith('softmax'):
        z = rs.randn(hw) * TEMPERATURES[int(kind[-1])]
        e = np.exp(z - z.max())
        a = (e / e.sum()).astype(np.float32)
    elif kind == 'half_integers':                         # 49 x 49: cmin 0, cmax 255, scale exactly 1, every .5 tie
        a = ((np.arange(hw) % 511) * 0.5).astype(np.float32)
    elif kind == 'negative':
        a = (rs.randn(hw) * 3.0 - 1.0).astype(np.float32)
    elif kind == 'constant':
        a = np.full(hw, rs.rand() + 0.25, np.float32)
    elif kind == 'one_hot':
        a = np.zeros(hw, np.float32)
        a[rs.randint(hw)] = 1.0
    elif kind == 'span_1e30':
        a = (10.0 ** rs.uniform(-30.0, 0.0, hw)).astype(np.float32)
        a[rs.randint(hw)] = 1.0
    elif kind == 'subnormal_entries':                     # a softmax's tail: half the cells below the least normal fp32
        a = rs.rand(hw).astype(np.float32)
        tiny = rs.rand(hw) < 0.5
        a[tiny] = (10.0 ** rs.uniform(-44.5, -38.5, int(tiny.sum()))).astype(np.float32)
        a[0], a[hw - 1] = np.float32(1e-42), np.float32(1.0)
    elif kind == 'subnormal_range':                       # cmax - cmin is itself a subnormal: 255 / cscale overflows fp32
        a = (rs.randint(0, 1000, hw).astype(np.float64) * 2.0 ** -149).astype(np.float32) + np.float32(2.0 ** -140)
    else:
        raise KeyError(kind)
    return a.reshape(h, w)


@functools.lru_cache(maxsize=None)
def maps(hw, n):
    """fp32 [n, h, w], read-only."""
    h, w = hw
    rs = np.random.RandomState(1000 * h + 10 * w + n)
    out = np.stack([one_map(kind_of(i), h, w, rs) for i in range(n)]).astype(np.float32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle(hw, out, n, filt='bilinear'):
    """(pooled float64, pooled_u8, bytes) of the case, read-only."""
    res = ref.avg_pool(maps(hw, n), out, filt)
    for r in res:
        r.setflags(write=False)
    return res
