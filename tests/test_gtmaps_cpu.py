"""CPU: the host side of the ground-truth gaze maps (include/rgp.h "ground-truth maps from fixation points",
gazemaps.py): the oracle of tests/gtmaps_ref.py against scipy and against the loader's dense route, pack_fixations,
and the C ABI's argument validation.  No kernel is launched here."""
import ctypes

import numpy as np
import pytest

import gtmaps_ref as ref
from recurrent_gaze_prediction_amd import _lib
from recurrent_gaze_prediction_amd import gazemaps as gm


def random_fixation_frame(rs, shape, n_points, n_observers=5):
    f = np.zeros(shape, np.float32)
    for _ in range(n_points):
        f[rs.randint(shape[0]), rs.randint(shape[1])] += 1.0
    return f / np.float32(n_observers)


# ------------------------------------------------------------------------------------------------ 1. the oracle
@pytest.mark.parametrize('shape, sigma', [((49, 49), 2.0), ((48, 48), 2.0), ((7, 7), 0.3), ((14, 14), 0.6), ((7, 9), 2.0)])
def test_oracle_filter_equals_scipy_bit_for_bit(shape, sigma):
    ndimage = pytest.importorskip('scipy.ndimage')
    rs = np.random.RandomState(shape[0] * 100 + shape[1])
    frames = [random_fixation_frame(rs, shape, rs.randint(1, 12)) for _ in range(6)]
    corners = np.zeros(shape, np.float32)
    corners[0, 0] = corners[-1, -1] = 0.2
    for f in frames + [corners]:
        want = ndimage.gaussian_filter(f, sigma)
        got = ref.gaussian_filter_f32(f, sigma)
        assert want.dtype == got.dtype == np.float32
        assert np.array_equal(want, got), np.abs(want - got).max()
    w, r = gm.gaussian_weights(sigma)
    w_ref, r_ref = ref.gaussian_weights(sigma)
    assert r == r_ref == int(4.0 * sigma + 0.5) and w.dtype == np.float64 and np.array_equal(w, w_ref)


def random_observers(seed, T, raw_shape, n_observers, lengths=None):
    rs = np.random.RandomState(seed)
    out = []
    for k in range(n_observers):
        length = T if lengths is None else lengths[k]
        n = rs.randint(length, 3 * length)
        t = rs.randint(0, length, n)
        a, b = rs.randint(0, raw_shape[0], n), rs.randint(0, raw_shape[1], n)
        if k < 2:       # observers 0 and 1 share a cell in every frame, and hit it twice each (raw rows 8 and 9 -> cell 4)
            every = np.arange(length)
            t, a, b = np.concatenate([t, every, every]), np.concatenate([a, every * 0 + 8, every * 0 + 9]), \
                np.concatenate([b, every * 0 + 20, every * 0 + 20])
        out.append((t, a, b, length))
    return out


def test_packed_oracle_equals_dense_oracle():
    T, raw, out_shape = 40, (97, 61), (49, 49)
    observers = random_observers(7, T, raw, 5)
    for frames in (np.arange(T), 'reference'):
        packed = gm.pack_fixations(observers, raw, frames=frames)
        sel = gm.reference_frames([T] * 5)[2] if isinstance(frames, str) else frames
        assert packed.n_observers == 5 and len(packed.frame_ptr) == len(sel) + 1
        counts = ref.fixation_counts(packed.frame_ptr, packed.samples, 5, raw, out_shape)
        dense = ref.dense_counts(observers, sel, raw, out_shape)
        assert counts.shape == (len(sel), 49, 49) and counts.max() >= 2
        assert np.array_equal(counts, dense)
        assert np.array_equal(ref.gazemaps_from_counts(counts, 5, 2.0), ref.gazemaps_from_counts(dense, 5, 2.0))
    assert list(sel) == [15, 20, 25]


# ------------------------------------------------------------------------------------------------ 2. pack_fixations
def frame_rows(packed, n):
    return sorted(map(tuple, packed.samples[packed.frame_ptr[n]:packed.frame_ptr[n + 1]].tolist()))


def test_pack_reference_frame_selection_and_short_observer():
    # recordings of 36, 31 and 25 frames: gazelen = max(36, 31) - 10 = 26, frames 15 and 20 and 25, the third observer
    # (25 < 26 frames) is dropped and the divisor is 2
    o0 = ([15, 15, 20, 3], [1, 2, 3, 9], [4, 5, 6, 9], 36)
    o1 = ([25, 20, 14], [7, 8, 0], [1, 2, 0], 31)
    o2 = ([15, 20], [5, 5], [5, 5], 25)
    gazelen, keep, sel = gm.reference_frames([36, 31, 25])
    assert (gazelen, keep, list(sel)) == (26, [0, 1], [15, 20, 25])
    p = gm.pack_fixations([o0, o1, o2], (10, 10))
    assert p.n_observers == 2 and p.raw_shape == (10, 10)
    assert p.frame_ptr.dtype == np.int32 and p.samples.dtype == np.int32 and list(p.frame_ptr) == [0, 2, 4, 5]
    assert frame_rows(p, 0) == [(0, 1, 4), (0, 2, 5)]
    assert frame_rows(p, 1) == [(0, 3, 6), (1, 8, 2)]
    assert frame_rows(p, 2) == [(1, 7, 1)]
    # an observer exactly gazelen frames long is kept (len > gazelen - 1)
    assert gm.reference_frames([36, 31, 26])[1] == [0, 1, 2]
    # too short for a single selected frame: no frames, not an error
    assert list(gm.pack_fixations([([0], [1], [1], 20), ([0], [1], [1], 20)], (10, 10)).frame_ptr) == [0]


def test_pack_explicit_frames():
    o0 = ([0, 2, 2, 5], [1, 2, 3, 4], [1, 2, 3, 4], 6)
    o1 = ([2, 7], [9, 8], [9, 8], 8)
    p = gm.pack_fixations([o0, o1], (10, 10), frames=[2, 7, 1, 2])
    assert p.n_observers == 2 and list(p.frame_ptr) == [0, 3, 4, 4, 7]
    assert frame_rows(p, 0) == frame_rows(p, 3) == [(0, 2, 2), (0, 3, 3), (1, 9, 9)]
    assert frame_rows(p, 1) == [(1, 8, 8)] and frame_rows(p, 2) == []
    with pytest.raises(ValueError):
        gm.pack_fixations([o0], (10, 10), frames=[-1])
    with pytest.raises(ValueError):
        gm.pack_fixations([([6], [1], [1], 6)], (10, 10), frames=[0])           # a sample past the recording
    with pytest.raises(ValueError):
        gm.pack_fixations([([1], [10], [1], 6)], (10, 10), frames=[0])          # a sample outside the raw frame
    with pytest.raises(ValueError):
        gm.pack_fixations([o0], (10, 10), frames='all')


def test_pack_fill_missing():
    # observer 0 has samples in frames 2 and 5 only: frames 0, 1 take frame 2's (the frame-0 case and its chain), 3 and 4
    # take frame 2's, 6 and 7 frame 5's; observer 1 has no sample at all and stays empty
    o0 = ([2, 5, 2], [1, 4, 2], [1, 4, 2], 8)
    o1 = ([], [], [], 8)
    p = gm.pack_fixations([o0, o1], (10, 10), frames=np.arange(8), fill_missing=True)
    two, five = [(0, 1, 1), (0, 2, 2)], [(0, 4, 4)]
    assert [frame_rows(p, n) for n in range(8)] == [two, two, two, two, two, five, five, five]
    assert p.n_observers == 2 and p.frame_ptr[-1] == len(p.samples) == 13
    q = gm.pack_fixations([o0, o1], (10, 10), frames=np.arange(8))
    assert [frame_rows(q, n) for n in range(8)] == [[], [], two, [], [], five, [], []]
    # against the loader's loop on a dense array (add_gazemap.py:57-74: frame 0 from the first later frame, the others
    # from the nearest earlier one)
    dense = np.zeros((8, 10, 10), int)
    dense[[2, 5, 2], [1, 4, 2], [1, 4, 2]] = 1
    j = 1
    while dense[0].sum() == 0:
        dense[0] = dense[j]
        j += 1
    for i in range(1, 8):
        j = i - 1
        while dense[i].sum() == 0:
            dense[i] = dense[j]
            j -= 1
    for n in range(8):
        assert sorted(zip(*np.nonzero(dense[n]))) == [(a, b) for _, a, b in frame_rows(p, n)]


# ------------------------------------------------------------------------------------------------ 3. the C ABI
def test_symbols_are_exported_and_bound():
    lib = _lib.load()
    for name in ('rgp_gtmaps_workspace_bytes', 'rgp_gazemaps_from_fixations', 'rgp_gtmaps_status'):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.rgp_gtmaps_workspace_bytes() == 64
    assert (_lib.RGP_GTMAPS_MAX_PIX, _lib.RGP_GTMAPS_MAX_OBSERVERS, _lib.RGP_GTMAPS_MAX_RADIUS) == (4096, 32, 32)
    assert gm.SIGMA_FOR_SHAPE == {(49, 49): 2.0, (48, 48): 2.0, (14, 14): 0.6, (7, 7): 0.3}


def good_args(**kw):
    """Arguments that pass every host check (the pointers are never dereferenced on the host; no test here reaches a
    launch: each case below is refused first, or has no frame)."""
    p = 4096       # any non-NULL, 8-byte aligned value
    a = dict(frame_ptr=p, samples=p, weights=p, n_frames=4, n_observers=5, raw_d1=97, raw_d2=61, out_s1=49, out_s2=49, radius=8,
             gazemaps=p, fixationmaps=p, labels=p, workspace=p, workspace_bytes=64)
    a.update(kw)
    return _lib.GtmapsArgs(**a)


@pytest.mark.parametrize('kw, word', [
    (dict(n_frames=-1), b'n_frames'),
    (dict(frame_ptr=None), b'frame_ptr'),
    (dict(samples=None), b'samples'),
    (dict(weights=None), b'weights'),
    (dict(gazemaps=None, fixationmaps=None, labels=None), b'gazemaps, fixationmaps and labels'),
    (dict(n_observers=0), b'n_observers'),
    (dict(n_observers=-2), b'n_observers'),
    (dict(n_observers=33), b'RGP_GTMAPS_MAX_OBSERVERS'),
    (dict(raw_d1=1), b'raw_d1'),
    (dict(raw_d2=1), b'raw_d2'),
    (dict(raw_d2=-5), b'raw_d2'),
    (dict(out_s1=65, out_s2=64), b'RGP_GTMAPS_MAX_PIX'),
    (dict(out_s1=0), b'out_s1'),
    (dict(out_s2=-1), b'out_s2'),
    (dict(out_s1=65536, out_s2=65536), b'RGP_GTMAPS_MAX_PIX'),            # the product does not wrap
    (dict(radius=33), b'RGP_GTMAPS_MAX_RADIUS'),
    (dict(radius=-1), b'radius'),
    (dict(workspace=None), b'workspace'),
    (dict(workspace_bytes=8), b'workspace'),
    (dict(workspace=4100), b'workspace'),                                   # misaligned
])
def test_bad_arguments_are_refused_on_the_host(kw, word):
    lib = _lib.load()
    assert lib.rgp_gazemaps_from_fixations(ctypes.byref(good_args(**kw)), None) == -1          # RGP_EINVAL
    assert word in lib.rgp_last_error(), lib.rgp_last_error()


def test_null_args_and_no_frames():
    lib = _lib.load()
    assert lib.rgp_gazemaps_from_fixations(None, None) == -1 and b'args' in lib.rgp_last_error()
    assert lib.rgp_gtmaps_status(None, None) == -1 and b'workspace' in lib.rgp_last_error()
    # n_frames == 0: RGP_OK, nothing is launched (and nothing else is looked at)
    assert lib.rgp_gazemaps_from_fixations(ctypes.byref(good_args(n_frames=0)), None) == 0
    assert lib.rgp_gazemaps_from_fixations(ctypes.byref(good_args(n_frames=0, gazemaps=None, fixationmaps=None, labels=None,
                                                                  workspace=None)), None) == 0


def test_python_entry_refuses_what_the_kernel_does_not_cover():
    packed = gm.PackedFixations(np.zeros(2, np.int32), np.zeros((0, 3), np.int32), 5, (97, 61))
    with pytest.raises(ValueError, match='RGP_GTMAPS_MAX_PIX'):
        gm.gazemaps_from_fixations(packed, out_shape=(405, 720), sigma=19)             # the original-scale path
    with pytest.raises(ValueError, match='RGP_GTMAPS_MAX_RADIUS'):
        gm.gazemaps_from_fixations(packed, out_shape=(49, 49), sigma=19)
    with pytest.raises(ValueError, match='sigma'):
        gm.gazemaps_from_fixations(packed, out_shape=(20, 20))
    with pytest.raises(ValueError, match='RGP_GTMAPS_MAX_OBSERVERS'):
        gm.gazemaps_from_fixations(packed._replace(n_observers=33))
    with pytest.raises(ValueError, match='want'):
        gm.gazemaps_from_fixations(packed, want=('heatmaps',))
    with pytest.raises(ValueError, match='frame_ptr'):
        gm.gazemaps_from_fixations(packed._replace(frame_ptr=np.array([0, 3], np.int32)))
