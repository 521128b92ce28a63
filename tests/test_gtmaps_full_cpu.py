"""CPU: the host side of the original-scale ground-truth maps (include/rgp.h "ground-truth maps at the frame's
resolution", gazemaps.gazemaps_original_scale): the oracle of tests/gtmaps_ref.py against scipy at every shape and sigma
the GPU test uses, the kernels' zero skipping restated in numpy against the full oracle, and the C ABI's limits,
workspace query and argument validation.  No kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest

import gtmaps_full_cases as cases
import gtmaps_ref as ref
from recurrent_gaze_prediction_amd import _lib
from recurrent_gaze_prediction_amd import gazemaps as gm

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'rgp.h')


# ------------------------------------------------------------------------------------------------ 1. the oracle
@pytest.mark.parametrize('name', cases.ORACLE_CASES)
def test_oracle_filter_equals_scipy_bit_for_bit(name):
    ndimage = pytest.importorskip('scipy.ndimage')
    p, sigma = cases.case(name)
    maps = cases.counts(name).astype(np.float32) / p.n_observers
    assert maps.dtype == np.float32
    for f in np.unique(maps, axis=0):
        want = ndimage.gaussian_filter(f, sigma)
        got = ref.gaussian_filter_f32(f, sigma)
        assert want.dtype == got.dtype == np.float32
        assert np.array_equal(want, got), np.abs(want - got).max()
    w, r = gm.gaussian_weights(sigma)
    w_ref, r_ref = ref.gaussian_weights(sigma)
    assert r == r_ref == int(4.0 * sigma + 0.5) and np.array_equal(w, w_ref)


def test_the_cases_are_what_they_are_for():
    assert gm.SIGMA_ORIGINAL_SCALE == 19 and gm.gaussian_weights(19)[1] == 76 == _lib.RGP_GTMAPS_FULL_LDS_RADIUS
    assert gm.gaussian_weights(cases.SIGMA_ABOVE_LDS)[1] == 160 > _lib.RGP_GTMAPS_FULL_LDS_RADIUS
    assert cases.RAW[1] < 76 < cases.RAW[0]
    assert cases.TILE_RAW[0] % _lib.RGP_GTMAPS_FULL_TILE_COLS == 1 and cases.TILE_RAW[1] % _lib.RGP_GTMAPS_FULL_TILE_ROWS == 1
    for n_obs in (1, 5, 32):
        fix, gaze = cases.oracle('obs%d' % n_obs)
        assert fix[cases.EMPTY].sum() == 0 and fix[cases.ONE].sum() == 1 and fix[cases.SHARED].max() == n_obs
        assert fix[cases.TWICE].max() == 1 and fix[cases.TWICE].sum() == 2
        assert all(fix[cases.CORNERS][y, x] >= 1 for y in (0, -1) for x in (0, -1))
        assert gaze[cases.EMPTY].max() == 0 and gaze[cases.ONE].max() == 1 and not np.isnan(gaze).any()
        p = cases.fixations(n_obs)
        assert p.frame_ptr[cases.MANY + 1] - p.frame_ptr[cases.MANY] == 300
    # 2 x 2, one observer, 300 samples: every cell is hit, the frame is constant and non-zero: NaN, as numpy
    assert np.isnan(cases.oracle('tiny22')[1][cases.MANY]).all() and cases.oracle('tiny22')[0][cases.MANY].min() == 1
    fix, gaze = cases.oracle('workload')
    assert fix.shape == (3, 405, 720) and [int(f.sum()) for f in fix] == [0, 1, 16] and gaze[1, 0, 719] == 1


# ------------------------------------------------------------------------------------------------ 2. the zero skipping
def sparse_axis_sum(x32, w, r, line_flag):
    """correlate1d along axis 0 of x32 [n, m], forming only the terms the LDS kernels form: the term of distance d enters
    output l when line l - d or line l + d (reflected) is flagged, in scipy's order, farthest first; a line that is not
    flagged is never read (a +0 stands in for it)."""
    x = np.where(line_flag[:, None], x32.astype(np.float64), 0.0)
    n = x.shape[0]
    l = np.arange(n)
    tmp = x * w[r]
    for i in range(-r, 0):
        lo, hi = ref.reflect_index(l + i, n), ref.reflect_index(l - i, n)
        formed = line_flag[lo] | line_flag[hi]
        tmp = np.where(formed[:, None], tmp + (x[lo] + x[hi]) * w[i + r], tmp)
    return tmp.astype(np.float32), formed


def filter_with_the_lds_kernels_skips(frame, w, r, strip_cols):
    """csrc/rgp_gtmaps_full.hip at a radius the LDS tiles hold.  Pass 1, per strip of `strip_cols` columns: a strip
    without a sample is +0; otherwise a row is flagged if it has a sample within the strip.  Pass 2: a column is flagged
    if it has a sample anywhere in the frame.  -> (maps, terms formed, terms of the full sums)"""
    D2, D1 = frame.shape
    has_sample = (frame != 0).any(axis=0)
    plane = np.zeros((D2, D1), np.float32)
    formed = 0
    for x0 in range(0, D1, strip_cols):
        strip = frame[:, x0:x0 + strip_cols]
        if not has_sample[x0:x0 + strip_cols].any():
            continue
        row_flag = (strip != 0).any(axis=1)
        plane[:, x0:x0 + strip_cols], _ = sparse_axis_sum(np.ascontiguousarray(strip), w, r, row_flag)
        formed += int(sum((row_flag[ref.reflect_index(np.arange(D2) + i, D2)] | row_flag[ref.reflect_index(np.arange(D2) - i, D2)]).sum()
                          for i in range(-r, 0))) * strip.shape[1]
    out_t, _ = sparse_axis_sum(np.ascontiguousarray(plane.T), w, r, has_sample)
    formed += int(sum((has_sample[ref.reflect_index(np.arange(D1) + i, D1)] | has_sample[ref.reflect_index(np.arange(D1) - i, D1)]).sum()
                      for i in range(-r, 0))) * D2
    return np.ascontiguousarray(out_t.T), formed, 2 * r * D1 * D2


def filter_with_the_direct_kernels_skips(frame, w, r, tile_cols):
    """The same file above RGP_GTMAPS_FULL_LDS_RADIUS: pass 1 leaves a column without a sample at +0; pass 2 leaves a
    tile of `tile_cols` columns at +0 if none of the columns its taps reach (its own and its halo's, reflected) has a
    sample, and otherwise forms the whole sums."""
    D2, D1 = frame.shape
    has_sample = (frame != 0).any(axis=0)
    plane = np.zeros((D2, D1), np.float32)
    plane[:, has_sample] = ref.filter_axis(np.ascontiguousarray(frame[:, has_sample]), w, r, 0)
    out = np.zeros((D2, D1), np.float32)
    skipped = 0
    for x0 in range(0, D1, tile_cols):
        T = min(tile_cols, D1 - x0)
        staged_cols = ref.reflect_index(np.arange(x0 - r, x0 + tile_cols + r), D1)
        if not has_sample[staged_cols].any():
            skipped += 1
            continue
        s = plane[:, staged_cols].astype(np.float64)
        tmp = s[:, r:r + T] * w[r]
        for i in range(-r, 0):
            tmp = tmp + (s[:, r + i:r + i + T] + s[:, r - i:r - i + T]) * w[i + r]
        out[:, x0:x0 + T] = tmp.astype(np.float32)
    return out, int((~has_sample).sum()), skipped


@pytest.mark.parametrize('name', ['obs5', 'odd', 'tile_plus_one', 'tiny53'])
def test_skipping_zero_terms_changes_no_bit(name):
    """Every term is >= +0 and x + (+0.0) == x: what the kernels leave out is +0 in the full oracle, sign included.  Held
    at every strip / tile width that divides RGP_GTMAPS_FULL_TILE_COLS, so it follows a change of tiling; both rule
    sets are held at every case, whatever path its radius takes on the device."""
    p, sigma = cases.case(name)
    w, r = ref.gaussian_weights(sigma)
    maps = np.unique(cases.counts(name).astype(np.float32) / p.n_observers, axis=0)
    formed = full_terms = cols_skipped = tiles_skipped = 0
    for f in maps:
        full = ref.gaussian_filter_f32(f, sigma)
        assert not np.signbit(full).any()
        for width in (16, 32, 64, _lib.RGP_GTMAPS_FULL_TILE_COLS):
            got, n_formed, n_full = filter_with_the_lds_kernels_skips(f, w, r, width)
            assert np.array_equal(got, full) and not np.signbit(got).any(), (name, width)
            formed += n_formed
            full_terms += n_full
            got, c, t = filter_with_the_direct_kernels_skips(f, w, r, width)
            assert np.array_equal(got, full) and not np.signbit(got).any(), (name, width)
            cols_skipped += c
            tiles_skipped += t
    print('%s: %d of %d terms formed, %d columns and %d tiles skipped' % (name, formed, full_terms, cols_skipped, tiles_skipped))
    assert formed < full_terms and cols_skipped > 0
    if name == 'odd':               # sigma 5 on 257 columns: some 16-column tiles are further than 20 from every sample
        assert tiles_skipped > 0


# ------------------------------------------------------------------------------------------------ 3. the C ABI
def header_defines():
    with open(HEADER) as f:
        text = f.read()
    return {k: eval(v) for k, v in re.findall(r'#define (RGP_GTMAPS_FULL_\w+) (\(?[0-9 <]+\)?)\s', text)}


def test_symbols_limits_and_tile_constants():
    lib = _lib.load()
    for name in ('rgp_gtmaps_full_workspace_bytes', 'rgp_gazemaps_full_from_fixations', 'rgp_gtmaps_full_status'):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert (_lib.RGP_GTMAPS_FULL_MAX_PIX, _lib.RGP_GTMAPS_FULL_MAX_RADIUS) == (2 ** 22, 256)
    assert _lib.RGP_GTMAPS_FULL_MAX_PIX == _lib.RGP_METRICS_SCALED_MAX_PIX >= 1080 * 1920
    assert header_defines() == {k: getattr(_lib, k) for k in ('RGP_GTMAPS_FULL_MAX_PIX', 'RGP_GTMAPS_FULL_MAX_RADIUS',
                                                              'RGP_GTMAPS_FULL_LDS_RADIUS', 'RGP_GTMAPS_FULL_TILE_COLS',
                                                              'RGP_GTMAPS_FULL_TILE_ROWS')}
    assert gm.SIGMA_ORIGINAL_SCALE == 19 and gm.SIGMA_FOR_SHAPE == {(49, 49): 2.0, (48, 48): 2.0, (14, 14): 0.6, (7, 7): 0.3}
    # the old entry keeps its limits
    assert (_lib.RGP_GTMAPS_MAX_PIX, _lib.RGP_GTMAPS_MAX_OBSERVERS, _lib.RGP_GTMAPS_MAX_RADIUS) == (4096, 32, 32)


def test_workspace_query():
    q = _lib.load().rgp_gtmaps_full_workspace_bytes
    base = q(4, 720, 405)
    assert base >= 64 + 4 * 720 * 405 * 8 and base < 64 + 4 * 720 * 405 * 8 + 4096        # two 4-byte planes per frame and a small head
    assert q(5, 720, 405) > base and q(4, 721, 405) > base and q(4, 720, 406) > base     # grows with every argument
    assert q(0, 720, 405) >= 64
    # the largest arguments do not wrap: 2^31 - 1 frames of 2^22 cells are 2^56 bytes and more
    big = q(2 ** 31 - 1, 2048, 2048)
    assert big >= (2 ** 31 - 1) * 2 ** 22 * 8 and big < 2 ** 57
    assert q(2 ** 31 - 1, 2 ** 21, 2) >= (2 ** 31 - 1) * 2 ** 22 * 8
    # 0 for what the entry refuses
    for bad in ((-1, 720, 405), (4, 1, 405), (4, 720, 1), (4, 2049, 2048), (4, 65536, 65536), (4, -720, -405)):
        assert q(*bad) == 0, bad


def good_args(**kw):
    """Arguments that pass every host check (the pointers are never dereferenced on the host; no test here reaches a
    launch: each case below is refused first, or has no frame)."""
    p = 4096       # any non-NULL, 8-byte aligned value
    a = dict(frame_ptr=p, samples=p, weights=p, n_frames=4, n_observers=5, raw_d1=97, raw_d2=61, radius=76, gazemaps=p,
             fixationmaps=p, workspace=p, workspace_bytes=1 << 30)
    a.update(kw)
    return _lib.GtmapsFullArgs(**a)


@pytest.mark.parametrize('kw, word', [
    (dict(n_frames=-1), b'n_frames'),
    (dict(frame_ptr=None), b'frame_ptr'),
    (dict(samples=None), b'samples'),
    (dict(weights=None), b'weights'),
    (dict(gazemaps=None, fixationmaps=None), b'gazemaps and fixationmaps'),
    (dict(n_observers=0), b'n_observers'),
    (dict(n_observers=-2), b'n_observers'),
    (dict(n_observers=33), b'RGP_GTMAPS_MAX_OBSERVERS'),
    (dict(raw_d1=1), b'raw_d1'),
    (dict(raw_d2=1), b'raw_d2'),
    (dict(raw_d2=-5), b'raw_d2'),
    (dict(raw_d1=2049, raw_d2=2048), b'RGP_GTMAPS_FULL_MAX_PIX'),
    (dict(raw_d1=65536, raw_d2=65536), b'RGP_GTMAPS_FULL_MAX_PIX'),            # the product does not wrap
    (dict(radius=257), b'RGP_GTMAPS_FULL_MAX_RADIUS'),
    (dict(radius=-1), b'radius'),
    (dict(workspace=None), b'workspace'),
    (dict(workspace_bytes=64), b'workspace'),                                  # the old entry's size is short here
    (dict(workspace=4100), b'workspace'),                                       # misaligned
    (dict(n_frames=2 ** 31 - 1, raw_d1=2048, raw_d2=2048, workspace_bytes=2 ** 62), b'n_frames'),    # too many workgroups
])
def test_bad_arguments_are_refused_on_the_host(kw, word):
    lib = _lib.load()
    assert lib.rgp_gazemaps_full_from_fixations(ctypes.byref(good_args(**kw)), None) == -1          # RGP_EINVAL
    assert word in lib.rgp_last_error(), lib.rgp_last_error()


def test_workspace_one_byte_short_is_refused():
    lib = _lib.load()
    need = lib.rgp_gtmaps_full_workspace_bytes(4, 97, 61)
    assert lib.rgp_gazemaps_full_from_fixations(ctypes.byref(good_args(workspace_bytes=need - 1)), None) == -1
    assert b'workspace' in lib.rgp_last_error()


def test_null_args_and_no_frames():
    lib = _lib.load()
    assert lib.rgp_gazemaps_full_from_fixations(None, None) == -1 and b'args' in lib.rgp_last_error()
    assert lib.rgp_gtmaps_full_status(None, None, None) == -1 and b'workspace' in lib.rgp_last_error()
    # n_frames == 0: RGP_OK, nothing is launched (and nothing else is looked at)
    assert lib.rgp_gazemaps_full_from_fixations(ctypes.byref(good_args(n_frames=0)), None) == 0
    assert lib.rgp_gazemaps_full_from_fixations(ctypes.byref(good_args(n_frames=0, gazemaps=None, fixationmaps=None,
                                                                       workspace=None)), None) == 0


def test_python_entry_refuses_what_the_kernels_do_not_cover():
    packed = gm.PackedFixations(np.zeros(2, np.int32), np.zeros((0, 3), np.int32), 5, (97, 61))
    with pytest.raises(ValueError, match='labels'):
        gm.gazemaps_original_scale(packed, want=('gazemaps', 'labels'))
    with pytest.raises(ValueError, match='want'):
        gm.gazemaps_original_scale(packed, want=())
    with pytest.raises(ValueError, match='RGP_GTMAPS_FULL_MAX_PIX'):
        gm.gazemaps_original_scale(packed._replace(raw_shape=(2049, 2048)))
    with pytest.raises(ValueError, match='RGP_GTMAPS_FULL_MAX_RADIUS'):
        gm.gazemaps_original_scale(packed, sigma=65)                                   # radius 260
    with pytest.raises(ValueError, match='sigma'):
        gm.gazemaps_original_scale(packed, sigma=0)
    with pytest.raises(ValueError, match='RGP_GTMAPS_MAX_OBSERVERS'):
        gm.gazemaps_original_scale(packed._replace(n_observers=33))
    with pytest.raises(ValueError, match='at least 2'):
        gm.gazemaps_original_scale(packed._replace(raw_shape=(97, 1)))
    with pytest.raises(ValueError, match='frame_ptr'):
        gm.gazemaps_original_scale(packed._replace(frame_ptr=np.array([0, 3], np.int32)))
    with pytest.raises(ValueError, match='frames_per_call'):
        gm.gazemaps_original_scale(packed, frames_per_call=0)
    # the old entry still refuses this size
    with pytest.raises(ValueError, match='RGP_GTMAPS_MAX_PIX'):
        gm.gazemaps_from_fixations(packed, out_shape=(405, 720), sigma=19)
