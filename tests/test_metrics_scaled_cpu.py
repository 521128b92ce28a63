"""CPU: the ground the frame-resolution scorer stands on (csrc/rgp_metrics_scaled.hip, evaluation_metrics_gpu.py).

* the numpy spline oracle (tests/spline_ref.py, the kernel's order of operations) against scipy;
* the host module scores the GPU test's frames alike with scipy's resize and with the oracle's: the condition that
  lets the GPU test speak for the reference;
* pack_points, fixation_points, the union of ten on point lists, the C entry points' argument checks.
No kernel is launched here."""
import ctypes

import numpy as np
import pytest
import scipy.ndimage
import scipy.sparse
import torch

from recurrent_gaze_prediction_amd import _lib
from recurrent_gaze_prediction_amd import evaluation_metrics as em
from recurrent_gaze_prediction_amd import evaluation_metrics_gpu as emg
from recurrent_gaze_prediction_amd import gazemaps as gm

import gtmaps_ref
import metrics_scaled_cases as cases
import spline_ref

SHAPE_PAIRS = [((7, 7), (23, 31)), ((49, 49), (90, 160)), ((14, 14), (17, 40)), ((49, 49), (7, 9)), ((2, 3), (5, 4)),
               ((49, 49), (405, 720))]


@pytest.mark.parametrize('src, dst', SHAPE_PAIRS)
def test_oracle_equals_scipy(src, dst):
    x = np.random.RandomState(src[0] * 1000 + dst[1]).rand(*src)
    err = np.abs(spline_ref.resize(x, dst) - em.resize(x, dst)).max()
    cerr = np.abs(spline_ref.spline_coefficients(x) - scipy.ndimage.spline_filter(x, 3, mode='reflect')).max()
    print('%s -> %s: resize %.2e, coefficients %.2e' % (src, dst, err, cerr))
    assert err <= 1e-13 and cerr <= 1e-13
    assert np.array_equal(spline_ref.resize_fn(x, src), x)                      # the identity shortcut of the host's resize


def test_tables_are_scipys_taps():
    w, i = spline_ref.resize_tables(49, 720)
    assert w.shape == i.shape == (720, 4) and np.abs(w.sum(1) - 1.0).max() < 1e-15
    assert i.min() == 0 and i.max() == 48 and (i[0] == [1, 0, 0, 1]).all()       # x = -0.466: taps -2 .. 1 reflected
    w2, i2 = spline_ref.resize_tables(2, 5)                                      # the reflection repeats: period 4
    assert set(i2.ravel()) == {0, 1} and (i2[0] == [1, 0, 0, 1]).all() and (i2[4] == [0, 1, 1, 0]).all()


@pytest.mark.parametrize('name', list(cases.CASES))
def test_host_scores_with_the_oracle_swapped_in(name):
    """Every frame of the GPU test, the same seeds, all six metrics: patched host == host within TOL."""
    c = cases.case(name)
    plain = cases.host_scores(c, emg.METRICS, patched=False)
    patched = cases.patched_host(name)
    for m in emg.METRICS:
        cases.assert_close(patched[m], plain[m], '%s %s' % (name, m))
    n_fix = (c['fix'] > 0.5).reshape(len(c['fix']), -1).sum(1)
    if len(n_fix) > 4:
        assert n_fix[0] == 1 and n_fix[1] == 256 and n_fix[3] == 0
        for m in ('AUC_Judd', 'AUC_Borji', 'AUC_shuffled', 'NSS'):
            assert np.isnan(plain[m][3])
        assert np.isfinite(plain['sim'][3]) and np.isfinite(plain['cc'][3])
        assert all(np.isnan(plain[m][4]) for m in ('sim', 'cc', 'AUC_Borji', 'AUC_shuffled', 'NSS'))


def test_pack_points_over_its_input_forms():
    rs = np.random.RandomState(5)
    H, W = 9, 14
    dense = (rs.rand(6, H, W) > 0.9).astype(np.float32)
    dense[2] = 0                                                                 # an empty frame
    ptr, idx = emg.pack_points(dense, (H, W))
    assert ptr.dtype == idx.dtype == np.int32 and ptr[0] == 0 and ptr[-1] == len(idx) and ptr[2] == ptr[3]
    for n in range(6):
        assert np.array_equal(idx[ptr[n]:ptr[n + 1]], np.nonzero(dense[n].ravel())[0])
    tptr, tidx = emg.pack_points(torch.tensor(dense), (H, W))
    assert tptr.dtype == tidx.dtype == torch.int32
    assert np.array_equal(tptr.numpy(), ptr) and np.array_equal(tidx.numpy(), idx)
    sparse = [scipy.sparse.coo_matrix(d) for d in dense]
    sptr, sidx = emg.pack_points(sparse, (H, W))
    assert np.array_equal(sptr, ptr) and np.array_equal(sidx, idx)
    lptr, lidx = emg.pack_points([d for d in dense], (H, W))
    assert np.array_equal(lptr, ptr) and np.array_equal(lidx, idx)
    points = []
    for d in dense:                                                              # unsorted, with duplicates
        r, c = np.nonzero(d)
        order = rs.permutation(len(r))
        points.append((np.concatenate([r[order], r[:2]]), np.concatenate([c[order], c[:2]])))
    pptr, pidx = emg.pack_points(points, (H, W))
    assert np.array_equal(pptr, ptr) and np.array_equal(pidx, idx)
    dup = scipy.sparse.coo_matrix((np.ones(3), ([1, 1, 0], [2, 2, 5])), shape=(H, W))   # a duplicate entry
    assert np.array_equal(emg.pack_points([dup], (H, W))[1], [5, W + 2])
    with pytest.raises(ValueError, match='evaluation_metrics'):
        emg.pack_points(sparse + [scipy.sparse.coo_matrix((H, W + 1))], (H, W))
    with pytest.raises(ValueError, match='evaluation_metrics'):
        emg.pack_points(dense, (H + 1, W))
    with pytest.raises(ValueError, match='outside'):
        emg.pack_points([(np.array([H]), np.array([0]))], (H, W))


def test_union_of_ten_on_points_equals_the_dense_route():
    rs = np.random.RandomState(8)
    H, W = 45, 80
    dense = (rs.rand(14, H, W) > 0.995).astype(np.float32)
    ptr, idx = emg.pack_points(dense, (H, W))
    points = [idx[a:b] for a, b in zip(ptr[:-1], ptr[1:])]
    a, b = np.random.RandomState(3), np.random.RandomState(3)
    for _ in range(5):
        u_dense = emg.union_of_ten([scipy.sparse.coo_matrix(d) for d in dense], a)
        u_points = emg.union_of_ten_points(points, b)
        assert np.array_equal(np.nonzero(u_dense.ravel() > 0.5)[0], u_points)
    assert np.array_equal(a.get_state()[1], b.get_state()[1]) and a.get_state()[2] == b.get_state()[2]


def test_reference_draws_on_points_equal_the_dense_route():
    c = cases.case('tiny')
    pts = emg.pack_points(c['fix'], c['shape'])
    other = emg.pack_points(c['other'][None], c['shape'])
    for order in ('metric', 'frame'):
        np.random.seed(4)
        d = emg.draw_reference_samples(c['fix'], c['other'], emg.METRICS, n_rep=7, order=order)
        s1 = np.random.get_state()[1].copy()
        np.random.seed(4)
        p = emg.draw_reference_samples_points(pts, other, c['shape'], emg.METRICS, n_rep=7, order=order)
        assert np.array_equal(np.random.get_state()[1], s1)
        assert set(d) == set(p) and all(np.array_equal(d[k], p[k]) for k in d)


def test_fixation_points_scatter_to_the_fixation_maps():
    rs = np.random.RandomState(12)
    D1, D2 = 60, 40                                                              # raw extents of a and b
    observers = []
    for k in range(3):
        n = 70
        t = rs.randint(0, 50, n)
        observers.append((t, rs.randint(0, D1, n), rs.randint(0, D2, n), 50))
    packed = gm.pack_fixations(observers, (D1, D2), frames=np.arange(0, 50, 3))
    ptr, idx = gm.fixation_points(packed)
    counts = gtmaps_ref.fixation_counts(packed.frame_ptr, packed.samples, packed.n_observers, (D1, D2), (D1, D2))   # [N, D2, D1]
    assert ptr.dtype == idx.dtype == np.int32 and len(ptr) == len(counts) + 1
    for n in range(len(counts)):
        assert np.array_equal(idx[ptr[n]:ptr[n + 1]], np.nonzero(counts[n].ravel() > 0)[0])
    sptr, sidx = emg.pack_points((counts > 0).astype(np.float32), (D2, D1))
    assert np.array_equal(sptr, ptr) and np.array_equal(sidx, idx)


def test_symbols_and_constants():
    lib = _lib.load()
    for name in ('rgp_metrics_scaled_workspace_bytes', 'rgp_saliency_scores_scaled', 'rgp_spline_resize', 'rgp_spline_resize_workspace_bytes'):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert (_lib.RGP_METRICS_SCALED_MAX_PIX, _lib.RGP_METRICS_SCALED_MAX_OTHER) == (1 << 22, 4096)
    e = 1024 * 100 * 16
    plain = lib.rgp_metrics_scaled_workspace_bytes(1024, 100, 16, 405, 720, 0)
    dev = lib.rgp_metrics_scaled_workspace_bytes(1024, 100, 16, 405, 720, _lib.RGP_METRICS_DEVICE_DRAWS)
    assert plain >= 64 + 2 * e * 8 + (405 + 720) * 40 and dev >= plain + (2 * e + 1024) * 4
    assert lib.rgp_metrics_scaled_workspace_bytes(0, 100, 16, 405, 720, 0) == 0
    assert lib.rgp_spline_resize_workspace_bytes(405, 720) >= (405 + 720) * 40


def good_args(**kw):
    """Arguments that pass every host check; no test here reaches a launch: each case below is refused first."""
    p = 4096
    a = dict(pred=p, gt=p, fix_ptr=p, fix_idx=p, other_ptr=None, other_idx=None, fix_len=10, other_len=0, n_frames=4, height=49,
             width=49, target_height=405, target_width=720, metrics=63, flags=0, n_rep=100, neg_stride=8, step_size=0.1,
             judd_jitter=p, borji_neg=p, shuf_neg=p, shuf_cnt=p, seed=0, offset=0, workspace=p, workspace_bytes=64, scores=p)
    a.update(kw)
    return _lib.MetricsScaledArgs(**a)


@pytest.mark.parametrize('kw, word', [
    (dict(n_frames=0), b'n_frames'),
    (dict(height=1), b'height'),
    (dict(width=1), b'width'),
    (dict(height=65, width=64), b'RGP_METRICS_MAX_PIX'),
    (dict(target_height=0), b'target_height'),
    (dict(target_height=2048, target_width=2049), b'RGP_METRICS_SCALED_MAX_PIX'),
    (dict(neg_stride=257), b'RGP_METRICS_MAX_FIX'),
    (dict(neg_stride=0), b'neg_stride'),
    (dict(step_size=1e-6), b'step_size'),
    (dict(step_size=float('nan')), b'step_size'),
    (dict(n_rep=0), b'n_rep'),
    (dict(pred=None), b'pred'),
    (dict(fix_ptr=None), b'fix_ptr'),
    (dict(fix_idx=None), b'fix_idx'),
    (dict(scores=None), b'scores'),
    (dict(gt=None), b'gt'),
    (dict(fix_len=-1), b'fix_len'),
    (dict(other_ptr=4096), b'other_idx'),
    (dict(borji_neg=None), b'borji_neg'),
    (dict(shuf_cnt=None), b'shuf_cnt'),
    (dict(metrics=0), b'metric'),
    (dict(metrics=64), b'metric'),
    (dict(flags=32), b'flags'),
    (dict(flags=_lib.RGP_METRICS_DEVICE_DRAWS), b'DEVICE_DRAWS'),
    (dict(flags=_lib.RGP_METRICS_DEVICE_DRAWS, judd_jitter=None, borji_neg=None, shuf_neg=None, shuf_cnt=None), b'other_ptr'),
])
def test_scaled_scorer_refuses_bad_arguments_on_the_host(kw, word):
    lib = _lib.load()
    assert lib.rgp_saliency_scores_scaled(ctypes.byref(good_args(**kw)), None) == -1          # RGP_EINVAL
    assert word in lib.rgp_last_error(), lib.rgp_last_error()


def test_workspaces_and_resize_arguments_are_checked_on_the_host():
    lib = _lib.load()
    assert lib.rgp_saliency_scores_scaled(None, None) == -1
    assert lib.rgp_saliency_scores_scaled(ctypes.byref(good_args(workspace=None)), None) == -3    # RGP_EWORKSPACE
    assert lib.rgp_saliency_scores_scaled(ctypes.byref(good_args()), None) == -3                  # 64 bytes are too few
    assert b'workspace' in lib.rgp_last_error()
    p = 4096
    for args, word in (((None, 0, 1, 49, 49, p, 1, 90, 160, p, 1 << 20), b'src'), ((p, 0, 1, 49, 49, None, 1, 90, 160, p, 1 << 20), b'dst'),
                       ((p, 0, 0, 49, 49, p, 1, 90, 160, p, 1 << 20), b'n_frames'), ((p, 0, 1, 1, 49, p, 1, 90, 160, p, 1 << 20), b'height'),
                       ((p, 0, 1, 64, 65, p, 1, 90, 160, p, 1 << 20), b'RGP_METRICS_MAX_PIX'),
                       ((p, 0, 1, 49, 49, p, 1, 0, 160, p, 1 << 20), b'target'),
                       ((p, 0, 1, 49, 49, p, 1, 4096, 1025, p, 1 << 20), b'RGP_METRICS_SCALED_MAX_PIX')):
        assert lib.rgp_spline_resize(*args, None) == -1 and word in lib.rgp_last_error(), (args, lib.rgp_last_error())
    assert lib.rgp_spline_resize(p, 0, 1, 49, 49, p, 1, 90, 160, p, 8, None) == -3


def test_python_entries_refuse_what_the_kernels_do_not_cover():
    c = cases.case('tiny')
    with pytest.raises(ValueError, match='saliency_scores_single'):              # equal shapes are the other kernel's
        emg.saliency_scores_resized(c['pred'], c['gt'], np.zeros((12, 7, 7), np.float32), None, ['sim'])
    with pytest.raises(ValueError, match='differ in shape'):                     # ... which keeps refusing unequal ones
        emg.saliency_scores_single(c['pred'], c['gt'], c['fix'], None, ['sim'])
    with pytest.raises(ValueError, match='RGP_METRICS_MAX_FIX'):
        crowded = np.ones((12, 23, 31), np.float32)
        emg.saliency_scores_resized(c['pred'], c['gt'], crowded, None, ['sim'])
    with pytest.raises(ValueError, match='shape='):
        emg.saliency_scores_resized(c['pred'], c['gt'], emg.pack_points(c['fix'], (23, 31)), None, ['sim'])
    with pytest.raises(ValueError, match='RGP_METRICS_SCALED_MAX_PIX'):
        emg.saliency_scores_resized(c['pred'], c['gt'], (np.zeros(13, np.int32), np.zeros(0, np.int32)), None, ['sim'], shape=(2048, 2049))
    with pytest.raises(ValueError, match='RGP_METRICS_MAX_PIX'):
        emg.resize_maps(np.zeros((1, 65, 64)), (90, 160))
    with pytest.raises(ValueError, match='out_dtype'):
        emg.resize_maps(np.zeros((1, 7, 7)), (9, 9), out_dtype=torch.float16)
