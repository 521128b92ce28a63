"""Frames shared by tests/test_metrics_scaled_cpu.py and tests/test_metrics_scaled_gpu.py: maps of one shape,
fixation maps of another, and the host module's scores of them with the numpy spline oracle in place of scipy's.

The CPU test shows that the host module scores these very frames alike with scipy's ``resize`` and with
``spline_ref.resize_fn``; that is what lets the GPU test hold the kernel to the patched host.  A seed is changed
here and nowhere else."""
import functools
import warnings

import numpy as np

from recurrent_gaze_prediction_amd import evaluation_metrics as em
from recurrent_gaze_prediction_amd import evaluation_metrics_gpu as emg

import spline_ref

TOL = 1e-9
# name -> (source shape, target shape, frames, dtype of pred, seed)
CASES = {
    'tiny': ((7, 7), (23, 31), 12, np.float64, 7100),
    'mid64': ((49, 49), (90, 160), 12, np.float64, 7200),
    'mid32': ((49, 49), (90, 160), 12, np.float32, 7300),
    'frame': ((49, 49), (405, 720), 2, np.float32, 7400),
    'wide': ((7, 7), (3, 1600), 6, np.float64, 7500),      # H + W > 1536: the kernel reads its tap tables from global memory
}


def blobs(rs, n, shape):
    """Smooth positive maps: a Gaussian blob per frame on a little noise."""
    h, w = shape
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = rs.uniform(1, h - 2, (n, 1, 1)), rs.uniform(1, w - 2, (n, 1, 1))
    s = max(h, w) / 8.0
    return np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s)) + 0.05 * rs.rand(n, h, w)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict: pred, gt [N,h,w]; fix [N,H,W] float32 0/1; other [H,W] (the union of ten frames); seed.
    Frame 0: one fixation; 1: 256 fixations (2 frames: 40); 2: a fixation in each corner pixel plus three; 3: none;
    4: a prediction without contrast; the others 3 .. 16 random fixations."""
    (h, w), (H, W), N, dtype, seed = CASES[name]
    rs = np.random.RandomState(seed)
    gt = blobs(rs, N, (h, w)).astype(np.float32)
    pred = (gt + 0.3 * rs.rand(N, h, w) + 0.2 * np.roll(gt, 1, axis=2)).astype(dtype)
    fix = np.zeros((N, H * W), np.float32)
    counts = [1, 256, 3, 0, 5] + [int(v) for v in rs.randint(3, 17, max(N - 5, 0))]
    if N == 2:
        counts = [3, 40]
    for i in range(N):
        fix[i, rs.choice(H * W, counts[i], replace=False)] = 1.0
    corners = [0, W - 1, (H - 1) * W, H * W - 1]
    fix[0 if N == 2 else 2, corners] = 1.0
    if N > 4:
        pred[4] = 0.25
    fix = fix.reshape(N, H, W)
    members = rs.choice(N, min(N, 10), replace=False)
    other = (fix[members] > 0).sum(0).astype(np.float64)
    if (other > 0.5).sum() > 4096:
        raise AssertionError('negative set over the cap')
    return dict(pred=pred, gt=gt, fix=fix, other=other, seed=seed + 1, shape=(H, W))


def host_scores(c, metrics, other=None, order='metric', patched=True):
    """The host module on every frame (NaN where it raises: a map without contrast in the two sampled AUCs), consuming
    numpy's global RNG from ``c['seed']``; ``patched``: with the spline oracle in place of scipy's resize.
    other: None (the case's shared set) or one map per frame.  order: 'metric' (metric after metric) or 'frame'."""
    saved = em.resize
    if patched:
        em.resize = spline_ref.resize_fn
    out = {m: np.full(len(c['pred']), np.nan) for m in metrics}

    def one(m, i):
        o = c['other'] if other is None else other[i]
        try:
            out[m][i] = em.saliency_score_single(m, c['pred'][i], c['gt'][i], c['fix'][i], o)
        except ValueError as e:
            assert m in ('AUC_Borji', 'AUC_shuffled') and ('arange' in str(e) or 'zero-size' in str(e)), e
    try:
        np.random.seed(c['seed'])
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            if order == 'metric':
                for m in metrics:
                    for i in range(len(c['pred'])):
                        one(m, i)
            else:
                for i in range(len(c['pred'])):
                    for m in emg.FRAME_METRICS:
                        if m in metrics:
                            one(m, i)
    finally:
        em.resize = saved
    return out


@functools.lru_cache(maxsize=None)
def patched_host(name):
    """The reference of the GPU test, computed once per case."""
    return host_scores(case(name), emg.METRICS)


def assert_close(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, np.isnan(got).nonzero(), np.isnan(want).nonzero())
    err = np.nanmax(np.abs(got - want)) if np.isfinite(want).any() else 0.0
    print('%-34s max |difference| = %.3e over %d frames (%d NaN)' % (what, err, len(want), np.isnan(want).sum()))
    assert err < TOL, (what, err)
