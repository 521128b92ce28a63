"""GPU: the ground-truth gaze-map kernel (csrc/rgp_gtmaps.hip through gazemaps.py) against the numpy oracle of
tests/gtmaps_ref.py, which tests/test_gtmaps_cpu.py pins to scipy and to the loader's dense route.

Every operation behind `fixationmaps` and `gazemaps` is IEEE, element-wise, or a sum in a prescribed order, with
host-made weights: the claim is equality, not a tolerance.  `labels` has one sum whose order is the kernel's own: it is
held to 2^-22 relative per element against g / sum(g) in float64 (one fp32 rounding of the sum and one of the quotient,
2^-23 together, doubled for margin).

N = 24 frames, raw 97 x 61.  To 49 x 49, a * 48 / 96 ties at every odd a, which exercises round-half-to-even."""
import functools

import numpy as np
import pytest
import torch

import gtmaps_ref as ref
from recurrent_gaze_prediction_amd import _lib
from recurrent_gaze_prediction_amd import gazemaps as gm
from recurrent_gaze_prediction_amd import synthetic as syn

pytestmark = pytest.mark.gpu

RAW = (97, 61)
N = 24
SHAPES = [((49, 49), 2.0), ((48, 48), 2.0), ((14, 14), 0.6), ((7, 7), 0.3), ((7, 9), 2.0)]
OBSERVERS = [1, 5, 32]
EMPTY, ONE, TWICE, SHARED, CORNERS, MANY = 0, 1, 2, 3, 4, 5            # the frames made by construction


@functools.lru_cache(maxsize=None)
def fixations(n_obs):
    """24 frames of samples (observer, a, b), raw 97 x 61."""
    rs = np.random.RandomState(100 + n_obs)
    last = n_obs - 1
    frames = [[] for _ in range(N)]
    frames[ONE] = [(last, 33, 17)]
    frames[TWICE] = [(0, 8, 20), (0, 8, 20), (0, 9, 20), (last, 50, 3)]        # rows 8 and 9 share a cell at 49: 4.5 -> 4
    frames[SHARED] = [(u, 41, 30) for u in range(n_obs)] + [(0, 96, 0)]
    corners = [(0, 0), (96, 0), (0, 60), (96, 60)]
    frames[CORNERS] = [(k % n_obs, a, b) for k, (a, b) in enumerate(corners)] + [(last, a, b) for a, b in corners[:2]]
    frames[MANY] = [(rs.randint(n_obs), rs.randint(97), rs.randint(61)) for _ in range(300)]
    for n in range(MANY + 1, N):
        for u in range(n_obs):
            for _ in range(rs.randint(1, 4)):
                frames[n].append((u, 2 * rs.randint(48) + 1, rs.randint(61)))     # odd a: every rescale to 49 is a tie
    frame_ptr = np.cumsum([0] + [len(f) for f in frames]).astype(np.int32)
    samples = np.array([s for f in frames for s in f], np.int32).reshape(-1, 3)
    assert frame_ptr[MANY + 1] - frame_ptr[MANY] == 300 and frame_ptr[1] == 0
    return gm.PackedFixations(frame_ptr, samples, n_obs, RAW)


@functools.lru_cache(maxsize=None)
def oracle(n_obs, shape, sigma):
    """(fixationmaps fp32, gazemaps fp32), computed once per case and never written to."""
    p = fixations(n_obs)
    counts = ref.fixation_counts(p.frame_ptr, p.samples, n_obs, RAW, shape)
    fix, gaze = counts.astype(np.float32), ref.gazemaps_from_counts(counts, n_obs, sigma)
    fix.setflags(write=False)
    gaze.setflags(write=False)
    return fix, gaze


def sub(packed, lo, hi):
    fp = packed.frame_ptr
    return packed._replace(frame_ptr=fp[lo:hi + 1] - fp[lo], samples=packed.samples[fp[lo]:fp[hi]])


def same(t, a):
    """torch.equal, a NaN equal to a NaN in the same place (a constant non-zero frame is NaN on both sides)."""
    t, a = t.cpu(), torch.from_numpy(np.array(a))
    return t.shape == a.shape and torch.equal(torch.isnan(t), torch.isnan(a)) and torch.equal(torch.nan_to_num(t, nan=0.0), torch.nan_to_num(a, nan=0.0))


@pytest.mark.parametrize('n_obs', OBSERVERS)
@pytest.mark.parametrize('shape, sigma', SHAPES)
def test_maps_equal_the_oracle(gpu, shape, sigma, n_obs):
    packed = fixations(n_obs)
    fix, gaze = oracle(n_obs, shape, sigma)
    out = gm.gazemaps_from_fixations(packed, out_shape=shape, sigma=sigma, want=gm.OUTPUTS, device=gpu)
    assert set(out) == set(gm.OUTPUTS)
    for t in out.values():
        assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (N, shape[1], shape[0])
    # what the frames were made for
    assert fix[EMPTY].sum() == 0 and fix[ONE].sum() == 1 and fix[SHARED].max() == n_obs
    assert fix[TWICE].max() == 1 and (shape != (49, 49) or fix[TWICE].sum() == 2)
    assert all(fix[CORNERS][y, x] >= 1 for y in (0, -1) for x in (0, -1))
    assert gaze[EMPTY].max() == 0 and gaze[ONE].max() == 1
    # one observer on 7 x 7: the 300 samples cover every cell, the frame is constant and non-zero: NaN, as numpy
    constant = [MANY] if (n_obs, shape) == (1, (7, 7)) else []
    assert [n for n in range(N) if np.isnan(gaze[n]).any()] == constant and np.isnan(gaze[constant]).all()

    assert same(out['fixationmaps'], fix), (out['fixationmaps'].cpu().numpy() != fix).sum()
    d_gaze = out['gazemaps'].cpu().numpy()
    diff = ~((d_gaze == gaze) | (np.isnan(d_gaze) & np.isnan(gaze)))
    print('%s sigma %g, %d observers: %d of %d gaze cells differ, max |d| %.3g'
          % (shape, sigma, n_obs, diff.sum(), diff.size, np.nanmax(np.abs(d_gaze - gaze))))
    assert same(out['gazemaps'], gaze)

    want = ref.labels64(gaze)
    labels = out['labels'].cpu().numpy().astype(np.float64)
    rest = np.array([n for n in range(N) if n != EMPTY and n not in constant])
    assert np.isnan(labels[EMPTY]).all() and np.isnan(want[EMPTY]).all() and np.isnan(labels[constant]).all()
    assert not np.isnan(labels[rest]).any()
    err = np.abs(labels[rest] - want[rest])
    print('labels: max relative error %.3g (bound %.3g)' % ((err / np.maximum(want[rest], 1e-300)).max(), 2.0 ** -22))
    assert np.all(err <= 2.0 ** -22 * np.abs(want[rest]))

    # the outputs are independent of one another: a call that wants one of them gives the same bits
    only = gm.gazemaps_from_fixations(packed, out_shape=shape, sigma=sigma, want='labels', device=gpu)
    assert set(only) == {'labels'} and same(only['labels'], out['labels'].cpu().numpy())


def test_default_sigma_is_the_loaders(gpu):
    for shape, sigma in SHAPES[:4]:
        out = gm.gazemaps_from_fixations(fixations(5), out_shape=shape, device=gpu)
        assert set(out) == {'gazemaps', 'fixationmaps'} and same(out['gazemaps'], oracle(5, shape, sigma)[1])


@pytest.mark.parametrize('shape, sigma', [((49, 49), 2.0), ((7, 9), 2.0)])
def test_launch_geometry_does_not_matter(gpu, shape, sigma):
    packed = fixations(5)
    full = gm.gazemaps_from_fixations(packed, out_shape=shape, sigma=sigma, want=gm.OUTPUTS, device=gpu)
    part = gm.gazemaps_from_fixations(sub(packed, 5, 12), out_shape=shape, sigma=sigma, want=gm.OUTPUTS, device=gpu)
    for k in gm.OUTPUTS:
        assert tuple(part[k].shape)[0] == 7 and torch.equal(part[k], full[k][5:12]), k
    # 1000 frames by tiling the 24
    idx = np.arange(1000) % N
    fp, s = packed.frame_ptr, packed.samples
    rows = np.concatenate([np.arange(fp[i], fp[i + 1]) for i in idx])
    tiled = packed._replace(frame_ptr=np.concatenate([[0], np.cumsum((fp[1:] - fp[:-1])[idx])]).astype(np.int32), samples=s[rows])
    big = gm.gazemaps_from_fixations(tiled, out_shape=shape, sigma=sigma, want=gm.OUTPUTS, device=gpu)
    sel = torch.from_numpy(idx).to(gpu)
    full['labels'][EMPTY] = 0                     # NaN in both: compared as a number
    big['labels'][sel == EMPTY] = 0
    for k in gm.OUTPUTS:
        assert tuple(big[k].shape)[0] == 1000 and torch.equal(big[k], full[k][sel]), k
    fix, gaze = oracle(5, shape, sigma)
    assert same(big['gazemaps'], gaze[idx]) and same(big['fixationmaps'], fix[idx])


def test_no_frames(gpu):
    empty = gm.PackedFixations(np.zeros(1, np.int32), np.zeros((0, 3), np.int32), 5, RAW)
    out = gm.gazemaps_from_fixations(empty, device=gpu)
    assert tuple(out['gazemaps'].shape) == (0, 49, 49)
    # frames, but not one sample
    blank = gm.PackedFixations(np.zeros(4, np.int32), np.zeros((0, 3), np.int32), 5, RAW)
    out = gm.gazemaps_from_fixations(blank, want=gm.OUTPUTS, device=gpu)
    assert float(out['gazemaps'].abs().max()) == 0 and float(out['fixationmaps'].abs().max()) == 0
    assert bool(torch.isnan(out['labels']).all())


@pytest.mark.parametrize('column, value', [(1, 97), (1, -1), (2, 61), (0, 5), (0, -1)])
def test_a_bad_sample_refuses_its_frame_only(gpu, column, value):
    """Input validation on the device: the frame with an out-of-range a (b, observer id) is NaN in every output and
    counted in the status word, the other frames are computed, and the next clean call reports RGP_OK."""
    shape, sigma, bad_frame = (49, 49), 2.0, 7
    packed = fixations(5)
    fix, gaze = oracle(5, shape, sigma)
    samples = packed.samples.copy()
    samples[packed.frame_ptr[bad_frame] + 1, column] = value
    with pytest.raises(_lib.RgpError) as info:
        gm.gazemaps_from_fixations(packed._replace(samples=samples), out_shape=shape, sigma=sigma, want=gm.OUTPUTS, device=gpu)
    assert info.value.code == -1 and '1 frame(s) refused' in str(info.value)               # RGP_EINVAL
    out = info.value.outputs
    rest = np.arange(N) != bad_frame
    for k in gm.OUTPUTS:
        assert bool(torch.isnan(out[k][bad_frame]).all()), k
    assert same(out['gazemaps'][rest], gaze[rest]) and same(out['fixationmaps'][rest], fix[rest])
    assert not bool(torch.isnan(out['labels'][rest][1:]).any())
    clean = gm.gazemaps_from_fixations(packed, out_shape=shape, sigma=sigma, device=gpu)        # RGP_OK: does not raise
    assert same(clean['gazemaps'], gaze)


# ------------------------------------------------------------------------------------------------ consumers
def test_scorer_reads_the_device_maps(gpu):
    """The maps as `gt` / `fix` of evaluation_metrics_gpu (device tensors, read in place) give the scores host-built
    maps give: equal, since the inputs are.  (The 300-sample frame is left out: the scorer's cap is 256 fixations.)"""
    from recurrent_gaze_prediction_amd import evaluation_metrics_gpu as emg
    shape, sigma = (49, 49), 2.0
    keep = np.array([n for n in range(N) if n != MANY])
    out = gm.gazemaps_from_fixations(fixations(5), out_shape=shape, sigma=sigma, device=gpu)
    fix, gaze = oracle(5, shape, sigma)
    pred = (np.random.RandomState(3).rand(len(keep), 49, 49) + 0.05).astype(np.float32)
    sel = torch.from_numpy(keep).to(gpu)
    metrics = ('sim', 'cc', 'NSS')
    dev = emg.saliency_scores_single(torch.from_numpy(pred).to(gpu), out['gazemaps'][sel], out['fixationmaps'][sel], None,
                                     metrics, draws='reference')
    host = emg.saliency_scores_single(pred, gaze[keep], fix[keep], None, metrics, draws='reference', device=gpu)
    for m in metrics:
        assert np.array_equal(dev[m], host[m], equal_nan=True), m
        assert np.isfinite(dev[m][1:]).all(), m                  # (frame 0 has no sample: NaN on every metric)


def test_grcn77_step_on_a_clip_from_fixations(gpu, tmp_path):
    """One validation step of gaze_grcn77 (B = 2, T = 4, 7 x 7) on a data.clip_from_fixations dataset gives the loss of
    the same step on maps built by the oracle."""
    from recurrent_gaze_prediction_amd import data
    from recurrent_gaze_prediction_amd.models.base import Session
    from recurrent_gaze_prediction_amd.models.gaze_grcn77 import GazePredictionGRCN, GRUModelConfig
    B, T, shape = 2, 4, (7, 7)
    rs = np.random.RandomState(11)
    observers = []
    for length in (65, 60, 40):                   # gazelen = 55: frames 15, 20 .. 50; the 40-frame observer is dropped
        t = np.concatenate([np.arange(length), rs.randint(0, length, length)])       # a sample in every frame
        observers.append((t, rs.randint(0, RAW[0], len(t)), rs.randint(0, RAW[1], len(t)), length))
    packed = gm.pack_fixations(observers, RAW)
    assert packed.n_observers == 2 and len(packed.frame_ptr) == B * T + 1
    counts = ref.fixation_counts(packed.frame_ptr, packed.samples, 2, RAW, shape)
    images = rs.rand(B * T, 98, 98, 3).astype(np.float32)
    c3d = syn.c3d_features(12, 1, B * T).reshape(B * T, 512, 2, 7, 7)
    pupils = np.zeros(B * T, np.float32)
    ours = data.clip_from_fixations(images, observers, RAW, c3d, pupils, 'clip', T, out_shape=shape, device=gpu)
    theirs = data.clip_to_dataset(images, ref.gazemaps_from_counts(counts, 2, 0.3), counts.astype(np.float32), c3d, pupils,
                                  'clip', T)
    assert len(ours) == len(theirs) == B + 1                 # seq2batch: two whole chunks and the re-taken tail
    assert np.array_equal(ours.gazemaps, theirs.gazemaps) and np.array_equal(ours.fixationmaps, theirs.fixationmaps)
    assert ours.gazemaps.shape == (B + 1, T, 7, 7) and ours.gazemaps.dtype == np.float32

    cfg = GRUModelConfig()
    cfg.batch_size, cfg.n_lstm_steps, cfg.loss_type, cfg.compute_dtype = B, T, 'xentropy', 'bf16'
    cfg.trainable, cfg.train_dir = False, str(tmp_path)
    ds = type('DS', (), {})()
    ds.train = ds.valid = ours
    model = GazePredictionGRCN(Session(gpu), ds, cfg)
    model.load_state_dict(syn.grcn77_params(61))
    losses = []
    for dataset in (ours, theirs):
        model.single_step(train_mode=False, dataset=dataset)
        losses.append(float(model.loss))
    print('gaze_grcn77 validation loss on device-built / oracle-built maps:', losses)
    assert np.isfinite(losses[0]) and losses[0] == losses[1]
