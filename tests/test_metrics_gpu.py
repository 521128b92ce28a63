"""GPU: the saliency metrics kernel (csrc/rgp_metrics.hip through evaluation_metrics_gpu) against the host module
evaluation_metrics, which tests/test_metrics_cpu.py pins to the reference's own file.

Bound of the parity checks: 1e-9.  With the host's draws the device makes the same comparisons on the same fp64
values; what differs is the order of sums of at most 4096 terms of magnitude <= 1, about 4096 * 2^-53 = 5e-13."""
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

from recurrent_gaze_prediction_amd import _lib
from recurrent_gaze_prediction_amd import evaluation_metrics as em
from recurrent_gaze_prediction_amd import evaluation_metrics_gpu as emg
from recurrent_gaze_prediction_amd import synthetic as syn

pytestmark = pytest.mark.gpu
TOL = 1e-9
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'metrics_ref.npz'))


def frames(seed, n, kind):
    gt, centres = syn.gaze_maps(seed, n, 1)
    fix = syn.fixation_maps(seed + 1, centres)[:, 0]
    gt = gt[:, 0]
    rs = np.random.RandomState(seed + 2)
    if kind == 'random':          # random positive maps, fp64: the kernel's fp64 input path
        pred = rs.rand(*gt.shape) + 0.05
    else:                         # peaked maps that follow the fixations, fp32 like predict()'s output
        pred = (gt + 0.3 * rs.rand(*gt.shape) + 0.2 * np.roll(gt, 3, axis=2)).astype(np.float32)
    return pred, gt, fix


def union_of(fix, idx):
    return (fix[idx] > 0).sum(0).astype(np.float64)


def host_scores(metric, pred, gt, fix, other, jitter=True):
    """The host, frame by frame; NaN where it raises (a map without contrast or an empty negative set in the two
    sampled AUCs: the kernel documents NaN there).  ``other``: [H,W] or one map per frame."""
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for i, (p, g, f) in enumerate(zip(pred, gt, fix)):
            o = other if np.ndim(other) == 2 else other[i]
            try:
                if metric == 'AUC_Judd' and not jitter:
                    out.append(em.AUC_Judd(f, em.normalize_range(p), jitter=False))
                else:
                    out.append(em.saliency_score_single(metric, p, g, f, o))
            except ValueError as e:
                assert metric in ('AUC_Borji', 'AUC_shuffled') and ('arange' in str(e) or 'zero-size' in str(e)), e
                out.append(np.nan)
    return np.array(out, np.float64)


def assert_close(dev, host, what):
    dev, host = np.asarray(dev), np.asarray(host)
    assert np.array_equal(np.isnan(dev), np.isnan(host)), (what, np.isnan(dev).nonzero(), np.isnan(host).nonzero())
    err = np.nanmax(np.abs(dev - host)) if np.isfinite(host).any() else 0.0
    print('%-28s max |device - host| = %.3e over %d frames (%d NaN)' % (what, err, len(host), np.isnan(host).sum()))
    assert err < TOL, (what, err)


def compare_all(pred, gt, fix, other, seed, what, jitter=True, metrics=emg.METRICS):
    """Six metrics in one launch with the host's draws (metric after metric) against the host loop, same seed."""
    np.random.seed(seed)
    host = {m: host_scores(m, pred, gt, fix, other, jitter) for m in metrics}
    np.random.seed(seed)
    dev = emg.saliency_scores_single(pred, gt, fix, other, metrics, draws='reference', jitter=jitter)
    assert set(dev) == set(metrics)
    for m in metrics:
        assert dev[m].dtype == np.float64 and dev[m].shape == (len(pred),)
        assert_close(dev[m], host[m], '%s %s' % (what, m))
    return dev, host


@pytest.mark.parametrize('kind', ['random', 'peaked'])
def test_parity_with_the_host_per_frame(gpu, kind):
    pred, gt, fix = frames(100, 64, kind)
    n_fix = (fix > 0.5).reshape(64, -1).sum(1)
    other = union_of(fix, [3, 9, 14, 20, 27, 33, 41, 48, 55, 60])
    assert 4 <= n_fix.min() and n_fix.max() <= 6 and (other > 0.5).sum() <= 60          # inside both caps
    dev, host = compare_all(pred, gt, fix, other, 11, kind)
    assert all(np.isfinite(host[m]).all() for m in emg.METRICS)
    # one metric at a time gives the same numbers as all six at once (draw order 'metric')
    np.random.seed(11)
    for m in emg.METRICS:
        one = emg.saliency_scores_single(pred, gt, fix, other, [m], draws='reference')[m]
        assert np.array_equal(one, dev[m]), m
    # device tensors are read in place and give the same bits as uploaded arrays
    np.random.seed(11)
    t = emg.saliency_scores_single(torch.tensor(pred, device=gpu), torch.tensor(gt, device=gpu), torch.tensor(fix, device=gpu),
                                   torch.tensor(other, device=gpu), emg.METRICS, draws='reference')
    for m in emg.METRICS:
        assert np.array_equal(t[m], dev[m]), m


def test_parity_on_hand_made_frames(gpu):
    pred, gt, fix = frames(200, 8, 'peaked')
    pred, gt, fix = pred.copy(), gt.copy(), fix.copy()
    fix[0] = 0                                                       # no fixation
    pred[1] = 0.25                                                   # a constant prediction
    ys, xs = np.nonzero(fix[2])                                      # fixations with tied saliency
    pred[2, ys, xs] = 0.5
    pred[3] = np.round(pred[3] * 4) / 4                              # a map of five levels: ties everywhere
    gt[4] = 0.125                                                    # a constant ground truth: cc is NaN on the host
    fix[5] = 1.0                                                     # every pixel fixated would be over the cap ...
    fix[5].reshape(-1)[200:] = 0                                     # ... 200 fixations are not
    small = np.zeros((49, 49))
    small[7, 7] = small[30, 12] = 1                                  # a negative set smaller than n_fix
    per_frame = np.stack([union_of(fix, [(i + k) % 8 for k in range(1, 5)]) for i in range(8)])   # one union per frame
    for other, name in ((small, 'small negative set'), (per_frame, 'per-frame union')):
        for jitter in (True, False):
            dev, host = compare_all(pred, gt, fix, other, 21, '%s jitter=%d' % (name, jitter), jitter=jitter)
            for m in ('AUC_Judd', 'AUC_Borji', 'AUC_shuffled', 'NSS'):
                assert np.isnan(dev[m][0]), m                        # no fixation
            assert np.isnan(dev['sim'][1]) and np.isnan(dev['cc'][1]) and np.isnan(dev['NSS'][1])
            assert np.isnan(dev['AUC_Borji'][1]) and np.isfinite(dev['AUC_Judd'][1])       # as the host: see host_scores
            assert np.isnan(dev['cc'][4]) and np.isfinite(dev['sim'][4])
    empty = np.zeros((49, 49))                                       # no negatives at all: the host raises, the device says NaN
    np.random.seed(5)
    d = emg.saliency_scores_single(pred, gt, fix, empty, ['AUC_shuffled'], draws='reference')
    assert np.isnan(d['AUC_shuffled']).all()


def test_golden_scores_of_the_reference(gpu):
    """The twelve cases of tests/golden/metrics_ref.npz (inputs as the `maps` fixture of tests/test_metrics_cpu.py builds
    them), recorded from the reference's own file with the global RNG re-seeded before each frame and, for AUC_shuffled,
    the union of the OTHER frames' fixations: scored frame by frame (N = 1 calls)."""
    seed, n = [int(v) for v in GOLD['config']]
    gt, centres = syn.gaze_maps(seed, n, 1)
    fix = syn.fixation_maps(seed + 1, centres)[:, 0]
    gt = gt[:, 0]
    rs = np.random.RandomState(seed + 2)
    pred = (gt + 0.3 * rs.rand(*gt.shape) + 0.2 * np.roll(gt, 3, axis=2)).astype(np.float32)
    assert n == 12

    both = emg.saliency_scores_single(pred, gt, fix, None, ['sim', 'cc'], draws='reference')
    assert_close(both['sim'], GOLD['sim'], 'golden sim')
    assert_close(both['cc'], GOLD['cc'], 'golden cc')
    got = {'AUC_Judd': [], 'AUC_Borji': [], 'AUC_shuffled': []}
    for i in range(n):
        other = np.zeros(fix[0].shape)
        for j in range(n):
            if j != i:
                other += (fix[j] > 0).astype(int)
        for metric, base in (('AUC_Judd', 1000), ('AUC_Borji', 2000), ('AUC_shuffled', 4000)):
            np.random.seed(base + i)
            s = emg.saliency_scores_single(pred[i:i + 1], gt[i:i + 1], fix[i:i + 1], other, [metric], draws='reference')
            got[metric].append(s[metric][0])
    for metric in got:
        assert_close(got[metric], GOLD[metric], 'golden ' + metric)
    for metric in ('sim', 'cc', 'AUC_Borji', 'AUC_shuffled'):       # saliency_score: the union of ten from the global RNG
        np.random.seed(3000)
        s = emg.saliency_score(metric, list(pred), list(gt), list(fix), draws='reference')
        print('golden score_%s: |device - reference| = %.3e' % (metric, abs(s - float(GOLD['score_' + metric]))))
        assert abs(s - float(GOLD['score_' + metric])) < TOL


def test_device_draws_are_reproducible_and_well_formed(gpu):
    pred, gt, fix = frames(300, 48, 'peaked')
    other = union_of(fix, range(10))
    members = set(np.nonzero(other.ravel() > 0.5)[0])
    drawn = ('AUC_Judd', 'AUC_Borji', 'AUC_shuffled')
    a = emg.saliency_scores_single(pred, gt, fix, other, emg.METRICS, draws='device', seed=7, return_draws=True)
    b = emg.saliency_scores_single(pred, gt, fix, other, emg.METRICS, draws='device', seed=7)
    c = emg.saliency_scores_single(pred, gt, fix, other, emg.METRICS, draws='device', seed=8)
    for m in emg.METRICS:
        assert np.array_equal(a[m], b[m]), m                                        # same seed, same bits
        assert np.isfinite(a[m]).all(), m
    assert not np.array_equal(a['AUC_Borji'], c['AUC_Borji']) and not np.array_equal(a['AUC_shuffled'], c['AUC_shuffled'])
    # one call or two halves with the matching offset; a subset of the metrics
    lo = emg.saliency_scores_single(pred[:20], gt[:20], fix[:20], other, emg.METRICS, draws='device', seed=7)
    hi = emg.saliency_scores_single(pred[20:], gt[20:], fix[20:], other, drawn, draws='device', seed=7, offset=20)
    for m in drawn:
        assert np.array_equal(np.concatenate([lo[m], hi[m]]), a[m]), m
    shifted = emg.saliency_scores_single(pred[20:], gt[20:], fix[20:], other, drawn, draws='device', seed=7)
    assert not np.array_equal(shifted['AUC_Borji'], hi['AUC_Borji'])
    # what takes no draws equals the parity form bit for bit, and the host within the parity bound
    ref = emg.saliency_scores_single(pred, gt, fix, other, ['sim', 'cc', 'NSS', 'AUC_Judd'], draws='reference', jitter=False)
    nojit = emg.saliency_scores_single(pred, gt, fix, other, ['sim', 'cc', 'NSS', 'AUC_Judd'], draws='device', jitter=False, seed=3)
    for m in ('sim', 'cc', 'NSS', 'AUC_Judd'):
        assert np.array_equal(ref[m], nojit[m]), m
        assert_close(nojit[m], host_scores(m, pred, gt, fix, other, jitter=False), 'device draws, no draw: ' + m)
    for m in ('sim', 'cc', 'NSS'):
        assert np.array_equal(a[m], ref[m]), m
    # the drawn indices: range, membership, distinctness; feeding them back as the caller's draws gives the same scores
    d = a['draws']
    n_fix = (fix > 0.5).reshape(48, -1).sum(1)
    assert np.array_equal(d['n_fix'], n_fix) and d['neg_stride'] == n_fix.max()
    assert np.array_equal(d['shuf_cnt'], np.minimum(n_fix, len(members)))
    for i in range(48):
        bj = d['borji_neg'][i, :, :n_fix[i]]
        assert bj.min() >= 0 and bj.max() < 2401
        for rep in range(100):
            row = d['shuf_neg'][i, rep, :d['shuf_cnt'][i]]
            assert set(row) <= members and len(set(row)) == len(row)
    assert len(np.unique(d['borji_neg'][:, :, 0])) > 1500                           # spread over the map
    assert set().union(*[d['shuf_neg'][i, :, :d['shuf_cnt'][i]].ravel() for i in range(48)]) == members   # all get drawn
    back = dict(d, judd_jitter=None)
    again = emg.saliency_scores_single(pred, gt, fix, other, ['AUC_Borji', 'AUC_shuffled'], draws=back)
    assert np.array_equal(again['AUC_Borji'], a['AUC_Borji']) and np.array_equal(again['AUC_shuffled'], a['AUC_shuffled'])
    # a negative set smaller than n_fix: all of it, every repetition
    small = np.zeros((49, 49))
    small[7, 7] = small[30, 12] = 1
    s = emg.saliency_scores_single(pred, gt, fix, small, ['AUC_shuffled'], draws='device', seed=1, return_draws=True)
    assert (s['draws']['shuf_cnt'] == 2).all()
    assert (np.sort(s['draws']['shuf_neg'][:, :, :2], axis=-1) == np.array([7 * 49 + 7, 30 * 49 + 12])).all()
    np.random.seed(0)
    assert_close(s['AUC_shuffled'], host_scores('AUC_shuffled', pred, gt, fix, small), 'device draws, whole negative set')


def test_device_draw_means_lie_inside_the_host_seed_to_seed_spread(gpu):
    """Mean over 1024 frames: the host on the same inputs and the same union over 16 seeds gives mean mu and standard
    deviation sigma per metric; the device-draw mean must lie within 5 sigma of mu.  sigma is measured here."""
    pred, gt, fix = frames(400, 1024, 'random')
    pred = pred.astype(np.float32)
    other = union_of(fix, np.random.RandomState(1).choice(1024, 10, replace=False))
    metrics = ('AUC_Judd', 'AUC_Borji', 'AUC_shuffled')
    means = {m: [] for m in metrics}
    for seed in range(16):
        np.random.seed(1000 + seed)
        for m in metrics:
            means[m].append(np.mean(host_scores(m, pred, gt, fix, other)))
    dev = emg.saliency_scores_single(torch.tensor(pred, device=gpu), torch.tensor(gt, device=gpu), torch.tensor(fix, device=gpu),
                                     torch.tensor(other, device=gpu), metrics, draws='device', seed=2024)
    for m in metrics:
        mu, sigma = np.mean(means[m]), np.std(means[m], ddof=1)
        got = np.mean(dev[m])
        print('%-13s host mu %.6f sigma %.3e over 16 seeds; device draws %.6f = mu %+.2f sigma' % (m, mu, sigma, got, (got - mu) / sigma))
        assert abs(got - mu) <= 5 * sigma, (m, got, mu, sigma)


def make_model(gpu, tmp_path, B=2, T=4):
    from recurrent_gaze_prediction_amd.models.base import Session
    from recurrent_gaze_prediction_amd.models.gaze_grcn import GazePredictionGRCN, GRUModelConfig
    cfg = GRUModelConfig()
    cfg.batch_size, cfg.n_lstm_steps, cfg.compute_dtype, cfg.train_dir, cfg.trainable = B, T, 'bf16', str(tmp_path), False
    ds = type('DS', (), {})()
    ds.train = ds.valid = syn.SyntheticDataSet(8, T, seed=21)
    m = GazePredictionGRCN(Session(gpu), ds, cfg)
    m.load_state_dict(syn.grcn_params(22, T, gru_std=0.05, random_bn=True))
    return m, ds


def test_evaluate_with_a_device_scorer(gpu, tmp_path):
    model, ds = make_model(gpu, tmp_path)
    ret = model.generate(ds.valid, max_instances=8)
    np.random.seed(31)
    parent = {m: em.saliency_score(m, ret['pred_gazemap_list'], ret['gt_gazemap_list'], ret['fixationmap_list'])
              for m in em.AVAILABLE_METRICS}                          # what evaluate() was before the keyword existed
    np.random.seed(31)
    default = model.evaluate(**ret)
    np.random.seed(31)
    host = model.evaluate(scorer='host', **ret)
    assert default == parent and host == parent                       # bit-identical without the keyword
    np.random.seed(31)
    ref = model.evaluate(scorer='device-reference', **ret)
    assert set(ref) == set(host)
    for m in host:
        print('evaluate %-13s host %.12f device-reference %.12f' % (m, host[m], ref[m]))
        assert abs(ref[m] - host[m]) < TOL, m
    np.random.seed(31)
    dev = model.evaluate(scorer='device', seed=5, **ret)
    np.random.seed(31)
    dev2 = model.evaluate(scorer='device', seed=5, **ret)
    assert dev == dev2
    assert abs(dev['sim'] - host['sim']) < TOL and abs(dev['cc'] - host['cc']) < TOL
    assert abs(dev['AUC_Borji'] - host['AUC_Borji']) < 0.05 and abs(dev['AUC_shuffled'] - host['AUC_shuffled']) < 0.05
    with pytest.raises(ValueError):
        model.evaluate(scorer='gpu', **ret)
    np.random.seed(31)
    _, both = model.generate_and_evaluate(syn.SyntheticDataSet(8, 4, seed=21), max_instances=8, scorer='device-reference')
    assert set(both) == set(host)


def test_run_evaluation_with_a_device_scorer_writes_the_same_files(gpu, tmp_path):
    from recurrent_gaze_prediction_amd.models.evaluate_gaze import FRAME_METRICS, run_evaluation
    model, ds = make_model(gpu, tmp_path)
    outs = {}
    for scorer in ('host', 'device-reference', 'device'):
        ds.valid = syn.SyntheticDataSet(8, 4, seed=21)                # the loader has a cursor: same frames for each run
        out = str(tmp_path / scorer)
        state = np.random.get_state()[1].copy()
        overall = run_evaluation(model, ds, out, num_frames=12, seed=3, **({} if scorer == 'host' else {'scorer': scorer}))
        assert np.array_equal(np.random.get_state()[1], state)        # the global RNG is restored
        outs[scorer] = (overall, open(os.path.join(out, 'overall.txt')).read(),
                        [open(os.path.join(out, '%05d.scores.txt' % i)).read() for i in range(16)])
    host, ref, dev = outs['host'], outs['device-reference'], outs['device']
    assert list(ref[0]) == list(host[0]) == list(FRAME_METRICS)
    for m in FRAME_METRICS:
        assert abs(ref[0][m] - host[0][m]) < TOL, m
    assert ref[1] == host[1]                                          # overall.txt at its %.4f / %.3f formatting
    assert ref[2] == host[2]                                          # and every NNNNN.scores.txt
    assert dev[1].splitlines()[:4] == host[1].splitlines()[:4]        # sim and cc take no draws
    assert len(dev[1].splitlines()) == len(host[1].splitlines())
    with pytest.raises(ValueError):
        run_evaluation(model, ds, str(tmp_path / 'x'), num_frames=12, seed=3, scorer='gpu')


def test_a_frame_over_the_fixation_cap_is_refused(gpu):
    pred, gt, fix = frames(500, 6, 'peaked')
    crowded = fix.copy()
    crowded[4].reshape(-1)[:257] = 1                                  # 257 fixations
    for draws in ('reference', 'device'):                             # counted on the host: refused before any launch
        with pytest.raises(ValueError, match='evaluation_metrics'):
            emg.saliency_scores_single(pred, gt, crowded, fix[0], emg.METRICS, draws=draws)
    # a device tensor with a bound that does not hold: the kernel counts for itself
    with pytest.raises(ValueError, match='evaluation_metrics'):
        emg.saliency_scores_single(pred, gt, torch.tensor(crowded, device=gpu), fix[0], emg.METRICS, draws='device', max_fix=256)
    with pytest.raises(ValueError, match='evaluation_metrics'):       # ... or than the caller promised
        emg.saliency_scores_single(pred, gt, torch.tensor(fix, device=gpu), fix[0], emg.METRICS, draws='device', max_fix=3)
    # the C ABI: RGP_EINVAL through rgp_metrics_status, NaN in every score of that frame, the other frames scored
    lib = _lib.load()
    t = [torch.tensor(a, device=gpu) for a in (pred, gt, crowded, fix[0])]
    flags = _lib.RGP_METRICS_DEVICE_DRAWS
    ws = torch.empty(lib.rgp_metrics_workspace_bytes(6, 100, 256, flags), dtype=torch.uint8, device=gpu)
    scores = torch.zeros(6, 6, dtype=torch.float64, device=gpu)
    args = _lib.MetricsArgs(pred=t[0].data_ptr(), gt=t[1].data_ptr(), fix=t[2].data_ptr(), other=t[3].data_ptr(), other_stride=0,
                            n_frames=6, height=49, width=49, metrics=63, flags=flags, n_rep=100, neg_stride=256, step_size=0.1,
                            seed=1, offset=0, workspace=ws.data_ptr(), workspace_bytes=ws.numel(), scores=scores.data_ptr())
    stream = torch.cuda.current_stream(gpu).cuda_stream
    assert lib.rgp_saliency_scores(ctypes.byref(args), stream) == 0
    assert lib.rgp_metrics_status(ws.data_ptr(), stream) == -1        # RGP_EINVAL
    assert b'1 frame' in lib.rgp_last_error()
    s = scores.cpu().numpy()
    assert np.isnan(s[:, 4]).all() and np.isfinite(np.delete(s, 4, axis=1)).all()
    fix_ok = torch.tensor(fix, device=gpu)                            # the same call on frames inside the cap is clean
    args.fix = fix_ok.data_ptr()
    assert lib.rgp_saliency_scores(ctypes.byref(args), stream) == 0 and lib.rgp_metrics_status(ws.data_ptr(), stream) == 0
    assert np.isfinite(scores.cpu().numpy()).all()
    # indices out of range in the caller's draws are refused the same way, not read
    np.random.seed(1)
    d = emg.draw_reference_samples(fix, fix[0], ['AUC_Borji'])
    d['borji_neg'][2, 5, 0] = 2401
    with pytest.raises(ValueError, match='refused'):
        emg.saliency_scores_single(pred, gt, fix, fix[0], ['AUC_Borji'], draws=d)
