"""GPU: the saliency metrics at the fixation maps' shape (csrc/rgp_metrics_scaled.hip, evaluation_metrics_gpu.py).

The resized values are held to the numpy oracle (tests/spline_ref.py) bit for bit; the scores, with the host's own
draws, to the host module with that oracle in place of scipy's resize (tests/test_metrics_scaled_cpu.py shows on these
very frames that the swap does not move the host's scores) within the project's TOL = 1e-9, far above the
order-of-summation bound H W 2^-53 = 3.2e-11 at 405 x 720."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse
import torch

from recurrent_gaze_prediction_amd import _lib
from recurrent_gaze_prediction_amd import evaluation_metrics as em
from recurrent_gaze_prediction_amd import evaluation_metrics_gpu as emg
from recurrent_gaze_prediction_amd import synthetic as syn

import metrics_scaled_cases as cases
import spline_ref

pytestmark = pytest.mark.gpu
TOL = cases.TOL


def nan_equal(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


# ------------------------------------------------------------------ the resize, bit for bit
@pytest.mark.parametrize('src_dtype', [np.float32, np.float64])
@pytest.mark.parametrize('src, dst', [((7, 7), (23, 31)), ((49, 49), (90, 160)), ((14, 14), (17, 40)), ((49, 49), (7, 9)),
                                      ((2, 3), (5, 4)), ((7, 7), (3, 1600))])
def test_resize_equals_the_oracle_bit_for_bit(gpu, src, dst, src_dtype):
    x = np.random.RandomState(src[0] * 100 + dst[1]).rand(3, *src).astype(src_dtype)
    want = np.stack([spline_ref.resize(m, dst) for m in x])
    got = emg.resize_maps(x, dst, device=gpu)
    assert got.dtype == torch.float64 and tuple(got.shape) == (3,) + dst
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    assert torch.equal(emg.resize_maps(torch.tensor(x, device=gpu), dst).cpu(), torch.from_numpy(want))    # read in place
    got32 = emg.resize_maps(x, dst, out_dtype=torch.float32, device=gpu)
    assert got32.dtype == torch.float32 and torch.equal(got32.cpu(), torch.from_numpy(want.astype(np.float32)))   # rounded once
    x[1, src[0] // 2, src[1] // 2] = np.nan                                      # a NaN stays in its frame
    bad = emg.resize_maps(x, dst, device=gpu).cpu()
    assert torch.isnan(bad[1]).any() and torch.equal(bad[0], torch.from_numpy(want[0])) and torch.equal(bad[2], torch.from_numpy(want[2]))


# ------------------------------------------------------------------ scores, the host's own draws
@pytest.mark.parametrize('name', list(cases.CASES))
def test_scores_equal_the_patched_host(gpu, name):
    c, host = cases.case(name), cases.patched_host(name)
    np.random.seed(c['seed'])
    dev = emg.saliency_scores_resized(c['pred'], c['gt'], c['fix'], c['other'], emg.METRICS, draws='reference', device=gpu)
    assert set(dev) == set(emg.METRICS)
    for m in emg.METRICS:
        assert dev[m].dtype == np.float64 and dev[m].shape == (len(c['pred']),)
        cases.assert_close(dev[m], host[m], '%s %s' % (name, m))
    if len(c['pred']) > 4:
        for m in ('AUC_Judd', 'AUC_Borji', 'AUC_shuffled', 'NSS'):               # no fixation
            assert np.isnan(dev[m][3])
        assert np.isfinite(dev['sim'][3]) and np.isfinite(dev['cc'][3])
        assert all(np.isnan(dev[m][4]) for m in ('sim', 'cc', 'AUC_Borji', 'AUC_shuffled', 'NSS'))   # no contrast
        ok = [i for i in range(len(c['pred'])) if i not in (3, 4)]
        assert all(np.isfinite(dev[m][ok]).all() for m in emg.METRICS)


def test_points_tensors_and_sparse_maps_give_the_same_bits(gpu):
    c = cases.case('tiny')
    np.random.seed(c['seed'])
    draws = emg.draw_reference_samples(c['fix'], c['other'], emg.METRICS)
    base = emg.saliency_scores_resized(c['pred'], c['gt'], c['fix'], c['other'], emg.METRICS, draws=draws, device=gpu)
    forms = {
        'packed': (emg.pack_points(c['fix'], c['shape']), emg.pack_points(c['other'][None], c['shape'])),
        'sparse': ([scipy.sparse.coo_matrix(f) for f in c['fix']], scipy.sparse.coo_matrix(c['other'])),
        'tensor': (torch.tensor(c['fix'], device=gpu), torch.tensor(c['other'], device=gpu)),
    }
    for what, (fix, other) in forms.items():
        pred, gt = (torch.tensor(c[k], device=gpu) for k in ('pred', 'gt')) if what == 'tensor' else (c['pred'], c['gt'])
        got = emg.saliency_scores_resized(pred, gt, fix, other, emg.METRICS, draws=draws, shape=c['shape'], device=gpu)
        assert all(nan_equal(got[m], base[m]) for m in emg.METRICS), what


def test_frame_order_of_draws_and_one_negative_set_per_frame(gpu):
    """What evaluate_gaze.handle_frame consumes: frame after frame, FRAME_METRICS order, a negative set per frame."""
    c = cases.case('tiny')
    N = len(c['pred'])
    rs = np.random.RandomState(77)
    others = np.stack([(c['fix'][rs.choice(N, 10, replace=False)] > 0).sum(0).astype(np.float64) for _ in range(N)])
    host = cases.host_scores(c, emg.FRAME_METRICS, other=others, order='frame')
    np.random.seed(c['seed'])
    draws = emg.draw_reference_samples(c['fix'], others, emg.FRAME_METRICS, order='frame')
    dev = emg.saliency_scores_resized(c['pred'], c['gt'], c['fix'], others, emg.FRAME_METRICS, draws=draws, device=gpu)
    for m in emg.FRAME_METRICS:
        cases.assert_close(dev[m], host[m], 'frame order %s' % m)


# ------------------------------------------------------------------ device draws
def test_device_draws_are_reproducible_batch_independent_and_well_formed(gpu):
    c = cases.case('mid64')
    N, (H, W) = len(c['pred']), c['shape']
    kw = dict(draws='device', seed=9, n_rep=20, device=gpu)
    full = emg.saliency_scores_resized(c['pred'], c['gt'], c['fix'], c['other'], emg.METRICS, return_draws=True, **kw)
    again = emg.saliency_scores_resized(c['pred'], c['gt'], c['fix'], c['other'], emg.METRICS, **kw)
    part = emg.saliency_scores_resized(c['pred'][3:8], c['gt'][3:8], c['fix'][3:8], c['other'], emg.METRICS, offset=3, **kw)
    other_seed = emg.saliency_scores_resized(c['pred'], c['gt'], c['fix'], c['other'], emg.METRICS, **dict(kw, seed=10))
    for m in emg.METRICS:
        assert nan_equal(again[m], full[m]), m
        assert nan_equal(part[m], full[m][3:8]), m                               # frames 3 .. 7 of the call = a call at offset 3
    assert not nan_equal(other_seed['AUC_Borji'], full['AUC_Borji'])
    # the indices the kernel used, fed back as the caller's draws, give the same scores
    d = full['draws']
    n_fix = (c['fix'] > 0.5).reshape(N, -1).sum(1)
    assert np.array_equal(d['n_fix'], n_fix) and d['neg_stride'] == 256
    back = dict(judd_jitter=None, borji_neg=d['borji_neg'], shuf_neg=d['shuf_neg'], shuf_cnt=d['shuf_cnt'], neg_stride=d['neg_stride'])
    fed = emg.saliency_scores_resized(c['pred'], c['gt'], c['fix'], c['other'], ('AUC_Borji', 'AUC_shuffled'), draws=back, n_rep=20,
                                      device=gpu)
    assert nan_equal(fed['AUC_Borji'], full['AUC_Borji']) and nan_equal(fed['AUC_shuffled'], full['AUC_shuffled'])
    members = np.nonzero(c['other'].ravel() > 0.5)[0]
    assert np.array_equal(d['shuf_cnt'], np.minimum(n_fix, len(members)))
    for i in range(N):
        k = int(n_fix[i])
        if k == 0:
            continue
        assert d['borji_neg'][i, :, :k].min() >= 0 and d['borji_neg'][i, :, :k].max() < H * W
        for rep in range(20):
            row = d['shuf_neg'][i, rep, :d['shuf_cnt'][i]]
            assert len(set(row.tolist())) == len(row) and np.isin(row, members).all()
    # sim and cc take no draws: the reference-draws run gives the same bits
    np.random.seed(c['seed'])
    ref = emg.saliency_scores_resized(c['pred'], c['gt'], c['fix'], c['other'], ('sim', 'cc'), draws='reference', device=gpu)
    assert nan_equal(ref['sim'], full['sim']) and nan_equal(ref['cc'], full['cc'])
    # without jitter AUC_Judd needs no draw either: reproducible across seeds
    a = emg.saliency_scores_resized(c['pred'], c['gt'], c['fix'], None, ['AUC_Judd'], jitter=False, **kw)
    b = emg.saliency_scores_resized(c['pred'], c['gt'], c['fix'], None, ['AUC_Judd'], jitter=False, **dict(kw, seed=11))
    assert nan_equal(a['AUC_Judd'], b['AUC_Judd'])


# ------------------------------------------------------------------ what only the device can see
def launch(gpu, c, fix, other, neg_stride, flags, n_rep=5, draws=None, metrics=63, shared=True):
    """rgp_saliency_scores_scaled through the C ABI -> (status code, last error, scores [6, N])."""
    lib = _lib.load()
    N, (h, w), (H, W) = len(c['pred']), c['pred'].shape[1:], c['shape']
    keep = [torch.tensor(c['pred'], device=gpu), torch.tensor(c['gt'], device=gpu)]
    pts = [torch.tensor(np.ascontiguousarray(v, np.int32), device=gpu) for v in (fix[0], fix[1], other[0], other[1])]
    flags |= (_lib.RGP_METRICS_PRED_F64 if c['pred'].dtype == np.float64 else 0) | (_lib.RGP_METRICS_SCALED_OTHER_SHARED if shared else 0)
    ws = torch.empty(lib.rgp_metrics_scaled_workspace_bytes(N, n_rep, neg_stride, H, W, flags), dtype=torch.uint8, device=gpu)
    scores = torch.zeros(6, N, dtype=torch.float64, device=gpu)
    d = {k: (None if draws is None or draws.get(k) is None else torch.tensor(draws[k], device=gpu))
         for k in ('judd_jitter', 'borji_neg', 'shuf_neg', 'shuf_cnt')}
    args = _lib.MetricsScaledArgs(
        pred=keep[0].data_ptr(), gt=keep[1].data_ptr(), fix_ptr=pts[0].data_ptr(), fix_idx=pts[1].data_ptr(), other_ptr=pts[2].data_ptr(),
        other_idx=pts[3].data_ptr(), fix_len=len(fix[1]), other_len=len(other[1]), n_frames=N, height=h, width=w, target_height=H,
        target_width=W, metrics=metrics, flags=flags, n_rep=n_rep, neg_stride=neg_stride, step_size=0.1,
        judd_jitter=None if d['judd_jitter'] is None else d['judd_jitter'].data_ptr(),
        borji_neg=None if d['borji_neg'] is None else d['borji_neg'].data_ptr(),
        shuf_neg=None if d['shuf_neg'] is None else d['shuf_neg'].data_ptr(),
        shuf_cnt=None if d['shuf_cnt'] is None else d['shuf_cnt'].data_ptr(),
        seed=1, offset=0, workspace=ws.data_ptr(), workspace_bytes=ws.numel(), scores=scores.data_ptr())
    stream = torch.cuda.current_stream(gpu).cuda_stream
    assert lib.rgp_saliency_scores_scaled(ctypes.byref(args), stream) == 0, lib.rgp_last_error()
    rc = lib.rgp_metrics_status(ws.data_ptr(), stream)
    return rc, lib.rgp_last_error(), scores.cpu().numpy()


def test_the_device_refuses_a_frame_and_scores_the_others(gpu):
    c = dict(cases.case('mid64'))
    c['pred'], c['gt'] = c['pred'].copy(), c['gt']
    c['pred'][4] = c['pred'][5]                                                  # every frame has contrast here
    N, (H, W) = len(c['pred']), c['shape']
    fix = np.zeros((N, H * W), np.float32)
    rs = np.random.RandomState(3)
    for i in range(N):
        fix[i, rs.choice(H * W, 6, replace=False)] = 1
    ptr, idx = emg.pack_points(fix.reshape(N, H, W), (H, W))
    other = emg.pack_points(c['other'][None], (H, W))
    dev = _lib.RGP_METRICS_DEVICE_DRAWS

    def refused(frame, rc, msg, s):
        assert rc == -1 and b'1 frame' in msg, (rc, msg)                         # RGP_EINVAL with the count
        assert np.isnan(s[:, frame]).all() and np.isfinite(np.delete(s, frame, axis=1)).all()

    rc, msg, s = launch(gpu, c, (ptr, idx), other, 256, dev)
    assert rc == 0 and np.isfinite(s).all(), msg
    bad = idx.copy()
    bad[ptr[3] - 1] = H * W                                                      # frame 2: an index equal to H W
    refused(2, *launch(gpu, c, (ptr, bad), other, 256, dev))
    bad = idx.copy()
    bad[ptr[7]], bad[ptr[7] + 1] = idx[ptr[7] + 1], idx[ptr[7]]                  # frame 7: a decreasing pair
    refused(7, *launch(gpu, c, (ptr, bad), other, 256, dev))
    crowd = np.concatenate([idx[:ptr[5]], np.arange(257, dtype=np.int32), idx[ptr[6]:]])     # frame 5: 257 fixations
    cptr = ptr.copy()
    cptr[6:] += 257 - 6
    refused(5, *launch(gpu, c, (cptr, crowd), other, 256, dev))
    members = other[1]                                                           # frame 6: a negative set of 4097 members
    sets = [np.arange(4097, dtype=np.int32) if i == 6 else members for i in range(N)]
    optr = np.concatenate([[0], np.cumsum([len(v) for v in sets])]).astype(np.int32)
    refused(6, *launch(gpu, c, (ptr, idx), (optr, np.concatenate(sets)), 256, dev, shared=False))
    sets[6] = np.arange(4096, dtype=np.int32)                                    # at the cap it is scored
    optr = np.concatenate([[0], np.cumsum([len(v) for v in sets])]).astype(np.int32)
    rc, msg, s = launch(gpu, c, (ptr, idx), (optr, np.concatenate(sets)), 256, dev, shared=False)
    assert rc == 0 and np.isfinite(s).all(), msg
    np.random.seed(2)
    d = emg.draw_reference_samples_points((ptr, idx), other, (H, W), emg.METRICS, n_rep=5)
    rc, msg, s = launch(gpu, c, (ptr, idx), other, d['neg_stride'], 0, draws=d)
    assert rc == 0 and np.isfinite(s).all(), msg
    d['shuf_neg'] = d['shuf_neg'].copy()
    d['shuf_neg'][9, 2, 1] = H * W                                               # frame 9: a draw index out of range
    refused(9, *launch(gpu, c, (ptr, idx), other, d['neg_stride'], 0, draws=d))
    d['shuf_neg'][9, 2, 1] = 0
    rc, msg, s = launch(gpu, c, (ptr, idx), other, d['neg_stride'], 0, draws=d)   # the same call, cleaned
    assert rc == 0 and np.isfinite(s).all()
    with pytest.raises(ValueError, match='refused'):                             # the Python entry raises
        emg.saliency_scores_resized(c['pred'], c['gt'], (ptr, bad), None, ['sim'], shape=(H, W), device=gpu)


def test_fixation_points_are_the_fixation_maps_of_the_gtmaps_kernel(gpu):
    """gazemaps.fixation_points at a raw shape small enough for the ground-truth kernel: its points are the cells
    ``fixationmaps > 0`` of gazemaps_from_fixations(out_shape=raw_shape), packed on the device without a round trip."""
    from recurrent_gaze_prediction_amd import gazemaps as gm
    rs = np.random.RandomState(12)
    D1, D2 = 60, 40
    observers = [(rs.randint(0, 50, 70), rs.randint(0, D1, 70), rs.randint(0, D2, 70), 50) for _ in range(3)]
    packed = gm.pack_fixations(observers, (D1, D2), frames=np.arange(0, 50, 3))
    maps = gm.gazemaps_from_fixations(packed, out_shape=(D1, D2), sigma=1.0, want='fixationmaps', device=gpu)['fixationmaps']
    assert tuple(maps.shape[1:]) == (D2, D1)
    dptr, didx = emg.pack_points(maps, (D2, D1))
    assert dptr.is_cuda and didx.is_cuda
    ptr, idx = gm.fixation_points(packed)
    assert np.array_equal(dptr.cpu().numpy(), ptr) and np.array_equal(didx.cpu().numpy(), idx)


# ------------------------------------------------------------------ models and driver
class SparseFixations(object):
    """A model whose generate() hands out scipy.sparse fixation maps of 45 x 80 -- what the reference's loader does with
    fixation_original_scale=True -- beside its own 49 x 49 maps."""
    def __init__(self, model):
        self.model, self.n_lstm_steps = model, model.n_lstm_steps

    def generate(self, dataset, max_instances=50):
        ret = self.model.generate(dataset, max_instances)
        rs = np.random.RandomState(41)
        maps = []
        for _ in range(len(ret['pred_gazemap_list'])):
            k = rs.randint(3, 9)
            maps.append(scipy.sparse.coo_matrix((np.ones(k, np.float32), (rs.randint(0, 45, k), rs.randint(0, 80, k))), shape=(45, 80)))
        ret['fixationmap_list'] = maps
        return ret


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


def test_evaluate_and_run_evaluation_at_frame_resolution(gpu, tmp_path):
    from recurrent_gaze_prediction_amd.models.evaluate_gaze import FRAME_METRICS, run_evaluation
    model, ds = make_model(gpu, tmp_path)
    wrapped = SparseFixations(model)
    ret = wrapped.generate(ds.valid, max_instances=8)
    assert ret['fixationmap_list'][0].shape == (45, 80) and np.asarray(ret['pred_gazemap_list']).shape[1:] == (49, 49)
    np.random.seed(31)
    host = model.evaluate(scorer='host', **ret)
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
    assert dev == dev2 and abs(dev['sim'] - host['sim']) < TOL and abs(dev['cc'] - host['cc']) < TOL

    outs = {}
    for scorer in ('host', 'device-reference', 'device'):
        ds.valid = syn.SyntheticDataSet(8, 4, seed=21)                # the loader has a cursor: same frames for each run
        out = str(tmp_path / scorer)
        overall = run_evaluation(wrapped, ds, out, num_frames=12, seed=3, scorer=scorer)
        outs[scorer] = (overall, open(os.path.join(out, 'overall.txt')).read(),
                        [open(os.path.join(out, '%05d.scores.txt' % i)).read() for i in range(16)])
    host, ref, dev = outs['host'], outs['device-reference'], outs['device']
    assert list(ref[0]) == list(host[0]) == list(FRAME_METRICS)
    assert ref[1] == host[1]                                          # overall.txt, character for character
    assert ref[2] == host[2]                                          # and every NNNNN.scores.txt
    assert dev[1].splitlines()[:4] == host[1].splitlines()[:4]        # sim and cc take no draws
    ds.valid = syn.SyntheticDataSet(8, 4, seed=21)
    assert run_evaluation(wrapped, ds, str(tmp_path / 'again'), num_frames=12, seed=3, scorer='device') == dev[0]
    with pytest.raises(ValueError, match='differ in shape'):          # the equal-shape entry is as it was
        emg.saliency_scores_single(ret['pred_gazemap_list'], ret['gt_gazemap_list'],
                                   np.stack([f.toarray() for f in ret['fixationmap_list']]), None, ['sim'])
