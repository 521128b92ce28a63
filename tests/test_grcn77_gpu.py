"""GPU: gaze_grcn77 / gaze_rnn77 through the C ABI against the float64 helper (tests/grcn77_ref.py).

The read-out (csrc/head_point.hip.h) is fp32 arithmetic on the fp32 ConvGRU state in both plan dtypes, so it is held to the
project's f32 bound (2e-5 of the tensor's max, tests/test_grcn_gpu.py) for bf16 plans too, measured against float64 on the
SAME device states; the projection and the ConvGRU keep the bounds of tests/test_grcn_gpu.py, gradients those of
tests/test_backward_gpu.py (relative Frobenius per tensor; out_b under xentropy is exactly zero in theory and is bounded as
that file bounds it, |g| < 1e-6).  Both recurrence paths are asked for by name.  Every test prints its figures before it
asserts (-s); the measured values are in DESIGN.md, "gaze_grcn77 / gaze_rnn77"."""
import numpy as np
import pytest
import torch

import grcn77_ref as ref
from recurrent_gaze_prediction_amd import synthetic as syn

pytestmark = pytest.mark.gpu

F32 = 2e-5                                            # of the tensor's max: the project's f32 bound
TOL = {'f32': 2e-5, 'bf16': 2e-2}                     # tests/test_grcn_gpu.py: TOL, TOL_H_MAX, TOL_H_RMS
TOL_H_MAX = {'f32': 5e-5, 'bf16': 6e-2}
TOL_H_RMS = {'f32': 1e-5, 'bf16': 1e-2}
GRAD_TOL = {'f32': 2e-4, 'bf16': 3e-2}                # tests/test_backward_gpu.py: TOL
GRAD_TOL_35 = {'f32': 1e-3, 'bf16': 3e-2}             # ... its 35-step bounds
# 3 x 4: B != T (a time-major / frame-major mix-up shows), 588 rows; 33 x 3: ragged last group of the persistent kernel,
# 99 frames = 24 blocks of 4 + 3; 2 x 16: a longer recurrence
SHAPES = [(3, 4), (33, 3), (2, 16)]
PLANS = [('f32', False), ('bf16', False), ('bf16', True)]        # (dtype, per_step)


def rel_err(a, r):
    a, r = np.asarray(a, np.float64), np.asarray(r, np.float64)
    return np.abs(a - r).max() / max(np.abs(r).max(), 1e-30)


def fro_err(a, r):
    a, r = np.asarray(a, np.float64), np.asarray(r, np.float64)
    return np.linalg.norm(a - r) / max(np.linalg.norm(r), 1e-30)


_CASE, _GRADS = {}, {}


def case(B, T):
    """(params, features, labels, float64 (logits, states, emb)), computed once per session and left unchanged."""
    if (B, T) not in _CASE:
        p = syn.grcn77_params(51)
        x = syn.c3d_features(52 + B, B, T)
        _CASE[(B, T)] = (p, x, ref.normalized_labels(53 + B, B, T), ref.forward_f64(x, p))
    return _CASE[(B, T)]


def ref_grads(B, T, loss_type):
    if (B, T, loss_type) not in _GRADS:
        p, x, g, _ = case(B, T)
        _GRADS[(B, T, loss_type)] = ref.loss_and_grads(x, g, p, loss_type)
    return _GRADS[(B, T, loss_type)]


def engine(B, T, dtype, gpu, per_step=False, save=False, params=None):
    from recurrent_gaze_prediction_amd.engine import Grcn77Engine
    eng = Grcn77Engine(B, T, dtype=dtype, device=gpu, per_step=per_step, save_for_backward=save)
    assert eng.persistent == (dtype == 'bf16' and not per_step)
    if params is not None:
        eng.set_weights(params)
    return eng


def head64(states, p):
    return ref.head_f64(torch.tensor(np.asarray(states, np.float64)), torch.tensor(p['out_W'], dtype=torch.float64),
                        torch.tensor(p['out_b'], dtype=torch.float64)).numpy()


# ------------------------------------------------------------------------------------------------ 1. the head alone
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('B,T', SHAPES)
def test_head_on_the_device_states(gpu, dtype, B, T):
    p, x, _, _ = case(B, T)
    eng = engine(B, T, dtype, gpu, params=p)
    logits, probs = eng.forward(torch.tensor(x, device=gpu))
    h = eng.read_buffer('rcn_outputs').cpu().numpy().reshape(B, T, 7, 7, 128)
    z, pr = logits.cpu().numpy(), probs.cpu().numpy()
    assert z.shape == (B, T, 7, 7) and np.isfinite(z).all() and np.abs(h).max() > 0.1
    e_z, e_p = rel_err(z, head64(h, p)), rel_err(pr, ref.softmax49(z))
    e_s = np.abs(pr.reshape(B * T, 49).astype(np.float64).sum(-1) - 1).max()
    print('head %s %dx%d: logits %.2e probs %.2e |sum-1| %.2e' % (dtype, B, T, e_z, e_p, e_s))
    assert e_z < F32 and e_p < F32 and e_s < 1e-5
    z2, p2 = eng.head_forward()                                # the stage on the plan's own states: the same launch
    assert torch.equal(z2, logits) and torch.equal(p2, probs)


# ------------------------------------------------------------------------------------------------ 2. states, end to end
@pytest.mark.parametrize('dtype,per_step', PLANS)
@pytest.mark.parametrize('B,T', SHAPES)
def test_states_and_logits_match_float64(gpu, dtype, per_step, B, T):
    p, x, _, (ref_z, ref_h, ref_emb) = case(B, T)
    eng = engine(B, T, dtype, gpu, per_step=per_step, params=p)
    logits, _ = eng.forward(torch.tensor(x, device=gpu))
    emb = eng.read_buffer('c3d_embedded').cpu().numpy().reshape(ref_emb.shape)
    h = eng.read_buffer('rcn_outputs').cpu().numpy().reshape(ref_h.shape)
    e_emb, e_h = rel_err(emb, ref_emb), rel_err(h, ref_h)
    e_rms = np.sqrt(((h - ref_h) ** 2).mean()) / np.sqrt((ref_h ** 2).mean())
    e_z = rel_err(logits.cpu().numpy(), ref_z)
    print('states %s per_step=%d %dx%d: emb %.2e h max %.2e rms %.2e logits %.2e' % (dtype, per_step, B, T, e_emb, e_h, e_rms, e_z))
    assert e_emb < TOL[dtype], 'projection'
    assert e_h < TOL_H_MAX[dtype] and e_rms < TOL_H_RMS[dtype], 'ConvGRU states'
    if dtype == 'f32':
        assert e_z < F32, 'end-to-end logits'


# ------------------------------------------------------------------------------------------------ 3. the head stage
@pytest.mark.parametrize('B,T', [(3, 4), (33, 3)])
def test_head_stage_on_callers_states(gpu, B, T):
    p = case(B, T)[0]
    eng = engine(B, T, 'f32', gpu, params=p)
    rs = np.random.RandomState(7 + B)
    # (a) logits of about +-200: sigma = 95 * sqrt(128) * 0.1 / sqrt(3) = 62, the largest of B*T*49 draws is > 3 sigma
    s = torch.tensor((rs.randn(B, T, 7, 7, 128) * 95).astype(np.float32), device=gpu)
    z, pr = eng.head_forward(s)
    zc, pc = z.cpu().numpy(), pr.cpu().numpy()
    e_z, e_p = rel_err(zc, head64(s.cpu().numpy(), p)), rel_err(pc, ref.softmax49(zc))
    e_s = np.abs(pc.reshape(B * T, 49).astype(np.float64).sum(-1) - 1).max()
    print('head stage %dx%d: max|logit| %.1f logits %.2e probs %.2e |sum-1| %.2e' % (B, T, np.abs(zc).max(), e_z, e_p, e_s))
    assert 150 < np.abs(zc).max() < 400 and np.isfinite(pc).all()
    assert e_z < F32 and e_p < F32 and e_s < 1e-5
    # (d) two calls: the same bits
    z2, p2 = eng.head_forward(s)
    assert torch.equal(z, z2) and torch.equal(pr, p2)
    # (b) one frame's states NaN: exactly that frame is NaN, every other frame keeps its bits
    fb, ft = B - 1, 1
    bad = s.clone()
    bad[fb, ft] = float('nan')
    zb, pb = eng.head_forward(bad)
    nan_z, nan_p = torch.isnan(zb).reshape(B * T, 49), torch.isnan(pb).reshape(B * T, 49)
    f = fb * T + ft
    assert nan_z[f].all() and nan_p[f].all() and int(nan_z.sum()) == 49 and int(nan_p.sum()) == 49
    keep = torch.ones(B * T, dtype=torch.bool, device=gpu)
    keep[f] = False
    assert torch.equal(zb.reshape(B * T, 49)[keep], z.reshape(B * T, 49)[keep])
    assert torch.equal(pb.reshape(B * T, 49)[keep], pr.reshape(B * T, 49)[keep])
    # (c) clips permuted: the logits are the same permutation, bit for bit
    perm = torch.tensor(rs.permutation(B), device=gpu)
    zp, pp = eng.head_forward(s[perm].contiguous())
    assert torch.equal(zp, z[perm]) and torch.equal(pp, pr[perm])


# ------------------------------------------------------------------------------------------------ 4. gradients
def check_grads(gpu, B, T, dtype, per_step, loss_type, tol):
    p, x, g, _ = case(B, T)
    _, _, want, want_dx = ref_grads(B, T, loss_type)
    eng = engine(B, T, dtype, gpu, per_step=per_step, save=True, params=p)
    xd, gd = torch.tensor(x, device=gpu), torch.tensor(g, device=gpu)
    logits, probs = eng.forward(xd)
    grads = {k: v.clone() for k, v in eng.backward(logits, probs, gd, loss_type).items()}
    d_h = eng.read_buffer('d_rcn_outputs').clone()
    d_rows = eng.backward_input().cpu().numpy()
    # the head's state gradient against float64 from the device logits / probs (the function dlogits_kernel computes)
    a = (logits if loss_type == 'l2' else probs).cpu().numpy().astype(np.float64)
    g64 = g.astype(np.float64)
    gs = 1.0 if loss_type == 'l2' else g64.reshape(B, T, 49).sum(-1).reshape(B, T, 1, 1)
    dz = (a * gs - g64) / (B * T)
    want_dh = dz[..., None] * p['out_W'].astype(np.float64).reshape(128)
    e_dh = rel_err(d_h.cpu().numpy().reshape(B, T, 7, 7, 128), want_dh)
    errs = {k: fro_err(grads[k].cpu().numpy(), want[k]) for k in ref.KEYS if not (k == 'out_b' and loss_type == 'xentropy')}
    errs['d_rows'] = fro_err(d_rows, ref.rows_of(want_dx))
    print('grads %s per_step=%d %s %dx%d: d_rcn_outputs %.2e; ' % (dtype, per_step, loss_type, B, T, e_dh) +
          ' '.join('%s %.2e' % (k.replace('GRU_Conv_', ''), v) for k, v in errs.items()))
    assert e_dh < F32
    if loss_type == 'xentropy':            # d loss / d out_b = sum_j (p_j sum(g) - g_j) / (BT) = 0 exactly: round-off remains
        print('out_b (xentropy): %.2e' % abs(grads['out_b'].item()))
        assert abs(grads['out_b'].item()) < 1e-6 and abs(want['out_b'].item()) < 1e-12
    assert max(errs.values()) < tol, errs
    # a second backward: the read-out's results keep their bits
    again = eng.backward(logits, probs, gd, loss_type)
    assert torch.equal(again['out_W'], grads['out_W']) and torch.equal(again['out_b'], grads['out_b'])
    assert torch.equal(eng.read_buffer('d_rcn_outputs'), d_h)


@pytest.mark.parametrize('dtype,per_step', PLANS)
@pytest.mark.parametrize('loss_type', ['xentropy', 'l2'])
@pytest.mark.parametrize('B,T', [(3, 4), (33, 3)])
def test_gradients_match_autograd(gpu, dtype, per_step, loss_type, B, T):
    check_grads(gpu, B, T, dtype, per_step, loss_type, GRAD_TOL[dtype])


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_bptt_through_35_steps_matches_autograd(gpu, dtype):
    check_grads(gpu, 2, 35, dtype, False, 'xentropy', GRAD_TOL_35[dtype])


# ------------------------------------------------------------------------------------------------ 5. the two recurrence paths
@pytest.mark.parametrize('B,T', [(3, 4), (33, 3)])
def test_persistent_agrees_with_per_step(gpu, B, T):
    p, x, _, _ = case(B, T)
    out = []
    for per_step in (False, True):
        eng = engine(B, T, 'bf16', gpu, per_step=per_step, params=p)
        logits, _ = eng.forward(torch.tensor(x, device=gpu))
        out.append((eng.read_buffer('rcn_outputs').cpu().numpy(), logits.cpu().numpy()))
        if per_step:
            with pytest.raises(NotImplementedError):
                eng.inject_fault('seq')
    e_h, e_z = rel_err(out[0][0], out[1][0]), rel_err(out[0][1], out[1][1])
    print('persistent vs per-step %dx%d: h %.2e logits %.2e' % (B, T, e_h, e_z))
    assert e_h < 2e-2 and e_z < 1e-2                            # tests/test_grcn_gpu.py:160


def test_c_abi_argument_checks(gpu):
    from recurrent_gaze_prediction_amd import _lib
    eng = engine(2, 2, 'bf16', gpu)
    x = torch.zeros(2, 2, 1024, 7, 7, device=gpu)
    with pytest.raises(_lib.RgpError, match='weights not set') as info:
        eng.forward(x)
    assert info.value.code == -4
    eng.set_weights(syn.grcn77_params(1))
    eng.forward(x)
    with pytest.raises(_lib.RgpError, match='unknown intermediate'):
        eng.read_buffer('d_rcn_outputs')                       # an inference plan has none
    assert eng.read_buffer_elems('rcn_outputs') == 2 * 2 * 49 * 128 and eng.read_buffer_elems('bn') == 0


# ------------------------------------------------------------------------------------------------ 6. model classes
def make_model(gpu, tmp_path, T=3, B=2, dtype='bf16', trainable=True, loss_type='xentropy'):
    from recurrent_gaze_prediction_amd.models.base import Session
    from recurrent_gaze_prediction_amd.models.gaze_grcn77 import CONSTANTS, GazePredictionGRCN, GRUModelConfig
    assert CONSTANTS.gazemap_height == 7
    cfg = GRUModelConfig()
    cfg.batch_size, cfg.n_lstm_steps, cfg.loss_type, cfg.compute_dtype = B, T, loss_type, dtype
    cfg.trainable, cfg.train_dir = trainable, str(tmp_path)
    ds = type('DS', (), {})()
    ds.train = ds.valid = syn.SyntheticDataSet(12, T, seed=5, gazemap_hw=7)
    return GazePredictionGRCN(Session(gpu), ds, cfg), ds


def test_model_trains_and_generates_7x7_maps(gpu, tmp_path):
    model, ds = make_model(gpu, tmp_path)
    assert (model.gazemap_height, model.gazemap_width) == (7, 7) and not model._has_dropout()
    model.load_state_dict(syn.grcn77_params(61))
    model.config.use_flip_batch = False
    model.config.initial_learning_rate = 1e-3
    model.initial_learning_rate = 1e-3
    before = model.state_dict()
    fixed = syn.SyntheticDataSet(2, 3, seed=5, gazemap_hw=7)            # two clips: every step sees the same batch
    losses = []
    for _ in range(6):
        model.single_step(train_mode=True, dataset=fixed)
        losses.append(model.loss)
    print('grcn77 training losses', ' '.join('%.4f' % v for v in losses))
    assert losses[-1] < losses[0] - 1e-3, losses
    after = model.state_dict()
    assert all(not np.array_equal(before[k], after[k]) for k in ref.KEYS)
    ret = model.generate(ds.valid, max_instances=4)
    assert ret['pred_gazemap_list'].shape == (4 * 3, 7, 7) and ret['gt_gazemap_list'].shape == (12, 7, 7)
    assert np.allclose(ret['pred_gazemap_list'].reshape(12, -1).sum(-1), 1.0, atol=1e-5)


def test_model_per_step_config_is_honoured(gpu, tmp_path):
    from recurrent_gaze_prediction_amd.models.base import Session
    from recurrent_gaze_prediction_amd.models.gaze_grcn77 import GazePredictionGRCN, GRUModelConfig
    cfg = GRUModelConfig()
    cfg.batch_size, cfg.n_lstm_steps, cfg.trainable, cfg.train_dir, cfg.convgru_per_step = 2, 2, False, str(tmp_path), True
    model = GazePredictionGRCN(Session(gpu), None, cfg)
    assert model.engine.per_step and not model.engine.persistent
    assert not model._recover_from_timeout()                    # already the fall-back


def test_model_checkpoint_evaluation_and_long_clip(gpu, tmp_path):
    from recurrent_gaze_prediction_amd import checkpoint
    from recurrent_gaze_prediction_amd.evaluation_metrics import AVAILABLE_METRICS
    from recurrent_gaze_prediction_amd.models.evaluate_gaze import predict_long_clip
    model, ds = make_model(gpu, tmp_path, trainable=False)
    p = syn.grcn77_params(62)
    model.load_state_dict(p)
    _, _, _, c3d, _, _ = syn.SyntheticDataSet(12, 3, seed=5, gazemap_hw=7).next_batch(2)
    model.predict(c3d)
    z1 = model.predicted_gazemaps_logit.clone()
    state = model.state_dict()
    assert all(np.array_equal(state[k], p[k]) for k in ref.KEYS)
    tf_vars = {k + ':0': v for k, v in checkpoint.export_model_variables('gaze_grcn77', state).items()}
    assert 'RCNBottom/out_W:0' in tf_vars and 'proj_c3d_W:0' in tf_vars
    model2, _ = make_model(gpu, tmp_path / 'b', trainable=False)
    model2.load_state_dict(checkpoint.import_model_variables('gaze_grcn77', tf_vars))
    model2.predict(c3d)
    assert torch.equal(model2.predicted_gazemaps_logit, z1)    # bit for bit
    ret = model.generate(ds.valid, max_instances=4)            # 12 frames, fixation maps from syn.fixation_maps(hw=7)
    scores = model.evaluate(scorer='device', seed=3, **ret)
    print('grcn77 device scores', scores)
    assert set(scores) == set(AVAILABLE_METRICS) and all(np.isfinite(v) for v in scores.values())
    for pool in (False, True):                                 # a clip longer than T; 7x7 maps are at the pooled size already
        maps = predict_long_clip(model, syn.c3d_features(31, 1, 7)[0], pool_to_7x7=pool)
        assert maps.shape == (7, 7, 7) and np.allclose(maps.reshape(7, -1).sum(-1), 1.0, atol=1e-5)


def test_gaze_rnn77_model_class(gpu, tmp_path):
    """gaze_rnn77.GazePredictionGRU: the parent's fc-GRU with a 7x7 read-out, against oracle.torch_ref.fcgru_forward(gh=7, gw=7)
    within the fc-GRU model-class bound of tests/test_fcgru_gpu.py (1e-4 of max, f32); l2 loss by default: raw maps."""
    from oracle import torch_ref
    from recurrent_gaze_prediction_amd.models.base import Session
    from recurrent_gaze_prediction_amd.models.gaze_rnn77 import GazePredictionGRU, GRUModelConfig
    cfg = GRUModelConfig()
    assert (cfg.n_lstm_steps, cfg.batch_size, cfg.loss_type) == (35, 7, 'l2')
    cfg.batch_size, cfg.n_lstm_steps, cfg.compute_dtype, cfg.train_dir = 2, 4, 'f32', str(tmp_path)
    ds = type('DS', (), {})()
    ds.train = ds.valid = syn.SyntheticDataSet(10, 4, seed=9, gazemap_hw=7)
    model = GazePredictionGRU(Session(gpu), ds, cfg)
    assert (model.gazemap_height, model.gazemap_width) == (7, 7)
    assert model.variables['proj_out_W'].shape == (1617, 49)
    _, _, _, c3d, _, _ = syn.SyntheticDataSet(10, 4, seed=9, gazemap_hw=7).next_batch(2)
    got = model.predict(c3d).cpu().numpy()
    pt = {k: torch.tensor(v) for k, v in model.variables.items()}
    want = torch_ref.fcgru_forward(torch.tensor(c3d.reshape(2, 4, 1024, 7, 7)), pt, gh=7, gw=7).numpy()
    e = rel_err(got, want)
    print('gaze_rnn77 forward: %.2e' % e)
    assert got.shape == (2, 4, 7, 7) and e < 1e-4
    model.config.use_flip_batch = False
    before = model.state_dict()
    assert model.single_step(train_mode=True) == 1 and np.isfinite(model.loss)
    after = model.state_dict()
    assert any(not np.array_equal(before[k], after[k]) for k in before)
