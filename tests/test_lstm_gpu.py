"""GPU: gaze_lstm through the C ABI against the float64 helper (tests/lstm_ref.py): f32 plans within the project's f32 bound,
bf16 plans (the persistent kernel and the per-step path, each) within twice the error of the bf16-operand emulation, the two
paths against each other, determinism and batch independence of the persistent kernel, gradients against float64 autograd,
the time-out path, and the model class (training step, checkpoint, evaluation).

bf16 bounds: for every shape and tensor the emulation's own error against float64 is computed here (relative Frobenius per
step, max-abs over max|ref|); the device may be at most twice as far.  Max-abs is asserted for T <= 16 only.  Every test prints
its figures before it asserts (-s).  Both recurrence paths are asked for by name, so the tests hold whatever the default is.
Measured on an MI355X ("gaze_lstm"): h_t at the worst step 4.4 - 4.6e-3 relative Frobenius on both paths, on top of
the emulation's own 4.4 - 4.6e-3; f32 <= 6.8e-6 of max|h|; gradients f32 <= 2.2e-6, bf16 <= 1.7e-2."""
import numpy as np
import pytest
import torch

import lstm_ref as ref
from recurrent_gaze_prediction_amd import synthetic as syn

pytestmark = pytest.mark.gpu

F32_TOL = 2e-5                                  # of the tensor's max (the project's f32 bound, tests/test_grcn_gpu.py)
GRAD_TOL = {'f32': 1e-3, 'bf16': 3e-2}          # relative Frobenius (the project's gradient bounds)
SHAPES = [(3, 4), (2, 16), (2, 42), (64, 16), (33, 5)]      # 33 x 5 is ragged: the last group of the persistent kernel has one clip
TENSORS = ('emb', 'i', 'f', 'g', 'o', 'c', 'h', 'logits')


def rel_err(a, r):
    a, r = np.asarray(a, np.float64), np.asarray(r, np.float64)
    return np.abs(a - r).max() / max(np.abs(r).max(), 1e-30)


def fro_err(a, r):
    a, r = np.asarray(a, np.float64), np.asarray(r, np.float64)
    return np.linalg.norm(a - r) / max(np.linalg.norm(r), 1e-300)


_ORACLE = {}


def oracle(B, T):
    """(params, features, {tensor: float64 [B,T,...]}, {tensor: (fro per step, max-abs) of the bf16 emulation}), once per session."""
    if (B, T) not in _ORACLE:
        p = syn.lstm_params(31)
        x = syn.c3d_features(32 + B, B, T)
        logits, it = ref.forward_f64(x, p)
        want = dict(it, logits=logits)
        want['emb'] = want['emb'].reshape(B, T, 49, 512)
        el, ei = ref.forward_f64(x, p, emulate_bf16=True)
        emu = dict(ei, logits=el)
        emu['emb'] = ref.bf16(torch.tensor(emu['emb'])).numpy().reshape(B, T, 49, 512)      # the operand the x convolutions read
        bound = {k: ref.step_errors(emu[k], want[k]) for k in TENSORS}
        _ORACLE[(B, T)] = (p, x, want, bound)
    return _ORACLE[(B, T)]


def engine(B, T, dtype, gpu, per_step=False, save=False, params=None):
    """Both recurrence paths are asked for by name (bf16: RGP_LSTM_PERSISTENT / RGP_LSTM_PER_STEP), whatever the default is."""
    from recurrent_gaze_prediction_amd.engine import LstmEngine
    eng = LstmEngine(B, T, dtype=dtype, device=gpu, per_step=per_step, persistent=(dtype == 'bf16' and not per_step),
                     save_for_backward=save)
    if params is not None:
        eng.set_weights(params)
    return eng


def read_all(eng, logits, B, T):
    out = {'logits': logits.cpu().numpy()}
    for k in TENSORS[:-1]:
        shape = (B, T, 49, 512) if k == 'emb' else (B, T, 7, 7, 128)
        out[k] = eng.read_buffer(k).cpu().numpy().reshape(shape)
    return out


@pytest.mark.parametrize('B,T', SHAPES)
def test_f32_forward_matches_float64(gpu, B, T):
    p, x, want, _ = oracle(B, T)
    eng = engine(B, T, 'f32', gpu, save=True, params=p)
    assert not eng.persistent
    logits, probs = eng.forward(torch.tensor(x, device=gpu))
    got = read_all(eng, logits, B, T)
    for k in TENSORS:
        err = rel_err(got[k], want[k])
        print('f32 %dx%d %s: %.3e of max %.3f' % (B, T, k, err, np.abs(want[k]).max()))
        assert err < F32_TOL, k
    pr = probs.cpu().numpy().astype(np.float64).reshape(B * T, -1)
    assert np.abs(pr.sum(-1) - 1.0).max() < 1e-4


def check_bf16(tag, got, want, bound, T):
    for k in TENSORS:
        fro, mx = ref.step_errors(got[k], want[k])
        efro, emx = bound[k]
        worst = int(np.argmax(fro / efro))
        print('%s %s: fro step %d %.3e (emulation %.3e), max-abs %.3e (emulation %.3e)' % (tag, k, worst, fro[worst], efro[worst], mx, emx))
    for k in TENSORS:
        fro, mx = ref.step_errors(got[k], want[k])
        efro, emx = bound[k]
        assert (fro <= 2.0 * efro).all(), (k, fro, efro)
        if T <= 16:
            assert mx <= 2.0 * emx, (k, mx, emx)


@pytest.mark.parametrize('per_step', [False, True], ids=['persistent', 'per_step'])
@pytest.mark.parametrize('B,T', SHAPES)
def test_bf16_forward_within_twice_the_emulation_error(gpu, B, T, per_step):
    p, x, want, bound = oracle(B, T)
    eng = engine(B, T, 'bf16', gpu, per_step=per_step, save=True, params=p)
    assert eng.persistent == (not per_step)
    logits, probs = eng.forward(torch.tensor(x, device=gpu))
    eng.status()
    got = read_all(eng, logits, B, T)
    assert all(np.isfinite(v).all() for v in got.values())
    check_bf16('bf16 %s %dx%d' % ('per-step' if per_step else 'persistent', B, T), got, want, bound, T)
    assert np.abs(probs.cpu().numpy().astype(np.float64).reshape(B * T, -1).sum(-1) - 1.0).max() < 1e-4


@pytest.mark.parametrize('B,T', SHAPES)
def test_persistent_against_per_step_same_inputs(gpu, B, T):
    p, x, want, bound = oracle(B, T)
    xd = torch.tensor(x, device=gpu)
    a = engine(B, T, 'bf16', gpu, params=p)
    b = engine(B, T, 'bf16', gpu, per_step=True, params=p)
    la, _ = a.forward(xd)
    lb, _ = b.forward(xd)
    ga, gb = read_all_inference(a, la, B, T), read_all_inference(b, lb, B, T)
    for k in ('c', 'h', 'logits'):
        d = ga[k] - gb[k]
        t_axis = d.transpose(1, 0, *range(2, d.ndim)).reshape(T, -1)
        r = want[k].transpose(1, 0, *range(2, d.ndim)).reshape(T, -1)
        fro = np.sqrt((t_axis ** 2).sum(1)) / np.sqrt((r ** 2).sum(1))
        mx = np.abs(d).max() / np.abs(want[k]).max()
        print('persistent vs per-step %dx%d %s: fro %.3e (bound %.3e), max-abs %.3e' % (B, T, k, fro.max(), 2 * bound[k][0].max(), mx))
        assert (fro <= 2.0 * bound[k][0]).all(), k
        if T <= 16:
            assert mx <= 2.0 * bound[k][1], k


def read_all_inference(eng, logits, B, T):
    return {'logits': logits.cpu().numpy(), 'c': eng.read_buffer('c').cpu().numpy().reshape(B, T, 7, 7, 128),
            'h': eng.read_buffer('h').cpu().numpy().reshape(B, T, 7, 7, 128)}


def test_persistent_is_deterministic_and_independent_of_the_batch(gpu):
    p, x, _, _ = oracle(64, 16)
    xd = torch.tensor(x, device=gpu)
    eng = engine(64, 16, 'bf16', gpu, params=p)
    assert eng.persistent and eng.persistent_workgroups == 256
    l1, p1 = [t.clone() for t in eng.forward(xd)]
    h1 = eng.read_buffer('h').clone()
    l2, p2 = eng.forward(xd)
    assert torch.equal(l1, l2) and torch.equal(p1, p2) and torch.equal(h1, eng.read_buffer('h'))
    two = engine(2, 16, 'bf16', gpu, params=p)                  # one clip per group, 4 row fragments instead of 7
    for k in (0, 1, 37, 63):                                   # both slots of a group, somewhere in the middle, the last clip
        pair = torch.stack([xd[k], xd[(k + 5) % 64]]).contiguous()
        lk, pk = two.forward(pair)
        hk = two.read_buffer('h').reshape(2, 16, 49, 128)
        assert torch.equal(hk[0], h1.reshape(64, 16, 49, 128)[k]), k
        assert torch.equal(lk[0], l1[k]) and torch.equal(pk[0], p1[k]), k


def test_default_paths(gpu):
    """flags = 0: the persistent kernel where it applies (measured faster at both benchmark shapes), else per step."""
    from recurrent_gaze_prediction_amd.engine import LstmEngine
    assert LstmEngine(2, 2, dtype='bf16', device=gpu).persistent
    assert not LstmEngine(2, 2, dtype='f32', device=gpu).persistent
    assert not LstmEngine(65, 1, dtype='bf16', device=gpu).persistent
    assert not LstmEngine(2, 2, dtype='bf16', device=gpu, per_step=True).persistent


def labels_for(seed, B, T):
    gt, _ = syn.gaze_maps(seed, B, T)
    return (gt / gt.sum((2, 3), keepdims=True)).astype(np.float32)


@pytest.mark.parametrize('dtype,per_step,B,T,loss_type', [
    ('f32', True, 2, 3, 'xentropy'), ('f32', True, 2, 3, 'l2'), ('bf16', False, 2, 3, 'xentropy'), ('bf16', False, 2, 3, 'l2'),
    ('bf16', True, 2, 3, 'xentropy'), ('f32', True, 2, 35, 'xentropy'), ('bf16', False, 2, 35, 'xentropy')])
def test_gradients_match_float64_autograd(gpu, dtype, per_step, B, T, loss_type):
    p = syn.lstm_params(71)
    x = syn.c3d_features(72, B, T)
    gt = labels_for(73, B, T)
    _, _, want = ref.loss_and_grads(x, gt, p, loss_type)
    assert want['ConvLSTM_Whc'] is None
    eng = engine(B, T, dtype, gpu, per_step=per_step, save=True, params=p)
    xd, gd = torch.tensor(x, device=gpu), torch.tensor(gt, device=gpu)
    logits, probs = eng.forward(xd)
    grads = {k: v.clone() for k, v in eng.backward(logits, probs, gd, loss_type).items()}
    assert set(grads) == set(ref.KEYS)
    assert grads['ConvLSTM_Whc'].abs().max().item() == 0.0     # exactly zero
    assert eng.flat_grads.numel() == sum(v.numel() for k, v in grads.items() if k != 'ConvLSTM_Whc')
    bad = []
    for k in ref.KEYS:
        if k == 'ConvLSTM_Whc':
            continue
        if k == 'out_b' and loss_type == 'xentropy':
            # d loss / d out_b = 0 exactly for normalised labels: only round-off remains (tests/test_c3d_conv_gpu.py)
            assert abs(grads[k].item()) < 1e-6 and abs(want[k].item()) < 1e-12
            continue
        err = fro_err(grads[k].cpu().numpy(), want[k])
        print('grad %s %s %s %dx%d %s: %.3e' % (dtype, 'per-step' if per_step else 'persistent', loss_type, B, T, k, err))
        if not err <= GRAD_TOL[dtype]:
            bad.append((k, err))
    assert not bad, bad


def to_rows(xd, dtype):
    """[B,T,1024,7,7] (channel c*2+d) -> conv5b rows [B*T*49, 1024] with column d*512+c, as C3DEngine writes them."""
    td = torch.bfloat16 if dtype == 'bf16' else torch.float32
    return xd.permute(0, 1, 3, 4, 2).reshape(-1, 512, 2).transpose(1, 2).reshape(-1, 1024).contiguous().to(td)


def rows_grad_to_input(d_rows, B, T):
    """d_rows [B*T*49, 1024] (column d*512+c) -> the gradient in the placeholder layout [B,T,1024,7,7] (channel c*2+d)."""
    d = np.asarray(d_rows, np.float64).reshape(B, T, 7, 7, 2, 512)            # (.., d, c)
    return d.transpose(0, 1, 5, 4, 2, 3).reshape(B, T, 1024, 7, 7)


# forward_rows feeds the same products to the projection in another K order (d*512+c instead of c*2+d): fp32 sums differ in
# their last bits, and in bf16 plans a few elements of the bf16 projection output may then round the other way.  Bounds set
# beforehand: the project's f32 bound, and for bf16 the 1e-3 of max|logit| tests/test_c3d_conv_gpu.py allows for the same thing.
ROWS_TOL = {'f32': 2e-5, 'bf16': 1e-3}


@pytest.mark.parametrize('dtype,per_step', [('f32', True), ('bf16', False), ('bf16', True)])
@pytest.mark.parametrize('B,T', [(3, 4), (33, 5)])
def test_forward_rows_matches_forward(gpu, dtype, per_step, B, T):
    p, x, want, _ = oracle(B, T)
    xd = torch.tensor(x, device=gpu)
    eng = engine(B, T, dtype, gpu, per_step=per_step, params=p)
    lf, pf = [t.clone() for t in eng.forward(xd)]
    hf = eng.read_buffer('h').clone()
    ef = eng.read_buffer('emb').clone()
    lr, pr = eng.forward_rows(to_rows(xd, dtype))
    scale = np.abs(want['logits']).max()
    e_emb = (eng.read_buffer('emb') - ef).abs().max().item() / np.abs(want['emb']).max()
    e_h = (eng.read_buffer('h') - hf).abs().max().item() / np.abs(want['h']).max()
    e_l = (lr - lf).abs().max().item() / scale
    print('forward_rows vs forward %s %s %dx%d: emb %.3e, h %.3e, logits %.3e' % (dtype, 'per-step' if per_step else 'persistent', B, T, e_emb, e_h, e_l))
    assert e_l < ROWS_TOL[dtype] and rel_err(lr.cpu().numpy(), want['logits']) < (2e-5 if dtype == 'f32' else 2e-2)
    assert (pr - pf).abs().max().item() < ROWS_TOL[dtype]
    if dtype == 'f32':
        assert e_emb < 2e-5 and e_h < 2e-5


@pytest.mark.parametrize('dtype,per_step,loss_type', [('f32', True, 'xentropy'), ('f32', True, 'l2'), ('bf16', False, 'xentropy'),
                                                      ('bf16', True, 'l2')])
@pytest.mark.parametrize('from_rows', [False, True], ids=['placeholder', 'rows'])
def test_input_gradient_and_rows_training_match_float64_autograd(gpu, dtype, per_step, loss_type, from_rows):
    """backward_input (d loss / d conv5b rows) against autograd's d loss / d c3d_input, after forward() and after
    forward_rows() on a training plan; in the second case every variable's gradient is checked again too (the plan keeps
    X in the placeholder's channel order for the projection's filter gradient)."""
    B, T = 2, 3
    p = syn.lstm_params(71)
    x = syn.c3d_features(72, B, T)
    gt = labels_for(73, B, T)
    _, _, want = ref.loss_and_grads(x, gt, p, loss_type, want_input_grad=True)
    eng = engine(B, T, dtype, gpu, per_step=per_step, save=True, params=p)
    xd, gd = torch.tensor(x, device=gpu), torch.tensor(gt, device=gpu)
    logits, probs = eng.forward_rows(to_rows(xd, dtype)) if from_rows else eng.forward(xd)
    grads = eng.backward(logits, probs, gd, loss_type)
    d_rows = eng.backward_input()
    assert tuple(d_rows.shape) == (B * T * 49, 1024)
    err = fro_err(rows_grad_to_input(d_rows.cpu().numpy(), B, T), want['c3d_input'])
    print('d_rows %s %s %s %s: %.3e' % (dtype, 'per-step' if per_step else 'persistent', loss_type, 'rows' if from_rows else 'placeholder', err))
    assert err <= GRAD_TOL[dtype]
    bad = []
    for k in ref.KEYS:
        if k == 'ConvLSTM_Whc' or (k == 'out_b' and loss_type == 'xentropy'):
            continue
        e = fro_err(grads[k].cpu().numpy(), want[k])
        if not e <= GRAD_TOL[dtype]:
            bad.append((k, e))
    assert not bad, bad
    from recurrent_gaze_prediction_amd import _lib
    with pytest.raises(_lib.RgpError, match='after rgp_lstm_backward'):
        engine(B, T, dtype, gpu, per_step=per_step, save=True, params=p).backward_input()


def test_backward_call_order_is_checked(gpu):
    from recurrent_gaze_prediction_amd import _lib
    eng = engine(1, 2, 'bf16', gpu, save=True, params=syn.lstm_params(74))
    z = torch.zeros(1, 2, 49, 49, device=gpu)
    with pytest.raises(_lib.RgpError, match='no forward'):
        eng.backward(z, z, z)
    with pytest.raises(AssertionError):
        engine(1, 2, 'bf16', gpu, params=syn.lstm_params(74)).backward(z, z, z)


def test_lost_group_member_is_loud(gpu):
    """Mirrors tests/test_grcn_gpu.py: one workgroup of group 0 returns at launch, the group gives up at its deadline."""
    from recurrent_gaze_prediction_amd import _lib
    B, T = 3, 4                                                # one clip per group: group 0 = clip 0
    eng = engine(B, T, 'bf16', gpu, params=syn.lstm_params(81))
    x = torch.tensor(syn.c3d_features(82, B, T), device=gpu)
    good_logits, good_probs = [t.clone() for t in eng.forward(x)]
    eng.status()                                               # clean
    eng.inject_fault('seq')
    logits, probs = eng.forward(x)
    with pytest.raises(_lib.RgpError, match='lost a group member') as info:
        eng.status()
    assert info.value.code == _lib.RGP_ETIMEOUT
    assert torch.isnan(logits[0]).all() and torch.isnan(probs[0]).all()
    assert torch.equal(logits[1:], good_logits[1:])            # the other groups never noticed
    eng.status()                                               # reported once, then clear
    eng.inject_fault('seq')
    eng.forward(x)
    torch.cuda.synchronize()
    with pytest.raises(_lib.RgpError, match='lost a group member'):
        eng.forward(x)                                         # the error also surfaces on the next call
    logits2, _ = eng.forward(x)
    assert torch.equal(logits2, good_logits)                   # the plan is usable again, bit for bit
    with pytest.raises(_lib.RgpError):
        engine(B, T, 'bf16', gpu, per_step=True, params=syn.lstm_params(81)).inject_fault('seq')


# ---------------------------------------------------------------------------------------------------- model class
def make_model(gpu, tmp_path, T=3, B=2, dtype='bf16', trainable=True, per_step=False):
    from recurrent_gaze_prediction_amd.models.base import Session
    from recurrent_gaze_prediction_amd.models.gaze_lstm import CONSTANTS, GazePredictionLSTM, GRUModelConfig
    assert CONSTANTS.gazemap_height == 49
    cfg = GRUModelConfig()
    cfg.batch_size, cfg.n_lstm_steps, cfg.loss_type, cfg.compute_dtype = B, T, 'xentropy', dtype
    cfg.trainable, cfg.convlstm_path = trainable, ('per_step' if per_step else 'persistent')
    cfg.train_dir = str(tmp_path)
    ds = type('DS', (), {})()
    ds.train = ds.valid = syn.SyntheticDataSet(12, T, seed=5)
    return GazePredictionLSTM(Session(gpu), ds, cfg), ds


def test_model_recomputes_a_timed_out_batch_per_step(gpu, tmp_path):
    model, _ = make_model(gpu, tmp_path, trainable=False)
    model.load_state_dict(syn.lstm_params(91))
    _, _, _, c3d, _, _ = syn.SyntheticDataSet(12, 3, seed=5).next_batch(2)
    assert model.engine.persistent
    good = model.predict(c3d).cpu().numpy()
    model.engine.inject_fault('seq')
    again = model.predict(c3d).cpu().numpy()                   # RGP_ETIMEOUT inside: recomputed on the per-step path
    assert model.engine.per_step and not model.engine.persistent and np.isfinite(again).all()
    assert rel_err(again, good) < 2e-2


def test_one_training_step_moves_every_variable_but_w_hc(gpu, tmp_path):
    model, _ = make_model(gpu, tmp_path, B=2)
    model.load_state_dict(syn.lstm_params(92))
    model.config.use_flip_batch = False
    before = model.state_dict()
    assert model.single_step(train_mode=True) == 1
    after = model.state_dict()
    assert float(model.grad_norm.item()) > 0
    for k in ref.KEYS:
        if k == 'ConvLSTM_Whc':
            assert np.array_equal(before[k], after[k])
        else:
            assert not np.array_equal(before[k], after[k]), k


def test_checkpoint_export_import_and_evaluation(gpu, tmp_path):
    from recurrent_gaze_prediction_amd import checkpoint
    from recurrent_gaze_prediction_amd.models.evaluate_gaze import FRAME_METRICS, predict_long_clip, run_evaluation
    model, ds = make_model(gpu, tmp_path, trainable=False)
    p = syn.lstm_params(93)
    model.load_state_dict(p)
    _, _, _, c3d, _, _ = syn.SyntheticDataSet(12, 3, seed=5).next_batch(2)
    model.predict(c3d)
    z1 = model.predicted_gazemaps_logit.clone()
    tf_vars = {k + ':0': v for k, v in checkpoint.export_model_variables('gaze_lstm', model.state_dict()).items()}
    assert np.array_equal(tf_vars['RGP/RCNBottom/ConvLSTM_Whc:0'], p['ConvLSTM_Whc'])
    model2, _ = make_model(gpu, tmp_path / 'b', trainable=False)
    model2.load_state_dict(checkpoint.import_model_variables('gaze_lstm', tf_vars))
    model2.predict(c3d)
    assert torch.equal(model2.predicted_gazemaps_logit, z1)    # bit for bit
    overall = run_evaluation(model, ds, str(tmp_path / 'eval'), num_frames=12, seed=3, scorer='device')
    assert set(overall) == set(FRAME_METRICS) and all(np.isfinite(v) for v in overall.values())
    maps = predict_long_clip(model, syn.c3d_features(31, 1, 7)[0])
    assert maps.shape == (7, 49, 49) and np.allclose(maps.reshape(7, -1).sum(-1), 1.0, atol=1e-4)
