"""GPU: the fc-GRU recurrence of f32 plans as one persistent launch (RGP_FCGRU_PERSISTENT_F32, csrc/fcgru_seq_f32.hip.h).

Shapes (B, T): (3,4) one partial row fragment, (17,3) a full one plus a ragged one, (33,2) three fragments, (64,3) the full four;
(3,4) once more with the 49x49 map.  Every gate of every step against the one-step float64 reference on the device's own fp32
operands (tests/fcgru_f32_local_ref.py: gates GATE_TOL, blend BLEND_TOL, rh / hp / slot (b, 0) exact); the logits against
oracle.torch_ref.fcgru_forward at the f32 bound of tests/test_fcgru_gpu.py, 5e-5, the per-step f32 plan held to the same bound
beside it (the two paths sum K in different orders: they are NOT compared bit for bit); the per-step backward behind the
persistent forward against float64 autograd at that file's f32 bound, 5e-4; determinism and counter reset; streaming
(tests/fcgru_stream_ref.py); gaze_rnn77.  status() is clean after each.  Figures are printed before the asserts (-s)."""
import numpy as np
import pytest
import torch

import fcgru_local_ref as ref
import fcgru_f32_local_ref as ref32
import fcgru_stream_ref as sr
from oracle import torch_ref
from recurrent_gaze_prediction_amd import synthetic as syn

pytestmark = pytest.mark.gpu
TOL_F32 = 5e-5                 # tests/test_fcgru_gpu.py TOL['f32'], tests/fcgru_stream_ref.py TOL['f32']
GRAD_TOL_F32 = 5e-4            # tests/test_fcgru_gpu.py:71
SHAPES = [(3, 4, 7), (17, 3, 7), (33, 2, 7), (64, 3, 7), (3, 4, 49)]
BUFFERS = ('xpre', 'h', 'u', 'r', 'c', 'hp', 'rh')
_cache = {}


def rel_err(a, r):
    a, r = np.asarray(a, np.float64), np.asarray(r, np.float64)
    return np.abs(a - r).max() / max(np.abs(r).max(), 1e-30)


def case(B, T, GH):
    """Inputs, weights and the float64 logits of a shape, computed once."""
    key = (B, T, GH)
    if key not in _cache:
        p, x = ref.params(161 + GH, GH), ref.features(B, T)
        pt = {k: torch.tensor(v, dtype=torch.float64) for k, v in p.items()}
        _cache[key] = (p, x, torch_ref.fcgru_forward(torch.tensor(x, dtype=torch.float64), pt, GH, GH).numpy())
    return _cache[key]


def engine(gpu, B, T, GH, p, **kw):
    from recurrent_gaze_prediction_amd.engine import FcGruEngine
    eng = FcGruEngine(B, T, (GH, GH), dtype='f32', device=gpu, **kw)
    eng.set_weights(p)
    return eng


@pytest.mark.parametrize('B,T,GH', SHAPES)
def test_every_gate_of_every_step_and_the_logits(gpu, B, T, GH):
    p, x, want = case(B, T, GH)
    eng = engine(gpu, B, T, GH, p, save_for_backward=True, persistent=True)
    assert eng.persistent and eng.persistent_workgroups == 203 and not eng.bptt_persistent
    logits, probs = eng.forward(torch.tensor(x, device=gpu))
    eng.status()
    dev = {k: eng.read_buffer(k).cpu().numpy() for k in BUFFERS}
    assert dev['xpre'].shape == (B, T, 3, 1617) and dev['h'].shape == (T + 1, B, 1617) and dev['hp'].shape == (B, T + 1, 1617)
    errs = ref32.check(dev, p)
    ref32.report('f32 persistent B=%d T=%d GH=%d' % (B, T, GH), errs)
    got = logits.cpu().numpy()
    per_clip = np.abs(got.astype(np.float64) - want).reshape(B, -1).max(1) / np.abs(want).reshape(B, -1).max(1)
    # the inference plan of the same shape runs the other instantiation (one rh buffer, the two-slot state ring)
    inf = engine(gpu, B, T, GH, p, persistent=True)
    zi, _ = inf.forward(torch.tensor(x, device=gpu))
    inf.status()
    # the per-step f32 plan, against the same float64 logits at the same bound
    ps = engine(gpu, B, T, GH, p, per_step=True)
    zp, _ = ps.forward(torch.tensor(x, device=gpu))
    e_ps = rel_err(zp.cpu().numpy(), want)
    print('f32 B=%d T=%d GH=%d: logits persistent %.3e (share %.3f), per step %.3e, worst clip %d at %.3e' %
          (B, T, GH, rel_err(got, want), rel_err(got, want) / TOL_F32, e_ps, int(per_clip.argmax()), per_clip.max()))
    assert not np.any(dev['h'][0]) and np.abs(dev['h'][-1]).max() > 0.1
    assert ref32.violations(errs) == [], errs
    assert np.isfinite(got).all()
    assert rel_err(got, want) < TOL_F32 and e_ps < TOL_F32
    assert per_clip.max() < TOL_F32, (int(per_clip.argmax()), float(per_clip.max()))     # every clip on its own scale
    assert torch.equal(zi, logits)
    want_p = torch.softmax(torch.tensor(want).reshape(B, T, -1), -1).reshape(want.shape).numpy()
    assert rel_err(probs.cpu().numpy(), want_p) < TOL_F32


def test_gradients_behind_the_persistent_forward_match_autograd(gpu):
    B, T, GH = 3, 4, 7
    p = syn.fcgru_params(141, GH, GH)
    p['gates_bias'] = p['gates_bias'] + np.linspace(-0.3, 0.3, p['gates_bias'].size).astype(np.float32)
    x = syn.c3d_features(142, B, T)
    rs = np.random.RandomState(143)
    gt = rs.rand(B, T, GH, GH).astype(np.float32)
    gt /= gt.sum(axis=(2, 3), keepdims=True)
    pt = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in p.items()}
    logits_ref = torch_ref.fcgru_forward(torch.tensor(x, dtype=torch.float64), pt, GH, GH)
    torch_ref.gaze_loss(logits_ref, torch.tensor(gt, dtype=torch.float64), 'xentropy').backward()
    eng = engine(gpu, B, T, GH, p, save_for_backward=True, persistent=True)
    assert eng.persistent
    logits, probs = eng.forward(torch.tensor(x, device=gpu))
    grads = eng.backward(logits, probs, torch.tensor(gt, device=gpu), 'xentropy')
    eng.status()
    errs = {k: rel_err(grads[k].cpu().numpy(), pt[k].grad.numpy()) for k in p}
    print('f32 gradients behind the persistent forward:', {k: '%.2e' % v for k, v in errs.items()})
    assert all(np.abs(pt[k].grad.numpy()).max() > 0 for k in p)
    assert max(errs.values()) < GRAD_TOL_F32, errs


def test_bptt_persistent_stays_refused_on_f32_plans(gpu):
    from recurrent_gaze_prediction_amd import _lib
    from recurrent_gaze_prediction_amd.engine import FcGruEngine
    with pytest.raises(_lib.RgpError, match='dtype'):
        FcGruEngine(3, 4, (7, 7), dtype='f32', device=gpu, save_for_backward=True, persistent=True, bptt_persistent=True)


def test_persistent_is_deterministic_and_resets_its_counters(gpu):
    B, T, GH = 17, 3, 7
    p, x, _ = case(B, T, GH)
    X = torch.tensor(x, device=gpu)
    Y = torch.tensor(syn.c3d_features(977, B, T), device=gpu)

    def run(eng, inp):
        z, _ = eng.forward(inp, want_probs=False)
        return z, eng.read_buffer('h')
    a = engine(gpu, B, T, GH, p, save_for_backward=True, persistent=True)
    z1, h1 = run(a, X)
    z2, h2 = run(a, X)
    assert torch.equal(z1, z2) and torch.equal(h1, h2)
    a.status()
    zy, hy = run(a, Y)
    assert not torch.equal(zy, z1)
    z3, h3 = run(a, X)
    assert torch.equal(z3, z1) and torch.equal(h3, h1)
    a.status()
    # two persistent f32 plans back to back on one stream: each equal to its solo run
    b = engine(gpu, B, T, GH, p, save_for_backward=True, persistent=True)
    zb_solo, hb_solo = run(b, Y)
    torch.cuda.synchronize(gpu)
    za, _ = a.forward(X, want_probs=False)
    zb, _ = b.forward(Y, want_probs=False)
    ha, hb = a.read_buffer('h'), b.read_buffer('h')
    assert torch.equal(za, z1) and torch.equal(ha, h1)
    assert torch.equal(zb, zb_solo) and torch.equal(hb, hb_solo) and torch.equal(zb, zy)
    a.status()
    b.status()
    assert torch.isfinite(z1).all()


# ------------------------------------------------------------------------------------------------ streaming
CUTS = [(4, 4, 2), (3, 3, 3, 1), (1,) * 10, (2, 4, 4)]
saves = pytest.mark.parametrize('save', [False, True], ids=['inference', 'training'])


@saves
@pytest.mark.parametrize('B', [2, 17])
def test_a_stream_does_not_depend_on_where_it_is_cut(gpu, B, save):
    T, S, gh = 4, 10, 7
    eng = sr.engine(gpu, B, T, gh, 'f32', 'persistent', save=save)
    x = torch.tensor(sr.features(B, S), device=gpu)
    runs = [sr.run_stream(eng, x, cuts, pad_value=3.0 + i) for i, cuts in enumerate(CUTS)]
    z0, s0 = runs[0]
    eng.status()
    want = sr.forward_f64(sr.features(B, S), sr.params(gh))[0].reshape(B, S, gh, gh)
    print('f32 persistent stream B=%d %s: logits vs float64 %.3e' % (B, 'training' if save else 'inference', sr.rel_err(z0.cpu().numpy(), want)))
    assert torch.isfinite(z0).all() and float(s0.abs().max()) > 0.1
    for cuts, (z, s) in zip(CUTS[1:], runs[1:]):
        assert torch.equal(z, z0), (cuts, float((z - z0).abs().max()))
        assert torch.equal(s, s0), (cuts, float((s - s0).abs().max()))
    assert sr.rel_err(z0.cpu().numpy(), want) < TOL_F32
    assert len({tuple(r[:8].tolist()) for r in z0.reshape(B, -1).cpu()}) == B
    eng.status()


@saves
def test_null_state_is_the_plain_forward_also_behind_a_seeded_call(gpu, save):
    B, T, gh = 3, 4, 7
    eng = sr.engine(gpu, B, T, gh, 'f32', 'persistent', save=save)
    x = torch.tensor(sr.features(B, T), device=gpu)
    y = torch.tensor(sr.features(B, T + 1)[:, 1:], device=gpu)
    z0, p0 = eng.forward(x)

    def same_as_plain():
        z, p, s = eng.forward_stream(x)
        assert torch.equal(z, z0) and torch.equal(p, p0) and s.numel() == B * 1617
        if save:
            assert torch.equal(eng.read_buffer('h')[T].reshape(-1), s)
            assert not eng.read_buffer('h')[0].any() and not eng.read_buffer('hp')[:, 0].any()
        return s
    s = same_as_plain()
    zy, _, sy = eng.forward_stream(y, state=s, n_valid=2)                    # seeds a state ...
    assert not torch.equal(zy, z0) and not torch.equal(sy, s)
    assert torch.equal(same_as_plain(), s)                                   # ... and the next zero-state call does not see it
    eng.forward_stream(y, state=s, n_valid=T)
    z1, p1 = eng.forward(x)
    assert torch.equal(z1, z0) and torch.equal(p1, p0)
    eng.status()


@pytest.mark.parametrize('B', [3, 17])
def test_the_seeded_step_on_the_devices_own_operands(gpu, B):
    T, gh = 4, 7
    p = sr.params(gh)
    eng = sr.engine(gpu, B, T, gh, 'f32', 'persistent', save=True)
    x = torch.tensor(sr.features(B, 2 * T), device=gpu)
    _, _, s = eng.forward_stream(x[:, :T].contiguous())
    z, _, s2 = eng.forward_stream(x[:, T:].contiguous(), state=s)
    eng.status()
    dev = {k: eng.read_buffer(k).cpu().numpy() for k in BUFFERS}
    sn = s.cpu().numpy().reshape(B, 1617)
    errs = ref32.check(dev, p, zero_state=False)
    ref32.report('f32 persistent B=%d seeded' % B, errs)
    assert np.abs(sn).max() > 0.1
    assert np.array_equal(dev['h'][0], sn)                                   # fp32 h_{-1}: the caller's state, exactly
    assert np.array_equal(dev['hp'][:, 0], sn)                               # the operand rows of step 0: the fp32 state itself
    assert np.array_equal(dev['h'][T], s2.cpu().numpy().reshape(B, 1617))
    assert ref32.violations(errs) == [], errs
    want = sr.forward_f64(sr.features(B, 2 * T), p)[0][:, T:].reshape(B, T, gh, gh)
    assert sr.rel_err(z.cpu().numpy(), want) < TOL_F32


# ------------------------------------------------------------------------------------------------ model
def test_gaze_rnn77_on_the_f32_persistent_path(gpu, tmp_path):
    """predict() returns the engine's maps, and five training steps at 1e-4 (the rate tests/test_fcgru_persistent_gpu.py works
    out for the 49-way softmax) lower the loss on a fixed batch."""
    from recurrent_gaze_prediction_amd.models import gaze_rnn77 as mod
    from recurrent_gaze_prediction_amd.models.base import Session
    cfg = mod.GRUModelConfig()
    cfg.batch_size, cfg.n_lstm_steps, cfg.compute_dtype, cfg.train_dir = 2, 4, 'f32', str(tmp_path)
    cfg.initial_learning_rate, cfg.loss_type, cfg.fcgru_path = 1e-4, 'xentropy', 'persistent'
    data = lambda: syn.SyntheticDataSet(8, 4, seed=9, gazemap_hw=7)
    ds = type('DS', (), {})()
    ds.train = ds.valid = data()
    model = mod.GazePredictionGRU(Session(gpu), ds, cfg)
    assert model.engine.persistent and model.engine.persistent_workgroups == 203 and model.engine.dtype == 'f32'
    x = syn.c3d_features(31, 2, 4)
    maps = model.predict(x).clone()
    _, probs = model.engine.forward(torch.tensor(x, device=gpu))
    assert torch.equal(maps.reshape(probs.shape), probs)
    streamed, state = model.predict_stream(x)                                  # from zeros: predict()
    assert torch.equal(streamed.reshape(probs.shape), maps.reshape(probs.shape)) and state.numel() == 2 * 1617
    assert np.allclose(probs.cpu().numpy().reshape(8, -1).sum(-1), 1.0, atol=1e-5)
    model.single_step(train_mode=False, dataset=data())
    loss0 = model.loss
    np.random.seed(1)
    for i in range(5):
        assert model.single_step(train_mode=True) == i + 1
    model.single_step(train_mode=False, dataset=data())
    print('gaze_rnn77 f32 persistent: loss %.5f -> %.5f' % (loss0, model.loss))
    assert np.isfinite(model.loss) and model.loss < loss0, (loss0, model.loss)
    assert model.engine.persistent and cfg.fcgru_path == 'persistent'          # no fall-back happened
    model.engine.status()
