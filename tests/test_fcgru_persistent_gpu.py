"""GPU: the fc-GRU recurrence as one persistent launch (RGP_FCGRU_PERSISTENT, csrc/fcgru_seq.hip.h), bf16 plans.

Shapes (B, T, GH): (3,4,7) one partial row fragment, (17,3,49) a full one plus a partial one, (64,3,7) four full ones.
The logits against oracle.torch_ref.fcgru_forward at the bound of tests/test_fcgru_gpu.py; every gate of every step of BOTH
recurrence paths against the one-step float64 reference on the device's own operands (tests/fcgru_local_ref.py; the bounds
and what they rest on are stated there); determinism and counter reset; the gradients behind a persistent forward; the two
model classes.  status() is RGP_OK after each.  Figures are printed before the asserts (-s)."""
import numpy as np
import pytest
import torch

import fcgru_local_ref as ref
from oracle import torch_ref
from recurrent_gaze_prediction_amd import synthetic as syn

pytestmark = pytest.mark.gpu
TOL_BF16 = 3e-2                # tests/test_fcgru_gpu.py TOL['bf16']
GRAD_TOL_BF16 = 5e-2           # tests/test_fcgru_gpu.py:71
SHAPES = [(3, 4, 7), (17, 3, 49), (64, 3, 7)]
BUFFERS = ('xpre', 'h', 'u', 'r', 'c', 'hp', 'rh')


def rel_err(a, r):
    a, r = np.asarray(a, np.float64), np.asarray(r, np.float64)
    return np.abs(a - r).max() / max(np.abs(r).max(), 1e-30)


_cache = {}


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
    eng = FcGruEngine(B, T, (GH, GH), dtype='bf16', device=gpu, **kw)
    eng.set_weights(p)
    return eng


@pytest.mark.parametrize('B,T,GH', SHAPES)
def test_persistent_forward_matches_oracle(gpu, B, T, GH):
    p, x, want = case(B, T, GH)
    eng = engine(gpu, B, T, GH, p, persistent=True)
    assert eng.persistent_workgroups == 203 and eng.persistent
    logits, probs = eng.forward(torch.tensor(x, device=gpu))
    eng.status()
    got = logits.cpu().numpy()
    want_p = torch.softmax(torch.tensor(want).reshape(B, T, -1), -1).reshape(want.shape).numpy()
    per_clip = np.abs(got.astype(np.float64) - want).reshape(B, -1).max(1) / np.abs(want).reshape(B, -1).max(1)
    print('persistent B=%d T=%d: logits %.3e, probs %.3e, worst clip %d at %.3e' %
          (B, T, rel_err(got, want), rel_err(probs.cpu().numpy(), want_p), int(per_clip.argmax()), per_clip.max()))
    assert np.isfinite(got).all()
    assert rel_err(got, want) < TOL_BF16
    assert rel_err(probs.cpu().numpy(), want_p) < TOL_BF16
    if B == 64:      # every clip on its own scale: a row fragment that dropped or repeated a clip would show in that clip
        assert per_clip.max() < TOL_BF16, (int(per_clip.argmax()), float(per_clip.max()))


@pytest.mark.parametrize('path', ['per_step', 'persistent'])
@pytest.mark.parametrize('B,T,GH', SHAPES)
def test_every_gate_of_every_step_on_the_devices_own_operands(gpu, B, T, GH, path):
    """Training plans of both paths: the per-step path is held to the same bounds, so the checker is about the arithmetic,
    not about one kernel."""
    p, x, _ = case(B, T, GH)
    eng = engine(gpu, B, T, GH, p, save_for_backward=True, **{path: True})
    assert eng.persistent == (path == 'persistent')
    eng.forward(torch.tensor(x, device=gpu))
    eng.status()
    dev = {k: eng.read_buffer(k).cpu().numpy() for k in BUFFERS}
    assert dev['xpre'].shape == (B, T, 3, 1617) and dev['h'].shape == (T + 1, B, 1617) and dev['hp'].shape == (B, T + 1, 1617)
    errs = ref.check(dev, p)
    ref.report('%s B=%d T=%d' % (path, B, T), errs)
    assert not np.any(dev['h'][0]) and np.abs(dev['h'][-1]).max() > 0.1
    assert ref.violations(errs) == [], errs


def test_persistent_is_deterministic_and_resets_its_counters(gpu):
    B, T, GH = 17, 3, 49
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
    zy, hy = run(a, Y)
    assert not torch.equal(zy, z1)
    z3, h3 = run(a, X)
    assert torch.equal(z3, z1) and torch.equal(h3, h1)
    a.status()
    # two persistent plans back to back on one stream: each equal to its solo run
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


def test_gradients_behind_a_persistent_forward_match_autograd(gpu):
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
    print('gradients behind the persistent forward:', {k: '%.2e' % v for k, v in errs.items()})
    assert all(np.abs(pt[k].grad.numpy()).max() > 0 for k in p)
    assert max(errs.values()) < GRAD_TOL_BF16, errs


@pytest.mark.parametrize('name,path', [('gaze_rnn', 'persistent'), ('gaze_rnn77', 'persistent'), ('gaze_rnn77', 'per_step')])
def test_model_classes_on_the_persistent_path(gpu, tmp_path, name, path):
    """generate() returns maps that sum to 1 and five training steps lower the loss on a fixed batch, as the config-2 model
    test of tests/test_fcgru_gpu.py does per step.  gaze_rnn runs that test's learning rate, 1e-3.  gaze_rnn77 runs 1e-4:
    Adam's first steps move every weight by about the learning rate whatever the gradient's scale, a logit sums 1617
    units, so 1e-3 moves a logit by up to ~0.5 per step -- a large part of the ln 49 = 3.9 a 49-way softmax spans, where
    the 2401-way one of gaze_rnn starts at 7.8 -- and five such steps overshoot on EITHER recurrence path (measured: the
    per-step path 3.950 -> 5.665, the persistent one 3.950 -> 5.664; at 1e-4 3.950 -> 3.639 on both).  The per-step case of
    gaze_rnn77 at 1e-4 stands beside the persistent one, so that "the same on both paths" is asserted, not quoted."""
    import importlib
    from recurrent_gaze_prediction_amd.models.base import Session
    mod = importlib.import_module('recurrent_gaze_prediction_amd.models.' + name)
    hw = 49 if name == 'gaze_rnn' else 7
    cfg = mod.GRUModelConfig()
    cfg.batch_size, cfg.n_lstm_steps, cfg.compute_dtype, cfg.train_dir = 2, 4, 'bf16', str(tmp_path)
    cfg.initial_learning_rate, cfg.loss_type, cfg.fcgru_path = (1e-3 if name == 'gaze_rnn' else 1e-4), 'xentropy', path
    data = lambda: syn.SyntheticDataSet(8, 4, seed=9, gazemap_hw=hw)
    ds = type('DS', (), {})()
    ds.train = ds.valid = data()
    model = mod.GazePredictionGRU(Session(gpu), ds, cfg)
    assert model.engine.persistent == (path == 'persistent') and model.engine.persistent_workgroups == (203 if path == 'persistent' else 0)
    ret = model.generate(data(), max_instances=4)
    assert ret['pred_gazemap_list'].shape == (4 * 4, hw, hw)
    assert np.allclose(ret['pred_gazemap_list'].reshape(16, -1).sum(-1), 1.0, atol=1e-5)
    model.single_step(train_mode=False, dataset=data())
    loss0 = model.loss
    np.random.seed(1)
    for i in range(5):
        assert model.single_step(train_mode=True) == i + 1
    model.single_step(train_mode=False, dataset=data())
    print('%s %s: loss %.5f -> %.5f' % (name, path, loss0, model.loss))
    assert np.isfinite(model.loss) and model.loss < loss0, (loss0, model.loss)
    assert model.engine.persistent == (path == 'persistent') and cfg.fcgru_path == path          # no fall-back happened
    model.engine.status()
