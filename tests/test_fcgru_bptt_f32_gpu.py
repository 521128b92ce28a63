"""GPU: the fc-GRU backward-through-time pass of f32 plans as one persistent launch (RGP_FCGRU_BPTT_PERSISTENT_F32,
csrc/fcgru_bptt_f32.hip.h).

Shapes (B, T, GH): (2,1,7) first and last step coincide; (3,4,7) one partial row fragment; (17,3,7) a full one plus a partial
one; (33,2,7) three fragments; (64,3,7) four full ones -- the four instantiations of the kernel -- and (3,4,49) the 49x49 map.
Every part of every step's gate-gradient rows and the final carry against the float64 reference on the device's own buffers
(tests/fcgru_f32_bptt_ref.py; the bounds and what they rest on are stated there): the persistent BPTT behind the per-step and
the persistent f32 forward, and the per-step BPTT -- the parent's arithmetic, the yardstick -- beside them.  The gradients of
all parameters against float64 autograd; determinism and counter reset; the plumbing; the two model classes.  status() is RGP_OK
after each.  Figures are printed before the asserts (-s)."""
import numpy as np
import pytest
import torch

import fcgru_f32_bptt_ref as ref
import fcgru_local_ref as fref
from oracle import torch_ref
from recurrent_gaze_prediction_amd import _lib
from recurrent_gaze_prediction_amd import synthetic as syn

pytestmark = pytest.mark.gpu
GRAD_TOL_F32 = 5e-4            # tests/test_fcgru_gpu.py:71, :129 -- what the per-step f32 backward is held to
RGP_ESTATE = -4                # include/rgp.h
LOCAL_SHAPES = [(2, 1, 7), (3, 4, 7), (17, 3, 7), (33, 2, 7), (64, 3, 7), (3, 4, 49)]
# (forward path, BPTT path): the persistent BPTT behind both forwards, the per-step BPTT beside them
PATHS = [('per_step', 'per_step'), ('per_step', 'persistent'), ('persistent', 'persistent')]


def rel_err(a, r):
    a, r = np.asarray(a, np.float64), np.asarray(r, np.float64)
    return np.abs(a - r).max() / max(np.abs(r).max(), 1e-30)


_cache = {}


def case(B, T, GH):
    """Weights, inputs and labels of a shape, made once."""
    key = (B, T, GH)
    if key not in _cache:
        gt = np.random.RandomState(143 + B).rand(B, T, GH, GH).astype(np.float32)
        gt /= gt.sum(axis=(2, 3), keepdims=True)
        _cache[key] = (fref.params(161 + GH, GH), fref.features(B, T), gt)
    return _cache[key]


def engine(gpu, B, T, GH, p, fwd='per_step', bptt='per_step'):
    from recurrent_gaze_prediction_amd.engine import FcGruEngine
    eng = FcGruEngine(B, T, (GH, GH), dtype='f32', device=gpu, save_for_backward=True, bptt_persistent_f32=bptt == 'persistent',
                      **{fwd: True})
    eng.set_weights(p)
    assert eng.persistent == (fwd == 'persistent') and eng.bptt_persistent == (bptt == 'persistent')
    return eng


def step(eng, x, gt, loss='xentropy'):
    logits, probs = eng.forward(x)
    return eng.backward(logits, probs, gt, loss)


@pytest.mark.parametrize('fwd,bptt', PATHS)
@pytest.mark.parametrize('B,T,GH', LOCAL_SHAPES)
def test_every_step_of_the_f32_bptt_on_the_devices_own_buffers(gpu, B, T, GH, fwd, bptt):
    """The per-step path is the parent's arithmetic and is held to the same bounds, so the checker is about the arithmetic, not
    about one kernel."""
    p, x, gt = case(B, T, GH)
    eng = engine(gpu, B, T, GH, p, fwd, bptt)
    step(eng, torch.tensor(x, device=gpu), torch.tensor(gt, device=gpu))
    eng.status()
    dev = {k: eng.read_buffer(k).cpu().numpy() for k in ref.BUFFERS}
    assert dev['dxpre'].shape == (B, T, 3, 1617) and dev['dh_head'].shape == (B, T, 1617) and dev['dh0'].shape == (B, 1617)
    errs = ref.check(dev, p)
    ref.report('f32, %s forward, %s BPTT, B=%d T=%d GH=%d' % (fwd, bptt, B, T, GH), errs)
    print('   shares of the bounds used (part, dh0): %.3f %.3f' % ref.shares(errs))
    assert np.isfinite(dev['dxpre']).all() and np.isfinite(dev['dh0']).all()
    # (dr_pre carries the factor h_{t-1}: all zero at step 0, so at T = 1 altogether)
    assert all(np.abs(dev['dxpre'][:, :, k]).max() > 0 for k in ((0, 2) if T == 1 else (0, 1, 2))) and np.abs(dev['dh0']).max() > 0
    assert ref.violations(errs) == [], {k: errs[k] for k in ref.violations(errs)}


@pytest.mark.parametrize('B,T,GH,loss', [(3, 4, 7, 'xentropy'), (17, 3, 49, 'l2'), (33, 2, 7, 'xentropy')])
def test_gradients_of_all_parameters_match_autograd(gpu, B, T, GH, loss):
    p, x, gt = case(B, T, GH)
    pt = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in p.items()}
    logits_ref = torch_ref.fcgru_forward(torch.tensor(x, dtype=torch.float64), pt, GH, GH)
    torch_ref.gaze_loss(logits_ref, torch.tensor(gt, dtype=torch.float64), loss).backward()
    eng = engine(gpu, B, T, GH, p, 'per_step', 'persistent')
    grads = step(eng, torch.tensor(x, device=gpu), torch.tensor(gt, device=gpu), loss)
    eng.status()
    errs = {k: rel_err(grads[k].cpu().numpy(), pt[k].grad.numpy()) for k in p}
    frob = {k: float(np.linalg.norm(grads[k].cpu().numpy().astype(np.float64) - pt[k].grad.numpy()) /
                     max(np.linalg.norm(pt[k].grad.numpy()), 1e-300)) for k in p}
    print('f32 gradients behind the persistent BPTT, B=%d T=%d %s: max-norm' % (B, T, loss), {k: '%.2e' % v for k, v in errs.items()})
    print('   relative Frobenius', {k: '%.2e' % v for k, v in frob.items()})
    assert all(np.abs(pt[k].grad.numpy()).max() > 0 for k in p)
    assert all(np.abs(grads[k].cpu().numpy()).max() > 0 for k in p)
    # the relative Frobenius error, and the max-norm figure tests/test_fcgru_gpu.py holds the per-step f32 backward to
    assert max(frob.values()) < GRAD_TOL_F32, frob
    assert max(errs.values()) < GRAD_TOL_F32, errs


def test_persistent_f32_bptt_is_deterministic_and_resets_its_counters(gpu):
    """dxpre and dh0 are sums in a fixed order: bit for bit.  (The filter gradients accumulate in an order the runtime chooses.)"""
    B, T, GH = 17, 3, 7
    p, x, gt = case(B, T, GH)
    X, G = torch.tensor(x, device=gpu), torch.tensor(gt, device=gpu)
    Y = torch.tensor(syn.c3d_features(977, B, T), device=gpu)

    def run(eng, inp):
        step(eng, inp, G)
        return eng.read_buffer('dxpre'), eng.read_buffer('dh0')
    a = engine(gpu, B, T, GH, p, 'per_step', 'persistent')
    d1, c1 = run(a, X)
    d2, c2 = run(a, X)
    assert torch.equal(d1, d2) and torch.equal(c1, c2)
    dy, cy = run(a, Y)
    assert not torch.equal(dy, d1)
    d3, c3 = run(a, X)
    assert torch.equal(d3, d1) and torch.equal(c3, c1)
    a.status()
    # two BPTT-persistent plans back to back on one stream: each equal to its solo run
    b = engine(gpu, B, T, GH, p, 'per_step', 'persistent')
    db_solo, cb_solo = run(b, Y)
    torch.cuda.synchronize(gpu)
    step(a, X, G)
    step(b, Y, G)
    da, ca, db, cb = a.read_buffer('dxpre'), a.read_buffer('dh0'), b.read_buffer('dxpre'), b.read_buffer('dh0')
    assert torch.equal(da, d1) and torch.equal(ca, c1)
    assert torch.equal(db, db_solo) and torch.equal(cb, cb_solo) and torch.equal(db, dy) and torch.equal(cb, cy)
    a.status()
    b.status()
    assert torch.isfinite(d1).all() and torch.isfinite(c1).all()


def test_plumbing(gpu):
    from recurrent_gaze_prediction_amd.engine import FcGruEngine
    B, T, GH = 3, 4, 7
    p, x, gt = case(B, T, GH)
    X, G = torch.tensor(x, device=gpu), torch.tensor(gt, device=gpu)
    eng = engine(gpu, B, T, GH, p, 'per_step', 'persistent')
    assert eng.bptt_persistent_workgroups == 203 and eng.bptt_persistent and eng.persistent_workgroups == 0
    eng.forward(X)
    for name in ('dxpre', 'dh_head', 'dh0'):
        with pytest.raises(_lib.RgpError) as e:
            eng.read_buffer(name)                                # a buffer of the backward, and none has run
        assert e.value.code == RGP_ESTATE
    assert eng.read_buffer('h').shape == (T + 1, B, 1617)       # the forward's names are there as before
    grads = {k: v.clone() for k, v in step(eng, X, G).items()}
    assert eng.read_buffer('dxpre').shape == (B, T, 3, 1617)
    # a backward behind a streaming call stays refused until a plain forward has run
    z, pr, _ = eng.forward_stream(X)
    with pytest.raises(_lib.RgpError) as e:
        eng.backward(z, pr, G)
    assert e.value.code == RGP_ESTATE and 'streaming' in str(e.value)
    again = step(eng, X, G)
    assert all(torch.isfinite(again[k]).all() for k in p)
    # a plan without the flag reports 0 and backs up as before: the same gradients within the gradient bound
    plain = engine(gpu, B, T, GH, p, 'per_step', 'per_step')
    assert plain.bptt_persistent_workgroups == 0 and not plain.bptt_persistent
    want = step(plain, X, G)
    assert plain.read_buffer('dh0').shape == (B, 1617)
    errs = {k: rel_err(grads[k].cpu().numpy(), want[k].cpu().numpy()) for k in p}
    print('f32 persistent BPTT against the per-step BPTT:', {k: '%.2e' % v for k, v in errs.items()})
    assert max(errs.values()) < GRAD_TOL_F32, errs
    eng.status()
    plain.status()
    # the flag on an inference plan or a bf16 plan is refused with the reason named; flag 8 on an f32 plan stays refused
    with pytest.raises(_lib.RgpError, match='SAVE_FOR_BACKWARD'):
        FcGruEngine(B, T, (GH, GH), dtype='f32', device=gpu, bptt_persistent_f32=True)
    with pytest.raises(_lib.RgpError, match='f32 plans'):
        FcGruEngine(B, T, (GH, GH), dtype='bf16', device=gpu, save_for_backward=True, bptt_persistent_f32=True)
    with pytest.raises(_lib.RgpError, match='bf16'):
        FcGruEngine(B, T, (GH, GH), dtype='f32', device=gpu, save_for_backward=True, bptt_persistent=True)


@pytest.mark.parametrize('name', ['gaze_rnn', 'gaze_rnn77'])
def test_model_classes_on_the_persistent_f32_bptt(gpu, tmp_path, name):
    """Five training steps at 1e-4 lower the loss on a fixed batch, as the model test of tests/test_fcgru_persistent_gpu.py does
    (why 1e-4: see there)."""
    import importlib
    from recurrent_gaze_prediction_amd.models.base import Session
    mod = importlib.import_module('recurrent_gaze_prediction_amd.models.' + name)
    hw = 49 if name == 'gaze_rnn' else 7
    cfg = mod.GRUModelConfig()
    cfg.batch_size, cfg.n_lstm_steps, cfg.compute_dtype, cfg.train_dir = 2, 4, 'f32', str(tmp_path)
    cfg.initial_learning_rate, cfg.loss_type, cfg.fcgru_bptt_path = 1e-4, 'xentropy', 'persistent'
    data = lambda: syn.SyntheticDataSet(8, 4, seed=9, gazemap_hw=hw)
    ds = type('DS', (), {})()
    ds.train = ds.valid = data()
    model = mod.GazePredictionGRU(Session(gpu), ds, cfg)
    assert model.engine.dtype == 'f32' and model.engine.bptt_persistent and not model.engine.persistent
    assert model.engine.bptt_persistent_workgroups == 203
    model.single_step(train_mode=False, dataset=data())
    loss0 = model.loss
    np.random.seed(1)
    for i in range(5):
        assert model.single_step(train_mode=True) == i + 1
    model.single_step(train_mode=False, dataset=data())
    print('%s, f32, persistent BPTT: loss %.5f -> %.5f' % (name, loss0, model.loss))
    assert np.isfinite(model.loss) and model.loss < loss0, (loss0, model.loss)
    assert model.engine.bptt_persistent and cfg.fcgru_bptt_path == 'persistent'       # no fall-back happened
    model.engine.status()
