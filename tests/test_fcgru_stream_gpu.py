"""GPU: fc-GRU streaming (rgp_fcgru_forward_stream, FcGruEngine.forward_stream, gaze_rnn / gaze_rnn77 predict_stream) on the three
plans of tests/fcgru_stream_ref.py: f32 per step, bf16 per step, bf16 persistent (csrc/fcgru_seq.hip.h, STREAM = true / false).

Bit-for-bit claims (torch.equal): NULL state = the plain forward; the cuts of a stream; lanes; the model classes.  Toleranced
claims: the logits against oracle.torch_ref.fcgru_forward in float64 at the project's fc-GRU bounds (f32 5e-5, bf16 3e-2); every
gate of a seeded call against the one-step float64 reference of tests/fcgru_local_ref.py at its own bounds; the final state at
twice the error of that file's CPU stand-in.  Figures are printed before the asserts (-s).

Measured on an MI355X (long-plan test, B = 2, 7 steps as 3 + 3 + 1 on a T = 3 plan; logits = rel. error against float64, bounds
5e-5 / 3e-2; state = max |h - float64|, bound 1.00e-2 at 7x7 and 8.63e-3 at 49x49, twice the stand-in's 5.0e-3 / 4.3e-3; the T = 3
stream and the T = 7 plan agreed bit for bit in every case, logits and state):
    f32 per step      logits 1.1e-6 (7x7)  5.2e-7 (49x49)   state 4.2e-7  5.1e-7
    bf16 per step     logits 5.51e-3       4.21e-3          state 5.01e-3 4.32e-3
    bf16 persistent   logits 5.46e-3       4.21e-3          state 5.01e-3 4.32e-3
A state dropped at the first cut: steps 3..6 miss the oracle by 0.52 / 0.47 / 0.43 / 0.38 of max |logit| on all three plans.
The cut-invariance case bf16-persistent-B64 is the one that found the blend's open contraction (csrc/fcgru_seq.hip.h):
before the blend was pinned, (4,4,2) -- the only cut whose first call launches STREAM = false -- missed the others by 5.9e-4.
"""
import numpy as np
import pytest
import torch

import fcgru_local_ref as ref
import fcgru_stream_ref as sr
from oracle import torch_ref
from recurrence_local_ref import bf16_rne, sigmoid
from recurrent_gaze_prediction_amd import _lib
from recurrent_gaze_prediction_amd import synthetic as syn

pytestmark = pytest.mark.gpu
plans = pytest.mark.parametrize('dtype,path', sr.PLANS, ids=sr.PLAN_IDS)
BUFFERS = ('xpre', 'h', 'u', 'r', 'c', 'hp', 'rh')
_oracle = {}


def oracle(B, S, gh):
    """float64 logits [B,S,gh,gh] of oracle.torch_ref.fcgru_forward from zeros, and the float64 states, once per case."""
    key = (B, S, gh)
    if key not in _oracle:
        p, x = sr.params(gh), sr.features(B, S)
        pt = {k: torch.tensor(v, dtype=torch.float64) for k, v in p.items()}
        _oracle[key] = (torch_ref.fcgru_forward(torch.tensor(x, dtype=torch.float64), pt, gh, gh).numpy(), sr.forward_f64(x, p)[1])
    return _oracle[key]


def labels(B, T, gh, seed=143):
    gt = np.random.RandomState(seed).rand(B, T, gh, gh).astype(np.float32)
    return gt / gt.sum(axis=(2, 3), keepdims=True)


# ------------------------------------------------------------------------------------------------ 5. NULL state = plain forward
@plans
@pytest.mark.parametrize('save', [False, True], ids=['inference', 'training'])
def test_null_state_is_the_plain_forward_also_behind_a_seeded_call(gpu, dtype, path, save):
    B, T, gh = 3, 4, 7
    eng = sr.engine(gpu, B, T, gh, dtype, path, save=save)
    x = torch.tensor(sr.features(B, T), device=gpu)
    y = torch.tensor(sr.features(B, T + 1)[:, 1:], device=gpu)
    z0, p0 = eng.forward(x)
    h_T = eng.read_buffer('h')[T].reshape(-1).clone() if save else None
    gt = torch.tensor(labels(B, T, gh), device=gpu)
    g0 = {k: v.clone() for k, v in eng.backward(z0, p0, gt, 'xentropy').items()} if save else None

    def same_as_plain():
        z, p, s = eng.forward_stream(x)
        assert torch.equal(z, z0) and torch.equal(p, p0) and s.numel() == B * 1617
        if save:
            assert torch.equal(s, h_T) and torch.equal(eng.read_buffer('h')[T].reshape(-1), s)
            assert not eng.read_buffer('h')[0].any() and not eng.read_buffer('hp')[:, 0].any()
        return s
    s = same_as_plain()
    zy, _, sy = eng.forward_stream(y, state=s, n_valid=2)                    # seeds a state ...
    assert not torch.equal(zy, z0) and not torch.equal(sy, s)
    s2 = same_as_plain()                                                     # ... and the next zero-state call does not see it
    assert torch.equal(s2, s)
    eng.forward_stream(y, state=s, n_valid=T)
    z1, p1 = eng.forward(x)
    assert torch.equal(z1, z0) and torch.equal(p1, p0)
    if save:     # a stale slot (b, 0) of hp_all would reach the h-side kernel gradients
        assert not eng.read_buffer('hp')[:, 0].any()
        g1 = eng.backward(z1, p1, gt, 'xentropy')
        assert all(torch.equal(g1[k], g0[k]) for k in g0), [k for k in g0 if not torch.equal(g1[k], g0[k])]
        fresh = sr.engine(gpu, B, T, gh, dtype, path, save=True)           # a plan that never streamed
        zf, pf = fresh.forward(x)
        gf = fresh.backward(zf, pf, gt, 'xentropy')
        assert torch.equal(zf, z0) and all(torch.equal(gf[k], g0[k]) for k in g0)
        assert all(float(g0[k].abs().max()) > 0 for k in g0)
    eng.status()


# ------------------------------------------------------------------------------------------------ 6. cut invariance
CUTS = [(4, 4, 2), (3, 3, 3, 1), (1,) * 10, (2, 4, 4)]
CUT_CASES = [(d, pa, B) for d, pa in sr.PLANS for B in (2, 17)] + [('bf16', 'persistent', 64)]


@pytest.mark.parametrize('dtype,path,B', CUT_CASES, ids=['%s-%s-B%d' % c for c in CUT_CASES])
@pytest.mark.parametrize('save', [False, True], ids=['inference', 'training'])
def test_a_stream_does_not_depend_on_where_it_is_cut(gpu, dtype, path, B, save):
    T, S, gh = 4, 10, 7
    eng = sr.engine(gpu, B, T, gh, dtype, path, save=save)
    x = torch.tensor(sr.features(B, S), device=gpu)
    runs = [sr.run_stream(eng, x, cuts, pad_value=3.0 + i) for i, cuts in enumerate(CUTS)]
    z0, s0 = runs[0]
    assert torch.isfinite(z0).all() and float(s0.abs().max()) > 0.1
    for cuts, (z, s) in zip(CUTS[1:], runs[1:]):
        assert torch.equal(z, z0), (cuts, float((z - z0).abs().max()))
        assert torch.equal(s, s0), (cuts, float((s - s0).abs().max()))
    # every clip has its own maps: a row fragment that dropped or repeated a clip would show
    flat = z0.reshape(B, -1)
    assert len({tuple(r[:8].tolist()) for r in flat.cpu()}) == B
    eng.status()


# ------------------------------------------------------------------------------------------------ 7. the seeded step
def check_gates(dev, p, dtype):
    """Every gate of every step on the device's own operands: tests/fcgru_local_ref.check for bf16 plans (its hp0 entry asks for
    a zero h_0 and is replaced by the caller's exact comparison).  f32 plans keep fp32 operands, so the same one-step float64
    reference is taken on unrounded kernels, and their operand rows must be the fp32 values themselves."""
    if dtype == 'bf16':
        errs = ref.check(dev, p)
        del errs['hp0']
        return errs
    wu, wr, wc = ref.h_kernels(p, rnd=lambda a: np.asarray(a, np.float64))
    f32, f64 = (lambda a: np.asarray(a, np.float32)), (lambda a: np.asarray(a, np.float64))
    T = dev['u'].shape[0]
    hp = f64(dev['hp'])[:, :T].transpose(1, 0, 2)
    xp = f64(dev['xpre']).transpose(1, 0, 2, 3)
    h_prev, h_next = dev['h'][:-1], dev['h'][1:]
    rh = f64(dev['rh']).transpose(1, 0, 2)
    u, c = f64(dev['u']), f64(dev['c'])
    return {'u': ref._abs(dev['u'], sigmoid(xp[:, :, 0] + hp @ wu), ref.GATE_TOL),
            'r': ref._abs(dev['r'], sigmoid(xp[:, :, 1] + hp @ wr), ref.GATE_TOL),
            'rh': ref._abs(rh, f64(f32(dev['r']) * f32(h_prev)), 1e-30),          # one fp32 multiply, stored as it is
            'c': ref._abs(dev['c'], np.tanh(xp[:, :, 2] + rh @ wc), ref.GATE_TOL),
            'h': ref._abs(h_next, u * f64(h_prev) + (1.0 - u) * c, ref.BLEND_TOL),
            'hp': ref._abs(f64(dev['hp'])[:, 1:].transpose(1, 0, 2), f64(h_next), 1e-30)}


@plans
@pytest.mark.parametrize('B', [3, 17])
def test_the_seeded_step_on_the_devices_own_operands(gpu, dtype, path, B):
    T, gh = 4, 7
    p = sr.params(gh)
    eng = sr.engine(gpu, B, T, gh, dtype, path, save=True)
    x = torch.tensor(sr.features(B, 2 * T), device=gpu)
    _, _, s = eng.forward_stream(x[:, :T].contiguous())
    z, _, s2 = eng.forward_stream(x[:, T:].contiguous(), state=s)
    eng.status()
    dev = {k: eng.read_buffer(k).cpu().numpy() for k in BUFFERS}
    sn = s.cpu().numpy().reshape(B, 1617)
    assert np.abs(sn).max() > 0.1
    assert np.array_equal(dev['h'][0], sn)                                   # fp32 h_{-1}: the caller's state, exactly
    want_rows = bf16_rne(sn).astype(np.float32) if dtype == 'bf16' else sn
    assert np.array_equal(dev['hp'][:, 0], want_rows)                        # the operand rows of step 0: the epilogues' rounding
    assert np.array_equal(dev['h'][T], s2.cpu().numpy().reshape(B, 1617))
    errs = check_gates(dev, p, dtype)
    ref.report('%s %s B=%d seeded' % (dtype, path, B), errs)
    assert ref.violations(errs) == [], errs
    # step 0 on its own (the step that reads the seed): same bounds
    first = {k: (v[:, :2] if k == 'hp' else v[:, :1] if k in ('xpre', 'rh') else v[:2] if k == 'h' else v[:1]) for k, v in dev.items()}
    errs0 = check_gates(first, p, dtype)
    ref.report('%s %s B=%d step 0' % (dtype, path, B), errs0)
    assert ref.violations(errs0) == [], errs0
    # and the seed matters to it: against a zero h_{-1} the gates of step 0 are far off
    zero = dict(first, hp=np.concatenate([np.zeros_like(first['hp'][:, :1]), first['hp'][:, 1:]], 1))
    assert 'u' in ref.violations(check_gates(zero, p, dtype))


# ------------------------------------------------------------------------------------------------ 8. / 9. a longer plan, the oracle
@plans
@pytest.mark.parametrize('gh', [7, 49])
def test_a_short_plans_stream_against_a_long_plan_and_the_oracle(gpu, dtype, path, gh):
    B, S = 2, sum(sr.LONG_CUTS)
    want, h64 = oracle(B, S, gh)
    x = torch.tensor(sr.features(B, S), device=gpu)
    short = sr.engine(gpu, B, max(sr.LONG_CUTS), gh, dtype, path)
    z3, s3 = sr.run_stream(short, x, sr.LONG_CUTS)
    long_ = sr.engine(gpu, B, S, gh, dtype, path)
    z7, _, s7 = long_.forward_stream(x)
    short.status()
    long_.status()
    e3, e7 = sr.rel_err(z3.cpu().numpy(), want), sr.rel_err(z7.cpu().numpy(), want)
    bound = 2.0 * sr.standin_final_state_error(sr.features(B, S), sr.params(gh))
    es3 = float(np.abs(s3.cpu().numpy().reshape(B, -1).astype(np.float64) - h64[-1]).max())
    es7 = float(np.abs(s7.cpu().numpy().reshape(B, -1).astype(np.float64) - h64[-1]).max())
    d37 = float((z3 - z7).abs().max())
    print('%s %s gh=%d: logits T=3 stream %.3e, T=7 plan %.3e (bound %.1e); final state %.3e / %.3e (bound %.3e); '
          'max |T=3 - T=7| logits %.3e, states equal: %s' % (dtype, path, gh, e3, e7, sr.TOL[dtype], es3, es7, bound, d37,
                                                           torch.equal(s3, s7)))
    assert e3 < sr.TOL[dtype] and e7 < sr.TOL[dtype]
    assert es3 <= bound and es7 <= bound
    assert sr.rel_err(z3.cpu().numpy(), z7.cpu().numpy()) < sr.TOL[dtype]


@plans
def test_a_dropped_state_misses_the_oracle(gpu, dtype, path):
    B, S, gh = 2, sum(sr.LONG_CUTS), 7
    want, _ = oracle(B, S, gh)
    x = torch.tensor(sr.features(B, S), device=gpu)
    eng = sr.engine(gpu, B, max(sr.LONG_CUTS), gh, dtype, path)
    z, _ = sr.run_stream(eng, x, sr.LONG_CUTS, drop_state_at_call=(1,))       # forgotten at the first cut, carried at the second
    miss = sr.per_step_miss(z.cpu().numpy(), want)
    print('%s %s: state dropped at step 3, miss per step %s' % (dtype, path, miss))
    assert (miss[:3] < sr.TOL[dtype]).all()
    assert (miss[3:] > sr.MARGIN * sr.TOL['bf16']).all(), miss


# ------------------------------------------------------------------------------------------------ 10. lanes
class _EngineModel(object):
    """What stream.GazeStream needs of a model, on a bare engine."""
    STATE_PARTS = 1

    def __init__(self, eng):
        self.engine, self.batch_size, self.n_lstm_steps = eng, eng.B, eng.T

    def predict_stream(self, c3d, state=None, n_valid=None, position=0):
        z, _, s = self.engine.forward_stream(c3d.contiguous(), state=state, n_valid=n_valid)
        return z, s


@plans
def test_a_reset_lane_is_a_fresh_stream_and_the_other_lane_is_undisturbed(gpu, dtype, path):
    from recurrent_gaze_prediction_amd.stream import GazeStream
    B, T, gh = 2, 4, 7
    model = _EngineModel(sr.engine(gpu, B, T, gh, dtype, path))
    x = torch.tensor(sr.features(B, 2 * T), device=gpu)
    a = GazeStream(model)
    a0 = a.push_features(x[:, :T]).clone()
    a.reset([1])
    a1 = a.push_features(x[:, T:]).clone()
    u = GazeStream(model)                       # undisturbed
    u0 = u.push_features(x[:, :T]).clone()
    u1 = u.push_features(x[:, T:]).clone()
    f = GazeStream(model)                       # fresh at the second chunk
    f1 = f.push_features(x[:, T:]).clone()
    assert torch.equal(a0, u0)
    assert torch.equal(a1[0], u1[0]) and torch.equal(a.state.view(B, -1)[0], u.state.view(B, -1)[0])
    assert torch.equal(a1[1], f1[1]) and torch.equal(a.state.view(B, -1)[1], f.state.view(B, -1)[1])
    assert not torch.equal(a1[1], u1[1]) and not torch.equal(f1[0], u1[0])
    model.engine.status()


# ------------------------------------------------------------------------------------------------ 11. models
@pytest.mark.parametrize('name', ['gaze_rnn', 'gaze_rnn77'])
@pytest.mark.parametrize('path', ['per_step', 'persistent'])
def test_model_classes_stream(gpu, tmp_path, name, path):
    import importlib
    from recurrent_gaze_prediction_amd.models.base import Session
    from recurrent_gaze_prediction_amd.models.evaluate_gaze import predict_long_clip
    from recurrent_gaze_prediction_amd.stream import predict_long_clips
    mod = importlib.import_module('recurrent_gaze_prediction_amd.models.' + name)
    hw = 49 if name == 'gaze_rnn' else 7
    cfg = mod.GRUModelConfig()
    cfg.batch_size, cfg.n_lstm_steps, cfg.compute_dtype, cfg.train_dir = 2, 4, 'bf16', str(tmp_path)
    cfg.loss_type, cfg.fcgru_path, cfg.trainable = 'xentropy', path, False
    model = mod.GazePredictionGRU(Session(gpu), None, cfg)
    assert model.STREAMS is True and model.engine.persistent == (path == 'persistent')
    x = syn.c3d_features(91, 2, 4)
    maps, state = model.predict_stream(x)                                     # no longer raises
    assert tuple(maps.shape) == (2, 4, hw, hw) and state.numel() == 2 * 1617 == model.engine.state_elems
    assert torch.equal(maps, model.predict(x))                                # from zeros: predict()
    clips = [syn.c3d_features(92 + i, 1, n)[0] for i, n in enumerate((5, 9, 2))]
    together = predict_long_clips(model, clips)
    for c, m in zip(clips, together):
        alone = predict_long_clips(model, [c])[0]                             # lane 0, lane 1 idle
        assert m.shape == (len(c), hw, hw) and np.array_equal(m, alone)
        assert np.allclose(m.reshape(len(c), -1).sum(-1), 1.0, atol=1e-4)
    clip = syn.c3d_features(95, 1, 9)[0]
    chunked = predict_long_clip(model, clip)
    carried = predict_long_clip(model, clip, carry_state=True)
    assert chunked.shape == carried.shape == (9, hw, hw)
    assert np.array_equal(carried[:4], chunked[:4])
    d = np.abs(carried - chunked).reshape(9, -1).max(-1)
    print('%s %s carried vs chunked, max |d map| per step: %s' % (name, path, d))
    assert (d[4:] > 0).all()
    assert model.engine.persistent == (path == 'persistent') and cfg.fcgru_path == path          # no fall-back happened
    model.engine.status()


# ------------------------------------------------------------------------------------------------ 12. training plans
@plans
def test_backward_behind_a_streaming_call_is_refused_until_a_plain_forward(gpu, dtype, path):
    B, T, gh = 2, 3, 7
    eng = sr.engine(gpu, B, T, gh, dtype, path, save=True)
    x = torch.tensor(sr.features(B, T), device=gpu)
    gt = torch.tensor(labels(B, T, gh), device=gpu)
    z, p, s = eng.forward_stream(x)
    with pytest.raises(_lib.RgpError) as e:
        eng.backward(z, p, gt, 'xentropy')
    assert e.value.code == -4 and 'stream' in str(e.value)                    # RGP_ESTATE
    eng.forward_stream(x, state=s, n_valid=1)
    with pytest.raises(_lib.RgpError):
        eng.backward(z, p, gt, 'xentropy')
    z, p = eng.forward(x)                                                     # re-arms it
    g = eng.backward(z, p, gt, 'xentropy')
    assert all(torch.isfinite(v).all() for v in g.values()) and float(g['gates_kernel'].abs().max()) > 0
    eng.status()
