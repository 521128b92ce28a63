"""Training across the carried state of gaze_grcn on the device: rgp_grcn_backward_stream, GrcnEngine.backward_stream and
train_long_clip on a GrcnEngine, on the three plans of tests/grcn_tbptt_ref.PLANS (f32 per step, bf16 per step, bf16 with the
persistent BPTT kernel) at P = 512, S = 128, T = 3, with B = 3 (one clip per group, <4>, a group count that is no multiple of 8)
and B = 33 (two clips per group, <7>, a ragged last group).

The float64 reference (grcn_tbptt_ref.chunk_backward) is computed per case (3 - 5 s at B = 33)."""
import ctypes

import numpy as np
import pytest
import torch

import grcn_tbptt_ref as tb
import stream_ref
from recurrent_gaze_prediction_amd import _lib

pytestmark = pytest.mark.gpu
RGP_EINVAL, RGP_ESTATE = -1, -4       # include/rgp.h
T, FILM = 3, 7
PLAN_PARAMS = [pytest.param(p, id=i) for p, i in zip(tb.PLANS, tb.PLAN_IDS)]
_engines = {}


def engine(gpu, plan, B, T_=T, p=None, key=None):
    """A training engine of the plan (cached per key: the tests of one plan and size share it)."""
    from recurrent_gaze_prediction_amd.engine import GrcnEngine
    dtype, kw = plan
    k = (dtype, kw['per_step'], B, T_, key)
    if key is None or k not in _engines:
        eng = GrcnEngine(B, T_, dtype=dtype, save_for_backward=True, device=gpu, **kw)
        assert eng.persistent == (dtype == 'bf16' and not kw['per_step'])
        eng.set_weights(p if p is not None else tb.params(T_))
        if key is None:
            return eng
        _engines[k] = eng
    return _engines[k]


def dev(a, gpu):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(gpu)


def np_grads(grads):
    return {k: grads[k].detach().cpu().numpy().astype(np.float64) for k in tb.FIELDS}


def check_grads(tag, dtype, got, want, loss_type, d_in=None, d_in_want=None, want_f64=True):
    """The fifteen gradients (and d_state_in) at the per-tensor relative Frobenius bounds of tests/test_backward_gpu.py; out_b
    under xentropy as that file treats it (zero in theory: only round-off remains; want_f64=False: `want` is a device result
    too and is held to the device's bound)."""
    errs = {}
    for k in tb.FIELDS:
        if k == 'out_b' and loss_type == 'xentropy':
            assert abs(got[k].item()) < 1e-6 and abs(want[k].item()) < (1e-12 if want_f64 else 1e-6), (tag, got[k], want[k])
            continue
        errs[k] = tb.fro_err(got[k], want[k])
    if d_in_want is not None:
        errs['d_state_in'] = tb.fro_err(d_in, d_in_want)
    print(tag, {k: '%.2e' % v for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v < tb.TOL[dtype]}
    assert not bad, (tag, bad)
    return errs


# ------------------------------------------------------------------------------------------------ 1. behind a plain forward
NO_ATOMICS = ('bn_gamma', 'bn_beta', 'out_b', 'dh_head')      # the loss gradient, the head's dgrad and the batch-norm backward
# What two runs of ONE computation may differ by where float atomics reach it, as a share of the tensor's maximum.  f32 plans:
# 2^-20 = 16 ulps of an fp32 sum of that magnitude; the sums have up to B T 49 = 4851 terms, and a reordered sum of n terms moves
# by about sqrt(n) of the ulps of its partial sums.  bf16 plans: 2^-8, one ulp of a bf16 operand: what the atomics reorder is
# rounded to bf16 operand images downstream (dxpre_pad, dE), a rounding that flips now and then, and a flipped element moves
# what is computed from it by up to that share.  These are floors under the measured spread, not replacements of it.
RUN_TO_RUN = {'f32': 2.0 ** -20, 'bf16': 2.0 ** -8}


def outputs(eng):
    out = {k: v.clone() for k, v in eng.grads.items()}
    out.update(dxpre=eng.read_buffer('dxpre'), dh_head=eng.read_buffer('dh_head'), d_rows=eng.backward_input())
    return out


@pytest.mark.parametrize('B', [3, 33])
@pytest.mark.parametrize('plan', PLAN_PARAMS)
def test_behind_a_plain_forward_it_is_the_plain_backward(gpu, plan, B):
    """backward_stream behind forward() with loss_frames = B T and no state gradient against backward() of a twin plan.  Which
    outputs of backward() itself are byte-stable from plan to plan is established first (two twin plans, the second one run
    four times: five plain results).  The outputs no float atomic reaches (NO_ATOMICS; on the persistent plan dxpre too) must
    come out stable and must be torch.equal.  The others (split-K partial sums and filter gradients added with float atomics,
    and what is computed from them) are held to 4 x the plain-against-plain spread measured here, relative to the tensor's
    maximum, and never to less than RUN_TO_RUN: a handful of plain runs does not bound the next one (on the bf16 per-step plan
    at B = 33 the spread of proj_c3d_W was 7.0e-5 in one run of this test and 3.3e-5 in another: rare bf16 rounding flips
    behind the atomics), and a tensor can come out equal in every plain run by luck (at B = 3 most do) and differ in the
    next."""
    x, g = dev(tb.features(B, T), gpu), dev(tb.labels(B, T), gpu)
    plain = []
    for _ in range(2):
        eng = engine(gpu, plan, B)
        z, pr = eng.forward(x)
        eng.backward(z, pr, g)
        plain.append(outputs(eng))
    for _ in range(3):                                                # the second twin three more times
        z, pr = eng.forward(x)
        eng.backward(z, pr, g)
        plain.append(outputs(eng))
    eng = engine(gpu, plan, B)
    z, pr = eng.forward(x)
    grads, d_in = eng.backward_stream(z, pr, g, d_state=None, loss_frames=B * T, want_d_state=False)
    assert d_in is None
    got = outputs(eng)
    eng.status()
    a = plain[0]
    stable = [k for k in a if all(torch.equal(a[k], o[k]) for o in plain[1:])]
    spread = {k: max(float((a[k] - o[k]).abs().max()) for o in plain[1:]) / max(float(a[k].abs().max()), 1e-30) for k in a if k not in stable}
    print(tb.PLAN_IDS[tb.PLANS.index(plan)], B, 'stable:', stable, 'spread:', {k: '%.2e' % v for k, v in spread.items()})
    exact = NO_ATOMICS + (('dxpre',) if eng.persistent else ())
    for k in exact:
        assert k in stable and torch.equal(got[k], a[k]), k
    for k in a:
        if k not in exact:
            d = float((got[k] - a[k]).abs().max()) / max(float(a[k].abs().max()), 1e-30)
            assert d <= max(4 * spread.get(k, 0.0), RUN_TO_RUN[plan[0]]), (k, d, spread.get(k, 0.0))
    assert all(float(a[k].abs().max()) > 0 for k in a if k != 'out_b')


# ------------------------------------------------------------------------------------------------ 2. a chunk seeded both ways
def run_seeded_chunk(gpu, plan, B, phase, nv, loss_type, wrong=()):
    """The chunk at film steps [T, T + nv) run with `phase`: the state from the device's previous chunk, the state gradient from
    the reference's next chunk; a full plain backward on other data immediately before; features behind n_valid 7.0, labels
    7.0 / random.  wrong: keyword sets that replace arguments of the reference call (the mistakes test 4 must see).
    -> (device grads, d_state_in, buffers, reference (grads, d_state_in), [the same of each wrong reference])."""
    eng = engine(gpu, plan, B, key='seeded')
    p = tb.params(T)
    xf, gf = tb.features(B, 2 * T + 1), tb.labels(B, 2 * T + 1)
    rs = np.random.RandomState(100 * phase + 10 * nv + B)
    x = tb.pad_chunk(xf, T, nv, T, 7.0)
    g = tb.pad_chunk(gf, T, nv, T, rs.rand(B, T - nv, 49, 49).astype(np.float32) if loss_type == 'l2' else 7.0)
    xo, go = dev(tb.features(B, T, seed=5), gpu), dev(tb.labels(B, T, seed=6), gpu)
    z, pr = eng.forward(xo)                                           # stale rows of a backward over all T steps
    eng.backward(z, pr, go, loss_type)
    _, _, state = eng.forward_stream(dev(xf[:, :T], gpu), state=None, n_valid=T, bn_phase=0, want_probs=False)
    h0 = state.cpu().numpy().reshape(B, 7, 7, tb.S)
    # the reference's next chunk (one step) from the reference's state behind this one -> d loss / d state_out
    kw = dict(h0=h0, n_valid=nv, phase=phase, loss_frames=B * FILM, loss_type=loss_type)
    state_out = tb.chunk_backward(x, p, g, forward_only=True, **kw)[2]
    x_next, g_next = tb.pad_chunk(xf, T + nv, 1, T, 0.0), tb.pad_chunk(gf, T + nv, 1, T, 0.0)
    d_out = tb.chunk_backward(x_next, p, g_next, h0=state_out, n_valid=1, phase=(phase + nv) % T, loss_frames=B * FILM,
                              loss_type=loss_type)[1]
    kw['d_state_out'] = d_out
    want = tb.chunk_backward(x, p, g, **kw)[:2]
    wrongs = [tb.chunk_backward(x, p, g, **dict(kw, **w))[:2] for w in wrong]
    d_state = dev(d_out, gpu)
    held_state, held_d = state.clone(), d_state.clone()
    z, pr, new_state = eng.forward_stream(dev(x, gpu), state=state, n_valid=nv, bn_phase=phase)
    grads, d_in = eng.backward_stream(z, pr, dev(g, gpu), d_state=d_state, loss_frames=B * FILM, loss_type=loss_type)
    bufs = {'dxpre': eng.read_buffer('dxpre').reshape(B, T, -1), 'dh_head': eng.read_buffer('dh_head').reshape(T, B, -1),
            'd_rows': eng.backward_input().reshape(B, T, -1)}
    eng.status()
    assert torch.equal(state, held_state) and torch.equal(d_state, held_d)
    assert tb.fro_err(new_state.cpu().numpy().reshape(state_out.shape), state_out) < tb.TOL[plan[0]]
    return np_grads(grads), d_in.cpu().numpy().astype(np.float64), bufs, want, wrongs


CROSS = [(ph, nv, lt) for ph in (0, 2) for nv in (1, 2, T) for lt in ('xentropy', 'l2')]
CASES = [(B,) + c for B in (3, 33) for c in CROSS]


@pytest.mark.parametrize('B,phase,nv,loss_type', CASES)
@pytest.mark.parametrize('plan', PLAN_PARAMS)
def test_a_chunk_seeded_in_both_directions_matches_float64(gpu, plan, B, phase, nv, loss_type):
    got, d_in, bufs, (want, d_in_want), _ = run_seeded_chunk(gpu, plan, B, phase, nv, loss_type)
    tag = '%s B=%d phase=%d n_valid=%d %s' % (tb.PLAN_IDS[tb.PLANS.index(plan)], B, phase, nv, loss_type)
    check_grads(tag, plan[0], got, want, loss_type, d_in, d_in_want)
    # what lies behind n_valid: exactly zero
    assert float(bufs['dxpre'][:, nv:].abs().max() if nv < T else 0.0) == 0.0
    assert float(bufs['dh_head'][nv:].abs().max() if nv < T else 0.0) == 0.0
    assert float(bufs['d_rows'][:, nv:].abs().max() if nv < T else 0.0) == 0.0
    assert float(bufs['dxpre'][:, :nv].abs().max()) > 0 and float(bufs['d_rows'][:, :nv].abs().max()) > 0
    for t in range(nv, T):
        slot = (phase + t) % T
        assert not got['bn_gamma'][slot].any() and not got['bn_beta'][slot].any(), slot
    for t in range(nv):
        assert got['bn_gamma'][(phase + t) % T].any()


# ------------------------------------------------------------------------------------------------ 4. the test can see the mistakes
@pytest.mark.parametrize('plan', [PLAN_PARAMS[0], PLAN_PARAMS[2]])
def test_a_reference_without_the_seed_or_with_the_unshifted_slot_breaks_the_bound(gpu, plan):
    """The case (B = 3, phase 2, n_valid 2, xentropy) of the test above against three wrong references: no state gradient, batch-norm
    slot t instead of (2 + t) % T, and the zero state.  Each must break the bound the right reference holds."""
    B, phase, nv, lt = 3, 2, 2, 'xentropy'
    tol = tb.TOL[plan[0]]
    got, d_in, _, (want, d_in_want), wrongs = run_seeded_chunk(gpu, plan, B, phase, nv, lt,
                                                               wrong=({'d_state_out': None}, {'phase': 0}, {'h0': None}))
    check_grads('right reference', plan[0], got, want, lt, d_in, d_in_want)
    (no_seed, d_no_seed), (unshifted, _), (zero_state, _) = wrongs
    errs = tb.grad_errs(got, no_seed, skip=('out_b',))
    print('no seed', {k: '%.2e' % v for k, v in errs.items()}, tb.fro_err(d_in, d_no_seed))
    assert all(errs[k] > tol for k in tb.RECURRENT) and tb.fro_err(d_in, d_no_seed) > tol
    errs = tb.grad_errs(got, unshifted, skip=('out_b',))
    print('unshifted slot', {k: '%.2e' % v for k, v in errs.items()})
    assert errs['bn_gamma'] > tol and errs['bn_beta'] > tol and errs['GRU_Conv_U'] > tol
    errs = tb.grad_errs(got, zero_state, skip=('out_b',))
    print('zero state', {k: '%.2e' % v for k, v in errs.items()})
    assert errs['GRU_Conv_U'] > tol and errs['GRU_Conv_Uz'] > tol


# ------------------------------------------------------------------------------------------------ 3. composition on the device
_uncut = {}


def uncut(B):
    if B not in _uncut:
        x, g = tb.features(B, FILM), tb.labels(B, FILM)
        _uncut[B] = (x, g, tb.uncut_backward(x, tb.params(T), g, T)[0])
    return _uncut[B]


def run_film(gpu, eng, x, g, chunks, chain):
    """The film in chunks on the device, as train_long_clip(mode='exact') drives it -> the summed gradients (float64)."""
    B = x.shape[0]
    cuts = tb.cuts_of(chunks)
    states = [None]
    xs = [dev(tb.pad_chunk(x, s, n, T, 7.0), gpu) for s, n in cuts]
    gs = [dev(tb.pad_chunk(g, s, n, T, 7.0), gpu) for s, n in cuts]
    for (s, n), xc in zip(cuts, xs):
        states.append(eng.forward_stream(xc, state=states[-1], n_valid=n, bn_phase=s % T, want_probs=False)[2])
    total, d = None, None
    for i in reversed(range(len(cuts))):
        s, n = cuts[i]
        z, pr, _ = eng.forward_stream(xs[i], state=states[i], n_valid=n, bn_phase=s % T)
        grads, d_in = eng.backward_stream(z, pr, gs[i], d_state=d if chain else None, loss_frames=B * FILM, want_d_state=i > 0)
        d = d_in
        gr = np_grads(grads)
        total = gr if total is None else {k: total[k] + gr[k] for k in tb.FIELDS}
    eng.status()
    return total


@pytest.mark.parametrize('chunks', [(3, 3, 1), (2, 3, 2)], ids=['3-3-1', '2-3-2'])
@pytest.mark.parametrize('plan', PLAN_PARAMS)
def test_chained_chunks_compose_to_the_film_and_truncated_ones_miss(gpu, plan, chunks):
    """Seven steps on a plan of three, B = 3, chained with loss_frames = B 7: against float64 autograd of the uncut film and
    against backward() of a seven-step plan whose batch-norm rows are the three rows tiled, both at the bounds of
    tests/test_backward_gpu.py.  Without the chain the recurrent filters miss by far more than the bf16 bound."""
    B, dtype = 3, plan[0]
    x, g, want = uncut(B)
    eng = engine(gpu, plan, B, key='seeded')
    total = run_film(gpu, eng, x, g, chunks, chain=True)
    tag = '%s %s' % (tb.PLAN_IDS[tb.PLANS.index(plan)], chunks)
    check_grads(tag + ' vs float64', dtype, total, want, 'xentropy')
    long = engine(gpu, plan, B, FILM, p=stream_ref.tile_bn(tb.params(T), FILM), key='long')
    z, pr = long.forward(dev(x, gpu))
    lg = np_grads(long.backward(z, pr, dev(g, gpu)))
    for k in ('bn_gamma', 'bn_beta'):                                # row s of the long plan is row s % T of the short one
        lg[k] = np.stack([lg[k][r::T].sum(0) for r in range(T)])
    check_grads(tag + ' vs the 7-step plan', dtype, total, lg, 'xentropy', want_f64=False)
    trunc = run_film(gpu, eng, x, g, chunks, chain=False)
    miss = {k: tb.fro_err(trunc[k], want[k]) for k in tb.RECURRENT}
    print(tag, 'truncated', {k: '%.2e' % v for k, v in miss.items()})
    for k in ('GRU_Conv_Uz', 'GRU_Conv_Ur', 'GRU_Conv_U', 'GRU_Conv_Wz', 'GRU_Conv_Wr', 'GRU_Conv_W', 'proj_c3d_W'):
        assert miss[k] > 5 * tb.TOL['bf16'], (k, miss[k])


# ------------------------------------------------------------------------------------------------ 5. refusals
def _code(e):
    return e.value.code


@pytest.mark.parametrize('plan', PLAN_PARAMS)
def test_refusals_and_what_the_call_leaves_alone(gpu, plan):
    from recurrent_gaze_prediction_amd.engine import GrcnEngine
    B = 3
    dtype, kw = plan
    x, g = dev(tb.features(B, T), gpu), dev(tb.labels(B, T), gpu)
    z0 = torch.zeros(B, T, 49, 49, device=gpu)
    # an inference plan
    inf = GrcnEngine(B, T, dtype=dtype, save_for_backward=False, device=gpu, **kw)
    inf.set_weights(tb.params(T))
    inf.save_for_backward = True                                     # (past the Python assert: the library must refuse)
    zi, pi = inf.forward(x)
    with pytest.raises(_lib.RgpError) as e:
        inf.backward_stream(zi, pi, g)
    assert _code(e) == RGP_ESTATE and 'save_for_backward' in str(e.value)
    # no forward yet
    eng = engine(gpu, plan, B)
    with pytest.raises(_lib.RgpError) as e:
        eng.backward_stream(z0, z0, g)
    assert _code(e) == RGP_ESTATE and 'no forward' in str(e.value)
    state = torch.full((B, 7, 7, tb.S), 0.05, device=gpu)
    z, pr, _ = eng.forward_stream(x, state=state, n_valid=2, bn_phase=1)
    # an aliased state gradient, a non-positive divisor
    d_state = torch.full((B, 7, 7, tb.S), 1e-3, device=gpu)
    from recurrent_gaze_prediction_amd import engine as E
    if eng.grads is None:
        eng.flat_grads, eng.grads = E._flat_views(eng.PARAM_TO_FIELD, eng.weights, eng.device, eng.UNTRAINED)
    st = E._struct(eng.WEIGHTS, eng.PARAM_TO_FIELD, eng.grads)
    call = lambda d_out, d_in, lf: eng.lib.rgp_grcn_backward_stream(eng._h, E._ptr(z), E._ptr(pr), E._ptr(g), E._ptr(d_out), E._ptr(d_in),
                                                                    lf, ctypes.byref(st), 0, E._stream_ptr(eng.device))
    assert call(d_state, d_state, B * 2) == RGP_EINVAL and b'alias' in eng.lib.rgp_last_error()
    assert call(d_state, None, 0) == RGP_EINVAL and b'loss_frames' in eng.lib.rgp_last_error()
    assert call(d_state, None, -3) == RGP_EINVAL and b'loss_frames' in eng.lib.rgp_last_error()
    # the plain backward keeps refusing behind a streaming forward
    with pytest.raises(_lib.RgpError) as e:
        eng.backward(z, pr, g)
    assert _code(e) == RGP_ESTATE and 'streaming' in str(e.value)
    # state_in / d_state_out bit-unchanged, d_state_in a fresh tensor with the same values
    held_s, held_d = state.clone(), d_state.clone()
    _, d_in = eng.backward_stream(z, pr, g, d_state=d_state)
    assert torch.equal(state, held_s) and torch.equal(d_state, held_d) and d_in.data_ptr() != d_state.data_ptr()
    _, d_in2 = eng.backward_stream(z, pr, g, d_state=d_state)
    assert d_in2.data_ptr() != d_in.data_ptr() and tuple(d_in.shape) == (B, 7, 7, tb.S)
    assert float((d_in - d_in2).abs().max()) <= RUN_TO_RUN[dtype] * float(d_in.abs().max()) and float(d_in.abs().max()) > 0
    assert eng.backward_stream(z, pr, g, want_d_state=False)[1] is None
    z, pr = eng.forward(x)                                           # a plain forward re-arms the plain backward
    eng.backward(z, pr, g)
    eng.status()


# ------------------------------------------------------------------------------------------------ 6. the model
def make_model(gpu, tmp_path, dtype, per_step, T_, p, loss_type='xentropy'):
    from recurrent_gaze_prediction_amd.models import gaze_grcn
    from recurrent_gaze_prediction_amd.models.base import Session
    cfg = gaze_grcn.GRUModelConfig()
    cfg.batch_size, cfg.n_lstm_steps, cfg.compute_dtype, cfg.train_dir = 2, T_, dtype, str(tmp_path)
    cfg.convgru_per_step, cfg.init_seed, cfg.loss_type = per_step, 3, loss_type
    model = gaze_grcn.GazePredictionGRCN(Session(gpu), None, cfg)
    model.load_state_dict(p)
    return model


MODELS = [pytest.param('f32', False, id='f32'), pytest.param('bf16', False, id='bf16-persistent')]


@pytest.mark.parametrize('dtype,per_step', MODELS)
def test_exact_mode_takes_the_step_of_a_plan_as_long_as_the_film(gpu, tmp_path, dtype, per_step):
    """'exact' on 7 steps with T = 3 against one train_op step of a T = 7 model with the batch-norm rows tiled: gradients,
    grad_norm and loss at the bounds of tests/test_backward_gpu.py."""
    p = tb.params(T)
    model = make_model(gpu, tmp_path, dtype, per_step, T, p)
    long = make_model(gpu, tmp_path, dtype, per_step, FILM, stream_ref.tile_bn(p, FILM))
    x, g = tb.features(2, FILM), tb.labels(2, FILM)
    before = model.state_dict()
    long.predict(x, train=True)
    long_loss = long.compute_loss(g)
    long.train_op(long.predicted_gazemaps_logit, long.predicted_gazemaps, dev(g, gpu))
    loss = model.train_long_clip(x, g, mode='exact')
    assert model.global_step == 1 and long.global_step == 1
    want = np_grads(long.engine.grads)
    for k in ('bn_gamma', 'bn_beta'):
        want[k] = np.stack([want[k][r::T].sum(0) for r in range(T)])
    errs = check_grads('model ' + dtype, dtype, np_grads(model.engine.grads), want, 'xentropy', want_f64=False)
    # the clip norm: the long model's sees the tiled rows one by one, the short model's their sums
    extra = dict(loss=abs(loss - long_loss) / long_loss)
    gn = float(np.sqrt(sum(float((v ** 2).sum()) for v in want.values())))
    extra['grad_norm'] = abs(float(model.grad_norm.item()) - gn) / gn
    print(dtype, {k: '%.2e' % v for k, v in extra.items()})
    assert max(extra.values()) < tb.TOL[dtype], extra
    after = model.state_dict()
    assert all(not np.array_equal(after[k], before[k]) for k in before if k != 'out_b') and errs


@pytest.mark.parametrize('dtype,per_step', MODELS)
def test_truncated_mode_steps_per_chunk_on_the_states_predict_stream_hands_out(gpu, tmp_path, dtype, per_step):
    p = tb.params(T)
    model, probe = make_model(gpu, tmp_path, dtype, per_step, T, p), make_model(gpu, tmp_path, dtype, per_step, T, p)
    x, g = tb.features(2, FILM), tb.labels(2, FILM)
    weights, step = [], model._reduce_clip_step

    def recording():
        weights.append(model.state_dict())
        step()
    model._reduce_clip_step = recording
    trace = {}
    loss = model.train_long_clip(x, g, mode='truncated', trace=trace)
    assert np.isfinite(loss) and loss > 0
    assert model.global_step == 3 and len(weights) == 3
    assert not np.array_equal(weights[0]['GRU_Conv_U'], weights[1]['GRU_Conv_U'])
    state = None
    for (s, n), w, want in zip(tb.cuts_of((3, 3, 1)), weights, trace['states']):
        probe.load_state_dict(w)
        _, state = probe.predict_stream(tb.pad_chunk(x, s, n, T, 0.0), state=state, n_valid=n, position=s)
        assert torch.equal(state, want)
