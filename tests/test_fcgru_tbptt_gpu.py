"""GPU: training across the fc-GRU's carried state (rgp_fcgru_backward_stream, FcGruEngine.backward_stream,
GazePredictionGRU.train_long_clip) on four plans: f32 and bf16 with the per-step BPTT, bf16 with the persistent BPTT kernel,
f32 with the persistent f32 BPTT kernel.  References: tests/fcgru_tbptt_ref.py (float64, checked against autograd on the CPU).
Nothing here provokes a time-out."""
import numpy as np
import pytest
import torch

import fcgru_bptt_ref as bref
import fcgru_f32_bptt_ref as f32ref
import fcgru_tbptt_ref as tb

pytestmark = pytest.mark.gpu
N, T, S = tb.N, 3, 7
RGP_ESTATE = -4                              # include/rgp.h
PLANS = pytest.mark.parametrize('plan', tb.PLANS, ids=tb.PLAN_IDS)
_ref = {}


def engine(gpu, plan, B, T_=T, gh=7):
    from recurrent_gaze_prediction_amd.engine import FcGruEngine
    dtype, kw = plan
    eng = FcGruEngine(B, T_, (gh, gh), dtype=dtype, device=gpu, save_for_backward=True, **kw)
    assert eng.bptt_persistent == any(k.startswith('bptt') for k in kw)
    eng.set_weights(tb.params(gh))
    return eng


def dev(a, gpu):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(gpu)


def film(B, gh, chunks):
    """The float64 reference of a film of S steps cut into `chunks` on a T-step plan (shared, never modified)."""
    key = (B, gh, chunks)
    if key not in _ref:
        x, g = tb.features(B, sum(chunks)), tb.labels(B, sum(chunks), gh)
        total, per = tb.film_backward(x, tb.params(gh), g, chunks, T=T, pad_seed=3)
        _ref[key] = (x, g, total, per)
    return _ref[key]


def chunk_inputs(x, g, chunks, i, seed=3):
    """Chunk i of the film as the device gets it: 7.0 behind n_valid, random labels there."""
    s, n = tb.cuts_of(chunks)[i]
    rs = np.random.RandomState(100 + seed + i)
    return (tb.pad_chunk(x, s, n, T, 7.0), tb.pad_chunk(g, s, n, T, rs.rand(x.shape[0], T - n, *g.shape[2:]).astype(np.float32)), n)


def np_grads(grads):
    return {k: grads[k].detach().cpu().numpy() for k in tb.FIELDS}


# ------------------------------------------------------------------------------------------------ 5. the plain path is untouched
@pytest.mark.parametrize('plan,B', [(p, b) for p in tb.PLANS for b in (3, 17) + ((64,) if len(p[1]) > 1 else ())],
                         ids=['%s-B%d' % (i, b) for i, p in zip(tb.PLAN_IDS, tb.PLANS) for b in (3, 17) + ((64,) if len(p[1]) > 1 else ())])
def test_behind_a_plain_forward_it_is_the_plain_backward_bit_for_bit(gpu, plan, B):
    """torch.equal against backward() on a twin plan: the gate-gradient rows, dh_head, the final carry and the gradients.
    One exception, and it is the plain backward's own: proj_c3d_W is summed over F * 49 pixel rows by several workgroups with
    fp32 atomics (wgrad.hip.h), in an order that changes from launch to launch, so from 17 clips on backward() does not
    reproduce ITSELF bit for bit -- measured on twin plans, plain against plain, all four plans: equal at B = 3, max
    difference 1.0e-7 of the gradient's maximum at B = 17 and 2.4e-7 at B = 64, and exactly the same figures plain against
    backward_stream; the other seven gradients and the three buffers were bit-equal in every case.  There it is held to
    2^-20 of its maximum: 4 x the largest spread the plain backward showed against itself, a bound from the reference's own
    error, not from this call -- and a THIRD plan's plain backward is held to the same bound against the twin's in the same
    run, so the reference's own spread is measured beside the figure it excuses.  Its operand is covered bit for bit all the
    same: proj_c3d_b is the column sum of the same d E rows, and dxpre is what d E is computed from."""
    x, g = dev(tb.features(B, T), gpu), dev(tb.labels(B, T, 7), gpu)
    eng, twin = engine(gpu, plan, B), engine(gpu, plan, B)
    z, p = twin.forward(x)
    twin.backward(z, p, g)
    if B > 3:                                              # plain against plain: the reference against itself
        third = engine(gpu, plan, B)
        third.backward(*third.forward(x), g)
        own = float((third.grads['proj_c3d_W'] - twin.grads['proj_c3d_W']).abs().max() / twin.grads['proj_c3d_W'].abs().max())
        print('%s B=%d proj_c3d_W: plain backward against plain backward %.2e of its maximum' % (plan, B, own))
        assert own <= 2.0 ** -20, own
        assert all(torch.equal(third.grads[k], twin.grads[k]) for k in tb.FIELDS if k != 'proj_c3d_W')
        del third
    z2, p2 = eng.forward(x)
    assert torch.equal(z, z2)

    def same_as_twin():
        for k in tb.FIELDS:
            a, b = eng.grads[k], twin.grads[k]
            if k == 'proj_c3d_W' and B > 3:
                d = float((a - b).abs().max() / b.abs().max())
                print('%s B=%d proj_c3d_W: %.2e of its maximum from the twin plan' % (plan, B, d))
                assert d <= 2.0 ** -20, d
            else:
                assert torch.equal(a, b), k
    grads, d_in = eng.backward_stream(z2, p2, g, d_state=None, loss_frames=B * T)
    same_as_twin()
    assert float(eng.flat_grads.abs().max()) > 0 and bool(torch.isfinite(eng.flat_grads).all())
    for name in ('dxpre', 'dh_head', 'dh0'):
        assert torch.equal(eng.read_buffer(name), twin.read_buffer(name)), name
    assert tuple(d_in.shape) == (B, N) and torch.equal(d_in, eng.read_buffer('dh0'))
    # the default divisor is B n_valid of the last forward
    eng.backward_stream(z2, p2, g)
    same_as_twin()
    eng.status()


# ------------------------------------------------------------------------------------------------ 6. each chunk against float64
def run_seeded_chunk(gpu, eng, B, gh, chunks, i=1):
    """Chunk i of the film on the device, seeded in both directions: the state from the device's own previous chunks, d_state from
    the reference's next chunk; a full backward on other data runs on the plan immediately before (stale rows of all T steps)."""
    x, g, _, per = film(B, gh, chunks)
    state = None
    for k in range(i):
        xk, _, nk = chunk_inputs(x, g, chunks, k)
        state = eng.forward_stream(dev(xk, gpu), state=state, n_valid=nk)[2]
    stale_x, stale_g = dev(tb.features(B, T)[:, ::-1], gpu), dev(tb.labels(B, T, gh, seed=5), gpu)
    z, p = eng.forward(stale_x)
    eng.backward(z, p, stale_g)
    xi, gi, n = chunk_inputs(x, g, chunks, i)
    want, d_in_want, _, d_out = per[i]
    d_state = None if d_out is None else dev(d_out, gpu)
    held = None if d_state is None else d_state.clone()
    z, p, _ = eng.forward_stream(dev(xi, gpu), state=state, n_valid=n)
    grads, d_in = eng.backward_stream(z, p, dev(gi, gpu), d_state=d_state, loss_frames=B * sum(chunks))
    eng.status()
    assert d_state is None or torch.equal(d_state, held)
    return np_grads(grads), d_in.cpu().numpy(), want, d_in_want, d_state, n


def check_chunk(tag, dtype, got, d_in, want, d_in_want):
    errs = dict(tb.grad_errs(got, want), d_state_in=tb.rel_err(d_in, d_in_want))
    print(tag, {k: '%.2e' % v for k, v in errs.items()})
    assert np.abs(d_in_want).max() > 0 and all(np.abs(want[k]).max() > 0 for k in tb.RECURRENT)
    assert max(errs.values()) < tb.GRAD_TOL[dtype], errs


@PLANS
@pytest.mark.parametrize('B', [3, 17])
@pytest.mark.parametrize('chunks', [(3, 3, 1), (3, 1, 3)], ids=['n_valid=T', 'n_valid=1'])
def test_a_seeded_chunk_matches_float64(gpu, plan, B, chunks):
    eng = engine(gpu, plan, B)
    got, d_in, want, d_in_want, _, _ = run_seeded_chunk(gpu, eng, B, 7, chunks)
    check_chunk('%s B=%d %s' % (plan, B, chunks), plan[0], got, d_in, want, d_in_want)


@pytest.mark.parametrize('plan', [tb.PLANS[0], tb.PLANS[2]], ids=[tb.PLAN_IDS[0], tb.PLAN_IDS[2]])
def test_a_seeded_chunk_matches_float64_at_49x49(gpu, plan):
    eng = engine(gpu, plan, 3, gh=49)
    got, d_in, want, d_in_want, _, _ = run_seeded_chunk(gpu, eng, 3, 49, (3, 2, 2))
    check_chunk('%s 49x49' % (plan,), plan[0], got, d_in, want, d_in_want)


# ------------------------------------------------------------------------------------------------ 7. composition on the device
def run_film(gpu, eng, B, chunks, chain):
    x, g, _, _ = film(B, 7, chunks)
    ins = [chunk_inputs(x, g, chunks, i) for i in range(len(chunks))]
    states = [None]
    for xi, _, n in ins:
        states.append(eng.forward_stream(dev(xi, gpu), state=states[-1], n_valid=n)[2])
    acc, d_state = None, None
    for i in reversed(range(len(chunks))):
        xi, gi, n = ins[i]
        z, p, _ = eng.forward_stream(dev(xi, gpu), state=states[i], n_valid=n)
        _, d_in = eng.backward_stream(z, p, dev(gi, gpu), d_state=d_state if chain else None, loss_frames=B * S)
        acc = eng.flat_grads.clone() if acc is None else acc + eng.flat_grads
        d_state = d_in
    eng.status()
    eng.flat_grads.copy_(acc)
    return np_grads(eng.grads)


@PLANS
def test_chained_chunks_compose_to_the_film_and_truncated_ones_miss(gpu, plan):
    B = 3
    tol = tb.GRAD_TOL[plan[0]]
    x, g, want, _ = film(B, 7, (3, 3, 1))
    long = engine(gpu, plan, B, T_=S)
    z, p = long.forward(dev(x, gpu))
    plain7 = np_grads(long.backward(z, p, dev(g, gpu)))
    del long
    eng = engine(gpu, plan, B)
    for chunks in ((3, 3, 1), (2, 3, 2)):
        assert max(tb.grad_errs(film(B, 7, chunks)[2], want).values()) < 1e-12          # one film, however it is cut
        got = run_film(gpu, eng, B, chunks, chain=True)
        errs, vs7 = tb.grad_errs(got, want), tb.grad_errs(got, plain7)
        print(plan, chunks, 'chained vs float64', {k: '%.2e' % v for k, v in errs.items()})
        print(plan, chunks, 'chained vs the T = 7 plan', {k: '%.2e' % v for k, v in vs7.items()})
        assert max(errs.values()) < tol and max(vs7.values()) < tol, (errs, vs7)
    trunc = run_film(gpu, eng, B, (3, 3, 1), chain=False)
    miss = tb.grad_errs(trunc, want)
    print(plan, 'truncated vs float64', {k: '%.2e' % v for k, v in miss.items()})
    assert all(miss[k] > tb.TRUNCATED_MISS for k in tb.RECURRENT), miss
    assert tb.TRUNCATED_MISS / tb.GRAD_TOL['bf16'] > 5.999              # at least 6 x the widest tolerance


# ------------------------------------------------------------------------------------------------ 8. per-step locality
@PLANS
@pytest.mark.parametrize('B', [3, 17])
def test_every_step_of_a_seeded_call_on_the_devices_own_operands(gpu, plan, B):
    eng = engine(gpu, plan, B)
    _, _, _, _, d_state, n = run_seeded_chunk(gpu, eng, B, 7, (3, 2, 2))
    assert n == 2 and d_state is not None
    bufs = {k: eng.read_buffer(k).cpu().numpy() for k in bref.BUFFERS}
    assert not bufs['dxpre'][:, n:].any(), 'rows behind n_valid must be exactly zero'
    assert np.abs(bufs['dxpre'][:, :n]).max() > 0
    view = tb.seeded_view(bufs, d_state.cpu().numpy(), n)
    ref = bref if plan[0] == 'bf16' else f32ref
    errs = ref.check(view, tb.params(7))
    ref.report('%s B=%d seeded, n_valid=%d' % (plan, B, n), errs)
    assert not ref.violations(errs), ref.violations(errs)
    # the seed enters at step n_valid - 1: without it that step's reference is far off
    blind = ref.check(tb.seeded_view(bufs, None, n), tb.params(7))
    assert 'du_pre[%d]' % (n - 1) in ref.violations(blind)


# ------------------------------------------------------------------------------------------------ 9. refusals and state
@PLANS
def test_refusals_and_what_the_call_leaves_alone(gpu, plan):
    from recurrent_gaze_prediction_amd import _lib
    B = 3
    eng = engine(gpu, plan, B)
    x, g = dev(tb.features(B, T), gpu), dev(tb.labels(B, T, 7), gpu)
    z = torch.zeros(B, T, 7, 7, device=gpu)
    with pytest.raises(_lib.RgpError) as e:
        eng.backward_stream(z, z, g)
    assert e.value.code == RGP_ESTATE, e.value                  # no forward yet
    z, p, state = eng.forward_stream(x, n_valid=2)
    with pytest.raises(_lib.RgpError) as e:
        eng.backward(z, p, g)
    assert e.value.code == RGP_ESTATE and 'streaming' in str(e.value), e.value      # the plain backward keeps refusing
    d_state = torch.full((B, N), 1e-3, device=gpu)
    held = d_state.clone()
    grads, d_in = eng.backward_stream(z, p, g, d_state=d_state)
    assert torch.equal(d_state, held) and d_in.data_ptr() != d_state.data_ptr()
    _, d_in2 = eng.backward_stream(z, p, g, d_state=d_state)
    assert d_in2.data_ptr() != d_in.data_ptr() and torch.equal(d_in, d_in2)              # a fresh tensor, the same values
    assert eng.backward_stream(z, p, g, want_d_state=False)[1] is None
    z, p = eng.forward(x)                                            # a plain forward re-arms the plain backward
    eng.backward(z, p, g)
    eng.status()


# ------------------------------------------------------------------------------------------------ 10. the model
MODELS = [('gaze_rnn77', 'f32', None), ('gaze_rnn', 'bf16', 'persistent')]


def make_model(gpu, tmp_path, name, dtype, bptt, T_, keep=1.0, loss_type='xentropy'):
    import importlib
    from recurrent_gaze_prediction_amd.models.base import Session
    module = importlib.import_module('recurrent_gaze_prediction_amd.models.' + name)
    cfg = module.GRUModelConfig()
    cfg.batch_size, cfg.n_lstm_steps, cfg.compute_dtype, cfg.train_dir = 2, T_, dtype, str(tmp_path)
    cfg.train_keep_prob, cfg.fcgru_bptt_path, cfg.init_seed, cfg.loss_type = keep, bptt, 3, loss_type
    return module.GazePredictionGRU(Session(gpu), None, cfg)


def model_data(model):
    B = model.batch_size
    return tb.features(B, S), tb.labels(B, S, model.gazemap_height)


@pytest.mark.parametrize('name,dtype,bptt,loss_type', [m + ('xentropy',) for m in MODELS] + [MODELS[0] + ('l2',)],
                         ids=[m[0] for m in MODELS] + [MODELS[0][0] + '-l2'])
def test_exact_mode_takes_the_step_of_a_plan_as_long_as_the_film(gpu, tmp_path, name, dtype, bptt, loss_type):
    model = make_model(gpu, tmp_path, name, dtype, bptt, T, loss_type=loss_type)
    long = make_model(gpu, tmp_path, name, dtype, bptt, S, loss_type=loss_type)
    x, g = model_data(model)
    before = model.state_dict()
    long.predict(x, train=True)
    long.compute_loss(g)
    long.train_op(long.predicted_gazemaps_logit, long.predicted_gazemaps, dev(g, gpu))
    loss = model.train_long_clip(x, g, mode='exact')
    assert model.global_step == 1 and long.global_step == 1
    want = np_grads(long.engine.grads)
    errs = dict(tb.grad_errs(np_grads(model.engine.grads), want),
                grad_norm=abs(float(model.grad_norm.item()) - float(long.grad_norm.item())) / float(long.grad_norm.item()),
                loss=abs(loss - long.compute_loss(g)) / loss)
    print(name, {k: '%.2e' % v for k, v in errs.items()})
    assert all(np.abs(want[k]).max() > 0 for k in want)
    assert max(errs.values()) < tb.GRAD_TOL[dtype], errs
    after = model.state_dict()
    assert all(not np.array_equal(after[k], before[k]) for k in before)


@pytest.mark.parametrize('name,dtype,bptt', MODELS, ids=[m[0] for m in MODELS])
def test_exact_mode_recomputes_every_chunk_with_its_own_mask(gpu, tmp_path, name, dtype, bptt):
    model = make_model(gpu, tmp_path, name, dtype, bptt, T, keep=0.5)
    x, g = model_data(model)
    trace = {}
    model.train_long_clip(x, g, mode='exact', trace=trace)
    assert len(trace['logits']) == len(trace['logits_recomputed']) == 3 and model.engine.dropout.draws == 3
    for (s, n), a, b in zip(tb.cuts_of((3, 3, 1)), trace['logits'], trace['logits_recomputed']):
        assert torch.equal(a[:, :n], b[:, :n])
    assert not torch.equal(trace['logits'][0], trace['logits'][1])


@pytest.mark.parametrize('name,dtype,bptt', MODELS, ids=[m[0] for m in MODELS])
def test_truncated_mode_steps_per_chunk_on_the_states_predict_stream_hands_out(gpu, tmp_path, name, dtype, bptt):
    model, probe = make_model(gpu, tmp_path, name, dtype, bptt, T), make_model(gpu, tmp_path, name, dtype, bptt, T)
    x, g = model_data(model)
    weights, step = [], model._reduce_clip_step

    def recording():
        weights.append(model.state_dict())
        step()
    model._reduce_clip_step = recording
    trace = {}
    model.train_long_clip(x, g, mode='truncated', trace=trace)
    assert model.global_step == 3 and len(weights) == 3
    assert not np.array_equal(weights[0]['gates_kernel'], weights[1]['gates_kernel'])
    state = None
    for (s, n), w, want in zip(tb.cuts_of((3, 3, 1)), weights, trace['states']):
        probe.load_state_dict(w)
        _, state = probe.predict_stream(tb.pad_chunk(x, s, n, T, 0.0), state=state, n_valid=n)
        assert torch.equal(state, want)
