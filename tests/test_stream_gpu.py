"""GPU: streaming inference (rgp_*_forward_stream, engine.forward_stream, stream.GazeStream) of the three conv-recurrent
families on their three paths (f32 per step, bf16 persistent, bf16 per step; tests/stream_ref.py).

gaze_grcn's batch-norm gamma / beta are random per timestep in every test.  Every test prints its figures before it asserts (-s).

Bounds.  Cut invariance and the NULL-state call are bit-for-bit (torch.equal): one plan, the same GEMM shapes in every call,
every output row accumulated over K in one order wherever it sits, and a seed that rounds as the kernels do.  Streaming against
one long plan: 2e-5 of max|logits| (f32), 2e-2 (bf16): the project's bounds (tests/test_grcn_gpu.py TOL; the bf16 logits bound of
tests/test_lstm_gpu.py::test_forward_rows_matches_forward).  Against float64 the bounds are those of the family's own forward
test: gaze_grcn TOL / TOL_H_MAX / TOL_H_RMS of tests/test_grcn_gpu.py, gaze_grcn77 the same on the states and 2e-5 on f32
logits (tests/test_grcn77_gpu.py), gaze_lstm 2e-5 (f32) and twice the error of the bf16-operand emulation (bf16;
tests/test_lstm_gpu.py check_bf16: relative Frobenius per step, max-abs over max|ref|).  The rows form against the c3d_input
form: what tests/test_lstm_gpu.py::test_forward_rows_matches_forward bounds, as it bounds it -- logits (of their max) and softmax
maps (absolute) by ROWS_TOL, f32 states by 2e-5.  That test sets no bound on bf16 states; here they get the project's bound between
two bf16 evaluations of one recurrence, 2e-2 of max|h| (tests/test_grcn_gpu.py::
test_per_step_recurrence_agrees_with_persistent_kernels): the two projections accumulate over K in different orders, so single
elements of the bf16 operand E differ by one ulp (2^-8), which the saturated gates pass on to single state elements (the comment
at TOL_H_MAX there).  Measured values: DESIGN.md section 18."""
import numpy as np
import pytest
import torch

import stream_ref as sr
from recurrent_gaze_prediction_amd import _lib
from recurrent_gaze_prediction_amd import synthetic as syn

pytestmark = pytest.mark.gpu

TOL = {'f32': 2e-5, 'bf16': 2e-2}
TOL_H_MAX = {'f32': 5e-5, 'bf16': 6e-2}
TOL_H_RMS = {'f32': 1e-5, 'bf16': 1e-2}
ROWS_TOL = {'f32': 2e-5, 'bf16': 1e-3}
ROWS_STATE_TOL = {'f32': 2e-5, 'bf16': 2e-2}


def rel_err(a, r):
    a, r = np.asarray(a, np.float64), np.asarray(r, np.float64)
    return np.abs(a - r).max() / max(np.abs(r).max(), 1e-30)


def rms_err(a, r):
    a, r = np.asarray(a, np.float64), np.asarray(r, np.float64)
    return np.sqrt(((a - r) ** 2).mean()) / np.sqrt((r ** 2).mean())


# ---------------------------------------------------------------------------------- 1. a NULL state is the plain forward
@pytest.mark.parametrize('dtype,per_step', sr.PLANS, ids=sr.PLAN_IDS)
@pytest.mark.parametrize('family', sr.FAMILIES)
def test_null_state_is_the_plain_forward(gpu, family, dtype, per_step):
    B, T = 2, 3
    eng = sr.engine(family, B, T, dtype, per_step, gpu, sr.params(family, T))
    x = torch.tensor(syn.c3d_features(81, B, T), device=gpu)
    logits, probs = [t.clone() for t in eng.forward(x)]
    want_state = sr.last_state(family, eng, B, T).clone()
    assert eng.state_elems == want_state.numel() == sr.STATE_PARTS[family] * B * 49 * 128
    # behind a call WITH a state (slot 0 of every path seeded), so that a stale seed would show
    junk = torch.randn(eng.state_elems, device=gpu)
    eng.forward_stream(x, state=junk, n_valid=2, **({'bn_phase': 1} if family == 'grcn' else {}))
    ls, ps, state = eng.forward_stream(x, state=None, n_valid=T)
    eng.status()
    assert torch.equal(ls, logits) and torch.equal(ps, probs)
    assert torch.equal(state, want_state)
    assert torch.isfinite(state).all() and float(state.abs().max()) > 1e-3
    l2, p2 = eng.forward(x)                                    # and the plain forward behind streaming calls is what it was
    assert torch.equal(l2, logits) and torch.equal(p2, probs)
    assert torch.equal(sr.last_state(family, eng, B, T), want_state)


# ---------------------------------------------------------------------------------- 2. cut invariance, bit for bit
CUTS = [(4, 4, 2), (3, 3, 3, 1), (1,) * 10, (2, 4, 4)]
CUT_CASES = [(B, d, ps) for B in (2, 8) for d, ps in sr.PLANS] + [(33, 'bf16', False)]


@pytest.mark.parametrize('B,dtype,per_step', CUT_CASES, ids=['B%d-%s' % (B, sr.PLAN_IDS[sr.PLANS.index((d, ps))]) for B, d, ps in CUT_CASES])
@pytest.mark.parametrize('family', sr.FAMILIES)
def test_cut_invariance_bit_for_bit(gpu, family, B, dtype, per_step):
    """T = 4, a 10-step stream; B = 8: placement branch ngroups % 8 == 0; B = 33: two clips per group, ragged last group, the <7>
    kernels.  The steps behind n_valid are fed 3.0, not zeros: they must not matter."""
    T, N = 4, 10
    eng = sr.engine(family, B, T, dtype, per_step, gpu, sr.params(family, T))
    x = torch.tensor(syn.c3d_features(82, B, N), device=gpu)
    ref_logits, ref_state = sr.run_stream(family, eng, x, CUTS[0], pad_value=3.0)
    eng.status()
    assert torch.isfinite(ref_logits).all() and torch.isfinite(ref_state).all()
    # the state matters: the second call of the stream is not the zero-state forward of its chunk
    zero_start = eng.forward(x[:, 4:8].contiguous())[0]
    assert not torch.equal(zero_start, ref_logits[:, 4:8])
    for cuts in CUTS[1:]:
        logits, state = sr.run_stream(family, eng, x, cuts, pad_value=3.0)
        eng.status()
        bad = [s for s in range(N) if not torch.equal(logits[:, s], ref_logits[:, s])]
        print('%s B=%d %s per_step=%d cuts %s: steps that differ %s, max |d logits| %.3e, max |d state| %.3e' % (
            family, B, dtype, per_step, cuts, bad, float((logits - ref_logits).abs().max()), float((state - ref_state).abs().max())))
        assert not bad, (cuts, bad)
        assert torch.equal(state, ref_state), cuts


# ---------------------------------------------------------------------------------- 3. one long plan, the float64 reference
_REF = {}


def reference(family, B):
    """(params of the T = 3 plan, the 7-step stream, float64 logits / states, bf16-emulation errors for gaze_lstm), once."""
    if family not in _REF:
        p = sr.params(family, 3)
        x = syn.c3d_features(83, B, 7)
        logits, st = sr.reference_f64(family, x, p, 3)
        emu = None
        if family == 'lstm':
            import lstm_ref
            el, es = sr.reference_f64(family, x, p, 3, emulate_bf16=True)
            emu = {'logits': lstm_ref.step_errors(el, logits), 'h': lstm_ref.step_errors(es['h'], st['h']),
                   'c': lstm_ref.step_errors(es['c'], st['c'])}
        _REF[family] = (p, x, logits, st, emu)
    return _REF[family]


@pytest.mark.parametrize('dtype,per_step', sr.PLANS, ids=sr.PLAN_IDS)
@pytest.mark.parametrize('family', sr.FAMILIES)
def test_stream_against_one_long_plan_and_float64(gpu, family, dtype, per_step):
    """A T = 3 plan, calls of 3, 3 and 1 steps, against a T = 7 plan's zero-state forward (batch-norm rows tiled s % 3) and against
    float64 over the 7 steps."""
    B = 2
    p, x, ref_logits, ref_st, emu = reference(family, B)
    xd = torch.tensor(x, device=gpu)
    eng = sr.engine(family, B, 3, dtype, per_step, gpu, p)
    logits, state = sr.run_stream(family, eng, xd, (3, 3, 1))
    eng.status()
    long_eng = sr.engine(family, B, 7, dtype, per_step, gpu, sr.tile_bn(p, 7) if family == 'grcn' else p)
    long_logits = long_eng.forward(xd)[0]
    long_eng.status()
    long_state = sr.last_state(family, long_eng, B, 7)
    e_long = float((logits - long_logits).abs().max() / long_logits.abs().max())
    e_long_s = float((state - long_state).abs().max() / long_state.abs().max())
    got, got_st = logits.cpu().numpy(), sr.state_parts(family, state, B)
    e_z = rel_err(got, ref_logits)
    e_h = {k: rel_err(got_st[k], ref_st[k][:, -1]) for k in got_st}
    e_rms = {k: rms_err(got_st[k], ref_st[k][:, -1]) for k in got_st}
    print('%s %s per_step=%d: vs T=7 plan logits %.3e state %.3e; vs float64 logits %.3e, final state max %s rms %s' % (
        family, dtype, per_step, e_long, e_long_s, e_z, {k: '%.3e' % v for k, v in e_h.items()}, {k: '%.3e' % v for k, v in e_rms.items()}))
    assert e_long <= TOL[dtype] and e_long_s <= TOL_H_MAX[dtype]
    if family == 'lstm' and dtype == 'bf16':
        import lstm_ref
        fro, mx = lstm_ref.step_errors(got, ref_logits)
        print('  logits fro per step %s (emulation %s), max-abs %.3e (emulation %.3e)' % (fro, emu['logits'][0], mx, emu['logits'][1]))
        assert (fro <= 2.0 * emu['logits'][0]).all() and mx <= 2.0 * emu['logits'][1]
        for k in ('h', 'c'):
            f1, m1 = lstm_ref.step_errors(got_st[k][:, None], ref_st[k][:, -1:])
            print('  final %s: fro %.3e (emulation %.3e)' % (k, f1[0], emu[k][0][-1]))
            assert f1[0] <= 2.0 * emu[k][0][-1], k
    elif family == 'lstm':
        assert e_z < TOL['f32'] and all(v < TOL['f32'] for v in e_h.values())
    else:
        if family == 'grcn' or dtype == 'f32':
            assert e_z < TOL[dtype]
        assert e_h['h'] < TOL_H_MAX[dtype] and e_rms['h'] < TOL_H_RMS[dtype]


# ---------------------------------------------------------------------------------- 4. conv5b rows as the input
@pytest.mark.parametrize('dtype,per_step', sr.PLANS, ids=sr.PLAN_IDS)
@pytest.mark.parametrize('family', sr.FAMILIES)
def test_rows_input_equals_the_c3d_input_form(gpu, family, dtype, per_step):
    B, T, N = 2, 3, 5
    eng = sr.engine(family, B, T, dtype, per_step, gpu, sr.params(family, T))
    x = torch.tensor(syn.c3d_features(84, B, N), device=gpu)
    pa, pb = [], []
    la, sa = sr.run_stream(family, eng, x, (3, 2), probs_out=pa)
    lb, sb = sr.run_stream(family, eng, x, (3, 2), use_rows=lambda c: sr.to_rows(c, dtype), probs_out=pb)
    eng.status()
    e_l = float((la - lb).abs().max() / la.abs().max())
    e_p = float((torch.cat(pa, 1) - torch.cat(pb, 1)).abs().max())
    e_s = float((sa - sb).abs().max() / sa.abs().max())
    print('rows vs c3d_input %s %s per_step=%d: logits %.3e probs %.3e state %.3e' % (family, dtype, per_step, e_l, e_p, e_s))
    assert e_l < ROWS_TOL[dtype] and e_p < ROWS_TOL[dtype]
    assert e_s < ROWS_STATE_TOL[dtype]


# ---------------------------------------------------------------------------------- 5. the models
def make_model(family, gpu, tmp_path, B=2, T=4):
    from recurrent_gaze_prediction_amd.models.base import Session
    if family == 'grcn':
        from recurrent_gaze_prediction_amd.models.gaze_grcn import GazePredictionGRCN as M, GRUModelConfig
    elif family == 'grcn77':
        from recurrent_gaze_prediction_amd.models.gaze_grcn77 import GazePredictionGRCN77 as M, GRUModelConfig
    else:
        from recurrent_gaze_prediction_amd.models.gaze_lstm import GazePredictionLSTM as M, GRUModelConfig
    cfg = GRUModelConfig()
    cfg.batch_size, cfg.n_lstm_steps, cfg.compute_dtype, cfg.train_dir, cfg.trainable = B, T, 'bf16', str(tmp_path), False
    m = M(Session(gpu), None, cfg)
    m.load_state_dict(sr.params(family, T))
    return m


@pytest.mark.parametrize('family', sr.FAMILIES)
def test_predict_long_clips_equals_each_clip_alone_in_lane_0(gpu, tmp_path, family):
    from recurrent_gaze_prediction_amd.stream import GazeStream, predict_long_clips
    model = make_model(family, gpu, tmp_path)
    clips = [syn.c3d_features(90 + i, 1, n)[0] for i, n in enumerate((5, 9, 2))]
    maps = predict_long_clips(model, clips)
    hw = sr.MAP_HW[family]
    for c, m in zip(clips, maps):
        st, alone = GazeStream(model), []
        for s in range(0, len(c), 4):
            part = c[s:s + 4]
            x = np.zeros((2, len(part), 1024, 7, 7), np.float32)
            x[0] = part
            alone.append(st.push_features(x)[0].cpu().numpy())
        alone = np.concatenate(alone)
        assert m.shape == (len(c), hw, hw) and np.isfinite(m).all()
        assert np.array_equal(m, alone)
    with pytest.raises(AssertionError):
        GazeStream(model).push_windows(None)                   # no C3D engine was given


@pytest.mark.parametrize('family', sr.FAMILIES)
def test_predict_long_clip_with_and_without_the_carried_state(gpu, tmp_path, family):
    from recurrent_gaze_prediction_amd.models.evaluate_gaze import predict_long_clip
    model = make_model(family, gpu, tmp_path)
    clip = syn.c3d_features(95, 1, 9)[0]
    chunked = predict_long_clip(model, clip)
    carried = predict_long_clip(model, clip, carry_state=True)
    assert chunked.shape == carried.shape == (9, sr.MAP_HW[family], sr.MAP_HW[family])
    assert np.array_equal(carried[:4], chunked[:4])            # the first chunk starts from zeros either way
    d = np.abs(carried - chunked).reshape(9, -1).max(-1)
    print('%s carried vs chunked, max |d map| per step: %s' % (family, d))
    assert (d[4:] > 0).all()                                   # from step 4 on the model remembers


def test_other_models_refuse(gpu, tmp_path):
    from recurrent_gaze_prediction_amd.models.base import Session
    from recurrent_gaze_prediction_amd.models.gaze_c3d_conv import GazePredictionConv
    from recurrent_gaze_prediction_amd.models.gaze_rnn import GRUModelConfig
    cfg = GRUModelConfig()
    cfg.batch_size, cfg.n_lstm_steps, cfg.compute_dtype, cfg.train_dir, cfg.trainable = 2, 3, 'bf16', str(tmp_path), False
    with pytest.raises(NotImplementedError):
        GazePredictionConv(Session(gpu), None, cfg).predict_stream(syn.c3d_features(1, 2, 3))


# ---------------------------------------------------------------------------------- 6. training plans
@pytest.mark.parametrize('family', sr.FAMILIES)
def test_backward_behind_a_streaming_call_is_refused(gpu, family):
    B, T = 2, 3
    eng = sr.engine(family, B, T, 'bf16', False, gpu, sr.params(family, T), save=True)
    x = torch.tensor(syn.c3d_features(85, B, T), device=gpu)
    hw = sr.MAP_HW[family]
    labels = torch.full((B, T, hw, hw), 1.0 / (hw * hw), device=gpu)
    logits, probs, state = eng.forward_stream(x)               # accepted on a training plan
    assert torch.isfinite(logits).all()
    with pytest.raises(_lib.RgpError) as e:
        eng.backward(logits, probs, labels)
    assert e.value.code == -4, e.value                         # RGP_ESTATE: no truncated BPTT
    l2, p2 = eng.forward(x)                                    # a plain forward re-arms the backward
    assert torch.equal(l2, logits)
    grads = eng.backward(l2, p2, labels)
    assert all(torch.isfinite(g).all() for g in grads.values())
