"""GPU: the recurrences of gaze_grcn and gaze_lstm, each gate of each step of each clip, on the device's OWN operands
(tests/recurrence_local_ref.py): the persistent kernels convgru_seq_kernel<4|7, STREAM> / convlstm_seq_kernel and the per-step
launches, on bf16 training plans, which keep every intermediate.

The end-to-end bounds of tests/test_grcn_gpu.py, test_lstm_gpu.py and test_stream_gpu.py have to allow for bf16 operand rounding
that compounds over T steps (6e-2 on the ConvGRU states).  Given the device's h_{t-1} (c_{t-1}), xpre / emb and gates, one step has no
compounding and only roundings that are known exactly, so a bf16 plan is held to the project's f32 bound here:

  gates u, r, c / i, f, g, o, and the LSTM's h' = tanh(c') o      |dev - ref| <= 2e-5
  h' = u h + (1-u) c and c' = f c + i g from the device's gates   <= 2^-22 (doubled per binade of |c'| above 2: BLEND_TOL there)
  xpre                                                            <= 2e-5 of its max
  bn, emb (stored in bf16)                                        the bf16-rounded reference, or one ulp from it; not equal: at most
                                                                  0.1 % (bn) / 1 % (emb) of the elements (conditions, not
                                                                  measurements; the rule for values near zero: _bf16 there)

Shapes: (1, 2) one group; (3, 4) one clip per group, <4>; (33, 3) two clips per group, a ragged last group, <7>; (64, 2) every CU.
Filters are scaled so that the gates are active (asserted: a saturated gate hides its operands), batch-norm rows differ per slot.
Streaming calls (STREAM = true, seq_seed_kernel) start from a random fp32 state that bf16 cannot represent, with n_valid = T - 1 and
bn_phase = 2; a training plan writes r and c on a streaming call as well, so they are checked as in the plain forward.
tests/test_recurrence_local_cpu.py shows on a stand-in that these bounds hold with margin and catch each mistake they are meant for.
Every test prints its figures before it asserts (-s); measured values: DESIGN.md section 2."""
import numpy as np
import pytest
import torch

import recurrence_local_ref as rl

pytestmark = pytest.mark.gpu

SHAPES = [(1, 2), (3, 4), (33, 3), (64, 2)]
STREAM_SHAPES = [(3, 4), (33, 3)]
PATHS = [False, True]
PATH_IDS = ['persistent', 'per_step']
_INPUTS = {}


def inputs(family, B, T):
    """(params, features, float64 projection of them), once per session."""
    if (family, B, T) not in _INPUTS:
        p, x = rl.active_params(family, T), rl.features(B, T)
        _INPUTS[(family, B, T)] = (p, x, rl.projection(x, p))
    return _INPUTS[(family, B, T)]


def engine(family, B, T, per_step, gpu, p):
    """A bf16 training plan on the path asked for by name."""
    from recurrent_gaze_prediction_amd import engine as E
    if family == 'grcn':
        eng = E.GrcnEngine(B, T, dtype='bf16', device=gpu, per_step=per_step, save_for_backward=True)
    else:
        eng = E.LstmEngine(B, T, dtype='bf16', device=gpu, per_step=per_step, persistent=not per_step, save_for_backward=True)
    assert eng.persistent == (not per_step)
    eng.set_weights(p)
    return eng


def read(family, eng, B, T):
    """Every intermediate of the plan's last call as [B,T,49,C] numpy."""
    get = lambda k: eng.read_buffer(k).cpu().numpy()
    if family == 'grcn':
        dev = {'emb': get('c3d_embedded').reshape(B, T, 49, rl.P), 'xpre': get('xpre').reshape(B, T, 49, 3 * rl.S),
               'h': get('rcn_outputs').reshape(B, T, 49, rl.S), 'bn': get('bn').reshape(B, T, 49, rl.S)}
        for k in 'urc':                                            # [T,B,49,S] as the kernels write them
            dev[k] = np.ascontiguousarray(get(k).reshape(T, B, 49, rl.S).transpose(1, 0, 2, 3))
        return dev
    dev = {k: get(k).reshape(B, T, 49, rl.S) for k in 'ifgoch'}
    dev['emb'] = get('emb').reshape(B, T, 49, rl.P)
    return dev


def judge(tag, family, dev, errs):
    rl.report(tag, errs)
    act = rl.activity(dev, 'ur' if family == 'grcn' else 'ifo', 'c' if family == 'grcn' else 'g')
    print('%s: %.1f %% of the gates in (0.1, 0.9), %.1f %% of the candidates below 0.9' % (tag, 100 * act[0], 100 * act[1]))
    assert all(np.isfinite(v).all() for v in dev.values())
    assert act[0] >= 0.5 and act[1] >= 0.5
    assert rl.violations(errs) == [], {k: errs[k] for k in rl.violations(errs)}


@pytest.mark.parametrize('per_step', PATHS, ids=PATH_IDS)
@pytest.mark.parametrize('B,T', SHAPES)
@pytest.mark.parametrize('family', ['grcn', 'lstm'])
def test_every_gate_of_every_step_on_the_devices_own_operands(gpu, family, B, T, per_step):
    p, x, emb_ref = inputs(family, B, T)
    eng = engine(family, B, T, per_step, gpu, p)
    eng.forward(torch.tensor(x, device=gpu))
    eng.status()
    dev = read(family, eng, B, T)
    check = rl.check_gru if family == 'grcn' else rl.check_lstm
    errs = check(dev, x, p, emb_ref=emb_ref)
    judge('%s %s %dx%d' % (family, PATH_IDS[per_step], B, T), family, dev, errs)


@pytest.mark.parametrize('per_step', PATHS, ids=PATH_IDS)
@pytest.mark.parametrize('B,T', STREAM_SHAPES)
@pytest.mark.parametrize('family', ['grcn', 'lstm'])
def test_streaming_call_from_a_state_bf16_cannot_represent(gpu, family, B, T, per_step):
    """Step 0 reads bf16_rne(state_in) as its operand image and the fp32 state_in in r.h, the blend and the peepholes; the
    batch-norm slots are rotated by bn_phase; the state handed back is the device's h (and c) of step n_valid - 1, bit for bit."""
    p, x, emb_ref = inputs(family, B, T)
    eng = engine(family, B, T, per_step, gpu, p)
    state = rl.random_state(family, B)
    assert not np.array_equal(rl.bf16_rne(state), state)
    n = T - 1
    kw = {'bn_phase': 2} if family == 'grcn' else {}
    xd = torch.tensor(x, device=gpu)
    eng.forward(xd)                                                # the streaming call must not see what a plain forward left
    _, _, new_state = eng.forward_stream(xd, state=torch.tensor(state.reshape(-1), device=gpu), n_valid=n, **kw)
    eng.status()
    dev = read(family, eng, B, T)
    if family == 'grcn':
        errs = rl.check_gru(dev, x, p, state, 2, n, emb_ref=emb_ref)
        want_state = eng.read_buffer('rcn_outputs').reshape(B, T, -1)[:, n - 1].reshape(-1)
    else:
        errs = rl.check_lstm(dev, x, p, state, n, emb_ref=emb_ref)
        want_state = torch.stack([eng.read_buffer(k).reshape(B, T, -1)[:, n - 1] for k in ('h', 'c')]).reshape(-1)
    judge('stream %s %s %dx%d' % (family, PATH_IDS[per_step], B, T), family, {k: v[:, :n] for k, v in dev.items()}, errs)
    assert torch.equal(new_state, want_state)
