"""Host-only: the one-step references of tests/recurrence_local_ref.py are pinned to the oracle's cells, their bounds are validated
on a stand-in device (the same operands, fp32 products, fp32 accumulation), and every mistake the bounds are meant to catch is
seeded into that stand-in and must be caught by a factor of ten.  Every test prints its figures before it asserts (-s)."""
import numpy as np
import pytest
import torch

import lstm_ref
import recurrence_local_ref as rl
from oracle import torch_ref

S = rl.S


def _rand_step(seed, n, P=rl.P):
    rs = np.random.RandomState(seed)
    return rs.randn(n, 49, P), rs.uniform(-1, 1, (n, 49, S)), rs.uniform(-1, 1, (n, 49, S))


# ------------------------------------------------------------------------------------------------ 1. the helper is the cell
def test_gru_step_without_rounding_is_the_oracle_cell():
    p = rl.active_params('grcn', 2)
    x, h, _ = _rand_step(1, 2)
    xpre = rl.gru_xpre(x[:, None], p, rnd=rl.same)[:, 0]
    got = rl.gru_step(xpre, h, p, rnd=rl.same)['h']
    pt = {k: torch.tensor(np.asarray(v), dtype=torch.float64) for k, v in p.items()}
    want = torch_ref.grcn_cell(torch.tensor(x).reshape(2, 7, 7, -1), torch.tensor(h).reshape(2, 7, 7, S), pt).numpy().reshape(2, 49, S)
    err = np.abs(got - want).max()
    print('gru step, no rounding, against torch_ref.grcn_cell: %.3e' % err)
    assert err < 1e-12


def test_lstm_step_without_rounding_is_the_oracle_cell():
    p = rl.active_params('lstm', 2)
    x, h, c = _rand_step(2, 2)
    got = rl.lstm_step(x, c, h, rl.lstm_params_t(p), rnd=None)
    with torch.no_grad():
        cell = lstm_ref.lstm_cell(torch.tensor(x).reshape(2, 7, 7, -1), torch.tensor(c).reshape(2, 7, 7, S),
                                  torch.tensor(h).reshape(2, 7, 7, S), rl.lstm_params_t(p))
    loops = lstm_ref.lstm_cell_numpy(x[1].reshape(7, 7, -1), c[1].reshape(7, 7, S), h[1].reshape(7, 7, S), p)
    for k in 'ifgoch':
        e1 = np.abs(got[k] - cell[k].numpy().reshape(2, 49, S)).max()
        e2 = np.abs(got[k][1] - loops[k].reshape(49, S)).max()
        print('lstm step, no rounding, %s: against lstm_cell %.3e, against the numpy loops %.3e' % (k, e1, e2))
        assert e1 < 1e-12 and e2 < 1e-12, k


def _gru_emulation(x, p):
    """gaze_grcn's forward with bf16 operands, from the oracle's operators, as lstm_ref.lstm_forward(emulate_bf16=True) is built:
    x, emb, h, r.h and every filter rounded in front of each contraction, everything else float64."""
    q = lstm_ref.bf16
    pt = {k: torch.tensor(np.asarray(v), dtype=torch.float64) for k, v in p.items()}
    xt = torch.tensor(x, dtype=torch.float64)
    b, t = xt.shape[:2]
    emb = q(q(xt.permute(0, 1, 3, 4, 2)).reshape(-1, 1024) @ q(pt['proj_c3d_W']) + pt['proj_c3d_b']).reshape(b, t, 7, 7, -1)
    cs = torch_ref.conv2d_same
    h = torch.zeros(b, 7, 7, S, dtype=torch.float64)
    steps = {k: [] for k in 'urch'}
    for k in range(t):
        e, hb = emb[:, k], q(h)
        u = torch.sigmoid(cs(e, q(pt['GRU_Conv_Wz'])) + cs(hb, q(pt['GRU_Conv_Uz'])))
        r = torch.sigmoid(cs(e, q(pt['GRU_Conv_Wr'])) + cs(hb, q(pt['GRU_Conv_Ur'])))
        rh = (r.to(torch.float32) * h.to(torch.float32)).to(torch.bfloat16).to(torch.float64)
        c = torch.tanh(cs(e, q(pt['GRU_Conv_W'])) + cs(rh, q(pt['GRU_Conv_U'])))
        h = u * h + (1 - u) * c
        for name, v in zip('urch', (u, r, c, h)):
            steps[name].append(v.numpy().reshape(b, 49, S))
    return emb.numpy().reshape(b, t, 49, -1), {k: np.stack(v, 1) for k, v in steps.items()}


def test_chained_gru_steps_reproduce_the_bf16_emulation():
    B, T = 2, 3
    p, x = rl.active_params('grcn', T), rl.features(B, T)
    emb, want = _gru_emulation(x, p)
    assert np.array_equal(emb, rl.bf16_rne(rl.projection(x, p)))
    xpre = rl.gru_xpre(emb, p)
    h = np.zeros((B, 49, S))
    for t in range(T):
        st = rl.gru_step(xpre[:, t], h, p)
        for k in 'urch':
            err = np.abs(st[k] - want[k][:, t]).max()
            print('chained gru step %d %s: %.3e' % (t, k, err))
            assert err < 1e-12, (t, k)
        h = st['h']


def test_chained_lstm_steps_reproduce_the_bf16_emulation():
    B, T = 2, 3
    p, x = rl.active_params('lstm', T), rl.features(B, T)
    _, want = lstm_ref.forward_f64(x, p, emulate_bf16=True)
    emb = rl.bf16_rne(want['emb']).reshape(B, T, 49, -1)
    pt = rl.lstm_params_t(p)
    h, c = np.zeros((B, 49, S)), np.zeros((B, 49, S))
    for t in range(T):
        st = rl.lstm_step(emb[:, t], c, h, pt)
        for k in 'ifgoch':
            err = np.abs(st[k] - want[k][:, t].reshape(B, 49, S)).max()
            print('chained lstm step %d %s: %.3e' % (t, k, err))
            assert err < 1e-12, (t, k)
        h, c = st['h'], st['c']


# ------------------------------------------------------------------------------------------------ 2. the bounds hold with margin
_STANDIN = {}


def standin(family, B, T, stream=False, fault=None):
    """(x, params, state_in, dev dict of the stand-in), once per case: the inputs tests/test_recurrence_local_gpu.py uses."""
    key = (family, B, T, stream, fault)
    if key not in _STANDIN:
        p, x = rl.active_params(family, T), rl.features(B, T)
        st = rl.random_state(family, B) if stream else None
        if family == 'grcn':
            dev = rl.standin_gru(x, p, st, 2 if stream else 0, fault)
        else:
            dev = rl.standin_lstm(x, p, st, fault)
        _STANDIN[key] = (x, p, st, dev)
    return _STANDIN[key]


def check(family, B, T, stream=False, fault=None):
    x, p, st, dev = standin(family, B, T, stream, fault)
    if family == 'grcn':
        return dev, rl.check_gru(dev, x, p, st, 2 if stream else 0, T - 1 if stream else None)
    return dev, rl.check_lstm(dev, x, p, st, T - 1 if stream else None)


@pytest.mark.parametrize('B,T,stream', [(3, 4, False), (33, 3, False), (3, 4, True)])
@pytest.mark.parametrize('family', ['grcn', 'lstm'])
def test_fp32_stand_in_passes_every_bound_with_margin(family, B, T, stream):
    """fp32 products and fp32 accumulation of the same operands: every F32_TOL bound with 4x to spare, the one-ulp flips of emb
    and bn under a tenth of their caps (the caps are conditions: what an fp32 evaluation that lands on the other side of a
    rounding tie may cost, and nothing more), the blends within their count of roundings -- and the gates active."""
    dev, errs = check(family, B, T, stream)
    tag = 'stand-in %s %dx%d%s' % (family, B, T, ' stream' if stream else '')
    rl.report(tag, errs)
    act = rl.activity(dev, 'ur' if family == 'grcn' else 'ifo', 'c' if family == 'grcn' else 'g')
    print('%s: %.1f %% of the gates in (0.1, 0.9), %.1f %% of the candidates below 0.9' % (tag, 100 * act[0], 100 * act[1]))
    assert rl.violations(errs, margin=4.0, cap_margin=10.0) == []
    assert act[0] >= 0.5 and act[1] >= 0.5


# ------------------------------------------------------------------------------------------------ 3. seeded faults are caught
FAULTS = [('grcn', f, t) for f, t in zip(rl.GRU_FAULTS, ('u', 'c', 'c', 'c', 'u', 'u', 'bn'))] + \
         [('lstm', f, t) for f, t in zip(rl.LSTM_FAULTS, ('o', 'g'))]


@pytest.mark.parametrize('family,fault,tensor', FAULTS, ids=[f for _, f, _ in FAULTS])
def test_seeded_fault_exceeds_a_bound_tenfold(family, fault, tensor):
    """One mistake in the stand-in, everything else as above: the tensor it corrupts must miss its bound by at least 10x at some
    element -- otherwise the weights or inputs would not be sensitive enough to show it on a device either."""
    _, errs = check(family, 3, 4, fault=fault)
    rl.report('fault %s' % fault, errs)
    assert errs[tensor]['ratio'] >= 10.0, errs[tensor]
    clean = set(errs) - {tensor} - {{'halo': 'r', 'next_clip_xpre': 'r'}.get(fault)}
    if fault == 'next_clip_xpre':
        clean -= {'c'}
    assert not set(rl.violations(errs)) & clean                  # and it is attributed: the other operators still pass
