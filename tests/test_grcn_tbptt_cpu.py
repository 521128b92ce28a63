"""Training across the carried state of gaze_grcn, the parts that need no GPU:

1. the reference of the device tests (tests/grcn_tbptt_ref.py, float64 autograd of one chunk): chunks chained through the state
   gradient sum to the gradient of the uncut film, truncated ones do not, and what lies behind n_valid changes no bit;
2. the refusals of rgp_grcn_backward_stream that come ahead of any device work;
3. train_long_clip on a stand-in GrcnEngine: both modes, the batch-norm phase of every chunk.

Every test here fails on a package without rgp_grcn_backward_stream (grcn_tbptt_ref looks the binding up on import).
"""
import ctypes

import numpy as np
import pytest
import torch

import grcn_tbptt_ref as tb
from recurrent_gaze_prediction_amd import _lib

RGP_EINVAL, RGP_EWORKSPACE, RGP_ESTATE = -1, -3, -4     # include/rgp.h

# ------------------------------------------------------------------------------------------------ 1. the reference
FILM, T3, B2 = 7, 3, 2
CUTS = [(3, 3, 1), (2, 3, 2), (1,) * 7]
_film = {}


def film():
    if not _film:
        p = tb.params(T3)
        x, g = tb.features(B2, FILM), tb.labels(B2, FILM)
        _film.update(p=p, x=x, g=g, uncut=tb.uncut_backward(x, p, g, T3))
    return _film


@pytest.mark.parametrize('chunks', CUTS, ids=['3-3-1', '2-3-2', '1x7'])
def test_chained_chunks_sum_to_the_film_and_truncated_ones_do_not(chunks):
    """Measured (float64, B = 2, P = 512, S = 128): chained, the largest difference of any of the fifteen gradients is
    1.2e-15 / 1.0e-15 / 2.4e-15 of the tensor's maximum with cuts (3, 3, 1) / (2, 3, 2) / (1,) x 7 (the fc-GRU's figure was
    1.4e-15); truncated, the six ConvGRU filters and the projection miss by 0.35 .. 0.63 of their maximum with cuts (3, 3, 1)
    and (2, 3, 2) and by 0.50 .. 0.70 with seven one-step chunks.  The bound on the chained sum is 1e-12: float64 round-off of
    sums of a few thousand terms of either sign, three orders above the measured figure and eleven below the truncated miss,
    which is held to "a tenth of the maximum" -- an order above any bound a device test uses."""
    f = film()
    want = f['uncut'][0]
    total, per = tb.film_backward(f['x'], f['p'], f['g'], chunks, T3, chain=True, pad_seed=5)
    errs = tb.grad_errs(total, want, err=tb.max_err, skip=('out_b',))
    print('chained', chunks, max(errs.values()))
    assert max(errs.values()) < 1e-12, errs
    assert abs(total['out_b'].item()) < 1e-12 and abs(want['out_b'].item()) < 1e-12      # zero in theory (xentropy)
    # d loss / d h0 of the first chunk is the film's
    assert tb.max_err(per[0][1], f['uncut'][1]) < 1e-12
    trunc, _ = tb.film_backward(f['x'], f['p'], f['g'], chunks, T3, chain=False, pad_seed=5)
    miss = tb.grad_errs(trunc, want, err=tb.max_err)
    print('truncated', chunks, {k: round(miss[k], 3) for k in tb.RECURRENT})
    for k in tb.RECURRENT:
        if k != 'proj_c3d_b':
            assert miss[k] > 0.1, (k, miss[k])


@pytest.mark.parametrize('loss_type', ['xentropy', 'l2'])
def test_what_lies_behind_n_valid_changes_no_bit(loss_type):
    f = film()
    rs = np.random.RandomState(3)
    h0 = rs.randn(B2, 7, 7, tb.S) * 0.1
    d_out = rs.randn(B2, 7, 7, tb.S) * 1e-3
    outs = []
    for pad_x, pad_g in ((7.0, 0.0), (rs.randn(B2, 2, 1024, 7, 7).astype(np.float32) * 50, rs.rand(B2, 2, 49, 49).astype(np.float32) * 7)):
        x = tb.pad_chunk(f['x'], 4, 1, T3, pad_x)
        g = tb.pad_chunk(f['g'], 4, 1, T3, pad_g)
        outs.append(tb.chunk_backward(x, f['p'], g, h0=h0, d_state_out=d_out, n_valid=1, phase=1, loss_frames=B2 * FILM,
                                      loss_type=loss_type))
    a, b = outs
    assert all(np.array_equal(a[0][k], b[0][k]) for k in tb.FIELDS)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]
    # the batch-norm rows of the slots the chunk did not use receive no gradient
    used = (1 + 0) % T3
    for k in ('bn_gamma', 'bn_beta'):
        assert all(np.all(a[0][k][s] == 0) for s in range(T3) if s != used) and np.any(a[0][k][used] != 0)


# ------------------------------------------------------------------------------------------------ 2. ABI without a device
P = lambda a: ctypes.c_void_p(a or None)      # noqa: E731   (never dereferenced: argument errors come first)
LOGITS, PROBS, LABELS, D_OUT, D_IN = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
B, T = 3, 4


def _grads(null_field=None):
    st = _lib.GrcnWeights()
    for i, k in enumerate(_lib.GrcnWeights.FIELDS):
        setattr(st, k, None if k == null_field else 0x100000 * (i + 1))
    return st


def _call(lib, h, logits=LOGITS, probs=PROBS, labels=LABELS, d_out=D_OUT, d_in=D_IN, loss_frames=B * T, grads='ok', loss_type=0):
    st = _grads() if grads == 'ok' else grads
    rc = lib.rgp_grcn_backward_stream(h, P(logits), P(probs), P(labels), P(d_out), P(d_in), loss_frames,
                                      ctypes.byref(st) if st is not None else None, loss_type, None)
    return rc, lib.rgp_last_error()


@pytest.fixture(params=[(_lib.RGP_F32, _lib.RGP_GRCN_SAVE_FOR_BACKWARD), (_lib.RGP_BF16, _lib.RGP_GRCN_SAVE_FOR_BACKWARD),
                        (_lib.RGP_BF16, _lib.RGP_GRCN_SAVE_FOR_BACKWARD | _lib.RGP_GRCN_PER_STEP)],
                ids=['f32', 'bf16', 'bf16-per_step'])
def plan(request):
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.rgp_grcn_create(ctypes.byref(h), B, T, 512, 128, request.param[0], request.param[1]) == 0
    yield lib, h
    lib.rgp_grcn_destroy(h)


def test_backward_stream_is_exported_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, 'rgp_grcn_backward_stream')
    res, args = _lib.SIGNATURES['rgp_grcn_backward_stream']
    assert res is ctypes.c_int and len(args) == 10 and args[6] is ctypes.c_longlong


def test_argument_errors_name_the_argument_and_come_before_the_bound_check(plan):
    lib, h = plan
    first, last = _lib.GrcnWeights.FIELDS[0], _lib.GrcnWeights.FIELDS[-1]
    cases = [({'logits': 0}, b'logits'), ({'labels': 0}, b'labels'), ({'grads': None}, b'grads'),
             ({'grads': _grads(first)}, b'gradient pointer 0'),
             ({'grads': _grads(last)}, b'gradient pointer %d' % (len(_lib.GrcnWeights.FIELDS) - 1)),
             ({'loss_frames': 0}, b'loss_frames'), ({'loss_frames': -7}, b'loss_frames'),
             ({'loss_type': 2}, b'loss_type'), ({'loss_type': -1}, b'loss_type'),
             ({'probs': 0}, b'probs'), ({'d_out': D_IN, 'd_in': D_IN}, b'd_state_in'),
             ({'d_out': D_OUT + 4}, b'16-byte'), ({'d_in': D_IN + 8}, b'16-byte')]
    for kw, word in cases:
        rc, msg = _call(lib, h, **kw)
        assert rc == RGP_EINVAL and word in msg and b'rgp_grcn_backward_stream' in msg, (kw, rc, msg)
    rc, msg = _call(lib, None)
    assert rc == RGP_EINVAL and b'plan' in msg, (rc, msg)
    # every argument in range, the optional ones NULL or not (l2 needs no probs): what is left is the unbound plan
    for kw in ({}, {'d_out': 0}, {'d_in': 0}, {'d_out': 0, 'd_in': 0}, {'probs': 0, 'loss_type': 1}, {'loss_frames': 1 << 40}):
        rc, msg = _call(lib, h, **kw)
        assert rc == RGP_EWORKSPACE and b'workspace' in msg, (kw, rc, msg)


def test_an_inference_plan_is_refused_with_estate():
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.rgp_grcn_create(ctypes.byref(h), B, T, 512, 128, _lib.RGP_BF16, 0) == 0
    try:
        rc, msg = _call(lib, h)
        assert rc == RGP_ESTATE and b'save_for_backward' in msg, (rc, msg)
        rc, msg = _call(lib, h, loss_frames=0)                  # the argument error still comes first
        assert rc == RGP_EINVAL and b'loss_frames' in msg, (rc, msg)
    finally:
        lib.rgp_grcn_destroy(h)


# ------------------------------------------------------------------------------------------------ 3. train_long_clip
NS = 49 * 128


class _StandInEngine(object):
    """What train_long_clip touches of GrcnEngine.  'Recurrence': state + the sum of the valid steps' feature [.., 0, 0, 0], in
    every element; the 'gradient' of a chunk is loss_frames in every element; d_state_in = d_state + 1.  An instance with
    lose_at = k reports RGP_ETIMEOUT at its k-th status() (persistent instances only are asked).  No dropout site."""
    made = []
    STREAM_BN_PHASE = True

    def __init__(self, batch, n_steps, dim_proj=512, dim_state=128, dtype='bf16', save_for_backward=False, device='cpu',
                 per_step=False, unfolded_head=False):
        self.B, self.T, self.P, self.S = batch, n_steps, dim_proj, dim_state
        self.dtype, self.device, self.save_for_backward, self.per_step = dtype, device, save_for_backward, per_step
        self.persistent = not per_step
        self.lose_at, self.n_status = None, 0
        self.weights = None
        self.flat_grads = torch.zeros(4)
        self.calls, self.steps = [], []
        _StandInEngine.made.append(self)

    def set_weights(self, params):
        self.weights = {k: torch.as_tensor(np.asarray(v)).clone() for k, v in params.items()}

    def status(self):
        self.n_status += 1
        if self.lose_at is not None and self.n_status == self.lose_at:
            e = _lib.RgpError('lost member')
            e.code = _lib.RGP_ETIMEOUT
            raise e

    def forward_stream(self, c3d_input=None, rows=None, state=None, n_valid=None, bn_phase=0, want_probs=True):
        x = c3d_input
        assert tuple(x.shape) == (self.B, self.T, 1024, 7, 7) and rows is None
        before = None if state is None else state.clone()
        s0 = torch.zeros(self.B, NS) if state is None else state.view(self.B, NS)
        new_state = (s0 + x[:, :n_valid, 0, 0, 0].sum(1, keepdim=True)).reshape(-1)
        assert state is None or torch.equal(state, before)
        z = torch.zeros(self.B, self.T, 49, 49)
        self.calls.append(('fwd', n_valid, None if state is None else float(state[0]), bn_phase, x[:, :, 0, 0, 0].clone()))
        return z, (z.clone() if want_probs else None), new_state

    def backward_stream(self, logits, probs, labels, d_state=None, loss_frames=None, loss_type='xentropy', want_d_state=True):
        assert tuple(labels.shape) == (self.B, self.T, 49, 49)
        self.flat_grads = torch.full((4,), float(loss_frames))
        d_in = (torch.zeros(self.B, NS) if d_state is None else d_state) + 1.0
        self.calls.append(('bwd', None if d_state is None else float(d_state.reshape(-1)[0]), loss_frames, loss_type, want_d_state,
                           labels[:, :, 0, 0].clone()))
        return None, (d_in if want_d_state else None)

    def adam_step(self, step, lr, max_grad_norm=10.0, method='adam'):
        self.steps.append((step, self.flat_grads.clone()))
        return torch.ones(1)


def _model(monkeypatch, tmp_path, loss_type='l2', n_steps=3, **cfg_kw):
    from recurrent_gaze_prediction_amd import engine
    from recurrent_gaze_prediction_amd.models import gaze_grcn
    from recurrent_gaze_prediction_amd.models.base import Session
    monkeypatch.setattr(engine, 'GrcnEngine', _StandInEngine)
    monkeypatch.setattr(gaze_grcn, 'GrcnEngine', _StandInEngine)
    _StandInEngine.made = []
    cfg = gaze_grcn.GRUModelConfig()
    cfg.batch_size, cfg.n_lstm_steps, cfg.train_dir, cfg.loss_type = 2, n_steps, str(tmp_path), loss_type
    for k, v in cfg_kw.items():
        setattr(cfg, k, v)
    model = gaze_grcn.GazePredictionGRCN(Session('cpu'), None, cfg)
    monkeypatch.setattr(model, '_chunk_loss_sum', lambda logits, labels, n: torch.full((1,), float(n)))
    return model


def _clip(n):
    x = np.zeros((2, n, 1024, 7, 7), np.float32)
    x[:, :, 0, 0, 0] = np.arange(1, 2 * n + 1).reshape(2, n)
    g = np.zeros((2, n, 49, 49), np.float32)
    g[:, :, 0, 0] = 100 + np.arange(2 * n).reshape(2, n)
    return x, g


def test_truncated_mode_steps_once_per_chunk_from_the_carried_state(monkeypatch, tmp_path):
    model = _model(monkeypatch, tmp_path)
    x, g = _clip(7)
    trace = {}
    loss = model.train_long_clip(x, g, mode='truncated', trace=trace)
    eng = model.engine
    fwd, bwd = [c for c in eng.calls if c[0] == 'fwd'], [c for c in eng.calls if c[0] == 'bwd']
    assert [c[0] for c in eng.calls] == ['fwd', 'bwd'] * 3
    assert [c[1] for c in fwd] == [3, 3, 1]
    assert [c[3] for c in fwd] == [0, 0, 0]                                          # position mod T: cuts at multiples of T
    assert fwd[0][4].tolist() == [[1, 2, 3], [8, 9, 10]] and fwd[2][4].tolist() == [[7, 0, 0], [14, 0, 0]]
    assert [c[2] for c in fwd] == [None, 6.0, 21.0]
    assert bwd[2][5].tolist() == [[106, 0, 0], [113, 0, 0]]
    assert all(c[1] is None and c[3] == 'l2' and c[4] is False for c in bwd)
    assert [c[2] for c in bwd] == [6, 6, 2]                                          # loss_frames = B n
    assert [s for s, _ in eng.steps] == [0, 1, 2] and model.global_step == 3
    assert [float(s[0]) for s in trace['states']] == [6.0, 21.0, 28.0]
    assert loss == pytest.approx(7.0 / 14.0)


def test_exact_mode_runs_the_chunks_in_reverse_and_steps_once(monkeypatch, tmp_path):
    model = _model(monkeypatch, tmp_path, loss_type='xentropy')
    x, g = _clip(8)
    loss = model.train_long_clip(x, g, mode='exact')
    eng = model.engine
    assert [c[0] for c in eng.calls] == ['fwd'] * 3 + ['fwd', 'bwd'] * 3
    first, second = eng.calls[:3], eng.calls[3:]
    assert [c[1] for c in first] == [3, 3, 2] and [c[2] for c in first] == [None, 6.0, 21.0]
    re_fwd, bwd = second[0::2], second[1::2]
    assert [c[1] for c in re_fwd] == [2, 3, 3] and [c[2] for c in re_fwd] == [21.0, 6.0, None]     # reverse order, their own states
    assert all(c[3] == 0 for c in first + re_fwd)
    assert [c[1] for c in bwd] == [None, 1.0, 2.0]                                 # the chain: None, then each d_state_in
    assert all(c[2] == 16 and c[3] == 'xentropy' for c in bwd)                     # loss_frames = B S
    assert [c[4] for c in bwd] == [True, True, False]
    assert len(eng.steps) == 1 and model.global_step == 1
    assert eng.steps[0][1].tolist() == [48.0] * 4                                  # the three chunk gradients, summed
    assert loss == pytest.approx(8.0 / 16.0)


def test_refusals(monkeypatch, tmp_path):
    model = _model(monkeypatch, tmp_path)
    x, g = _clip(4)
    with pytest.raises(ValueError):
        model.train_long_clip(x, g, mode='full')
    model.dist = object()                                             # a process group is attached
    with pytest.raises(NotImplementedError) as e:
        model.train_long_clip(x, g)
    assert 'data-parallel' in str(e.value)
    model.dist = None
    model.config.loss_type = 'KLD'
    with pytest.raises(NotImplementedError) as e:
        model.train_long_clip(x, g)
    assert 'KLD' in str(e.value)
    model.config.loss_type = 'l2'
    model.engine = type('OtherEngine', (), {})()                      # neither the fc-GRU's engine nor gaze_grcn's
    with pytest.raises(NotImplementedError) as e:
        model.train_long_clip(x, g)
    assert 'gaze_grcn' in str(e.value)
    assert not _StandInEngine.made[0].calls


def test_a_timeout_repeats_the_chunk_in_truncated_mode_and_the_whole_call_in_exact_mode(monkeypatch, tmp_path):
    x, g = _clip(7)
    model = _model(monkeypatch, tmp_path)
    first = model.engine
    assert first.persistent
    first.lose_at = 2
    model.train_long_clip(x, g, mode='truncated')
    second = model.engine
    assert second is not first and second.per_step and not second.persistent
    assert [c[:3] for c in first.calls if c[0] == 'fwd'] == [('fwd', 3, None), ('fwd', 3, 6.0)]
    assert [c[:3] for c in second.calls if c[0] == 'fwd'] == [('fwd', 3, 6.0), ('fwd', 1, 21.0)]      # the poisoned chunk again, same state
    assert len(first.steps) == 1 and [s for s, _ in second.steps] == [1, 2] and model.global_step == 3
    # exact: lost in the second pass -> everything again on the new engine, one step in all
    model = _model(monkeypatch, tmp_path)
    first = model.engine
    first.lose_at = 5                                                 # three forwards of pass 1, then the second backward
    model.train_long_clip(x, g, mode='exact')
    second = model.engine
    assert second is not first and not first.steps
    assert [c[0] for c in second.calls] == ['fwd'] * 3 + ['fwd', 'bwd'] * 3
    assert len(second.steps) == 1 and second.steps[0][1].tolist() == [42.0] * 4 and model.global_step == 1


def test_train_long_clips_accepts_the_model(monkeypatch, tmp_path):
    from recurrent_gaze_prediction_amd.stream import train_long_clips
    model = _model(monkeypatch, tmp_path)
    x, g = _clip(5)
    loss = train_long_clips(model, [x[0], x[1]], [g[0], g[1]], mode='exact')
    assert loss == pytest.approx(5.0 / 10.0) and model.global_step == 1
