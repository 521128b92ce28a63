"""CPU: what training across the fc-GRU's carried state (rgp_fcgru_backward_stream, FcGruEngine.backward_stream,
GazePredictionGRU.train_long_clip) can show without a device.

1. The reference of the GPU tests (fcgru_tbptt_ref.chunk_backward, float64 numpy) agrees with float64 torch autograd.
2. Composition: the chunk gradients of a cut film, the state gradient chained backwards, sum to the gradients of the uncut film;
   with the chain dropped the six variables of the recurrent path miss by far, the read-out pair does not move; what lies
   behind n_valid changes nothing.
3. The C ABI on unbound plans: argument errors are RGP_EINVAL, name their argument and come ahead of RGP_EWORKSPACE; an
   inference plan is RGP_ESTATE.
4. train_long_clip on a stand-in engine: chunking, states, reverse order, masks, divisors, optimizer steps, refusals, time-outs.
"""
import ctypes

import numpy as np
import pytest
import torch

import fcgru_tbptt_ref as tb
from recurrent_gaze_prediction_amd import _lib

RGP_EINVAL, RGP_EWORKSPACE, RGP_ESTATE = -1, -3, -4     # include/rgp.h
N = tb.N


# ------------------------------------------------------------------------------------------------ 1. the reference
def _autograd(x, p, g, h0, d_out, nv, lf, loss_type):
    f = lambda a: torch.tensor(np.asarray(a, np.float64))
    pt = {k: f(v).requires_grad_(True) for k, v in p.items()}
    h = f(h0).requires_grad_(True)
    B = x.shape[0]
    emb = (f(x[:, :nv]).permute(0, 1, 3, 4, 2).reshape(-1, 1024) @ pt['proj_c3d_W'] + pt['proj_c3d_b']).reshape(B, nv, -1)
    gt = f(g).reshape(B, g.shape[1], -1)
    state, loss = h, 0.0
    for t in range(nv):
        ru = torch.sigmoid(torch.cat([emb[:, t], state], 1) @ pt['gates_kernel'] + pt['gates_bias'])
        r, u = ru[:, :N], ru[:, N:]
        c = torch.tanh(torch.cat([emb[:, t], r * state], 1) @ pt['candidate_kernel'] + pt['candidate_bias'])
        state = u * state + (1.0 - u) * c
        z = state @ pt['proj_out_W'] + pt['proj_out_b']
        loss = loss + (-(gt[:, t] * torch.log_softmax(z, -1)).sum() if loss_type == 'xentropy' else 0.5 * ((z - gt[:, t]) ** 2).sum()) / lf
    (loss + (f(d_out) * state).sum()).backward()
    return {k: pt[k].grad.numpy() for k in p}, h.grad.numpy(), state.detach().numpy(), float(loss.detach())


@pytest.mark.parametrize('loss_type', ['xentropy', 'l2'])
def test_chunk_reference_agrees_with_autograd(loss_type):
    B, T, nv, gh = 2, 3, 2, 7
    p, x, g = tb.params(gh), tb.features(B, T), tb.labels(B, T, gh)
    rs = np.random.RandomState(5)
    h0, d_out = 0.3 * rs.randn(B, N), 1e-2 * rs.randn(B, N)
    gr, d_in, s_out, loss = tb.chunk_backward(x, p, g, h0, d_out, nv, 11, loss_type)
    want, d_want, s_want, l_want = _autograd(x, p, g, h0, d_out, nv, 11.0, loss_type)
    errs = dict(tb.grad_errs(gr, want), d_state_in=tb.rel_err(d_in, d_want), state_out=tb.rel_err(s_out, s_want),
                loss=abs(loss - l_want) / abs(l_want))
    print(loss_type, errs)
    assert all(np.abs(want[k]).max() > 0 for k in want) and np.abs(d_want).max() > 0
    assert max(errs.values()) < 1e-10, errs
    # a null state and a null gradient are zeros
    a = tb.chunk_backward(x, p, g, None, None, nv, 11, loss_type)
    b = tb.chunk_backward(x, p, g, np.zeros((B, N)), np.zeros((B, N)), nv, 11, loss_type)
    assert all(np.array_equal(a[0][k], b[0][k]) for k in tb.FIELDS) and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------ 2. composition
@pytest.mark.parametrize('gh', [7, 49])
def test_chained_chunks_sum_to_the_film_and_truncated_ones_do_not(gh):
    B, S = 2, 7
    p, x, g = tb.params(gh), tb.features(B, S), tb.labels(B, S, gh)
    film = tb.chunk_backward(x, p, g, None, None, S, B * S)[0]
    for chunks in ((3, 3, 1), (2, 3, 2), (1,) * 7):
        T = max(chunks)
        chained, per = tb.film_backward(x, p, g, chunks, T=T, pad_seed=3)
        errs = tb.grad_errs(chained, film)
        cut_grads = [float(np.abs(c[3]).max()) for c in per[:-1]]
        print(gh, chunks, 'chained', max(errs.values()), 'max |d state| at the cuts', cut_grads)
        assert max(errs.values()) < 1e-12, errs
        assert per[-1][3] is None and all(v > 0 for v in cut_grads)
        trunc, _ = tb.film_backward(x, p, g, chunks, T=T, chain=False, pad_seed=3)
        miss = tb.grad_errs(trunc, film)
        print(gh, chunks, 'truncated', miss)
        assert all(miss[k] > tb.TRUNCATED_MISS for k in tb.RECURRENT), miss
        assert all(np.array_equal(trunc[k], chained[k]) for k in ('proj_out_W', 'proj_out_b'))
        # what lies behind n_valid (features 7.0, random labels) reaches nothing
        plain, _ = tb.film_backward(x, p, g, chunks, T=T, pad_x=0.0, pad_seed=None)
        assert all(np.array_equal(plain[k], chained[k]) for k in tb.FIELDS)


# ------------------------------------------------------------------------------------------------ 3. ABI without a device
P = lambda a: ctypes.c_void_p(a or None)      # noqa: E731   (never dereferenced: argument errors come first)
LOGITS, PROBS, LABELS, D_OUT, D_IN = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
B, T = 3, 4


def _grads(null_field=None):
    st = _lib.FcGruWeights()
    for i, k in enumerate(_lib.FcGruWeights.FIELDS):
        setattr(st, k, None if k == null_field else 0x100000 * (i + 1))
    return st


def _call(lib, h, logits=LOGITS, probs=PROBS, labels=LABELS, d_out=D_OUT, d_in=D_IN, loss_frames=B * T, grads='ok', loss_type=0):
    st = _grads() if grads == 'ok' else grads
    rc = lib.rgp_fcgru_backward_stream(h, P(logits), P(probs), P(labels), P(d_out), P(d_in), loss_frames,
                                       ctypes.byref(st) if st is not None else None, loss_type, None)
    return rc, lib.rgp_last_error()


@pytest.fixture(params=[(_lib.RGP_F32, _lib.RGP_FCGRU_SAVE_FOR_BACKWARD), (_lib.RGP_BF16, _lib.RGP_FCGRU_SAVE_FOR_BACKWARD | _lib.RGP_FCGRU_PER_STEP)],
                ids=['f32', 'bf16-per_step'])
def plan(request):
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.rgp_fcgru_create_flags(ctypes.byref(h), B, T, 7, 7, request.param[0], request.param[1]) == 0
    yield lib, h
    lib.rgp_fcgru_destroy(h)


def test_backward_stream_is_exported_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, 'rgp_fcgru_backward_stream')
    res, args = _lib.SIGNATURES['rgp_fcgru_backward_stream']
    assert res is ctypes.c_int and len(args) == 10 and args[6] is ctypes.c_longlong


def test_argument_errors_name_the_argument_and_come_before_the_bound_check(plan):
    lib, h = plan
    cases = [({'logits': 0}, b'logits'), ({'labels': 0}, b'labels'), ({'grads': None}, b'grads'),
             ({'grads': _grads('candidate_bias')}, b'gradient pointer 5'), ({'grads': _grads('proj_c3d_W')}, b'gradient pointer 0'),
             ({'loss_frames': 0}, b'loss_frames'), ({'loss_frames': -7}, b'loss_frames'),
             ({'loss_type': 2}, b'loss_type'), ({'loss_type': -1}, b'loss_type'),
             ({'probs': 0}, b'probs'), ({'d_out': D_IN, 'd_in': D_IN}, b'd_state_in')]
    for kw, word in cases:
        rc, msg = _call(lib, h, **kw)
        assert rc == RGP_EINVAL and word in msg and b'rgp_fcgru_backward_stream' in msg, (kw, rc, msg)
    rc, msg = _call(lib, None)
    assert rc == RGP_EINVAL and b'plan' in msg, (rc, msg)
    # every argument in range, the optional ones NULL or not (l2 needs no probs): what is left is the unbound plan
    for kw in ({}, {'d_out': 0}, {'d_in': 0}, {'d_out': 0, 'd_in': 0}, {'probs': 0, 'loss_type': 1}, {'loss_frames': 1 << 40}):
        rc, msg = _call(lib, h, **kw)
        assert rc == RGP_EWORKSPACE and b'workspace' in msg, (kw, rc, msg)


def test_an_inference_plan_is_refused_with_estate():
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.rgp_fcgru_create_flags(ctypes.byref(h), B, T, 7, 7, _lib.RGP_BF16, 0) == 0
    try:
        rc, msg = _call(lib, h)
        assert rc == RGP_ESTATE and b'save_for_backward' in msg, (rc, msg)
        rc, msg = _call(lib, h, loss_frames=0)                  # the argument error still comes first
        assert rc == RGP_EINVAL and b'loss_frames' in msg, (rc, msg)
    finally:
        lib.rgp_fcgru_destroy(h)


# ------------------------------------------------------------------------------------------------ 4. train_long_clip
class _Dropout(object):
    """The site of a stand-in engine: a 'mask' that is the number of the draw."""

    def __init__(self):
        self.keep_prob, self.seed, self.draws, self.mask, self.log = 1.0, 0, 0, torch.zeros(1), []

    def configure(self, keep_prob, seed=0):
        self.keep_prob, self.seed, self.draws = float(keep_prob), int(seed), 0

    def arm(self, train):
        if train == 'keep':
            self.log.append(('keep', float(self.mask)))
        elif train and self.keep_prob < 1.0:
            self.draws += 1
            self.mask = torch.full((1,), float(self.draws))
            self.log.append(('draw', float(self.mask)))
        else:
            self.log.append(('off', None))

    def use(self, mask, keep_prob):
        self.mask = mask.clone()
        self.log.append(('use', float(mask)))


class _StandInEngine(object):
    """What train_long_clip touches of FcGruEngine.  'Recurrence': state + the sum of the valid steps' feature [.., 0, 0, 0], in
    every column; the 'gradient' of a chunk is loss_frames in every element; d_state_in = d_state + 1.  An instance with
    lose_at = k reports RGP_ETIMEOUT at its k-th status() (persistent instances only are asked)."""
    made = []
    STREAM_BN_PHASE = False

    def __init__(self, batch, n_steps, gazemap_hw=(49, 49), dtype='f32', device='cpu', save_for_backward=False, per_step=False,
                 persistent=False, bptt_persistent=False, bptt_persistent_f32=False):
        self.B, self.T, self.GH, self.GW = batch, n_steps, gazemap_hw[0], gazemap_hw[1]
        self.dtype, self.device, self.save_for_backward, self.per_step = dtype, device, save_for_backward, per_step
        self.persistent = bool(persistent)
        self.bptt_persistent = bool(bptt_persistent or bptt_persistent_f32)
        self.lose_at, self.n_status = None, 0
        self.weights = None
        self.adam_m = self.adam_v = None
        self.flat_grads = torch.zeros(4)
        self.dropout = _Dropout()
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

    def forward_stream(self, x, state=None, n_valid=None, want_probs=True, train=False):
        assert tuple(x.shape) == (self.B, self.T, 1024, 7, 7)
        self.dropout.arm(train)
        before = None if state is None else state.clone()
        s0 = torch.zeros(self.B, N) if state is None else state.view(self.B, N)
        new_state = (s0 + x[:, :n_valid, 0, 0, 0].sum(1, keepdim=True)).reshape(-1)
        assert state is None or torch.equal(state, before)
        z = torch.zeros(self.B, self.T, self.GH, self.GW) + float(self.dropout.mask)
        self.calls.append(('fwd', n_valid, None if state is None else float(state[0]), train, x[:, :, 0, 0, 0].clone()))
        return z, (z.clone() if want_probs else None), new_state

    def backward_stream(self, logits, probs, labels, d_state=None, loss_frames=None, loss_type='xentropy', want_d_state=True):
        assert tuple(labels.shape) == (self.B, self.T, self.GH, self.GW)
        self.flat_grads = torch.full((4,), float(loss_frames))
        d_in = (torch.zeros(self.B, N) if d_state is None else d_state) + 1.0
        self.calls.append(('bwd', None if d_state is None else float(d_state.reshape(-1)[0]), loss_frames, loss_type, want_d_state,
                           labels[:, :, 0, 0].clone()))
        return None, (d_in if want_d_state else None)

    def adam_step(self, step, lr, max_grad_norm=10.0, method='adam'):
        self.steps.append((step, self.flat_grads.clone()))
        return torch.ones(1)


def _model(monkeypatch, tmp_path, module, hw=None, loss_type='l2', **path):
    from recurrent_gaze_prediction_amd import engine
    from recurrent_gaze_prediction_amd.models.base import Session
    monkeypatch.setattr(engine, 'FcGruEngine', _StandInEngine)
    _StandInEngine.made = []
    cfg = module.GRUModelConfig()
    cfg.batch_size, cfg.n_lstm_steps, cfg.train_dir, cfg.loss_type = 2, 3, str(tmp_path), loss_type
    for k, v in path.items():
        setattr(cfg, k, v)
    kw = {} if hw is None else {'gazemap_height': hw, 'gazemap_width': hw}
    model = module.GazePredictionGRU(Session('cpu'), None, cfg, **kw)
    monkeypatch.setattr(model, '_chunk_loss_sum', lambda logits, labels, n: torch.full((1,), float(n)))
    return model


def _film(S, hw=7):
    x = np.zeros((2, S, 1024, 7, 7), np.float32)
    x[:, :, 0, 0, 0] = np.arange(1, 2 * S + 1).reshape(2, S)
    g = np.zeros((2, S, hw, hw), np.float32)
    g[:, :, 0, 0] = 100 + np.arange(2 * S).reshape(2, S)
    return x, g


def _modules():
    from recurrent_gaze_prediction_amd.models import gaze_rnn, gaze_rnn77
    return ((gaze_rnn, 7), (gaze_rnn77, None))


def test_truncated_mode_steps_once_per_chunk_from_the_carried_state(monkeypatch, tmp_path):
    for module, hw in _modules():
        model = _model(monkeypatch, tmp_path, module, hw)
        model.engine.dropout.configure(0.5)
        x, g = _film(7)
        trace = {}
        loss = model.train_long_clip(x, g, mode='truncated', trace=trace)
        eng = model.engine
        fwd, bwd = [c for c in eng.calls if c[0] == 'fwd'], [c for c in eng.calls if c[0] == 'bwd']
        assert [c[0] for c in eng.calls] == ['fwd', 'bwd'] * 3
        assert [c[1] for c in fwd] == [3, 3, 1] and all(c[3] is True for c in fwd)
        # the chunks, zero-padded behind n_valid, and the state each call starts from (lane 0: the running sum of 1 .. 7)
        assert fwd[0][4].tolist() == [[1, 2, 3], [8, 9, 10]] and fwd[2][4].tolist() == [[7, 0, 0], [14, 0, 0]]
        assert [c[2] for c in fwd] == [None, 6.0, 21.0]
        assert bwd[2][5].tolist() == [[106, 0, 0], [113, 0, 0]]
        assert all(c[1] is None and c[3] == 'l2' and c[4] is False for c in bwd)
        assert [c[2] for c in bwd] == [6, 6, 2]                                      # loss_frames = B n
        assert [s for s, _ in eng.steps] == [0, 1, 2] and model.global_step == 3
        assert [float(gr[0]) for _, gr in eng.steps] == [6.0, 6.0, 2.0]
        assert [float(s[0]) for s in trace['states']] == [6.0, 21.0, 28.0]
        assert loss == pytest.approx(7.0 / 14.0)


def test_exact_mode_runs_the_chunks_in_reverse_with_their_masks_and_steps_once(monkeypatch, tmp_path):
    for module, hw in _modules():
        model = _model(monkeypatch, tmp_path, module, hw, loss_type='xentropy')
        model.engine.dropout.configure(0.5)
        x, g = _film(8)
        loss = model.train_long_clip(x, g, mode='exact')
        eng = model.engine
        assert [c[0] for c in eng.calls] == ['fwd'] * 3 + ['fwd', 'bwd'] * 3
        first, second = eng.calls[:3], eng.calls[3:]
        assert [c[1] for c in first] == [3, 3, 2] and [c[2] for c in first] == [None, 6.0, 21.0]
        assert all(c[3] is True for c in first)
        re_fwd, bwd = second[0::2], second[1::2]
        assert [c[1] for c in re_fwd] == [2, 3, 3] and [c[2] for c in re_fwd] == [21.0, 6.0, None]     # reverse order, their own states
        assert all(c[3] == 'keep' for c in re_fwd)
        assert [c[1] for c in bwd] == [None, 1.0, 2.0]                                 # the chain: None, then each d_state_in
        assert all(c[2] == 16 and c[3] == 'xentropy' for c in bwd)                     # loss_frames = B S
        assert [c[4] for c in bwd] == [True, True, False]
        # masks: drawn 1, 2, 3 in the first pass, installed again 3, 2, 1
        log = eng.dropout.log
        assert log[:3] == [('draw', 1.0), ('draw', 2.0), ('draw', 3.0)]
        assert log[3:] == [('use', 3.0), ('keep', 3.0), ('use', 2.0), ('keep', 2.0), ('use', 1.0), ('keep', 1.0)]
        assert len(eng.steps) == 1 and model.global_step == 1
        assert eng.steps[0][1].tolist() == [48.0] * 4                                  # the three chunk gradients, summed
        assert loss == pytest.approx(8.0 / 16.0)
        # without dropout the site stays off in both passes
        model.engine.dropout.configure(1.0)
        model.engine.dropout.log = []
        model.train_long_clip(x, g, mode='exact')
        assert all(e == ('off', None) for e in model.engine.dropout.log) and model.global_step == 2


def test_refusals(monkeypatch, tmp_path):
    from recurrent_gaze_prediction_amd.models import gaze_rnn
    model = _model(monkeypatch, tmp_path, gaze_rnn, 7)
    x, g = _film(4)
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
    model.engine = type('OtherEngine', (), {})()                      # not the fc-GRU's engine
    with pytest.raises(NotImplementedError) as e:
        model.train_long_clip(x, g)
    assert 'gaze_rnn' in str(e.value)
    assert not _StandInEngine.made[0].calls


def test_a_timeout_repeats_the_chunk_in_truncated_mode_and_the_whole_call_in_exact_mode(monkeypatch, tmp_path):
    from recurrent_gaze_prediction_amd.models import gaze_rnn
    x, g = _film(7)
    # truncated: the second chunk's status reports the lost member
    model = _model(monkeypatch, tmp_path, gaze_rnn, 7, fcgru_bptt_path='persistent')
    first = model.engine
    assert first.bptt_persistent
    first.lose_at = 2
    model.train_long_clip(x, g, mode='truncated')
    second = model.engine
    assert second is not first and second.per_step and not second.bptt_persistent
    assert [c[:3] for c in first.calls if c[0] == 'fwd'] == [('fwd', 3, None), ('fwd', 3, 6.0)]
    assert [c[:3] for c in second.calls if c[0] == 'fwd'] == [('fwd', 3, 6.0), ('fwd', 1, 21.0)]      # the poisoned chunk again, same state
    assert len(first.steps) == 1 and [s for s, _ in second.steps] == [1, 2] and model.global_step == 3
    # exact: lost in the second pass -> everything again on the new engine, one step in all
    model = _model(monkeypatch, tmp_path, gaze_rnn, 7, fcgru_bptt_path='persistent')
    first = model.engine
    first.lose_at = 5                                                 # three forwards of pass 1, then the second backward
    model.train_long_clip(x, g, mode='exact')
    second = model.engine
    assert second is not first and not first.steps
    assert [c[0] for c in second.calls] == ['fwd'] * 3 + ['fwd', 'bwd'] * 3
    assert len(second.steps) == 1 and second.steps[0][1].tolist() == [42.0] * 4 and model.global_step == 1
    # a second loss is an error, not a loop
    model = _model(monkeypatch, tmp_path, gaze_rnn, 7, fcgru_bptt_path='persistent')
    model.engine.lose_at = 1
    orig = model._new_fcgru_engine

    def losing(*a, **kw):
        e = orig(*a, **kw)
        e.bptt_persistent, e.lose_at = True, 1
        return e
    monkeypatch.setattr(model, '_new_fcgru_engine', losing)
    with pytest.raises(_lib.RgpError):
        model.train_long_clip(x, g, mode='exact')


def test_train_long_clips_stacks_one_clip_per_lane():
    from recurrent_gaze_prediction_amd.stream import train_long_clips
    seen = {}

    class M(object):
        batch_size = 2

        def train_long_clip(self, c3d, gt, mode='truncated'):
            seen.update(x=c3d, g=gt, mode=mode)
            return 0.25
    x, g = _film(5)
    assert train_long_clips(M(), [x[0], x[1]], [g[0], g[1]], mode='exact') == 0.25
    assert seen['mode'] == 'exact' and np.array_equal(seen['x'], x) and np.array_equal(seen['g'], g)
    with pytest.raises(AssertionError):
        train_long_clips(M(), [x[0]], [g[0]])
