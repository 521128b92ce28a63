"""CPU: what fc-GRU streaming (rgp_fcgru_forward_stream, FcGruEngine.forward_stream, gaze_rnn / gaze_rnn77 predict_stream) can
show without a device.

1. The ABI: both symbols are exported and bound, rgp_fcgru_state_elems works on an unbound plan, and every argument error of
   rgp_fcgru_forward_stream is RGP_EINVAL, names its argument and comes ahead of the unbound plan's RGP_EWORKSPACE.
2. stream.GazeStream / predict_long_clips against a fake fc-GRU-shaped model (one [B, 1617] state part): lane hand-over and
   reset; the refusals that stay; STREAMS on an instance built through a stand-in engine.
3. predict_stream's recovery from RGP_ETIMEOUT on a stand-in engine: rebuilt per step, the call repeated with the same,
   untouched state.  Nothing is provoked on a device.
4. The float64 reference with an h_0 agrees with the oracle from zeros, composes across cuts, and SEES the state: dropping it
   at a cut moves the logits of each of the next four steps by at least 10 x the bf16 logits bound, on the GPU tests' own
   weights and inputs.
"""
import ctypes

import numpy as np
import pytest
import torch

import fcgru_stream_ref as sr
from recurrent_gaze_prediction_amd import _lib

RGP_EINVAL, RGP_EWORKSPACE = -1, -3     # include/rgp.h
P = lambda a: ctypes.c_void_p(a)      # noqa: E731   (never dereferenced: argument errors come first)
X, S_IN, S_OUT, LOGITS = 0x10000, 0x30000, 0x40000, 0x50000
B, T = 3, 4


# ------------------------------------------------------------------------------------------------ 1. ABI
def test_stream_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('rgp_fcgru_forward_stream', 'rgp_fcgru_state_elems'):
        assert hasattr(lib, name), 'missing export ' + name
        assert name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES['rgp_fcgru_state_elems'][0] is ctypes.c_size_t
    assert len(_lib.SIGNATURES['rgp_fcgru_forward_stream'][1]) == 8          # no rows entry, no bn_phase


@pytest.fixture(params=[0, _lib.RGP_FCGRU_SAVE_FOR_BACKWARD, _lib.RGP_FCGRU_PER_STEP | _lib.RGP_FCGRU_SAVE_FOR_BACKWARD],
                ids=['inference', 'training', 'training-per_step'])
def plan(request):
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.rgp_fcgru_create_flags(ctypes.byref(h), B, T, 7, 7, _lib.RGP_BF16, request.param) == 0
    yield lib, h
    lib.rgp_fcgru_destroy(h)


def test_state_elems_on_unbound_plans(plan):
    lib, h = plan
    assert lib.rgp_fcgru_state_elems(h) == B * 1617
    assert lib.rgp_fcgru_state_elems(None) == 0


def call(plan, c3d=X, s_in=S_IN, s_out=S_OUT, n_valid=T, logits=LOGITS):
    lib, h = plan
    rc = lib.rgp_fcgru_forward_stream(h, P(c3d or None), P(s_in or None), P(s_out or None), n_valid, P(logits or None), None, None)
    return rc, lib.rgp_last_error()


def test_argument_errors_come_before_the_bound_check(plan):
    for bad in (0, T + 1, -3):
        rc, msg = call(plan, n_valid=bad)
        assert rc == RGP_EINVAL and b'n_valid' in msg, (bad, rc, msg)
    rc, msg = call(plan, s_in=S_IN, s_out=S_IN)
    assert rc == RGP_EINVAL and b'state_out' in msg and b'state_in' in msg, (rc, msg)
    rc, msg = call(plan, c3d=0)
    assert rc == RGP_EINVAL and b'c3d_input' in msg, (rc, msg)
    rc, msg = call(plan, logits=0)
    assert rc == RGP_EINVAL and b'logits' in msg, (rc, msg)
    lib = plan[0]
    assert lib.rgp_fcgru_forward_stream(None, P(X), None, None, T, P(LOGITS), None, None) == RGP_EINVAL
    # every argument in range: what is left is the unbound plan, the optional arguments NULL or not
    for kw in ({}, {'s_in': 0}, {'s_out': 0}, {'s_in': 0, 's_out': 0}, {'n_valid': 1}):
        rc, msg = call(plan, **kw)
        assert rc == RGP_EWORKSPACE and b'workspace' in msg, (kw, rc, msg)


# ------------------------------------------------------------------------------------------------ 2. stream plumbing
LENGTHS = (5, 9, 2, 4)


def test_predict_long_clips_hands_lanes_over_with_one_state_part():
    from recurrent_gaze_prediction_amd.stream import predict_long_clips
    model = sr.FakeFcGruModel(2, 4)
    clips = [sr.fake_clip(20 + i, n) for i, n in enumerate(LENGTHS)]
    maps = predict_long_clips(model, clips)
    assert [m.shape for m in maps] == [(n, 7, 7) for n in LENGTHS]
    for c, m in zip(clips, maps):
        want = np.cumsum(c[:, 0, 0, 0].astype(np.float64))
        assert np.array_equal(m, np.broadcast_to(want[:, None, None], m.shape)), (m[:, 0, 0], want)
    assert [(n, pos) for n, pos, _ in model.stream_calls] == [(4, 0), (4, 4), (4, 8), (4, 12)]
    assert model.stream_calls[0][2] is None
    s2, s3 = (model.stream_calls[i][2].view(2, sr.N) for i in (2, 3))
    assert not s2[0].any() and s2[1, 0] == clips[1][:8, 0, 0, 0].sum() and (s2[1, 1:] == 2).all()      # lane 0 reset: the whole row
    assert not s3[0].any()


def test_gaze_stream_resets_one_lane_of_the_1617_wide_state():
    from recurrent_gaze_prediction_amd.stream import GazeStream
    model = sr.FakeFcGruModel(2, 4)
    st = GazeStream(model)
    x = np.stack([sr.fake_clip(1, 7), sr.fake_clip(2, 7)])
    m0 = st.push_features(x[:, :3])
    assert tuple(m0.shape) == (2, 3, 7, 7) and st.position == 3 and model.stream_calls[-1][:2] == (3, 0)
    m1 = st.push_features(x[:, 3:7], n_valid=2)
    assert st.position == 5 and model.stream_calls[-1][:2] == (2, 3)
    want = np.cumsum(x[:, :, 0, 0, 0].astype(np.float64), 1)
    assert np.array_equal(m0[:, :, 0, 0].numpy(), want[:, :3]) and np.array_equal(m1[:, :2, 0, 0].numpy(), want[:, 3:5])
    held, before = st.state, st.state.clone()
    assert held.numel() == 2 * sr.N
    st.reset([1])
    assert torch.equal(held, before) and st.state is not held
    now = st.state.view(2, sr.N)
    assert now[0, 0] == want[0, 4] and (now[0, 1:] == 1).all() and not now[1].any()
    # push_windows falls back to the features: the engine has no forward_rows
    feats = torch.as_tensor(np.stack([sr.fake_clip(3, 4), sr.fake_clip(4, 4)]))
    c3d = type('C', (), {'forward': lambda self, video, want_features=True: (feats.reshape(8, 1024, 7, 7),)})()
    st2 = GazeStream(model, c3d_engine=c3d)
    m = st2.push_windows(torch.zeros(8, 1))
    assert np.array_equal(m[:, :, 0, 0].numpy(), np.cumsum(feats[:, :, 0, 0, 0].double().numpy(), 1))


class _Dropout(object):
    keep_prob, seed, draws = 1.0, 0, 0

    def configure(self, keep_prob, seed=0):
        self.keep_prob, self.seed, self.draws = float(keep_prob), int(seed), 0

    def off(self):
        pass


class _StandInEngine(object):
    """What GazePredictionGRU touches of FcGruEngine, forward_stream included.  A persistent instance reports RGP_ETIMEOUT once
    and returns NaN until then.  The 'recurrence': new_state = state + sum of the valid steps' feature [.., 0, 0, 0]."""
    made = []
    STREAM_BN_PHASE = False

    def __init__(self, batch, n_steps, gazemap_hw=(49, 49), dtype='f32', device='cpu', save_for_backward=False, per_step=False,
                 persistent=False):
        self.B, self.T, self.GH, self.GW = batch, n_steps, gazemap_hw[0], gazemap_hw[1]
        self.dtype, self.device, self.save_for_backward, self.per_step = dtype, device, save_for_backward, per_step
        self.persistent = bool(persistent)
        self.lost = self.persistent
        self.weights = None
        self.adam_m = self.adam_v = None
        self.dropout = _Dropout()
        self.stream_calls = []
        _StandInEngine.made.append(self)

    def set_weights(self, params):
        self.weights = {k: torch.as_tensor(np.asarray(v)).clone() for k, v in params.items()}

    def status(self):
        if self.lost:
            self.lost = False
            e = _lib.RgpError('lost member')
            e.code = _lib.RGP_ETIMEOUT
            raise e

    @property
    def state_elems(self):
        return self.B * 1617

    def forward_stream(self, x, state=None, n_valid=None, want_probs=True):
        n_valid = self.T if n_valid is None else n_valid
        self.stream_calls.append((state, None if state is None else state.clone(), n_valid))
        s0 = torch.zeros(self.B, 1617) if state is None else state.view(self.B, 1617)
        run = s0[:, :1] + torch.cumsum(x[:, :, 0, 0, 0], 1)                       # [B, T]
        z = run[:, :, None, None].expand(self.B, self.T, self.GH, self.GW).clone()
        new_state = run[:, n_valid - 1:n_valid].expand(self.B, 1617).clone().reshape(-1)
        if self.lost:
            z, new_state = z * float('nan'), new_state * float('nan')
        return z, torch.softmax(z.reshape(self.B, self.T, -1), -1).reshape(z.shape), new_state


def _model(monkeypatch, tmp_path, module, path, hw=None):
    from recurrent_gaze_prediction_amd import engine
    from recurrent_gaze_prediction_amd.models.base import Session
    monkeypatch.setattr(engine, 'FcGruEngine', _StandInEngine)
    _StandInEngine.made = []
    cfg = module.GRUModelConfig()
    cfg.batch_size, cfg.n_lstm_steps, cfg.train_dir, cfg.fcgru_path, cfg.loss_type = 2, 3, str(tmp_path), path, 'l2'
    kw = {} if hw is None else {'gazemap_height': hw, 'gazemap_width': hw}
    return module.GazePredictionGRU(Session('cpu'), None, cfg, **kw), cfg


def test_streams_is_set_where_the_engine_is_built_and_the_refusals_stay(monkeypatch, tmp_path):
    from recurrent_gaze_prediction_amd.models import gaze_rnn, gaze_rnn77
    from recurrent_gaze_prediction_amd.models.gaze_c3d_conv import GazePredictionConv
    assert gaze_rnn.GazePredictionGRU.STREAMS is False and gaze_rnn77.GazePredictionGRU.STREAMS is False
    assert GazePredictionConv.STREAMS is False and gaze_rnn.GazePredictionGRU.STATE_PARTS == 1
    for cls in (gaze_rnn.GazePredictionGRU, gaze_rnn77.GazePredictionGRU, GazePredictionConv):
        m = cls.__new__(cls)                                               # no engine: nothing to stream with
        with pytest.raises(NotImplementedError) as e:
            m.predict_stream(None)
        assert all(n in str(e.value) for n in ('GazePredictionGRCN', 'GazePredictionGRCN77', 'GazePredictionLSTM', 'gaze_grcn_cascade',
                                               'gaze_rnn', 'gaze_rnn77'))
    for module, hw in ((gaze_rnn, 7), (gaze_rnn77, None)):
        model, _ = _model(monkeypatch, tmp_path, module, 'per_step', hw)
        assert model.STREAMS is True and type(model).STREAMS is False
        x = np.zeros((2, 3, 1024, 7, 7), np.float32)
        x[:, :, 0, 0, 0] = [[1, 2, 3], [4, 5, 6]]
        maps, state = model.predict_stream(x, n_valid=2)
        assert state.numel() == 2 * 1617 and state.view(2, 1617)[:, 0].tolist() == [3.0, 9.0]
        maps2, state2 = model.predict_stream(x, state=state)
        assert maps2[:, :, 0, 0].tolist() == [[4.0, 6.0, 9.0], [13.0, 18.0, 24.0]]


# ------------------------------------------------------------------------------------------------ 3. time-out recovery
def test_predict_stream_recovers_from_a_timeout_with_the_same_untouched_state(monkeypatch, tmp_path):
    from recurrent_gaze_prediction_amd.models import gaze_rnn, gaze_rnn77
    for module, hw in ((gaze_rnn, 7), (gaze_rnn77, None)):
        model, cfg = _model(monkeypatch, tmp_path, module, 'persistent', hw)
        first = model.engine
        assert first.persistent and not first.per_step and model.STREAMS is True
        state = torch.arange(2 * 1617, dtype=torch.float32)
        before = state.clone()
        x = np.zeros((2, 3, 1024, 7, 7), np.float32)
        x[:, :, 0, 0, 0] = [[1, 2, 3], [4, 5, 6]]
        maps, new_state = model.predict_stream(x, state=state, n_valid=3)
        assert model.engine is not first and model.engine.per_step and not model.engine.persistent and cfg.fcgru_path == 'per_step'
        assert model.STREAMS is True                                     # rebuilt through the same place
        assert len(_StandInEngine.made) == 2 and len(first.stream_calls) == 1 and len(model.engine.stream_calls) == 1
        for eng in (first, model.engine):                               # the same tensor, as it was, to both engines
            got, copy, n_valid = eng.stream_calls[0]
            assert got is state and torch.equal(copy, before) and n_valid == 3
        assert torch.equal(state, before)
        assert torch.isfinite(maps).all() and torch.isfinite(new_state).all()
        assert new_state.view(2, 1617)[:, 0].tolist() == [0.0 + 6.0, 1617.0 + 15.0]
        assert all(torch.equal(model.engine.weights[k], first.weights[k]) for k in first.weights)
        # a per-step engine is never asked for its status
        model.engine.lost = True
        model.predict_stream(x, state=new_state)
        assert model.engine.lost and len(_StandInEngine.made) == 2


# ------------------------------------------------------------------------------------------------ 4. the reference sees the state
@pytest.mark.parametrize('gh', [7, 49])
def test_the_f64_reference_composes_across_cuts_and_sees_a_dropped_state(gh):
    from oracle import torch_ref
    p, x = sr.params(gh), sr.features(2, 7)
    z, h = sr.forward_f64(x, p)
    pt = {k: torch.tensor(v, dtype=torch.float64) for k, v in p.items()}
    want = torch_ref.fcgru_forward(torch.tensor(x, dtype=torch.float64), pt, gh, gh).numpy().reshape(z.shape)
    assert sr.rel_err(z, want) < 1e-12
    # cut at the long-plan test's cuts, the state handed over: the same recurrence
    pos, state, parts = 0, None, []
    for n in sr.LONG_CUTS:
        zc, hc = sr.forward_f64(x[:, pos:pos + n], p, h0=state)
        parts.append(zc)
        state, pos = hc[-1], pos + n
    assert sr.rel_err(np.concatenate(parts, 1), z) < 1e-12 and np.abs(state - h[-1]).max() < 1e-12
    # the state dropped at the first cut: each of the four steps behind it misses by at least 10 x the bf16 logits bound
    zd, _ = sr.forward_f64(x, p, drop_state_at=(sr.LONG_CUTS[0],))
    miss = sr.per_step_miss(zd, z)
    print('gh=%d: a state dropped at step %d moves the logits per step by %s of max |logit|' % (gh, sr.LONG_CUTS[0], miss))
    assert not miss[:3].any()
    assert (miss[3:] >= sr.MARGIN * sr.TOL['bf16']).all(), miss
    # the gates work: neither saturated nor idle
    assert 0.3 < np.abs(h).max() < 1.0
