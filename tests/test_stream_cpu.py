"""CPU: the streaming ABI (rgp_*_forward_stream, rgp_*_state_elems) is exported, bound and validates its arguments ahead of
the plan's bound state; stream.GazeStream / predict_long_clips hand lanes over, reset, pad and trim as documented (against a
fake model whose maps are running sums); predict_long_clip(carry_state=False) makes the calls it made before."""
import ctypes

import numpy as np
import pytest
import torch

import stream_ref as sr
from recurrent_gaze_prediction_amd import _lib

FAMILY_ABI = {      # family -> (prefix, create args behind the plan pointer for B=3, T=4, takes bn_phase)
    'grcn': ('rgp_grcn_', (3, 4, 512, 128, _lib.RGP_BF16, 0), True),
    'grcn77': ('rgp_grcn77_', (3, 4, _lib.RGP_BF16, 0), False),
    'lstm': ('rgp_lstm_', (3, 4, _lib.RGP_BF16, 0), False),
}
P = lambda a: ctypes.c_void_p(a)      # noqa: E731   (never dereferenced: argument errors come first)
X, ROWS, S_IN, S_OUT, LOGITS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
RGP_EINVAL, RGP_EWORKSPACE = -1, -3     # include/rgp.h


def test_stream_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for prefix, _, _ in FAMILY_ABI.values():
        for name in (prefix + 'forward_stream', prefix + 'state_elems'):
            assert hasattr(lib, name), 'missing export ' + name
            assert name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES['rgp_grcn_state_elems'][0] is ctypes.c_size_t
    # bn_phase: gaze_grcn only
    assert len(_lib.SIGNATURES['rgp_grcn_forward_stream'][1]) == 10
    assert len(_lib.SIGNATURES['rgp_lstm_forward_stream'][1]) == len(_lib.SIGNATURES['rgp_grcn77_forward_stream'][1]) == 9


@pytest.fixture(params=sr.FAMILIES)
def plan(request):
    lib = _lib.load()
    prefix, args, has_phase = FAMILY_ABI[request.param]
    h = ctypes.c_void_p()
    assert getattr(lib, prefix + 'create')(ctypes.byref(h), *args) == 0
    yield request.param, lib, prefix, h, has_phase
    getattr(lib, prefix + 'destroy')(h)


def test_state_elems_on_unbound_plans(plan):
    family, lib, prefix, h, _ = plan
    want = 3 * 49 * 128 * (2 if family == 'lstm' else 1)
    assert getattr(lib, prefix + 'state_elems')(h) == want
    assert getattr(lib, prefix + 'state_elems')(None) == 0


def call(plan, c3d=X, rows=0, s_in=S_IN, s_out=S_OUT, n_valid=4, bn_phase=0, logits=LOGITS):
    _, lib, prefix, h, has_phase = plan
    phase = (bn_phase,) if has_phase else ()
    f = getattr(lib, prefix + 'forward_stream')
    rc = f(h, P(c3d or None), P(rows or None), P(s_in or None), P(s_out or None), n_valid, *(phase + (P(logits), None, None)))
    return rc, lib.rgp_last_error()


def test_argument_errors_come_before_the_bound_check(plan):
    T = 4
    for bad in (0, T + 1, -3):
        rc, msg = call(plan, n_valid=bad)
        assert rc == RGP_EINVAL and b'n_valid' in msg, (bad, rc, msg)
    rc, msg = call(plan, c3d=X, rows=ROWS)
    assert rc == RGP_EINVAL and b'c3d_input' in msg and b'c3d_rows' in msg
    rc, msg = call(plan, c3d=0, rows=0)
    assert rc == RGP_EINVAL and b'c3d_input' in msg and b'c3d_rows' in msg
    rc, msg = call(plan, s_in=S_IN, s_out=S_IN)
    assert rc == RGP_EINVAL and b'state_out' in msg and b'state_in' in msg
    if plan[4]:
        for bad in (-1, T):
            rc, msg = call(plan, bn_phase=bad)
            assert rc == RGP_EINVAL and b'bn_phase' in msg, (bad, rc, msg)
    # every argument in range: what is left is the unbound plan (RGP_EWORKSPACE), for either input form and the optional ones NULL
    for kw in ({}, {'c3d': 0, 'rows': ROWS}, {'s_in': 0}, {'s_out': 0}, {'n_valid': 1}, {'bn_phase': T - 1 if plan[4] else 0}):
        rc, msg = call(plan, **kw)
        assert rc == RGP_EWORKSPACE and b'workspace' in msg, (kw, rc, msg)


def test_flag_8_of_grcn_create_is_still_unknown():
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.rgp_grcn_create(ctypes.byref(h), 2, 2, 512, 128, _lib.RGP_BF16, 8) == RGP_EINVAL      # streaming is a call, not a flag


# ---------------------------------------------------------------------------------------------- GazeStream, host only
LENGTHS = (5, 9, 2, 4)


def test_predict_long_clips_hands_lanes_over():
    from recurrent_gaze_prediction_amd.stream import predict_long_clips
    model = sr.FakeStreamModel(2, 4)
    clips = [sr.fake_clip(10 + i, n) for i, n in enumerate(LENGTHS)]
    maps = predict_long_clips(model, clips)
    assert [m.shape for m in maps] == [(n, 2, 2) for n in LENGTHS]
    for c, m in zip(clips, maps):
        want = np.cumsum(c[:, 0, 0, 0].astype(np.float64))
        assert np.array_equal(m, np.broadcast_to(want[:, None, None], m.shape)), (m[:, 0, 0], want)
    # lanes: call 0 = clips 0, 1; call 1 = their second chunks; call 2 = clip 2 in lane 0 (reset), clip 1's last step in lane 1;
    # call 3 = clip 3 in lane 0 (reset again), lane 1 idle.  Whole calls only, so every clip starts at position % T == 0.
    assert [(n, pos) for n, pos, _ in model.stream_calls] == [(4, 0), (4, 4), (4, 8), (4, 12)]
    assert model.stream_calls[0][2] is None
    s2, s3 = model.stream_calls[2][2], model.stream_calls[3][2]
    assert s2[0] == 0 and s2[1] == clips[1][:8, 0, 0, 0].sum()          # lane 0 reset for clip 2, lane 1 carried
    assert s3[0] == 0                                                     # lane 0 reset for clip 3
    assert predict_long_clips(model, []) == []
    assert predict_long_clips(model, [np.zeros((0, 1024, 7, 7), np.float32)])[0].shape == (0, 2, 2)


def test_gaze_stream_pushes_resets_and_never_touches_old_states():
    from recurrent_gaze_prediction_amd.stream import GazeStream
    model = sr.FakeStreamModel(2, 4)
    st = GazeStream(model)
    a, b = sr.fake_clip(1, 7), sr.fake_clip(2, 7)
    x = np.stack([a, b])                                                   # [2, 7, ...]
    m0 = st.push_features(x[:, :3])                                        # 3 <= T steps: padded to T, n_valid = 3
    assert tuple(m0.shape) == (2, 3, 2, 2) and st.position == 3 and model.stream_calls[-1][:2] == (3, 0)
    m1 = st.push_features(x[:, 3:7], n_valid=2)                            # 4 pushed, the state advances by 2
    assert tuple(m1.shape) == (2, 4, 2, 2) and st.position == 5 and model.stream_calls[-1][:2] == (2, 3)
    want = np.cumsum(x[:, :, 0, 0, 0].astype(np.float64), 1)
    assert np.array_equal(m0[:, :, 0, 0].numpy(), want[:, :3]) and np.array_equal(m1[:, :2, 0, 0].numpy(), want[:, 3:5])
    assert np.array_equal(st.state.numpy(), want[:, 4])
    held = st.state
    before = held.clone()
    st.reset([1])
    assert torch.equal(held, before) and st.state is not held             # a fresh tensor: the old state is as it was
    assert st.state[0] == want[0, 4] and st.state[1] == 0 and st.position == 5
    st.reset()
    assert st.state is None and st.position == 0
    with pytest.raises(AssertionError):
        st.push_features(np.zeros((2, 5, 1024, 7, 7), np.float32))        # more than T steps in one call


def test_models_without_a_carried_state_refuse():
    from recurrent_gaze_prediction_amd.models.gaze_grcn import GazePredictionGRCN
    from recurrent_gaze_prediction_amd.models.gaze_grcn77 import GazePredictionGRCN77
    from recurrent_gaze_prediction_amd.models.gaze_lstm import GazePredictionLSTM
    from recurrent_gaze_prediction_amd.models.gaze_rnn import GazePredictionGRU
    from recurrent_gaze_prediction_amd.models.gaze_c3d_conv import GazePredictionConv
    assert GazePredictionGRCN.STREAMS and GazePredictionGRCN77.STREAMS and GazePredictionLSTM.STREAMS
    assert GazePredictionLSTM.STATE_PARTS == 2 and GazePredictionGRCN.STATE_PARTS == 1
    for cls in (GazePredictionGRU, GazePredictionConv):
        m = cls.__new__(cls)                                               # no engine: the refusal needs none
        with pytest.raises(NotImplementedError) as e:
            m.predict_stream(None)
        assert all(n in str(e.value) for n in ('GazePredictionGRCN', 'GazePredictionGRCN77', 'GazePredictionLSTM'))


def test_predict_long_clip_default_makes_todays_calls():
    from recurrent_gaze_prediction_amd.models.evaluate_gaze import predict_long_clip
    model = sr.FakeStreamModel(2, 4)
    clip = sr.fake_clip(5, 9)                                              # 3 chunks of 4: one call of 2 chunks, one of 1 + a zero chunk
    maps = predict_long_clip(model, clip)
    assert model.stream_calls == [] and len(model.predict_calls) == 2
    padded = np.zeros((4, 4, 1024, 7, 7), np.float32)
    padded.reshape(16, 1024, 7, 7)[:9] = clip
    assert np.array_equal(model.predict_calls[0], padded[:2]) and np.array_equal(model.predict_calls[1], padded[2:])
    v = clip[:, 0, 0, 0].astype(np.float64)
    want = np.concatenate([np.cumsum(v[:4]), np.cumsum(v[4:8]), np.cumsum(v[8:])])       # the state is forgotten at every chunk
    assert maps.shape == (9, 2, 2) and np.array_equal(maps[:, 0, 0], want)
    # carry_state=True: one recurrence, through predict_stream only
    model = sr.FakeStreamModel(2, 4)
    carried = predict_long_clip(model, clip, carry_state=True)
    assert model.predict_calls == [] and len(model.stream_calls) == 3
    assert np.array_equal(carried[:, 0, 0], np.cumsum(v)) and np.array_equal(carried[:4], maps[:4])
