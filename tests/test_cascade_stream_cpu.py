"""CPU: the cascade's streaming ABI (rgp_cascade_forward_stream, rgp_cascade_state_elems) is exported, bound and validates its
arguments ahead of the plan's bound state; the float64 reference with initial states is torch_ref.cascade_forward when they
are zeros and one recurrence when both are carried; stream.GazeStream / predict_long_clips / predict_long_clip hand frames
over beside the features and reset a two-part state lane by lane (against a fake model); the refusals."""
import ctypes

import numpy as np
import pytest
import torch

import cascade_stream_ref as cr
import stream_ref as sr
from oracle import torch_ref
from recurrent_gaze_prediction_amd import _lib

P = lambda a: ctypes.c_void_p(a or None)      # noqa: E731   (never dereferenced: argument errors come first)
FRAMES, X, S_IN, S_OUT, MAPS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
RGP_EINVAL, RGP_EWORKSPACE = -1, -3     # include/rgp.h
B, T = 3, 4


def test_cascade_stream_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('rgp_cascade_forward_stream', 'rgp_cascade_state_elems'):
        assert hasattr(lib, name), 'missing export ' + name
        assert name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES['rgp_cascade_state_elems'][0] is ctypes.c_size_t
    assert len(_lib.SIGNATURES['rgp_cascade_forward_stream'][1]) == 8


@pytest.fixture(params=[0, 1], ids=['inference', 'training'])
def plan(request):
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.rgp_cascade_create_ex(ctypes.byref(h), B, T, 98, _lib.RGP_BF16, request.param) == 0
    yield lib, h
    lib.rgp_cascade_destroy(h)


def call(plan, frames=FRAMES, c3d=X, s_in=S_IN, s_out=S_OUT, n_valid=T, maps=MAPS):
    lib, h = plan
    rc = lib.rgp_cascade_forward_stream(h, P(frames), P(c3d), P(s_in), P(s_out), n_valid, P(maps), None)
    return rc, lib.rgp_last_error()


def test_state_elems_on_an_unbound_plan(plan):
    lib, h = plan
    assert lib.rgp_cascade_state_elems(h) == B * 19747 == B * (cr.BOT + cr.TOP)
    assert lib.rgp_cascade_state_elems(None) == 0


def test_argument_errors_come_before_the_bound_check(plan):
    for bad in (0, T + 1):
        rc, msg = call(plan, n_valid=bad)
        assert rc == RGP_EINVAL and b'n_valid' in msg, (bad, rc, msg)
    rc, msg = call(plan, s_in=S_IN, s_out=S_IN)
    assert rc == RGP_EINVAL and b'state_out' in msg and b'state_in' in msg, (rc, msg)
    for kw in ({'s_in': S_IN + 4}, {'s_out': S_OUT + 8}):
        rc, msg = call(plan, **kw)
        assert rc == RGP_EINVAL and b'aligned' in msg and b'state_in' in msg and b'state_out' in msg, (kw, rc, msg)
    for kw, name in (({'frames': 0}, b'frame_images'), ({'c3d': 0}, b'c3d_input'), ({'maps': 0}, b'gazemaps')):
        rc, msg = call(plan, **kw)
        assert rc == RGP_EINVAL and name in msg, (kw, rc, msg)
    # every argument in range, the optional ones NULL or not: what is left is the unbound plan
    for kw in ({}, {'s_in': 0}, {'s_out': 0}, {'s_in': 0, 's_out': 0}, {'n_valid': 1}):
        rc, msg = call(plan, **kw)
        assert rc == RGP_EWORKSPACE and b'workspace' in msg, (kw, rc, msg)


# ---------------------------------------------------------------------------------------------- the float64 reference
def test_reference_with_zero_states_is_the_oracle_and_carrying_both_is_one_recurrence():
    p, frames, c3d, maps, hs, gs = cr.stream_reference(301)
    tp = cr.to_t(p)
    f, x = torch.tensor(frames, dtype=torch.float64), torch.tensor(c3d, dtype=torch.float64)
    with torch.no_grad():
        want, mid = torch_ref.cascade_forward(f, x, tp, want_all=True)
        assert np.array_equal(maps, want.numpy())                                   # exactly: the same operations in the same order
        assert np.array_equal(hs, mid['bottom'].numpy()) and np.array_equal(gs, mid['top'].numpy())
        # cut behind step 3, both states carried: the same recurrence (the per-frame stages are batched over other row counts)
        m2, h2, g2 = cr.cascade_forward_from(f[:, 3:], x[:, 3:], tp, torch.tensor(hs[:, 2]), torch.tensor(gs[:, 2]))
        assert cr.rel_err(m2.numpy(), maps[:, 3:]) < 1e-12 and cr.rel_err(g2.numpy(), gs[:, 3:]) < 1e-12
        # ... and either half dropped is far off at the first step behind the cut (the issue's table: 0.39-0.41 / 0.32-0.36)
        scale = np.abs(maps).max()
        for h0, g0 in ((torch.tensor(hs[:, 2]), None), (None, torch.tensor(gs[:, 2]))):
            m3 = cr.cascade_forward_from(f[:, 3:4], x[:, 3:4], tp, h0, g0)[0]
            assert np.abs(m3.numpy()[:, 0] - maps[:, 3]).max() / scale > 0.2


# ---------------------------------------------------------------------------------------------- GazeStream, host only
def test_reset_zeroes_the_lanes_of_every_part_of_a_two_part_state():
    from recurrent_gaze_prediction_amd.stream import GazeStream
    model = cr.FakeFramesModel(3, 4)
    st = GazeStream(model)
    held = torch.arange(1, 25, dtype=torch.float64)                        # [3 lanes x 3 | 3 lanes x 5]
    st.state, st.position = held, 4
    before = held.clone()
    st.reset([0, 2])
    assert torch.equal(held, before) and st.state is not held and st.position == 4
    want = before.clone()
    want[0:3] = 0; want[6:9] = 0                                           # lanes 0 and 2 of part 0 (3 each)
    want[9:14] = 0; want[19:24] = 0                                        # lanes 0 and 2 of part 1 (5 each)
    assert torch.equal(st.state, want)
    assert torch.equal(st.state[3:6], before[3:6]) and torch.equal(st.state[14:19], before[14:19])     # lane 1 untouched
    # a model that only has STATE_PARTS behaves as before
    m1 = sr.FakeStreamModel(2, 4)
    s1 = GazeStream(m1)
    s1.state = torch.tensor([5.0, 7.0], dtype=torch.float64)
    s1.reset([1])
    assert s1.state.tolist() == [5.0, 0.0]


def test_push_features_pads_the_frames_beside_the_features():
    from recurrent_gaze_prediction_amd.stream import GazeStream
    model = cr.FakeFramesModel(2, 4)
    st = GazeStream(model)
    x = np.stack([sr.fake_clip(1, 3), sr.fake_clip(2, 3)])
    f = np.stack([cr.fake_frames(1, 3), cr.fake_frames(2, 3)])
    maps = st.push_features(x, frames=f)
    n_valid, pos, state, got = model.stream_calls[-1]
    assert (n_valid, pos, state) == (3, 0, None) and got.shape == (2, 4, 2, 2, 3)
    assert np.array_equal(got[:, :3], f) and not got[:, 3:].any()
    want = np.cumsum(x[:, :, 0, 0, 0].astype(np.float64) + f[:, :, 0, 0, 0], 1)
    assert tuple(maps.shape) == (2, 3, 2, 2) and np.array_equal(maps[:, :, 0, 0].numpy(), want)
    with pytest.raises(ValueError):
        st.push_features(x)                                                # this model needs them: nothing is made up
    with pytest.raises(AssertionError):
        st.push_features(x, frames=f[:, :2])                               # frames of other steps than the features


LENGTHS = (5, 9, 2)


def test_predict_long_clips_hands_the_right_frame_slices_over():
    from recurrent_gaze_prediction_amd.stream import predict_long_clips
    model = cr.FakeFramesModel(2, 4)
    clips = [sr.fake_clip(10 + i, n) for i, n in enumerate(LENGTHS)]
    frames = [cr.fake_frames(20 + i, n) for i, n in enumerate(LENGTHS)]
    maps = predict_long_clips(model, clips, frames=frames)
    assert [m.shape for m in maps] == [(n, 2, 2) for n in LENGTHS]
    for c, f, m in zip(clips, frames, maps):
        want = np.cumsum(c[:, 0, 0, 0].astype(np.float64) + f[:, 0, 0, 0])
        assert np.array_equal(m[:, 0, 0], want), (m[:, 0, 0], want)
    # call 0: steps 0..3 of clips 0, 1; call 1: clip 0's last step (padded) and clip 1's steps 4..7; call 2: clip 2 in lane 0
    # (reset) and clip 1's last step in lane 1
    got = [c[3] for c in model.stream_calls]
    assert len(got) == 3
    assert np.array_equal(got[0][0], frames[0][:4]) and np.array_equal(got[0][1], frames[1][:4])
    assert np.array_equal(got[1][0, :1], frames[0][4:]) and not got[1][0, 1:].any() and np.array_equal(got[1][1], frames[1][4:8])
    assert np.array_equal(got[2][0, :2], frames[2]) and not got[2][0, 2:].any()
    assert np.array_equal(got[2][1, :1], frames[1][8:]) and not got[2][1, 1:].any()
    s2 = model.stream_calls[2][2]
    assert not s2[0:3].any() and not s2[6:11].any() and s2[3] != 0 and s2[11] != 0      # lane 0 reset in both parts, lane 1 carried
    with pytest.raises(ValueError):
        predict_long_clips(model, clips)                                   # required by a model that needs them
    # ... and with None nothing is passed to a model that takes none (its predict_stream has no such argument)
    plain = sr.FakeStreamModel(2, 4)
    assert [m.shape for m in predict_long_clips(plain, clips)] == [(n, 2, 2) for n in LENGTHS]


def test_predict_long_clip_carry_state_passes_frames_through():
    from recurrent_gaze_prediction_amd.models.evaluate_gaze import predict_long_clip
    model = cr.FakeFramesModel(2, 4)
    clip, frames = sr.fake_clip(5, 9), cr.fake_frames(6, 9)
    maps = predict_long_clip(model, clip, frames=frames, carry_state=True)
    want = np.cumsum(clip[:, 0, 0, 0].astype(np.float64) + frames[:, 0, 0, 0])
    assert maps.shape == (9, 2, 2) and np.array_equal(maps[:, 0, 0], want)
    assert len(model.stream_calls) == 3
    assert np.array_equal(np.concatenate([c[3][0] for c in model.stream_calls])[:9], frames)


# ---------------------------------------------------------------------------------------------- refusals
def test_the_cascade_streams_and_refuses_without_frames():
    from recurrent_gaze_prediction_amd.models.gaze_grcn_cascade import GazePredictionGRCN as Cascade
    assert Cascade.STREAMS and Cascade.STATE_LANE_ELEMS == (49 * 256, 2401 * 3)
    m = Cascade.__new__(Cascade)                                           # no engine: the refusal needs none
    with pytest.raises(ValueError) as e:
        m.predict_stream(None)
    assert 'frame' in str(e.value)


def test_models_without_a_carried_state_still_refuse_and_name_the_cascade():
    from recurrent_gaze_prediction_amd.models.gaze_rnn import GazePredictionGRU
    from recurrent_gaze_prediction_amd.models.gaze_c3d_conv import GazePredictionConv
    for cls in (GazePredictionGRU, GazePredictionConv):
        m = cls.__new__(cls)
        with pytest.raises(NotImplementedError) as e:
            m.predict_stream(None)
        assert all(n in str(e.value) for n in ('GazePredictionGRCN', 'GazePredictionGRCN77', 'GazePredictionLSTM', 'gaze_grcn_cascade'))


# ---------------------------------------------------------------------------------------------- frames and the other models
def test_models_that_take_no_frames_are_handed_none():
    """sr.FakeStreamModel's predict_stream has no `frames` argument, like the three single-level models': frames of any kind
    are accepted and dropped -- by predict_long_clips, push_features and predict_long_clip on both branches."""
    from recurrent_gaze_prediction_amd.models.evaluate_gaze import predict_long_clip
    from recurrent_gaze_prediction_amd.stream import GazeStream, predict_long_clips
    clips = [sr.fake_clip(10 + i, n) for i, n in enumerate(LENGTHS)]
    want = predict_long_clips(sr.FakeStreamModel(2, 4), clips)
    model = sr.FakeStreamModel(2, 4)
    frames = [cr.fake_frames(20 + i, n) for i, n in enumerate(LENGTHS)]
    got = predict_long_clips(model, clips, frames=frames)
    assert all(np.array_equal(a, b) for a, b in zip(got, want)) and len(model.stream_calls) == 3
    batch = np.zeros((2, 4, 2, 2, 3), np.float32)                          # the chunked branch's [B,T,hw,hw,3]: not parallel to clips
    got = predict_long_clips(model, clips, frames=[batch] * 3)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    clip = sr.fake_clip(5, 9)
    carried = predict_long_clip(sr.FakeStreamModel(2, 4), clip, carry_state=True)
    for f in (cr.fake_frames(6, 9), batch):
        assert np.array_equal(predict_long_clip(model, clip, frames=f, carry_state=True), carried)
        assert np.array_equal(predict_long_clip(model, clip, frames=f), predict_long_clip(model, clip))
    st = GazeStream(model)
    x = np.stack([sr.fake_clip(1, 3), sr.fake_clip(2, 3)])
    m = st.push_features(x, frames=np.zeros((2, 3, 2, 2, 3), np.float32))
    assert np.array_equal(m.numpy(), GazeStream(sr.FakeStreamModel(2, 4)).push_features(x).numpy())


def test_frames_of_the_wrong_shape_are_named():
    from recurrent_gaze_prediction_amd.models.evaluate_gaze import predict_long_clip
    from recurrent_gaze_prediction_amd.stream import predict_long_clips
    model = cr.FakeFramesModel(2, 4)
    clips = [sr.fake_clip(10 + i, n) for i, n in enumerate(LENGTHS)]
    frames = [cr.fake_frames(20 + i, n) for i, n in enumerate(LENGTHS)]
    with pytest.raises(AssertionError, match='parallel to clips'):
        predict_long_clips(model, clips, frames=frames[:2])
    with pytest.raises(AssertionError, match='parallel to clips'):
        predict_long_clips(model, clips, frames=[frames[0], frames[1][:8], frames[2]])
    with pytest.raises(AssertionError, match='share one'):
        predict_long_clips(model, clips, frames=[frames[0], cr.fake_frames(21, 9, hw=3), frames[2]])
    empty = [np.zeros((0, 1024, 7, 7), np.float32)]
    assert predict_long_clips(model, empty, frames=[np.zeros((0, 2, 2, 3), np.float32)])[0].shape == (0, 2, 2)
    assert model.stream_calls == []
    # predict_long_clip: [B,T,hw,hw,3] is the chunked branch's array, [N,hw,hw,3] the carried one's
    clip = sr.fake_clip(5, 9)
    with pytest.raises(ValueError, match='carry_state'):
        predict_long_clip(model, clip, frames=np.zeros((2, 4, 2, 2, 3), np.float32), carry_state=True)
    with pytest.raises(ValueError, match='carry_state'):
        predict_long_clip(model, clip, frames=cr.fake_frames(6, 8), carry_state=True)
