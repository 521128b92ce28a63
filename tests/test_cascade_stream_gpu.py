"""GPU: streaming inference of the two-level cascade (rgp_cascade_forward_stream, CascadeEngine.forward_stream, the model's
predict_stream, stream.GazeStream / predict_long_clips / predict_video): both recurrent states carried across calls.

Measured on an MI355X (max-abs error over the reference's max-abs, seven steps from calls of 3, 3, 1, seeds 301 / 411; the
same figures for inference and training plans -- their kernels are the same):
  f32   maps 1.4e-6 / 1.3e-6 (bound 6e-4), top state 1.8e-6 / 1.3e-6 (3e-4), bottom state 7.8e-6 / 8.4e-6 (1.5e-4)
  bf16  maps 5.4e-3 / 6.0e-3 (6e-2), top state 5.9e-3 / 5.1e-3 (6e-2), bottom state 2.3e-2 / 2.5e-2 (6e-2)
  first step behind the first cut (must be > 0.2): no state 0.59 / 0.56, top half dropped 0.39 / 0.38, bottom half dropped
  0.34 / 0.31; every other test here is bit for bit."""
import functools

import numpy as np
import pytest
import torch

import cascade_stream_ref as cr
from recurrent_gaze_prediction_amd import _lib
from recurrent_gaze_prediction_amd import synthetic as syn
from test_cascade_gpu import TOL

pytestmark = pytest.mark.gpu
RGP_ESTATE = -4         # include/rgp.h
PLANS = [('f32', False), ('f32', True), ('bf16', False), ('bf16', True)]          # (dtype, save_for_backward)
PLAN_IDS = ['f32-inference', 'f32-training', 'bf16-inference', 'bf16-training']
_engines = {}


@pytest.fixture(scope='module', autouse=True)
def _release_engines():
    yield
    _engines.clear()


@functools.lru_cache(maxsize=None)
def params(seed):
    return syn.cascade_params(seed)


def engine(gpu, dtype, save, B, T, seed):
    """One engine per plan shape for the whole module (plans are big to build); the weights of `seed` are set when they differ."""
    from recurrent_gaze_prediction_amd.engine import CascadeEngine
    key = (dtype, save, B, T)
    if key not in _engines:
        _engines[key] = [CascadeEngine(B, T, 98, dtype=dtype, device=gpu, save_for_backward=save), None]
    slot = _engines[key]
    if slot[1] != seed:
        slot[0].set_weights(params(seed))
        slot[1] = seed
    return slot[0]


def dev_inputs(gpu, seed, B, N):
    frames, c3d = cr.inputs(seed, B, N)
    return torch.tensor(frames, device=gpu), torch.tensor(c3d, device=gpu)


# ---------------------------------------------------------------------------------- 1. NULL state = the plain forward
@pytest.mark.parametrize('dtype,save', PLANS, ids=PLAN_IDS)
def test_null_state_is_the_plain_forward(gpu, dtype, save):
    B, T = 2, 4
    eng = engine(gpu, dtype, save, B, T, 301)
    frames, c3d = dev_inputs(gpu, 301, B, T)
    want = eng.forward(frames, c3d).clone()
    for n_valid in (T, 2):
        maps, state = eng.forward_stream(frames, c3d, state=None, n_valid=n_valid)
        assert torch.equal(maps, want)                                  # all T steps are computed, whatever n_valid
        bot, top = cr.split_state(state, B)
        h = eng.read_buffer('rcn_outputs').reshape(B, T, -1)[:, n_valid - 1]
        g = eng.read_buffer('gaze_rcn_outputs').reshape(B, T, -1)[:, n_valid - 1]
        assert float(bot.abs().max()) > 0 and float(top.abs().max()) > 0
        assert torch.equal(bot, h)                                      # fp32 snapshots either way
        if dtype == 'f32':
            assert torch.equal(top, g)
        else:                                                           # the buffer holds the operand-rounded copies: one bf16 rounding
            assert bool(((top - g).abs() <= 2.0 ** -8 * top.abs()).all())
    # directly behind a call that seeded a state (slot 0 of the snapshots and of the operand images): zeros again
    seeded, _ = eng.forward_stream(frames, c3d, state=state, n_valid=T)
    assert not torch.equal(seeded, want)
    again, _ = eng.forward_stream(frames, c3d, state=None, n_valid=T)
    assert torch.equal(again, want)
    eng.forward_stream(frames, c3d, state=state, n_valid=T)
    assert torch.equal(eng.forward(frames, c3d), want)


# ---------------------------------------------------------------------------------- 2. state_in is read-only
@pytest.mark.parametrize('dtype,save', PLANS, ids=PLAN_IDS)
def test_state_in_is_read_only(gpu, dtype, save):
    B, T = 2, 4
    eng = engine(gpu, dtype, save, B, T, 301)
    frames, c3d = dev_inputs(gpu, 301, B, T)
    _, state = eng.forward_stream(frames, c3d, n_valid=3)
    before = state.clone()
    _, new_state = eng.forward_stream(frames, c3d, state=state, n_valid=T)
    assert torch.equal(state, before)
    assert new_state.data_ptr() != state.data_ptr() and not torch.equal(new_state, state)


# ---------------------------------------------------------------------------------- 3. cut invariance
CUTS = ((4, 4, 2), (3, 3, 3, 1), (1,) * 10, (2, 4, 4))


@pytest.mark.parametrize('B', [2, 1])
@pytest.mark.parametrize('dtype,save', PLANS, ids=PLAN_IDS)
def test_maps_and_state_do_not_depend_on_the_cuts(gpu, dtype, save, B):
    """The kernels of a step do not depend on the cut and the seed converts as the epilogue does: bit for bit.  What lies behind
    n_valid (features and frames, filled with 3.0) reaches nothing."""
    T, N = 4, 10
    eng = engine(gpu, dtype, save, B, T, 301)
    frames, c3d = dev_inputs(gpu, 301, B, N)
    runs = [cr.run_stream(eng, frames, c3d, cuts, pad_value=3.0) for cuts in CUTS]
    maps0, state0 = runs[0]
    assert bool(torch.isfinite(maps0).all()) and float(maps0.abs().max()) > 0
    for cuts, (maps, state) in zip(CUTS[1:], runs[1:]):
        assert torch.equal(maps, maps0), (cuts, float((maps - maps0).abs().max()))
        assert torch.equal(state, state0), (cuts, float((state - state0).abs().max()))


# ---------------------------------------------------------------------------------- 4. against float64
@pytest.mark.parametrize('seed', cr.SEEDS)
@pytest.mark.parametrize('dtype,save', PLANS, ids=PLAN_IDS)
def test_stream_matches_float64(gpu, dtype, save, seed):
    """Seven steps from calls of 3, 3, 1 on a T = 3 plan against ONE float64 recurrence.  Bounds: those of tests/test_cascade_gpu.py
    (T = 3 and T = 35 cases); f32 times 3, the factor that file gives its 35-step case -- seven steps sit between the two."""
    B, T, N = 2, 3, 7
    p, frames, c3d, ref_maps, ref_h, ref_g = cr.stream_reference(seed)
    eng = engine(gpu, dtype, save, B, T, seed)
    maps, state = cr.run_stream(eng, torch.tensor(frames, device=gpu), torch.tensor(c3d, device=gpu), (3, 3, 1))
    bot, top = cr.split_state(state, B)
    errs = {'maps': cr.rel_err(maps.cpu().numpy(), ref_maps),
            'gaze_rcn_outputs': cr.rel_err(top.cpu().numpy().reshape(B, 49, 49, 3), ref_g[:, -1]),
            'rcn_outputs': cr.rel_err(bot.cpu().numpy().reshape(B, 7, 7, 256), ref_h[:, -1])}
    print('cascade stream vs float64 %s save=%d seed %d: %s' % (dtype, save, seed, {k: '%.3e' % v for k, v in errs.items()}))
    mul = 3 if dtype == 'f32' else 1
    for k, e in errs.items():
        assert e < mul * TOL[dtype][k], (k, errs)


# ---------------------------------------------------------------------------------- 5. each half of the state matters
@pytest.mark.parametrize('seed', cr.SEEDS)
@pytest.mark.parametrize('dtype,save', PLANS, ids=PLAN_IDS)
def test_each_half_of_the_state_matters(gpu, dtype, save, seed):
    """The same calls with no state, with the top half dropped and with the bottom half dropped: each misses the reference on the
    first step behind the first cut by more than 0.2 (float64: 0.58-0.62, 0.39-0.41, 0.32-0.36; any bound above is <= 6e-2).
    A seed that silently dropped one state would pass everything else but the float64 test."""
    B, T = 2, 3
    p, frames, c3d, ref_maps, _, _ = cr.stream_reference(seed)
    eng = engine(gpu, dtype, save, B, T, seed)
    f, x = torch.tensor(frames, device=gpu), torch.tensor(c3d, device=gpu)
    scale = np.abs(ref_maps).max()
    for carry in ('none', 'bottom', 'top'):
        maps, _ = cr.run_stream(eng, f, x, (3, 3, 1), carry=carry)
        e = float(np.abs(maps[:, 3].cpu().numpy() - ref_maps[:, 3]).max() / scale)
        print('cascade stream %s save=%d seed %d, carried: %s -> step-3 error %.3f' % (dtype, save, seed, carry, e))
        assert e > 0.2, (carry, e)
        assert cr.rel_err(maps[:, :3].cpu().numpy(), ref_maps[:, :3]) < (3 if dtype == 'f32' else 1) * TOL[dtype]['maps']   # ahead of the cut


# ---------------------------------------------------------------------------------- 6. training plans
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_backward_behind_a_streaming_call_is_refused_until_a_plain_forward(gpu, dtype):
    from recurrent_gaze_prediction_amd.engine import CascadeEngine
    B, T = 2, 3
    eng = engine(gpu, dtype, True, B, T, 301)
    frames, c3d = dev_inputs(gpu, 301, B, T)
    gt = torch.tensor((lambda g: g / g.max())(syn.gaze_maps(324, B, T)[0]).astype(np.float32), device=gpu)
    _, state = eng.forward_stream(frames, c3d, n_valid=T)
    maps, _ = eng.forward_stream(frames, c3d, state=state, n_valid=T)
    with pytest.raises(_lib.RgpError) as e:
        eng.backward(maps, gt)
    assert e.value.code == RGP_ESTATE and 'streaming' in str(e.value)
    maps = eng.forward(frames, c3d)                                     # re-arms it
    fresh = CascadeEngine(B, T, 98, dtype=dtype, device=gpu, save_for_backward=True)
    fresh.set_weights(params(301))
    assert torch.equal(maps, fresh.forward(frames, c3d))
    grads, _ = eng.backward(maps, gt)
    want, _ = fresh.backward(fresh.forward(frames, c3d), gt)
    # The same kernels on the same saved activations.  The backward is not bit for bit from run to run (fp32 atomics sum in
    # any order, and on a bf16 plan such a last-bit difference can flip the bf16 rounding of a gradient operand, 2^-8 of that
    # element), so the two engines are held to what tests/test_cascade_gpu.py allows a backward against autograd: (max, rms)
    # (1e-3, 3e-4) f32, (3e-1, 6e-2) bf16.  A slot (b, 0) of hp_all left seeded would move the top cell's recurrent filter
    # gradients by a third of their size: step 0 of 3 would read a wrong operand image.
    tol_max, tol_rms = (1e-3, 3e-4) if dtype == 'f32' else (3e-1, 6e-2)
    for k, g in grads.items():
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, k
        d = (g - want[k]).double()
        e_max = float(d.abs().max() / want[k].abs().max())
        e_rms = float(torch.sqrt((d ** 2).mean()) / torch.sqrt((want[k].double() ** 2).mean()))
        assert e_max < tol_max and e_rms < tol_rms, (k, e_max, e_rms)


# ---------------------------------------------------------------------------------- 7. the models
def make_model(gpu, tmp_path, B=2, T=4, trainable=True):
    from recurrent_gaze_prediction_amd.models.base import Session
    from recurrent_gaze_prediction_amd.models.gaze_grcn_cascade import GazePredictionGRCN, GRUModelConfig
    cfg = GRUModelConfig()
    cfg.batch_size, cfg.n_lstm_steps, cfg.compute_dtype, cfg.train_dir, cfg.init_seed = B, T, 'bf16', str(tmp_path), 3
    cfg.trainable = trainable
    return GazePredictionGRCN(Session(gpu), None, cfg)


def clip_inputs(seed, n):
    frames, c3d = cr.inputs(seed, 1, n)
    return c3d[0], frames[0]


def test_predict_long_clips_equals_each_clip_alone_in_lane_0(gpu, tmp_path):
    """Every GEMM row is a dot product in a fixed K order, whatever else is in the batch: bit for bit.  The model's default
    plan, a training plan."""
    from recurrent_gaze_prediction_amd.stream import GazeStream, predict_long_clips
    model = make_model(gpu, tmp_path)
    assert model.engine.net.save_for_backward
    pairs = [clip_inputs(90 + i, n) for i, n in enumerate((5, 9, 2))]
    maps = predict_long_clips(model, [c for c, _ in pairs], frames=[f for _, f in pairs])
    for (c, f), m in zip(pairs, maps):
        st, alone = GazeStream(model), []
        for s in range(0, len(c), 4):
            part, fpart = c[s:s + 4], f[s:s + 4]
            x = np.zeros((2, len(part), 1024, 7, 7), np.float32)
            fx = np.zeros((2, len(part), 98, 98, 3), np.float32)
            x[0], fx[0] = part, fpart
            alone.append(st.push_features(x, frames=fx)[0].cpu().numpy())
        alone = np.concatenate(alone)
        assert m.shape == (len(c), 49, 49) and np.isfinite(m).all() and np.abs(m).max() > 0
        assert np.array_equal(m, alone), float(np.abs(m - alone).max())
    with pytest.raises(ValueError):
        predict_long_clips(model, [c for c, _ in pairs])


def test_predict_long_clip_with_and_without_the_carried_state(gpu, tmp_path):
    from recurrent_gaze_prediction_amd.models.evaluate_gaze import predict_long_clip
    model = make_model(gpu, tmp_path, trainable=False)
    clip, frames = clip_inputs(95, 9)
    padded = np.zeros((12, 98, 98, 3), np.float32)
    padded[:9] = frames
    chunked = np.concatenate([predict_long_clip(model, clip[s:s + 4], frames=np.stack([padded[s:s + 4], np.zeros((4, 98, 98, 3), np.float32)]))
                              for s in (0, 4, 8)])
    carried = predict_long_clip(model, clip, frames=frames, carry_state=True)
    assert chunked.shape == carried.shape == (9, 49, 49)
    assert np.array_equal(carried[:4], chunked[:4])            # the first chunk starts from zeros either way
    d = np.abs(carried - chunked).reshape(9, -1).max(-1)
    print('cascade carried vs chunked, max |d map| per step: %s' % d)
    assert (d[4:] > 0).all()                                   # from step 4 on the model remembers


# ---------------------------------------------------------------------------------- 8. predict_video
@pytest.mark.parametrize('family', ['cascade', 'grcn'])
def test_predict_video_is_predict_long_clips_on_video_inputs(gpu, tmp_path, family):
    from recurrent_gaze_prediction_amd import c3d_frontend as fe
    from recurrent_gaze_prediction_amd import frames as fr
    from recurrent_gaze_prediction_amd.engine import C3DEngine
    from recurrent_gaze_prediction_amd.stream import predict_long_clips, predict_video
    if family == 'cascade':
        model = make_model(gpu, tmp_path, trainable=False)
    else:
        import stream_ref as sr
        from recurrent_gaze_prediction_amd.models.base import Session
        from recurrent_gaze_prediction_amd.models.gaze_grcn import GazePredictionGRCN, GRUModelConfig
        cfg = GRUModelConfig()
        cfg.batch_size, cfg.n_lstm_steps, cfg.compute_dtype, cfg.train_dir, cfg.trainable = 2, 4, 'bf16', str(tmp_path), False
        model = GazePredictionGRCN(Session(gpu), None, cfg)
        model.load_state_dict(sr.params('grcn', 4))
    clip = np.random.RandomState(41).randint(0, 256, size=(41, 37, 53, 3)).astype(np.uint8)
    c3d = C3DEngine(6, dtype='bf16', device=gpu)
    c3d.set_weights(syn.c3d_params(3))
    extractor = fe.C3DFeatureExtractor(c3d)
    maps = predict_video(model, clip, extractor)
    starts, feats, images = fr.video_inputs(clip, extractor, image_hw=98)
    assert len(starts) == 6 and maps.shape == (6, 49, 49) and np.isfinite(maps).all() and np.abs(maps).max() > 0
    kw = {'frames': [images]} if family == 'cascade' else {}
    want = predict_long_clips(model, [feats.reshape(6, 1024, 7, 7)], **kw)[0]
    assert np.array_equal(maps, want)


def test_push_windows_goes_through_the_features_for_an_engine_without_rows(gpu, tmp_path):
    from recurrent_gaze_prediction_amd.engine import C3DEngine
    from recurrent_gaze_prediction_amd.stream import GazeStream
    B, T = 2, 4
    model = make_model(gpu, tmp_path, trainable=False)
    c3d = C3DEngine(B * T, dtype='bf16', device=gpu)
    c3d.set_weights(syn.c3d_params(3))
    video = torch.tensor(syn.video_windows(7, B * T), device=gpu)
    images = torch.tensor(cr.inputs(97, B, T)[0], device=gpu)
    a, b = GazeStream(model, c3d_engine=c3d), GazeStream(model)
    for n_valid in (3, 4):                                         # the second call starts from the first one's state
        got = a.push_windows(video, n_valid=n_valid, frame_images=images)
        feats = c3d.forward(video, want_features=True)[0].reshape(B, T, 1024, 7, 7)
        want = b.push_features(feats, n_valid=n_valid, frames=images)
        assert tuple(got.shape) == (B, T, 49, 49) and torch.equal(got, want) and torch.equal(a.state, b.state)
    assert a.position == b.position == 7
    with pytest.raises(ValueError):
        GazeStream(model, c3d_engine=c3d).push_windows(video)      # no frame images
