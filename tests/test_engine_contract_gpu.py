"""GPU: what every engine class promises about the plan it owns and its master buffers, through the public API only, at the
smallest plan each family accepts (B = 1, T = 2: the per-timestep batch-norm shape check and n_valid = 1 < T stay in play).

Per class: weights[k] are views into flat_params and a second set_weights keeps the storage; on training plans the first
backward creates flat_grads, the second reuses it and grads[k] are views into it; adam_step returns a 1-element device tensor
and moves flat_params; optimizer_state -> load_optimizer_state round-trips the slots bit for bit; an engine can be deleted
and another created; the members the models probe for with hasattr are there or absent as the family's C ABI has them.
GrcnEngine / FcGruEngine: backward_stream with the default loss_frames is backward_stream with B * n_valid named."""
import numpy as np
import pytest
import torch

from recurrent_gaze_prediction_amd import synthetic as syn

pytestmark = pytest.mark.gpu
B, T = 1, 2


def dev(a, gpu):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(gpu)


def maps(seed, shape, gpu):
    """Strictly positive maps, each frame summing to one."""
    m = torch.rand(shape, generator=torch.Generator().manual_seed(seed)) + 0.01
    return (m / m.sum((-1, -2), keepdim=True)).to(gpu).contiguous()


def _gaze(cls_name, params, hw=49, **kw):
    def make(gpu, train=True):
        from recurrent_gaze_prediction_amd import engine as E
        eng = getattr(E, cls_name)(B, T, save_for_backward=train, device=gpu, **kw)
        return eng, params()

    def step(eng, gpu):
        z, p = eng.forward(dev(syn.c3d_features(3, B, T), gpu))[:2]
        return eng.backward(z, p, maps(4, (B, T, hw, hw), gpu))
    return make, step


def _shallownet():
    def make(gpu, train=True):
        from recurrent_gaze_prediction_amd.engine import ShallowNetEngine
        return ShallowNetEngine(max_frames=2, save_for_backward=train, device=gpu), syn.shallownet_params(5)

    def step(eng, gpu):
        sal, _ = eng.forward(torch.rand(2, 98, 98, 3, generator=torch.Generator().manual_seed(6)).to(gpu))
        return eng.backward(sal - maps(7, (2, 49, 49), gpu))
    return make, step


def _cascade():
    def make(gpu, train=True):
        from recurrent_gaze_prediction_amd.engine import CascadeEngine
        return CascadeEngine(B, T, save_for_backward=train, device=gpu), syn.cascade_params(8)

    def step(eng, gpu):
        frames = torch.rand(B, T, 98, 98, 3, generator=torch.Generator().manual_seed(9)).to(gpu)
        out = eng.forward(frames, dev(syn.c3d_features(3, B, T), gpu))
        return eng.backward(out, maps(10, (B, T, 49, 49), gpu))[0]
    return make, step


FAMILIES = {
    'GrcnEngine': _gaze('GrcnEngine', lambda: syn.grcn_params(1, T, random_bn=True)),
    'C3dConvEngine': _gaze('C3dConvEngine', lambda: syn.c3d_conv_params(1)),
    'LstmEngine': _gaze('LstmEngine', lambda: syn.lstm_params(1)),
    'Grcn77Engine': _gaze('Grcn77Engine', lambda: syn.grcn77_params(1), hw=7),
    'FcGruEngine': _gaze('FcGruEngine', lambda: syn.fcgru_params(1, 7, 7), hw=7, gazemap_hw=(7, 7)),
    'ShallowNetEngine': _shallownet(),
    'CascadeEngine': _cascade(),
}
# member -> the classes that have it (the families whose C ABI has the entry behind it)
MEMBERS = {
    'forward_rows': {'GrcnEngine', 'C3dConvEngine', 'LstmEngine', 'Grcn77Engine', 'ActionEngine'},
    'backward_input': {'GrcnEngine', 'C3dConvEngine', 'LstmEngine', 'Grcn77Engine'},
    'status': {'GrcnEngine', 'LstmEngine', 'Grcn77Engine', 'FcGruEngine'},
    'persistent': {'GrcnEngine', 'LstmEngine', 'Grcn77Engine', 'FcGruEngine'},
    'bptt_persistent': {'LstmEngine', 'FcGruEngine'},
    'forward_stream': {'GrcnEngine', 'LstmEngine', 'Grcn77Engine', 'FcGruEngine', 'CascadeEngine'},
    'state_elems': {'GrcnEngine', 'LstmEngine', 'Grcn77Engine', 'FcGruEngine', 'CascadeEngine'},
    'backward_stream': {'GrcnEngine', 'FcGruEngine'},
    'read_buffer_elems': {'GrcnEngine', 'C3dConvEngine', 'LstmEngine', 'Grcn77Engine', 'ShallowNetEngine', 'ActionEngine'},
}


def check_members(eng):
    name = type(eng).__name__
    for member, have in MEMBERS.items():
        assert hasattr(eng, member) == (name in have), (name, member)


def inside(view, flat):
    lo = flat.data_ptr()
    return lo <= view.data_ptr() and view.data_ptr() + view.numel() * 4 <= lo + flat.numel() * 4


def check_master(eng, params, trained=None):
    """weights[k] alias flat_params, which holds exactly the trained variables; a second set_weights keeps the storage."""
    eng.set_weights(params)
    trained = [k for k in eng.weights if inside(eng.weights[k], eng.flat_params)] if trained is None else trained
    assert trained and all(inside(eng.weights[k], eng.flat_params) for k in trained)
    assert sum(eng.weights[k].numel() for k in trained) == eng.flat_params.numel()
    assert eng.flat_params.dtype == torch.float32 and eng.flat_params.device == eng.device
    flat, ptrs = eng.flat_params, {k: v.data_ptr() for k, v in eng.weights.items() if k in trained}
    eng.set_weights(params)
    assert eng.flat_params is flat and ptrs == {k: eng.weights[k].data_ptr() for k in trained}
    return trained


def check_step_and_slots(eng, held):
    from recurrent_gaze_prediction_amd.engine import clip_step_multi, load_optimizer_state, optimizer_state
    # (the cascade's model steps its engine through clip_step_multi, which is what adam_step is everywhere else)
    norm = clip_step_multi([eng], 0, 1e-3) if type(eng).__name__ == 'CascadeEngine' else eng.adam_step(0, 1e-3)
    assert norm.is_cuda and norm.numel() == 1 and bool(torch.isfinite(norm).all())
    assert not torch.equal(eng.flat_params, held) and bool(torch.isfinite(eng.flat_params).all())
    state = optimizer_state(eng)
    assert set(state) == {'adam_m', 'adam_v'} and all(not v.is_cuda for v in state.values())
    assert float(state['adam_m'].abs().max()) > 0
    eng.adam_m, eng.adam_v = None, None
    load_optimizer_state(eng, state)
    assert all(torch.equal(getattr(eng, k).cpu(), v) and getattr(eng, k).device == eng.device for k, v in state.items())
    assert all(torch.equal(v, state[k]) for k, v in optimizer_state(eng).items())


@pytest.mark.parametrize('name', sorted(FAMILIES))
def test_a_training_plan_owns_its_buffers(gpu, name):
    make, step = FAMILIES[name]
    eng, params = make(gpu)
    check_members(eng)
    assert eng.workspace.is_cuda and eng.workspace.dtype == torch.uint8
    assert eng.flat_grads is None and eng.grads is None
    trained = check_master(eng, params)
    grads = step(eng, gpu)
    flat = eng.flat_grads
    assert grads is eng.grads and flat.numel() == eng.flat_params.numel()
    assert all(inside(grads[k], flat) and grads[k].shape == eng.weights[k].shape for k in trained)
    assert all(not inside(grads[k], flat) for k in grads if k not in trained)
    assert float(flat.abs().max()) > 0 and bool(torch.isfinite(flat).all())
    first = flat.clone()
    assert step(eng, gpu) is grads and eng.flat_grads is flat               # the second backward reuses the buffer
    assert float((flat - first).abs().max()) <= 2.0 ** -8 * float(first.abs().max())       # written, not accumulated
    check_step_and_slots(eng, eng.flat_params.clone())
    del eng
    eng, params = make(gpu)                                                  # a plan destroyed, the next one created
    eng.set_weights(params)
    step(eng, gpu)
    torch.cuda.synchronize()


@pytest.mark.parametrize('name', sorted(FAMILIES))
def test_an_inference_plan_refuses_backward_and_shares_the_layout(gpu, name):
    make, step = FAMILIES[name]
    eng, params = make(gpu, train=False)
    check_members(eng)
    check_master(eng, params)
    with pytest.raises(AssertionError) as e:
        step(eng, gpu)
    assert 'save_for_backward=True' in str(e.value) and eng.flat_grads is None


def test_c3d_owns_its_buffers_at_the_librarys_offsets(gpu):
    from recurrent_gaze_prediction_amd.engine import C3DEngine, C3D_LAYER_NAMES
    eng = C3DEngine(max_windows=1, save_for_backward=True, device=gpu)
    check_members(eng)
    names = [n + s for n in C3D_LAYER_NAMES for s in ('_w', '_b')]
    assert list(eng.weights) == names and not eng.weights_set
    check_master(eng, syn.c3d_params(5), trained=names)
    assert eng.weights_set and eng.flat_grads.numel() == eng.flat_params.numel()
    gv = eng.grad_views()
    assert list(gv) == names and all(inside(gv[k], eng.flat_grads) and gv[k].shape == eng.weights[k].shape for k in names)
    assert all(gv[k].data_ptr() - eng.flat_grads.data_ptr() == eng.weights[k].data_ptr() - eng.flat_params.data_ptr() for k in names)
    feats, _ = eng.forward(dev(syn.video_windows(7, 1), gpu))
    flat = eng.flat_grads
    assert eng.backward(d_features=torch.ones_like(feats)) is flat and float(flat.abs().max()) > 0
    assert eng.layer_grad_slice(0).data_ptr() == gv['conv1a_w'].data_ptr()
    del eng
    eng = C3DEngine(max_windows=1, device=gpu)
    assert eng.flat_grads is None
    torch.cuda.synchronize()


@pytest.mark.parametrize('mode', ['NN', 'SVM'])
def test_action_owns_its_buffers(gpu, mode):
    from recurrent_gaze_prediction_amd.engine import ActionEngine, load_optimizer_state, optimizer_state
    eng = ActionEngine(batch=2, mode=mode, save_for_backward=True, device=gpu)
    check_members(eng)
    params = syn.action_params(11, mode)
    trained = check_master(eng, params)
    assert tuple(trained) == eng.names == tuple(eng.weights) and eng.adam_m is None
    c3d = dev(syn.c3d_features(3, 2, 1), gpu).reshape(2, 1024, 49).contiguous()
    labels = torch.zeros(2, 13, device=gpu)
    labels[0, 3] = labels[1, 7] = 1.0
    held = eng.flat_params.clone()
    loss = eng.train_step(c3d, None, labels, 0)
    assert loss.is_cuda and loss.numel() == 1 and bool(torch.isfinite(loss).all())
    assert not torch.equal(eng.flat_params, held) and bool(torch.isfinite(eng.flat_params).all())
    got = eng.get_weights()
    assert all(torch.equal(got[k], eng.weights[k]) and not inside(got[k], eng.flat_params) for k in eng.names)
    state = optimizer_state(eng)
    assert set(state) == ({'adam_m', 'adam_v'} if mode == 'NN' else set())
    if mode == 'NN':
        m, v = eng.slots()
        assert all(inside(m[k], eng.adam_m) and inside(v[k], eng.adam_v) for k in eng.names)
        load_optimizer_state(eng, state)
        assert all(torch.equal(getattr(eng, k).cpu(), s) for k, s in state.items())
        eng.train_step(c3d, None, labels, 1)                 # the restored slots are bound again
        assert eng.slots()[0]['W1'].data_ptr() == eng.adam_m.data_ptr()
    del eng
    eng = ActionEngine(batch=2, mode=mode, device=gpu)
    eng.set_weights(params)
    logits, y = eng.forward(c3d)
    assert tuple(logits.shape) == (2, 13) and bool(torch.isfinite(y).all())


# What two runs of ONE computation may differ by where float atomics reach it (the projection's filter gradient), as a share of
# the tensor's maximum: the bounds of tests/test_fcgru_tbptt_gpu.py (f32 plans) and tests/test_grcn_tbptt_gpu.py (RUN_TO_RUN).
RUN_TO_RUN = {'f32': 2.0 ** -20, 'bf16': 2.0 ** -8}


@pytest.mark.parametrize('name,hw', [('FcGruEngine', 7), ('GrcnEngine', 49)])
def test_the_default_loss_frames_is_batch_times_n_valid_of_the_last_forward(gpu, name, hw):
    """Two engines built alike, one input, one state, n_valid = 1 of T = 2: equal streaming forwards.  One runs backward_stream
    with the default divisor, the other with B * n_valid named -- twice, which shows the gradients the call itself reproduces
    bit for bit.  Those must be equal between the two engines; the others are held to 4 x that spread, never less than
    RUN_TO_RUN."""
    make, _ = FAMILIES[name]
    x, g = dev(syn.c3d_features(3, B, T), gpu), maps(4, (B, T, hw, hw), gpu)
    engines, results = [], []
    for loss_frames in (None, B * 1):
        eng, params = make(gpu)
        eng.set_weights(params)
        state = torch.rand(eng.state_elems, generator=torch.Generator().manual_seed(12)).to(gpu) * 0.1
        runs = []
        for _ in range(1 if loss_frames is None else 2):
            z, p, new_state = eng.forward_stream(x, state=state, n_valid=1)
            kw = {} if loss_frames is None else {'loss_frames': loss_frames}
            grads, d_in = eng.backward_stream(z, p, g, d_state=None, **kw)
            assert tuple(d_in.shape) == ((B, 1617) if name == 'FcGruEngine' else (B, 7, 7, 128)) and d_in.numel() == eng.state_elems
            runs.append(dict({k: v.clone() for k, v in grads.items()}, d_state_in=d_in, z=z[:, :1].clone(), new_state=new_state))
        eng.status()
        engines.append(eng)
        results.append(runs)
    (default,), (named, again) = results
    assert torch.equal(default['z'], named['z']) and torch.equal(default['new_state'], named['new_state'])
    assert float(named['d_state_in'].abs().max()) > 0
    for k in named:
        scale = max(float(named[k].abs().max()), 1e-30)
        spread = float((named[k] - again[k]).abs().max()) / scale
        d = float((default[k] - named[k]).abs().max()) / scale
        print(name, k, 'named against named %.2e, default against named %.2e' % (spread, d))
        if spread == 0.0 and torch.equal(named[k], again[k]):
            assert torch.equal(default[k], named[k]), k
        else:
            assert d <= max(4 * spread, RUN_TO_RUN[engines[0].dtype]), (k, d, spread)
    # and the divisor is the one of the LAST forward: behind a plain forward the default is B * T
    eng = engines[0]
    z, p = eng.forward(x)[:2]
    eng.backward_stream(z, p, g)
    full = {k: v.clone() for k, v in eng.grads.items()}
    eng.backward_stream(z, p, g, loss_frames=B * T)
    for k in full:
        d = float((full[k] - eng.grads[k]).abs().max()) / max(float(full[k].abs().max()), 1e-30)
        assert d <= RUN_TO_RUN[eng.dtype], (k, d)
    eng.status()
