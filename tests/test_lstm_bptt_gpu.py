"""GPU: the persistent BPTT of gaze_lstm (csrc/convlstm_bptt.hip.h, RGP_LSTM_BPTT_PERSISTENT) through the C ABI.

1. gradients of every variable and backward_input() against float64 autograd (tests/lstm_ref.py), the project's bf16 bound;
2. the pre-activation gradients d_i .. d_o against the library's second implementation (the per-step BPTT loop) on bit-equal
   saved state: at the worst step the two paths may be at most 0.25 of the per-step path's own distance to float64
   (tests/lstm_bptt_ref.py) apart -- they round the same quantities to bf16 at the same places and differ only in fp32
   summation order, while a wrong term is of the order of the bf16 distance itself (tests/test_lstm_bptt_cpu.py);
3. determinism of everything that is computed without float atomics;
4. the flag's preconditions and what the plan reports;
5. the time-out path, on the plan and through the model class.

Shapes (engines are bf16 training plans with the persistent forward unless said otherwise): 3 x 4 (4 row fragments, 3 groups,
plain group map), 8 x 3 (8 groups: the XCD-contiguous group map; T = 3 reuses an exchange parity), 33 x 5 (7 row fragments,
last group ragged), 64 x 3 (32 groups, the whole chip), 2 x 35 (long carry chains).  Every test prints its figures before it
asserts (-s).  The float64 references and the device results are computed once per shape and shared, never modified.
Measured on an MI355X ("gaze_lstm"): gradients <= 8.2e-3; the ratio of 2. is <= 0.016 at T <= 5 and <= 0.11 at T = 35."""
import numpy as np
import pytest
import torch

import lstm_bptt_ref as bref
import lstm_ref as ref
from recurrent_gaze_prediction_amd import synthetic as syn

pytestmark = pytest.mark.gpu

GRAD_TOL = 3e-2                                 # relative Frobenius: the project's bf16 gradient bound (tests/test_lstm_gpu.py)
PARITY = 0.25                                   # persistent <-> per-step, as a fraction of per-step <-> float64
SHAPES = [(3, 4), (8, 3), (33, 5), (64, 3), (2, 35)]
DETERMINISTIC = ('ConvLSTM_Wci', 'ConvLSTM_Wcf', 'ConvLSTM_Wco', 'proj_c3d_W', 'proj_c3d_b')     # (wgrad_kernel outputs: fp32 atomics)


def labels_for(seed, B, T):
    gt, _ = syn.gaze_maps(seed, B, T)
    return (gt / gt.sum((2, 3), keepdims=True)).astype(np.float32)


def rows_grad_to_input(d_rows, B, T):
    """d_rows [B*T*49, 1024] (column d*512+c) -> the gradient in the placeholder layout [B,T,1024,7,7] (channel c*2+d)."""
    d = np.asarray(d_rows, np.float64).reshape(B, T, 7, 7, 2, 512)
    return d.transpose(0, 1, 5, 4, 2, 3).reshape(B, T, 1024, 7, 7)


_REF, _DEV = {}, {}


def reference(B, T, loss_type):
    """(params, x, labels, autograd's gradients incl. c3d_input, float64 d_i .. d_o of the kernel-form restatement)."""
    key = (B, T, loss_type)
    if key not in _REF:
        p = syn.lstm_params(171)
        x = syn.c3d_features(172 + B, B, T)
        gt = labels_for(173, B, T)
        _, _, want = ref.loss_and_grads(x, gt, p, loss_type, want_input_grad=True)
        saved, dh_head = bref.saved_and_head_grad(x, gt, p, loss_type)
        d = {k: v.numpy() for k, v in bref.bptt(saved, dh_head, p).items()}
        _REF[key] = (p, x, gt, want, d)
    return _REF[key]


def make_engine(B, T, gpu, bptt=True, fwd_per_step=False, params=None):
    from recurrent_gaze_prediction_amd.engine import LstmEngine
    eng = LstmEngine(B, T, dtype='bf16', device=gpu, save_for_backward=True, per_step=fwd_per_step, persistent=not fwd_per_step,
                     bptt_persistent=bptt)
    if params is not None:
        eng.set_weights(params)
    return eng


def read_d(eng, B, T):
    return {k: eng.read_buffer(k).reshape(B, T, 7, 7, 128).clone() for k in bref.GATES}


def device_run(B, T, loss_type, gpu, bptt=True, fwd_per_step=False):
    """One forward + backward: {'grads': {name: numpy}, 'd': {d_i ..: numpy}, 'rows': numpy, 'h', 'i': device tensors}."""
    key = (B, T, loss_type, bptt, fwd_per_step)
    if key not in _DEV:
        p, x, gt, _, _ = reference(B, T, loss_type)
        eng = make_engine(B, T, gpu, bptt, fwd_per_step, p)
        assert eng.bptt_persistent == bptt and eng.persistent == (not fwd_per_step)
        logits, probs = eng.forward(torch.tensor(x, device=gpu))
        grads = eng.backward(logits, probs, torch.tensor(gt, device=gpu), loss_type)
        rows = eng.backward_input()
        eng.status()
        _DEV[key] = {'grads': {k: v.cpu().numpy() for k, v in grads.items()}, 'd': {k: v.cpu().numpy() for k, v in read_d(eng, B, T).items()},
                     'rows': rows.cpu().numpy(), 'h': eng.read_buffer('h').clone(), 'c': eng.read_buffer('c').clone(),
                     'o': eng.read_buffer('o').clone()}
    return _DEV[key]


def check_gradients(tag, B, T, loss_type, got):
    _, _, _, want, _ = reference(B, T, loss_type)
    grads = got['grads']
    assert set(grads) == set(ref.KEYS)
    assert want['ConvLSTM_Whc'] is None and np.abs(grads['ConvLSTM_Whc']).max() == 0.0        # exactly zero
    bad = []
    for k in ref.KEYS:
        if k == 'ConvLSTM_Whc':
            continue
        if k == 'out_b' and loss_type == 'xentropy':
            # d loss / d out_b = 0 exactly for normalised labels: only round-off remains (tests/test_lstm_gpu.py)
            assert abs(grads[k].item()) < 1e-6 and abs(want[k].item()) < 1e-12
            continue
        err = bref.fro(grads[k], want[k])
        print('grad %s %dx%d %s %s: %.3e' % (tag, B, T, loss_type, k, err))
        if not err <= GRAD_TOL:
            bad.append((k, err))
    err = bref.fro(rows_grad_to_input(got['rows'], B, T), want['c3d_input'])
    print('d_rows %s %dx%d %s: %.3e' % (tag, B, T, loss_type, err))
    if not err <= GRAD_TOL:
        bad.append(('c3d_input', err))
    assert not bad, bad


@pytest.mark.parametrize('B,T,loss_type', [(B, T, 'xentropy') for B, T in SHAPES] + [(3, 4, 'l2')])
def test_gradients_match_float64_autograd(gpu, B, T, loss_type):
    check_gradients('persistent BPTT', B, T, loss_type, device_run(B, T, loss_type, gpu))


@pytest.mark.parametrize('B,T', SHAPES)
def test_persistent_against_per_step_bptt(gpu, B, T):
    _, _, _, _, d64 = reference(B, T, 'xentropy')
    a = device_run(B, T, 'xentropy', gpu, bptt=True)
    b = device_run(B, T, 'xentropy', gpu, bptt=False)
    for k in ('h', 'c', 'o'):                               # the same forward: the two BPTTs start from the same bits
        assert torch.equal(a[k], b[k]), k
    bad = {}
    for k in bref.GATES:
        ab, b64 = bref.step_fro(a['d'][k], b['d'][k]), bref.step_fro(b['d'][k], d64[k])
        # (d_f of step 0 is exactly zero on every path and in float64 -- c_0 = 0 --: 0 <= 0.25 x 0 holds, its ratio is left out)
        ratio = np.where(b64 > 0, ab / np.maximum(b64, 1e-300), 0.0)
        t = int(np.argmax(ratio))
        print('BPTT %dx%d %s: worst step %d persistent<->per-step %.3e, per-step<->float64 %.3e, ratio %.4f' % (B, T, k, t, ab[t], b64[t], ratio[t]))
        if not (np.isfinite(ab).all() and (ab <= PARITY * b64).all()):                  # at every step, hence at the worst
            bad[k] = (ab, b64)
    assert not bad, bad


def test_two_backward_calls_give_the_same_bits(gpu):
    B, T = 33, 5
    p, x, gt, _, _ = reference(B, T, 'xentropy')
    eng = make_engine(B, T, gpu, params=p)
    logits, probs = eng.forward(torch.tensor(x, device=gpu))
    gd = torch.tensor(gt, device=gpu)
    runs = []
    for _ in range(2):
        grads = eng.backward(logits, probs, gd)
        runs.append((read_d(eng, B, T), {k: grads[k].clone() for k in DETERMINISTIC}, eng.backward_input().clone()))
    eng.status()
    for k in bref.GATES:
        assert torch.equal(runs[0][0][k], runs[1][0][k]), k
    for k in DETERMINISTIC:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k
    assert torch.equal(runs[0][2], runs[1][2])


def test_flag_preconditions_and_reported_workgroups(gpu):
    from recurrent_gaze_prediction_amd import _lib
    from recurrent_gaze_prediction_amd.engine import LstmEngine
    with pytest.raises(_lib.RgpError, match='bf16'):
        LstmEngine(2, 2, dtype='f32', device=gpu, save_for_backward=True, bptt_persistent=True)
    with pytest.raises(_lib.RgpError, match='64 clips'):
        LstmEngine(65, 1, dtype='bf16', device=gpu, save_for_backward=True, bptt_persistent=True)
    with pytest.raises(_lib.RgpError, match='SAVE_FOR_BACKWARD'):
        LstmEngine(2, 2, dtype='bf16', device=gpu, bptt_persistent=True)
    today = LstmEngine(3, 4, dtype='bf16', device=gpu, save_for_backward=True)
    assert today.bptt_persistent_workgroups == 0 and not today.bptt_persistent and today.persistent
    assert make_engine(3, 4, gpu).bptt_persistent_workgroups == 24
    assert make_engine(33, 5, gpu).bptt_persistent_workgroups == 136
    both = make_engine(3, 4, gpu, fwd_per_step=True)
    assert both.bptt_persistent_workgroups == 24 and both.persistent_workgroups == 0 and not both.persistent


def test_persistent_bptt_behind_the_per_step_forward(gpu):
    check_gradients('per-step forward, persistent BPTT', 3, 4, 'xentropy', device_run(3, 4, 'xentropy', gpu, fwd_per_step=True))


def test_lost_group_member_is_loud(gpu):
    """Mirrors tests/test_lstm_gpu.py: one workgroup of group 0 returns at launch, the group gives up at its deadline (~1 s),
    the kernel returns normally.  Member 7 (state channels 112 .. 127) is the one that leaves: it writes nothing at all."""
    from recurrent_gaze_prediction_amd import _lib
    B, T = 3, 4                                                # one clip per group: group 0 = clip 0
    p, x, gt, _, _ = reference(B, T, 'xentropy')
    eng = make_engine(B, T, gpu, params=p)
    xd, gd = torch.tensor(x, device=gpu), torch.tensor(gt, device=gpu)

    out = []

    def step(forward=True):
        if forward:
            out[:] = eng.forward(xd)
        grads = eng.backward(out[0], out[1], gd)
        return read_d(eng, B, T), {k: grads[k].clone() for k in DETERMINISTIC}, eng.backward_input().clone()

    good = step()
    eng.status()                                               # clean
    eng.inject_fault('bptt')
    d, _, _ = step(forward=False)
    with pytest.raises(_lib.RgpError, match='lost a group member') as info:
        eng.status()
    assert info.value.code == _lib.RGP_ETIMEOUT
    eng.status()                                               # reported once, then clear
    assert torch.isnan(d['d_i'][0, 0, :, :, :112]).all()       # step 0 of clip 0, every member that was there
    for k in bref.GATES:
        assert torch.equal(d[k][1:], good[0][k][1:]), k        # the other groups never noticed
    again = step()
    eng.status()
    for k in bref.GATES:
        assert torch.equal(again[0][k], good[0][k]), k         # the plan is usable again, bit for bit
    for k in DETERMINISTIC:
        assert torch.equal(again[1][k], good[1][k]), k
    assert torch.equal(again[2], good[2])
    with pytest.raises(_lib.RgpError):
        make_engine(B, T, gpu, bptt=False).inject_fault('bptt')


def test_model_redoes_a_timed_out_training_step_per_step(gpu, tmp_path):
    from recurrent_gaze_prediction_amd.models.base import Session
    from recurrent_gaze_prediction_amd.models.gaze_lstm import GazePredictionLSTM, GRUModelConfig
    B, T = 2, 3
    cfg = GRUModelConfig()
    cfg.batch_size, cfg.n_lstm_steps, cfg.loss_type, cfg.compute_dtype = B, T, 'xentropy', 'bf16'
    cfg.trainable, cfg.convlstm_path, cfg.convlstm_bptt_path = True, 'persistent', 'persistent'
    cfg.train_dir = str(tmp_path)
    ds = type('DS', (), {})()
    ds.train = ds.valid = syn.SyntheticDataSet(12, T, seed=5)
    model = GazePredictionLSTM(Session(gpu), ds, cfg)
    model.load_state_dict(syn.lstm_params(192))
    model.config.use_flip_batch = False
    assert model.engine.bptt_persistent and model.engine.persistent
    before = model.state_dict()
    model.engine.inject_fault('bptt')
    assert model.single_step(train_mode=True) == 1             # RGP_ETIMEOUT inside: forward + backward again, per step
    assert model.engine.per_step and not model.engine.persistent and not model.engine.bptt_persistent
    assert model.config.convlstm_bptt_path == 'per_step'
    after = model.state_dict()
    assert all(np.isfinite(v).all() for v in after.values())
    assert not np.array_equal(before['ConvLSTM_Wxi_1'], after['ConvLSTM_Wxi_1'])
