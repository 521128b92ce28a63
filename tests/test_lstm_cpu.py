"""CPU: gaze_lstm -- the two restatements of the cell agree, closed forms, one probe per quirk of the reference cell
(g reuses W_hi, o reads the old c, W_hc is read by nothing), the checkpoint name table, the host-side optimizer layout that
leaves W_hc out, and the host-only part of the C ABI.  No kernel is launched here."""
import ctypes
import math

import numpy as np
import pytest
import torch

import lstm_ref as ref
from recurrent_gaze_prediction_amd import _lib, checkpoint
from recurrent_gaze_prediction_amd import synthetic as syn
from recurrent_gaze_prediction_amd.engine import LSTM_PARAM_TO_FIELD, LSTM_UNTRAINED, LstmEngine, lstm_flat_layout
from recurrent_gaze_prediction_amd.models.gaze_lstm import GazePredictionLSTM, LSTM_RCN_Cell

sig = lambda v: 1.0 / (1.0 + np.exp(-v))


def t64(p):
    return {k: torch.as_tensor(np.asarray(v), dtype=torch.float64) for k, v in p.items()}


def test_names_and_shapes():
    p = syn.lstm_params(3)
    assert tuple(LSTM_PARAM_TO_FIELD) == ref.KEYS and len(ref.KEYS) == 18
    assert tuple(_lib.LstmWeights.FIELDS) == tuple(LSTM_PARAM_TO_FIELD.values())
    assert p['ConvLSTM_Wxi'].shape == (3, 3, 512, 128) and p['ConvLSTM_Wxi_1'].shape == (3, 3, 128, 128)
    assert p['ConvLSTM_Whc'].shape == (3, 3, 128, 128)
    for k in ('ConvLSTM_Wci', 'ConvLSTM_Wcf', 'ConvLSTM_Wco'):
        assert p[k].shape == (7, 7, 128)                         # per position, not per channel (gaze_lstm.py:68)
    cell = LSTM_RCN_Cell(128, 512)
    assert cell.state_size == 256 and cell.output_size == 128 and cell.zero_state(3).shape == (3, 7, 7, 256)
    assert np.abs(cell.W_hi).max() <= 2e-4 + 1e-9               # the reference's own init: truncated normal, stddev 1e-4
    assert GazePredictionLSTM.RNN_STATE_SIZE == 128 and GazePredictionLSTM.DIM_CNN_PROJ == 512


def test_torch_and_numpy_cells_agree():
    p = syn.lstm_params(5)
    rs = np.random.RandomState(6)
    x = rs.randn(7, 7, 512) * 0.5
    c = rs.randn(7, 7, 128) * 2.0
    h = np.tanh(rs.randn(7, 7, 128))
    a = ref.lstm_cell(torch.tensor(x)[None], torch.tensor(c)[None], torch.tensor(h)[None], t64(p))
    b = ref.lstm_cell_numpy(x, c, h, p)
    for k in 'ifgoch':
        assert np.abs(a[k][0].numpy() - b[k]).max() < 1e-12, k


def test_zero_weights_give_the_uniform_map():
    p = {k: np.zeros_like(v) for k, v in syn.lstm_params(1).items()}
    x = syn.c3d_features(2, 1, 2)
    logits, _ = ref.forward_f64(x, p)
    pr = ref.softmax_maps(torch.tensor(logits)).numpy()
    assert np.abs(pr - 1.0 / 2401).max() < 1e-15
    gt = np.full((1, 2, 49, 49), 1.0 / 2401)
    assert abs(ref.gaze_loss(torch.tensor(logits), torch.tensor(gt)).item() - math.log(2401)) < 1e-9


def test_first_step_from_the_zero_state():
    p = syn.lstm_params(7)
    x = syn.c3d_features(8, 1, 1)
    _, it = ref.forward_f64(x, p)
    e = torch.tensor(it['emb']).reshape(1, 7, 7, 512)
    q = t64(p)
    cv = lambda k: ref.conv2d_same(e, q[k]).numpy()
    c1 = sig(cv('ConvLSTM_Wxi')) * np.tanh(cv('ConvLSTM_Wxc'))
    h1 = np.tanh(c1) * sig(cv('ConvLSTM_Wxo'))
    assert np.abs(it['c'][:, 0] - c1).max() < 1e-13 and np.abs(it['h'][:, 0] - h1).max() < 1e-13


def test_quirk_w_hc_is_read_by_nothing():
    p = syn.lstm_params(9)
    x = syn.c3d_features(10, 2, 3)
    gt = syn.gaze_maps(11, 2, 3)[0]
    gt = gt / gt.sum((2, 3), keepdims=True)
    l0, z0, g0 = ref.loss_and_grads(x, gt, p)
    assert g0['ConvLSTM_Whc'] is None                           # tf.gradients: None; the textbook cell would give a tensor
    p2 = dict(p, ConvLSTM_Whc=p['ConvLSTM_Whc'] + 1.0)
    l1, z1, g1 = ref.loss_and_grads(x, gt, p2)
    assert l0 == l1 and np.array_equal(z0, z1)
    for k in ref.KEYS:
        if k != 'ConvLSTM_Whc':
            assert g0[k] is not None and np.abs(g0[k]).max() > 0 and np.array_equal(g0[k], g1[k]), k


def test_quirk_w_hi_feeds_the_cell_input():
    p = syn.lstm_params(12)
    x = syn.c3d_features(13, 1, 2)
    _, a = ref.forward_f64(x, p)
    _, b = ref.forward_f64(x, dict(p, ConvLSTM_Wxi_1=p['ConvLSTM_Wxi_1'] * 1.5))
    assert np.array_equal(a['g'][:, 0], b['g'][:, 0])           # step 1: h_0 = 0
    assert np.abs(a['g'][:, 1] - b['g'][:, 1]).max() > 1e-3     # step 2: g moves with W_hi alone (gaze_lstm.py:125)
    q = t64(p)
    e = torch.tensor(a['emb']).reshape(1, 2, 7, 7, 512)
    h1 = torch.tensor(a['h'][:, 0])
    g2 = torch.tanh(ref.conv2d_same(e[:, 1], q['ConvLSTM_Wxc']) + ref.conv2d_same(h1, q['ConvLSTM_Wxi_1'])).numpy()
    assert np.abs(a['g'][:, 1] - g2).max() < 1e-13


def test_quirk_output_gate_reads_the_old_c():
    p = syn.lstm_params(14)
    x = syn.c3d_features(15, 1, 2)
    _, a = ref.forward_f64(x, p)
    q = t64(p)
    e = torch.tensor(a['emb']).reshape(1, 2, 7, 7, 512)
    h1 = torch.tensor(a['h'][:, 0])
    pre = (ref.conv2d_same(e[:, 1], q['ConvLSTM_Wxo']) + ref.conv2d_same(h1, q['ConvLSTM_Wxo_1'])).numpy()
    wco = np.asarray(p['ConvLSTM_Wco'], np.float64)
    o_old = sig(pre + wco * a['c'][:, 0])
    o_new = sig(pre + wco * a['c'][:, 1])
    assert np.abs(a['o'][:, 1] - o_old).max() < 1e-13           # c_1 . W_co (gaze_lstm.py:130)
    assert np.abs(a['o'][:, 1] - o_new).max() > 1e-2            # ... not c_2 . W_co, the textbook peephole


def test_bf16_emulation_is_close_but_not_equal():
    p = syn.lstm_params(16)
    x = syn.c3d_features(17, 1, 3)
    _, a = ref.forward_f64(x, p)
    _, b = ref.forward_f64(x, p, emulate_bf16=True)
    fro, mx = ref.step_errors(b['h'], a['h'])
    assert (fro > 1e-4).all() and (fro < 2e-2).all() and mx < 5e-2


def test_checkpoint_names_round_trip():
    p = syn.lstm_params(18)
    tf_vars = checkpoint.export_model_variables('gaze_lstm', p)
    assert len(tf_vars) == 18
    cell = {'RGP/RCNBottom/ConvLSTM_' + s for s in ('Wxi', 'Wxi_1', 'Wci', 'Wxf', 'Wxf_1', 'Wcf', 'Wxc', 'Whc', 'Wxo', 'Wxo_1', 'Wco')}
    assert cell <= set(tf_vars) and {'RGP/proj_c3d_W', 'RGP/Upsampling/weight3', 'RGP/out_b'} <= set(tf_vars)
    assert np.array_equal(tf_vars['RGP/RCNBottom/ConvLSTM_Wxi_1'], p['ConvLSTM_Wxi_1'])       # = W_hi
    for v in (tf_vars, {k + ':0': a for k, a in tf_vars.items()}, {k[len('RGP/'):]: a for k, a in tf_vars.items()}):
        extra = dict(v)
        extra['RGP/RCNBottom/ConvLSTM_Wxi/Adam'] = np.zeros(1)
        extra['global_step'] = np.zeros(1)
        back = checkpoint.import_model_variables('gaze_lstm', extra)
        assert set(back) == set(p)
        for k in p:
            assert back[k].dtype == np.float32 and np.array_equal(back[k], p[k]), k
    with pytest.raises(KeyError, match='ConvLSTM_Whc'):          # carried although nothing reads it
        checkpoint.import_lstm_variables({k: v for k, v in tf_vars.items() if 'Whc' not in k})


def test_optimizer_layout_leaves_w_hc_out():
    p = syn.lstm_params(19)
    shapes = {k: v.shape for k, v in p.items()}
    layout = lstm_flat_layout(shapes)
    names = [k for k, _, _ in layout]
    assert LSTM_UNTRAINED == ('ConvLSTM_Whc',) and 'ConvLSTM_Whc' not in names
    assert names == [k for k in LSTM_PARAM_TO_FIELD if k != 'ConvLSTM_Whc'] and len(names) == 17
    off = 0
    for k, o, n in layout:                                       # dense, in order: what the clip norm and the optimizer see
        assert o == off and n == p[k].size
        off += n
    assert off == sum(v.size for k, v in p.items()) - p['ConvLSTM_Whc'].size


def test_plan_creation_and_validation_are_host_only():
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.rgp_lstm_create(ctypes.byref(h), 64, 16, _lib.RGP_BF16, 0) == 0, lib.rgp_last_error()
    ws = lib.rgp_lstm_workspace_bytes(h)
    assert ws > 64 * 16 * 49 * 1024 * 2
    assert lib.rgp_lstm_buffer_elems(h, b'h') == 64 * 16 * 49 * 128 == lib.rgp_lstm_buffer_elems(h, b'c')
    assert lib.rgp_lstm_buffer_elems(h, b'emb') == 64 * 16 * 49 * 512
    assert lib.rgp_lstm_buffer_elems(h, b'i') == 0 and lib.rgp_lstm_buffer_elems(h, b'nope') == 0     # gates: training plans
    assert lib.rgp_lstm_forward(h, None, None, None, None) == -3 and b'workspace' in lib.rgp_last_error()
    assert lib.rgp_lstm_backward(h, None, None, None, None, 0, None) == -3
    lib.rgp_lstm_destroy(h)
    assert lib.rgp_lstm_create(ctypes.byref(h), 8, 35, _lib.RGP_F32, _lib.RGP_LSTM_SAVE_FOR_BACKWARD) == 0
    assert lib.rgp_lstm_buffer_elems(h, b'o') == 8 * 35 * 49 * 128
    lib.rgp_lstm_destroy(h)
    bad = ctypes.c_void_p()
    assert lib.rgp_lstm_create(ctypes.byref(bad), 0, 16, _lib.RGP_BF16, 0) == -1
    assert lib.rgp_lstm_create(ctypes.byref(bad), 2, 2, 7, 0) == -1
    assert lib.rgp_lstm_create(ctypes.byref(bad), 2, 2, _lib.RGP_BF16, 8) == -1 and b'flags' in lib.rgp_last_error()
    assert lib.rgp_lstm_create(ctypes.byref(bad), 2, 2, _lib.RGP_F32, _lib.RGP_LSTM_PERSISTENT) == -1
    assert lib.rgp_lstm_create(ctypes.byref(bad), 65, 2, _lib.RGP_BF16, _lib.RGP_LSTM_PERSISTENT) == -1
    assert lib.rgp_lstm_create(ctypes.byref(bad), 2, 2, _lib.RGP_BF16, _lib.RGP_LSTM_PER_STEP | _lib.RGP_LSTM_PERSISTENT) == -1
    assert lib.rgp_lstm_create(ctypes.byref(h), 65, 2, _lib.RGP_BF16, 0) == 0        # more than 64 clips: per-step launches
    lib.rgp_lstm_destroy(h)


def test_engine_refuses_to_run_without_gpu():
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    with pytest.raises(_lib.RgpError):
        LstmEngine(1, 1)
