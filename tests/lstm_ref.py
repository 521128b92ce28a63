"""torch-CPU restatement of gaze_lstm, the ConvLSTM member of the gaze family (test helper, built from the oracle's operators).

Reference lines followed: /root/reference/models/gaze_lstm.py
  projection                 :230-250   (both tf.nn.dropout sites :246-247, :342 are inert: __init__ :161-175 builds the graph
                                         through the parent and rebinds the placeholder afterwards)
  LSTM_RCN_Cell.__call__     :112-133   as written: :125 reuses W_hi for the cell input, :130 feeds the OLD c to the output
                                         gate's peephole, W_hc (:80) is read by nothing; zero_state :136-148, state = [c, h]
  unrolling                  :263-286
  the three transposed convs :312-339, out_W / out_b :341
softmax and loss are GazePredictionGRU's (gaze_rnn.py:149-159, 363-408): oracle.torch_ref.softmax_maps / gaze_loss.

Three forms: float64 torch (autograd gives the gradients), the cell in plain numpy loops, and a bf16-operand emulation of
the forward (x, the projection output, h and every filter rounded to bf16 before each contraction, everything else float64)
-- the yardstick of the bf16 bounds in tests/test_lstm_gpu.py.
"""
import numpy as np
import torch

from oracle.torch_ref import conv2d_same, conv2d_transpose, gaze_loss, softmax_maps  # noqa: F401

CELL = ('ConvLSTM_Wxi', 'ConvLSTM_Wxi_1', 'ConvLSTM_Wci', 'ConvLSTM_Wxf', 'ConvLSTM_Wxf_1', 'ConvLSTM_Wcf',
        'ConvLSTM_Wxc', 'ConvLSTM_Whc', 'ConvLSTM_Wxo', 'ConvLSTM_Wxo_1', 'ConvLSTM_Wco')
KEYS = ('proj_c3d_W', 'proj_c3d_b') + CELL + ('weight1', 'weight2', 'weight3', 'out_W', 'out_b')
# TF's unique names -> the attribute names of LSTM_RCN_Cell (gaze_lstm.py:64-88)
ATTR = {'ConvLSTM_Wxi': 'W_xi', 'ConvLSTM_Wxi_1': 'W_hi', 'ConvLSTM_Wci': 'W_ci', 'ConvLSTM_Wxf': 'W_xf', 'ConvLSTM_Wxf_1': 'W_hf',
        'ConvLSTM_Wcf': 'W_cf', 'ConvLSTM_Wxc': 'W_xc', 'ConvLSTM_Whc': 'W_hc', 'ConvLSTM_Wxo': 'W_xo', 'ConvLSTM_Wxo_1': 'W_ho',
        'ConvLSTM_Wco': 'W_co'}


def bf16(x):
    """Round a float64 tensor to bf16 (round to nearest even) and return it as float64."""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def lstm_cell(x, c, h, p, rnd=None):
    """gaze_lstm.py:112-133 on NHWC tensors -> dict(i, f, g, o, c, h) of the new step.  rnd: operand rounding (bf16 emulation)."""
    q = rnd if rnd is not None else (lambda v: v)
    w = {a: p[k] for k, a in ATTR.items()}
    hh = q(h)
    hi = conv2d_same(hh, q(w['W_hi']))
    i = torch.sigmoid(conv2d_same(x, q(w['W_xi'])) + hi + w['W_ci'] * c)
    f = torch.sigmoid(conv2d_same(x, q(w['W_xf'])) + conv2d_same(hh, q(w['W_hf'])) + w['W_cf'] * c)
    g = torch.tanh(conv2d_same(x, q(w['W_xc'])) + hi)                            # :125: W_hi, not W_hc
    new_c = f * c + i * g
    o = torch.sigmoid(conv2d_same(x, q(w['W_xo'])) + conv2d_same(hh, q(w['W_ho'])) + w['W_co'] * c)   # :130: the old c
    new_h = torch.tanh(new_c) * o
    return {'i': i, 'f': f, 'g': g, 'o': o, 'c': new_c, 'h': new_h}


def lstm_forward(c3d_input, p, want=False, emulate_bf16=False):
    """c3d_input [B,T,1024,7,7], p keyed by KEYS -> logits [B,T,49,49] (+ dict of emb [B*T*49,512] and i, f, g, o, c, h
    [B,T,7,7,128] when want)."""
    q = bf16 if emulate_bf16 else (lambda v: v)
    b, t = c3d_input.shape[:2]
    xr = q(c3d_input.permute(0, 1, 3, 4, 2))
    emb = (xr.reshape(-1, 1024) @ q(p['proj_c3d_W']) + p['proj_c3d_b'])
    e5 = q(emb).reshape(b, t, 7, 7, -1)
    s = p['ConvLSTM_Wxi'].shape[-1]
    c = torch.zeros(b, 7, 7, s, dtype=c3d_input.dtype)
    h = torch.zeros(b, 7, 7, s, dtype=c3d_input.dtype)
    steps = {k: [] for k in 'ifgoch'}
    for k in range(t):
        out = lstm_cell(e5[:, k], c, h, p, q if emulate_bf16 else None)
        c, h = out['c'], out['h']
        for name in steps:
            steps[name].append(out[name])
    hs = torch.stack(steps['h'], 1).reshape(b * t, 7, 7, s)
    y = conv2d_transpose(q(hs), q(p['weight1']), 3, 'VALID')
    y = conv2d_transpose(y, q(p['weight2']), 2, 'VALID')
    y = conv2d_transpose(y, q(p['weight3']), 1, 'SAME')
    logits = (y.reshape(-1, y.shape[-1]) @ p['out_W'] + p['out_b']).reshape(b, t, 49, 49)
    if not want:
        return logits
    inter = {k: torch.stack(v, 1) for k, v in steps.items()}
    inter['emb'] = emb
    return logits, inter


def _params(params, grad=False):
    return {k: torch.as_tensor(np.asarray(params[k]), dtype=torch.float64).clone().requires_grad_(grad) for k in KEYS}


def forward_f64(x, params, emulate_bf16=False):
    """numpy in -> (float64 logits, {name: float64 array}) out."""
    with torch.no_grad():
        logits, inter = lstm_forward(torch.as_tensor(np.asarray(x), dtype=torch.float64), _params(params), True, emulate_bf16)
    return logits.numpy(), {k: v.numpy() for k, v in inter.items()}


def loss_and_grads(x, gt, params, loss_type='xentropy', want_input_grad=False):
    """loss + d loss / d params (and d loss / d c3d_input) by float64 autograd; the gradient of a variable without a path to
    the loss is None (tf.gradients' answer too, base.py:278-281)."""
    p = _params(params, True)
    xt = torch.as_tensor(np.asarray(x), dtype=torch.float64).clone().requires_grad_(want_input_grad)
    logits = lstm_forward(xt, p)
    ls = gaze_loss(logits, torch.as_tensor(np.asarray(gt), dtype=torch.float64), loss_type)
    ls.backward()
    grads = {k: (None if v.grad is None else v.grad.detach().numpy()) for k, v in p.items()}
    if want_input_grad:
        grads['c3d_input'] = xt.grad.detach().numpy()
    return ls.item(), logits.detach().numpy(), grads


# ---- the cell once more, in plain numpy loops (no library convolution) ----
def _conv_same_np(x, w):
    """x [H,W,Cin], w [3,3,Cin,Cout] -> [H,W,Cout]; tf.nn.conv2d SAME, stride 1 (cross-correlation)."""
    hh, ww = x.shape[:2]
    out = np.zeros((hh, ww, w.shape[-1]))
    for y in range(hh):
        for xx in range(ww):
            for ky in range(3):
                for kx in range(3):
                    yy, xs = y + ky - 1, xx + kx - 1
                    if 0 <= yy < hh and 0 <= xs < ww:
                        out[y, xx] += x[yy, xs] @ w[ky, kx]
    return out


def lstm_cell_numpy(x, c, h, params):
    """One clip: x [7,7,512], c / h [7,7,128] float64 -> dict as lstm_cell."""
    w = {a: np.asarray(params[k], np.float64) for k, a in ATTR.items()}
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    hi = _conv_same_np(h, w['W_hi'])
    i = sig(_conv_same_np(x, w['W_xi']) + hi + w['W_ci'] * c)
    f = sig(_conv_same_np(x, w['W_xf']) + _conv_same_np(h, w['W_hf']) + w['W_cf'] * c)
    g = np.tanh(_conv_same_np(x, w['W_xc']) + hi)
    new_c = f * c + i * g
    o = sig(_conv_same_np(x, w['W_xo']) + _conv_same_np(h, w['W_ho']) + w['W_co'] * c)
    return {'i': i, 'f': f, 'g': g, 'o': o, 'c': new_c, 'h': np.tanh(new_c) * o}


def step_errors(a, ref_):
    """a, ref_ [B,T,...] -> (relative Frobenius error per step [T], max-abs error / max|ref| over everything)."""
    a, ref_ = np.asarray(a, np.float64), np.asarray(ref_, np.float64)
    t = a.shape[1]
    d = (a - ref_).transpose(1, 0, *range(2, a.ndim)).reshape(t, -1)
    r = ref_.transpose(1, 0, *range(2, a.ndim)).reshape(t, -1)
    fro = np.sqrt((d ** 2).sum(1)) / np.maximum(np.sqrt((r ** 2).sum(1)), 1e-300)
    return fro, np.abs(d).max() / max(np.abs(r).max(), 1e-300)
