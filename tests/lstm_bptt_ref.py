"""float64 restatement of the ConvLSTM's backward-through-time pass in the form the persistent kernel runs it
(csrc/convlstm_bptt.hip.h; test helper next to tests/lstm_ref.py, whose forward supplies the saved gates and states).

Two carries, three gradient blocks, one convolution per step, t = T-1 .. 0:
    dh  = dh_head[:, t] + carry_h           tc = tanh(c_t)
    d_o = dh tc o(1-o)                      dc = carry_c + dh o (1 - tc^2)
    d_i = dc g i(1-i)    d_f = dc c_{t-1} f(1-f)    d_g = dc i (1 - g^2)
    carry_c = dc f + d_i W_ci + d_f W_cf + d_o W_co          (all three peepholes read the OLD c, gaze_lstm.py:117,121,130)
    carry_h = conv3x3([d_i + d_g | d_f | d_o]; rot180 [W_hi | W_hf | W_ho]^T)       (:125: g reuses W_hi)
dh_head is the gradient reaching h_t from the head alone (autograd on the head, h detached).  d_i .. d_o are the gradients
of the gates' pre-activations; the gradients of the eleven cell variables follow from them without any further recurrence.

MUTATIONS names five wrong versions of the recurrence (what a kernel could plausibly get wrong); bptt(mutation=...) runs one,
and tests/test_lstm_bptt_cpu.py checks that each moves d_i .. d_o far enough for the GPU comparisons to see it.
"""
import numpy as np
import torch

import lstm_ref as ref
from oracle.torch_ref import conv2d_same, conv2d_transpose, gaze_loss

MUTATIONS = ('g_left_out_of_hi_block', 'o_peephole_on_new_c', 'peephole_term_missing', 'carry_c_without_dc_f', 'parity_swapped')
GATES = ('d_i', 'd_f', 'd_g', 'd_o')


def saved_and_head_grad(x, gt, params, loss_type='xentropy'):
    """numpy in -> ({'i','f','g','o','c','h': [B,T,7,7,128], 'emb': [B,T,7,7,512]} float64 tensors, dh_head [B,T,7,7,128])."""
    p = ref._params(params)
    xt = torch.as_tensor(np.asarray(x), dtype=torch.float64)
    b, t = xt.shape[:2]
    with torch.no_grad():
        _, inter = ref.lstm_forward(xt, p, True)
    inter['emb'] = inter['emb'].reshape(b, t, 7, 7, -1)
    h = inter['h'].clone().requires_grad_(True)
    y = conv2d_transpose(h.reshape(b * t, 7, 7, -1), p['weight1'], 3, 'VALID')       # the head, lstm_ref.lstm_forward's lines
    y = conv2d_transpose(y, p['weight2'], 2, 'VALID')
    y = conv2d_transpose(y, p['weight3'], 1, 'SAME')
    logits = (y.reshape(-1, y.shape[-1]) @ p['out_W'] + p['out_b']).reshape(b, t, 49, 49)
    gaze_loss(logits, torch.as_tensor(np.asarray(gt), dtype=torch.float64), loss_type).backward()
    return inter, h.grad.detach()


def _dgrad_filter(p):
    """rot180 [W_hi | W_hf | W_ho]^T as one HWIO filter [3,3,384,128] on the concatenated gradient blocks."""
    blocks = [p[k].flip(0, 1).transpose(2, 3) for k in ('ConvLSTM_Wxi_1', 'ConvLSTM_Wxf_1', 'ConvLSTM_Wxo_1')]
    return torch.cat(blocks, 2)


def bptt(saved, dh_head, params, mutation=None):
    """-> {'d_i','d_f','d_g','d_o': [B,T,7,7,128]} float64 tensors.  mutation: None or one of MUTATIONS."""
    assert mutation is None or mutation in MUTATIONS, mutation
    p = ref._params(params)
    w_ci, w_cf, w_co = p['ConvLSTM_Wci'], p['ConvLSTM_Wcf'], p['ConvLSTM_Wco']
    wd = _dgrad_filter(p)
    b, t_ = dh_head.shape[:2]
    zero = torch.zeros_like(dh_head[:, 0])
    carry_h, carry_c = zero, zero
    convs = {}                                             # step -> the convolution it produced (the carry meant for step - 1)
    out = {k: [None] * t_ for k in GATES}
    for t in range(t_ - 1, -1, -1):
        i, f, g, o = (saved[k][:, t] for k in 'ifgo')
        c_prev = saved['c'][:, t - 1] if t > 0 else zero
        tc = torch.tanh(saved['c'][:, t])
        if mutation == 'parity_swapped':                   # the exchange image of the other parity: step t + 2's hand-off
            carry_h = convs.get(t + 2, zero)
        dh = dh_head[:, t] + carry_h
        d_o = dh * tc * o * (1 - o)
        dc = carry_c + dh * o * (1 - tc * tc)
        if mutation == 'o_peephole_on_new_c':
            dc = dc + d_o * w_co
        d_i = dc * g * i * (1 - i)
        d_f = dc * c_prev * f * (1 - f)
        d_g = dc * i * (1 - g * g)
        carry_c = d_i * w_ci + d_o * w_co
        if mutation == 'o_peephole_on_new_c':
            carry_c = d_i * w_ci
        if mutation != 'peephole_term_missing':
            carry_c = carry_c + d_f * w_cf
        if mutation != 'carry_c_without_dc_f':
            carry_c = carry_c + dc * f
        blk0 = d_i if mutation == 'g_left_out_of_hi_block' else d_i + d_g
        carry_h = conv2d_same(torch.cat([blk0, d_f, d_o], -1), wd)
        convs[t] = carry_h
        for k, v in zip(GATES, (d_i, d_f, d_g, d_o)):
            out[k][t] = v
    return {k: torch.stack(v, 1) for k, v in out.items()}


def _wgrad(x, dy):
    """x [N,7,7,Cin], dy [N,7,7,Cout] -> d W [3,3,Cin,Cout] of y = conv2d_same(x, W)."""
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    return torch.stack([torch.stack([torch.einsum('nyxi,nyxo->io', xp[:, ky:ky + 7, kx:kx + 7], dy) for kx in range(3)])
                        for ky in range(3)])


def cell_grads(saved, d):
    """The gradients d_i .. d_o imply for the eleven cell variables (lstm_ref.CELL names; W_hc: None, nothing reads it)."""
    b, t_ = d['d_i'].shape[:2]
    flat = lambda v: v.reshape(b * t_, 7, 7, -1)
    zero = torch.zeros_like(saved['h'][:, :1])
    h_prev = flat(torch.cat([zero, saved['h'][:, :-1]], 1))
    c_prev = torch.cat([zero, saved['c'][:, :-1]], 1)
    e = flat(saved['emb'])
    g = {'ConvLSTM_Wxi': _wgrad(e, flat(d['d_i'])), 'ConvLSTM_Wxf': _wgrad(e, flat(d['d_f'])),
         'ConvLSTM_Wxc': _wgrad(e, flat(d['d_g'])), 'ConvLSTM_Wxo': _wgrad(e, flat(d['d_o'])),
         'ConvLSTM_Wxi_1': _wgrad(h_prev, flat(d['d_i'] + d['d_g'])), 'ConvLSTM_Wxf_1': _wgrad(h_prev, flat(d['d_f'])),
         'ConvLSTM_Wxo_1': _wgrad(h_prev, flat(d['d_o'])),
         'ConvLSTM_Wci': (d['d_i'] * c_prev).sum((0, 1)), 'ConvLSTM_Wcf': (d['d_f'] * c_prev).sum((0, 1)),
         'ConvLSTM_Wco': (d['d_o'] * c_prev).sum((0, 1)), 'ConvLSTM_Whc': None}
    return {k: (None if v is None else v.numpy()) for k, v in g.items()}


def fro(a, r):
    a, r = np.asarray(a, np.float64), np.asarray(r, np.float64)
    return np.linalg.norm(a - r) / max(np.linalg.norm(r), 1e-300)


def step_fro(a, r):
    """a, r [B,T,...] -> relative Frobenius distance per step [T]."""
    return ref.step_errors(a, r)[0]
