"""Helpers of tests/test_grcn_tbptt_cpu.py and tests/test_grcn_tbptt_gpu.py: training across the carried state of gaze_grcn
(rgp_grcn_backward_stream, GrcnEngine.backward_stream, train_long_clip on a GrcnEngine).

* chunk_backward: float64 torch autograd of ONE streaming call, built from oracle.torch_ref (grcn_cell, conv2d_transpose) --
  the forward from a state h0 (requires_grad) over the first n_valid steps, step t through batch-norm slot (phase + t) % T, the
  loss of gaze_rnn.py:363-408 summed over the valid frames and divided by loss_frames, plus <d_state_out, h_{n_valid}> -> the
  gradients w.r.t. the fifteen variables and h0.  What lies behind n_valid is never looked at.
* film_backward: a film cut into chunks, the state carried forwards and (chain=True) its gradient backwards, the chunk
  gradients summed.
* Parameters: tests/stream_ref.params('grcn', T) (batch-norm rows random per timestep: with the identity a wrong slot is
  invisible; gru_std 0.05: the state matters).  Labels: normalised maps.
* Tolerances of the gradients: those of tests/test_backward_gpu.py (per-tensor relative Frobenius error).
"""
import math

import numpy as np
import torch

import stream_ref
from oracle import torch_ref
from recurrent_gaze_prediction_amd import _lib
from recurrent_gaze_prediction_amd import synthetic as syn

# The entry this module is the reference of.  The lookup is not used: it is here so that importing this module fails on a package
# without the entry, which is what makes the pure-torch tests of the reference (composition, padding) fail there too.
BACKWARD_STREAM_ARGS = _lib.SIGNATURES['rgp_grcn_backward_stream'][1]

FIELDS = ('proj_c3d_W', 'proj_c3d_b', 'GRU_Conv_Wz', 'GRU_Conv_Uz', 'GRU_Conv_Wr', 'GRU_Conv_Ur', 'GRU_Conv_W', 'GRU_Conv_U',
          'weight1', 'weight2', 'weight3', 'out_W', 'out_b', 'bn_gamma', 'bn_beta')
RECURRENT = FIELDS[:8]                        # the projection and the six ConvGRU filters: what a state gradient reaches
TOL = {'f32': 2e-4, 'bf16': 3e-2}             # tests/test_backward_gpu.py:15
# (dtype, engine keywords) of the three plans of the GPU tests
PLANS = [('f32', {'per_step': False}), ('bf16', {'per_step': True}), ('bf16', {'per_step': False})]
PLAN_IDS = ['f32-per_step', 'bf16-per_step', 'bf16-persistent']
S = 128
_cache = {}


def params(T):
    return stream_ref.params('grcn', T)


def features(B, n, seed=311):
    key = ('x', B, n, seed)
    if key not in _cache:
        _cache[key] = syn.c3d_features(seed + B, B, n)
    return _cache[key]


def labels(B, n, seed=977):
    """Normalised maps [B,n,49,49] float32."""
    key = ('g', B, n, seed)
    if key not in _cache:
        g = np.random.RandomState(seed + 13 * B + n).rand(B, n, 49, 49).astype(np.float32)
        _cache[key] = g / g.sum(axis=(2, 3), keepdims=True)
    return _cache[key]


def fro_err(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(a - ref) / max(np.linalg.norm(ref), 1e-30))


def max_err(a, ref):
    """Largest difference as a share of the reference's largest magnitude."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30))


def chunk_backward(x, p, g, h0=None, d_state_out=None, n_valid=None, phase=0, loss_frames=None, loss_type='xentropy',
                   slots=None, forward_only=False):
    """x [B,T,1024,7,7], g [B,T,49,49], h0 / d_state_out [B,7,7,S] or None = zeros; step t uses batch-norm row
    (phase + t) % len(bn_gamma) (slots: an explicit list of rows instead) -> (grads {field: float64 array}, d_state_in,
    state_out, loss), all numpy float64 (forward_only: grads and d_state_in are None).  Only steps t < n_valid are read."""
    t64 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    B, T = x.shape[:2]
    nv = T if n_valid is None else int(n_valid)
    lf = float(B * nv if loss_frames is None else loss_frames)
    q = {k: t64(p[k]).clone().requires_grad_(True) for k in FIELDS}
    nbn = q['bn_gamma'].shape[0]
    h_in = (torch.zeros(B, 7, 7, S, dtype=torch.float64) if h0 is None else t64(h0).reshape(B, 7, 7, S).clone()).requires_grad_(True)
    xr = t64(x[:, :nv]).permute(0, 1, 3, 4, 2)
    emb = (xr.reshape(-1, 1024) @ q['proj_c3d_W'] + q['proj_c3d_b']).reshape(B, nv, 7, 7, -1)
    gg = t64(g[:, :nv]).reshape(B, nv, 2401)
    inv = 1.0 / math.sqrt(1.0 + torch_ref.BN_EPS)
    h, tot = h_in, 0.0
    for t in range(nv):
        h = torch_ref.grcn_cell(emb[:, t], h, q)
        slot = slots[t] if slots is not None else (phase + t) % nbn
        y = q['bn_gamma'][slot] * h * inv + q['bn_beta'][slot]
        y = torch_ref.conv2d_transpose(y, q['weight1'], 3, 'VALID')
        y = torch_ref.conv2d_transpose(y, q['weight2'], 2, 'VALID')
        y = torch_ref.conv2d_transpose(y, q['weight3'], 1, 'SAME')
        z = (y.reshape(-1, y.shape[-1]) @ q['out_W'] + q['out_b']).reshape(B, 2401)
        if loss_type == 'xentropy':
            tot = tot - (gg[:, t] * torch.log_softmax(z, -1)).sum()
        else:
            tot = tot + 0.5 * ((z - gg[:, t]) ** 2).sum()
    loss = tot / lf
    if forward_only:
        return None, None, h.detach().numpy().copy(), float(loss.item())
    obj = loss
    if d_state_out is not None:
        obj = obj + (t64(d_state_out).reshape(B, 7, 7, S) * h).sum()
    obj.backward()
    grads = {k: (q[k].grad if q[k].grad is not None else torch.zeros_like(q[k])).numpy().copy() for k in FIELDS}
    return grads, h_in.grad.numpy().copy(), h.detach().numpy().copy(), float(loss.item())


def cuts_of(chunks):
    """(3, 3, 1) -> [(0, 3), (3, 3), (6, 1)]"""
    out, s = [], 0
    for n in chunks:
        out.append((s, n))
        s += n
    return out


def pad_chunk(a, s, n, T, value):
    """Steps [s, s + n) of a [B,N,...] as a [B,T,...] chunk, `value` (a scalar or an array [B,T-n,...]) behind n."""
    out = np.empty((a.shape[0], T) + a.shape[2:], a.dtype)
    out[:, :n] = a[:, s:s + n]
    out[:, n:] = value
    return out


def film_backward(x, p, g, chunks, T, chain=True, loss_type='xentropy', pad_x=7.0, pad_seed=None):
    """The film x [B,N,...] / g cut into `chunks` on a plan of T steps; chunk at film step s runs with phase s % T; features
    behind a chunk's n_valid are pad_x, labels random (pad_seed) or zero.
    -> (summed grads, per chunk [(grads, d_state_in, h0, d_state_out, x chunk, g chunk, phase)])."""
    B, N = x.shape[:2]
    rs = np.random.RandomState(pad_seed) if pad_seed is not None else None
    cuts = cuts_of(chunks)
    xs, gs, h0s, h = [], [], [], None
    for s, n in cuts:
        xs.append(pad_chunk(x, s, n, T, pad_x))
        gs.append(pad_chunk(g, s, n, T, rs.rand(B, T - n, *g.shape[2:]).astype(g.dtype) if rs is not None else 0.0))
        h0s.append(h)
        h = chunk_backward(xs[-1], p, gs[-1], h0=h, n_valid=n, phase=s % T, loss_frames=B * N, loss_type=loss_type)[2]
    total, per, d = None, [None] * len(cuts), None
    for i in reversed(range(len(cuts))):
        s, n = cuts[i]
        gr, d_in, _, _ = chunk_backward(xs[i], p, gs[i], h0=h0s[i], d_state_out=d if chain else None, n_valid=n, phase=s % T,
                                        loss_frames=B * N, loss_type=loss_type)
        per[i] = (gr, d_in, h0s[i], d if chain else None, xs[i], gs[i], s % T)
        d = d_in
        total = gr if total is None else {k: total[k] + gr[k] for k in FIELDS}
    return total, per


def uncut_backward(x, p, g, T, loss_type='xentropy'):
    """Autograd of the uncut film: one chunk of N steps from zero, batch-norm row s % T for film step s."""
    N = x.shape[1]
    return chunk_backward(x, p, g, n_valid=N, loss_type=loss_type, slots=[s % T for s in range(N)])


def grad_errs(got, want, err=fro_err, skip=()):
    return {k: err(got[k], want[k]) for k in FIELDS if k not in skip}
