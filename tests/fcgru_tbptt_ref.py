"""Helpers of tests/test_fcgru_tbptt_cpu.py and tests/test_fcgru_tbptt_gpu.py: training across the carried state of the fc-GRU
(rgp_fcgru_backward_stream, FcGruEngine.backward_stream, GazePredictionGRU.train_long_clip).

* chunk_backward: a float64 numpy backward of ONE streaming call -- the first n_valid steps of a chunk started at h0, the loss of
  gaze_rnn.py:363-408 summed over the valid frames and divided by loss_frames, plus <d_state_out, state_out> -> the eight
  gradients and d loss / d h0.  Checked against float64 torch autograd on the CPU (test_fcgru_tbptt_cpu.py).  What lies behind
  n_valid is never looked at.
* film_backward: a film cut into chunks, the state carried forwards and (chain=True) its gradient backwards, the chunk gradients
  summed: equal to the gradient of the uncut film, chunk by chunk the reference of the device tests.
* Weights and features: tests/fcgru_stream_ref.py (update-gate bias + 1.5: the state matters).  Labels: normalised maps.
* seeded_view: the buffers of a seeded call in the form fcgru_bptt_ref.check / fcgru_f32_bptt_ref.check take (their bounds are
  imported by the tests, not restated): the first n_valid steps, the seed folded into dh_head of step n_valid - 1, where it enters.
* Tolerances of the gradients: those of tests/test_fcgru_gpu.py:71.
"""
import numpy as np

import fcgru_stream_ref as sref
from fcgru_stream_ref import N, NX, params, features, rel_err     # noqa: F401  (re-exported)
from recurrent_gaze_prediction_amd import _lib

# The entry this module is the reference of.  The lookup is not used: it is here so that importing this module fails on a package
# without the entry, which is what makes the pure-numpy tests of the reference (autograd agreement, composition) fail there too.
# Those tests run no code of the library and show nothing about it; they check the yardstick the device tests are held to.
BACKWARD_STREAM_ARGS = _lib.SIGNATURES['rgp_fcgru_backward_stream'][1]

FIELDS = ('proj_c3d_W', 'proj_c3d_b', 'gates_kernel', 'gates_bias', 'candidate_kernel', 'candidate_bias', 'proj_out_W', 'proj_out_b')
RECURRENT = FIELDS[:6]                        # the six variables on the recurrent path; the read-out pair sees no state gradient
GRAD_TOL = {'f32': 5e-4, 'bf16': 5e-2}        # tests/test_fcgru_gpu.py:71, relative error of the max
TRUNCATED_MISS = 0.3                          # a dropped chain misses the recurrent gradients by more than this share of their max
# the four plans of the GPU tests: (dtype, engine keywords)
PLANS = [('f32', {'per_step': True}), ('bf16', {'per_step': True}), ('bf16', {'per_step': True, 'bptt_persistent': True}),
         ('f32', {'per_step': True, 'bptt_persistent_f32': True})]
PLAN_IDS = ['f32-per_step', 'bf16-per_step', 'bf16-bptt_persistent', 'f32-bptt_persistent_f32']
_cache = {}


def labels(B, S, gh, seed=977):
    """Normalised maps [B,S,gh,gh] float32."""
    key = ('g', B, S, gh, seed)
    if key not in _cache:
        g = np.random.RandomState(seed + 13 * B + S).rand(B, S, gh, gh).astype(np.float32)
        _cache[key] = g / g.sum(axis=(2, 3), keepdims=True)
    return _cache[key]


def _sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def chunk_backward(x, p, labels, h0=None, d_state_out=None, n_valid=None, loss_frames=None, loss_type='xentropy'):
    """x [B,T,1024,7,7], labels [B,T,G...], h0 / d_state_out [B,N] or None = zeros -> (grads {field: float64}, d_state_in [B,N],
    state_out [B,N], loss).  Only steps t < n_valid are read."""
    f = lambda a: np.asarray(a, np.float64)
    B, T = x.shape[:2]
    nv = T if n_valid is None else int(n_valid)
    lf = float(B * nv if loss_frames is None else loss_frames)
    rows = np.ascontiguousarray(f(x[:, :nv]).transpose(0, 1, 3, 4, 2)).reshape(B, nv, 49, 1024)
    wp, bp = f(p['proj_c3d_W']), f(p['proj_c3d_b'])
    wg, bg, wc, bc = f(p['gates_kernel']), f(p['gates_bias']), f(p['candidate_kernel']), f(p['candidate_bias'])
    wo, bo = f(p['proj_out_W']), f(p['proj_out_b'])
    emb = (rows @ wp + bp).reshape(B, nv, NX)
    g = f(labels).reshape(B, labels.shape[1], -1)
    h = np.zeros((B, N)) if h0 is None else f(h0).reshape(B, N).copy()
    keep, loss = [], 0.0
    for t in range(nv):
        xin = np.concatenate([emb[:, t], h], 1)
        ru = _sigmoid(xin @ wg + bg)
        r, u = ru[:, :N], ru[:, N:]
        cin = np.concatenate([emb[:, t], r * h], 1)
        c = np.tanh(cin @ wc + bc)
        hn = u * h + (1.0 - u) * c
        z = hn @ wo + bo
        if loss_type == 'xentropy':
            zs = z - z.max(1, keepdims=True)
            lsm = zs - np.log(np.exp(zs).sum(1, keepdims=True))
            loss += -(g[:, t] * lsm).sum() / lf
            dz = (np.exp(lsm) * g[:, t].sum(1, keepdims=True) - g[:, t]) / lf
        else:
            loss += 0.5 * ((z - g[:, t]) ** 2).sum() / lf
            dz = (z - g[:, t]) / lf
        keep.append((xin, cin, h, r, u, c, hn, dz))
        h = hn
    state_out = h
    gr = {k: np.zeros_like(f(p[k])) for k in FIELDS}
    demb = np.zeros((B, nv, NX))
    carry = np.zeros((B, N)) if d_state_out is None else f(d_state_out).reshape(B, N).copy()
    for t in range(nv - 1, -1, -1):
        xin, cin, hp, r, u, c, hn, dz = keep[t]
        gr['proj_out_W'] += hn.T @ dz
        gr['proj_out_b'] += dz.sum(0)
        dh = dz @ wo.T + carry
        du, dc = dh * (hp - c), dh * (1.0 - u)
        carry = dh * u
        dcp = dc * (1.0 - c * c)
        gr['candidate_kernel'] += cin.T @ dcp
        gr['candidate_bias'] += dcp.sum(0)
        dcin = dcp @ wc.T
        demb[:, t] += dcin[:, :NX]
        drh = dcin[:, NX:]
        carry = carry + drh * r
        dru = np.concatenate([drh * hp * r * (1.0 - r), du * u * (1.0 - u)], 1)       # columns [r | u]
        gr['gates_kernel'] += xin.T @ dru
        gr['gates_bias'] += dru.sum(0)
        dxin = dru @ wg.T
        demb[:, t] += dxin[:, :NX]
        carry = carry + dxin[:, NX:]
    de = demb.reshape(B * nv * 49, 32)
    gr['proj_c3d_W'] = rows.reshape(-1, 1024).T @ de
    gr['proj_c3d_b'] = de.sum(0)
    return gr, carry, state_out, loss


def cuts_of(chunks):
    """(3, 3, 1) -> [(0, 3), (3, 3), (6, 1)]"""
    out, s = [], 0
    for n in chunks:
        out.append((s, n))
        s += n
    return out


def pad_chunk(a, s, n, T, value):
    """Steps [s, s + n) of a [B,S,...] as a [B,T,...] chunk, `value` (a scalar or an array [B,T-n,...]) behind n."""
    out = np.empty((a.shape[0], T) + a.shape[2:], a.dtype)
    out[:, :n] = a[:, s:s + n]
    out[:, n:] = value
    return out


def film_backward(x, p, g, chunks, T=None, chain=True, loss_type='xentropy', pad_x=7.0, pad_seed=None):
    """The film x [B,S,...] / g cut into `chunks` on a plan of T steps (default max(chunks)); features behind a chunk's n_valid are
    pad_x, labels random (pad_seed) or zero.  -> (summed grads, per chunk [(grads, d_state_in, h0, d_state_out)])."""
    B, S = x.shape[:2]
    T = max(chunks) if T is None else T
    rs = np.random.RandomState(pad_seed) if pad_seed is not None else None
    cuts = cuts_of(chunks)
    xs, gs, h0s, h = [], [], [], None
    for s, n in cuts:
        xs.append(pad_chunk(x, s, n, T, pad_x))
        gs.append(pad_chunk(g, s, n, T, rs.rand(B, T - n, *g.shape[2:]) if rs is not None else 0.0))
        h0s.append(h)
        h = chunk_backward(xs[-1], p, gs[-1], h0=h, n_valid=n, loss_frames=B * S, loss_type=loss_type)[2]
    total, per, d = None, [None] * len(cuts), None
    for i in reversed(range(len(cuts))):
        gr, d_in, _, _ = chunk_backward(xs[i], p, gs[i], h0=h0s[i], d_state_out=d if chain else None, n_valid=cuts[i][1],
                                        loss_frames=B * S, loss_type=loss_type)
        per[i] = (gr, d_in, h0s[i], d if chain else None)
        d = d_in
        total = gr if total is None else {k: total[k] + gr[k] for k in FIELDS}
    return total, per


def grad_errs(got, want):
    """{field: relative error of the max}"""
    return {k: rel_err(got[k], want[k]) for k in FIELDS}


def seeded_view(dev, seed, n_valid):
    """dev: fcgru_bptt_ref.BUFFERS of a call seeded with `seed` [B,N] (or None) over n_valid steps -> the buffers of the first
    n_valid steps with the seed added to dh_head of step n_valid - 1 (float64), for the plain pass's check()."""
    nv = int(n_valid)
    dhh = np.asarray(dev['dh_head'], np.float64)[:, :nv].copy()
    if seed is not None:
        dhh[:, nv - 1] += np.asarray(seed, np.float64).reshape(dhh.shape[0], N)
    return {'u': dev['u'][:nv], 'r': dev['r'][:nv], 'c': dev['c'][:nv], 'h': dev['h'][:nv + 1], 'dh_head': dhh,
            'dxpre': dev['dxpre'][:, :nv], 'dh0': dev['dh0']}
