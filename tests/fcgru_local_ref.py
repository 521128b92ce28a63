"""One-step float64 reference of the fc-GRU cell ON SUPPLIED OPERANDS (test helper of tests/test_fcgru_persistent_cpu.py and
tests/test_fcgru_persistent_gpu.py), in the style of recurrence_local_ref.py.

Given the device's OWN operand rows hp[t] (bf16 h_{t-1}), its own fp32 state h[t], its own xpre and its own gates, one step is a
short float64 computation whose only bf16 roundings are known exactly from the kernel source; products of bf16 operands are
exact in fp32 and both recurrence paths accumulate in fp32, so a bf16 plan must agree with this reference as closely as an f32
plan agrees with float64.  The step as both paths compose it (recurrent_gaze_prediction_amd/csrc: per step EpiGruZR / EpiGruC,
igemm.hip.h:250-305; persistent fcgru_seq.hip.h):
    u = sigmoid(xpre_u + hp W_u),  r = sigmoid(xpre_r + hp W_r)       W_* = bf16(h-side kernels), hp = the bf16 rows of h_{t-1}
    rh = bf16_rne(fp32 r * fp32 h_{t-1})                               ONE fp32 multiply of the fp32 gate and the fp32 state
    c = tanh(xpre_c + rh W_c)
    h_t = u h_{t-1} + (1 - u) c                                        from the device's own u, c, h_{t-1}
    hp[t+1] = bf16_rne(h_t)
Buffers as FcGruEngine.read_buffer returns them: xpre [B,T,3,n], h [T+1,B,n], u / r / c [T,B,n], hp [B,T+1,n], rh [B,T,n].

Bounds.  Gates: GATE_TOL = 5e-5, the project's fc-GRU f32 figure (tests/test_fcgru_gpu.py TOL['f32']), absolute: sigmoid' <= 1/4
and tanh' <= 1, so an error of the pre-activation is not amplified.  Blend: BLEND_TOL = 2^-22, a worst-case count of fp32
roundings for |h| < 1 (recurrence_local_ref.py).  bf16 buffers: equal to bf16_rne of the reference, at most FLIP_CAP = 1e-3 of the
elements exactly one ulp off.

Also here, so that the CPU test can validate bounds and sensitivity without a device: a stand-in "device" that runs the same
steps with fp32 products, K summed in four quarters as the kernel's four waves do, and the kernel's rounding sites, and that can
be told to make one of the mistakes of FAULTS.
"""
import numpy as np
import torch

from recurrent_gaze_prediction_amd import synthetic as syn
from recurrence_local_ref import bf16_ordinal, bf16_rne, bf16_trunc, sigmoid

GATE_TOL = 5e-5
BLEND_TOL = 2.0 ** -22
FLIP_CAP = 1e-3
N, NX, NP = 1617, 1568, 1664
UNITS = 8                      # units per member of the persistent launch (fcgru_seq.hip.h)
KQ = NP // 4                   # K quarter of a wave: 416 of the padded 1664

FAULTS = ('rh_trunc', 'rh_from_bf16_h', 'swap_ur', 'drop_k_quarter', 'next_clip_xpre', 'next_step_xpre', 'blend_swapped',
          'unit_shift')


def params(seed=161, gh=7):
    """syn.fcgru_params with the gate biases spread (as tests/test_fcgru_gpu.py does for the gradients): gates off 0.73."""
    p = syn.fcgru_params(seed, gh, gh)
    p['gates_bias'] = p['gates_bias'] + np.linspace(-0.3, 0.3, p['gates_bias'].size).astype(np.float32)
    return p


def features(B, T):
    return syn.c3d_features(163 + B, B, T)


def h_kernels(p, rnd=bf16_rne):
    """(W_u, W_r, W_c) [n, n]: the h-side rows of the TF kernels (gates_kernel columns [r | u]) as the operand dtype holds them."""
    g, c = np.asarray(p['gates_kernel']), np.asarray(p['candidate_kernel'])
    return rnd(g[NX:, N:]), rnd(g[NX:, :N]), rnd(c[NX:])


# ------------------------------------------------------------------------------------------------ comparisons
def _abs(got, ref, bound):
    d = np.abs(np.asarray(got, np.float64) - ref)
    i = np.unravel_index(int(np.argmax(d)), d.shape)
    return {'err': float(d[i]), 'bound': float(bound), 'where': tuple(int(k) for k in i), 'ratio': float(d[i] / bound)}


def _bf16(got, ref_before_store):
    o = bf16_ordinal(got).astype(np.int64)
    d = np.abs(o - bf16_ordinal(bf16_rne(ref_before_store)))
    off = float((d >= 1).mean())
    return {'err': float(d.max()), 'bound': 1.0, 'flips': off, 'cap': FLIP_CAP, 'n_flips': int((d >= 1).sum()), 'n': int(d.size),
            'ratio': max(float(d.max() > 1) * float(d.max()), off / FLIP_CAP)}


def check(dev, p):
    """dev: the buffers listed above (numpy) -> {tensor: figures} over every gate of every step."""
    wu, wr, wc = h_kernels(p)
    f32, f64 = (lambda a: np.asarray(a, np.float32)), (lambda a: np.asarray(a, np.float64))
    T = dev['u'].shape[0]
    hp = f64(dev['hp'])[:, :T].transpose(1, 0, 2)               # [T,B,n] operand rows of h_{t-1}
    xp = f64(dev['xpre']).transpose(1, 0, 2, 3)                 # [T,B,3,n]
    h_prev, h_next = dev['h'][:-1], dev['h'][1:]                # fp32 states in front of / behind each step
    out = {}
    out['u'] = _abs(dev['u'], sigmoid(xp[:, :, 0] + hp @ wu), GATE_TOL)
    out['r'] = _abs(dev['r'], sigmoid(xp[:, :, 1] + hp @ wr), GATE_TOL)
    out['rh'] = _bf16(f64(dev['rh']).transpose(1, 0, 2), f32(dev['r']) * f32(h_prev))
    out['c'] = _abs(dev['c'], np.tanh(xp[:, :, 2] + f64(dev['rh']).transpose(1, 0, 2) @ wc), GATE_TOL)
    u, c = f64(dev['u']), f64(dev['c'])
    out['h'] = _abs(h_next, u * f64(h_prev) + (1.0 - u) * c, BLEND_TOL)
    out['hp'] = _bf16(f64(dev['hp'])[:, 1:].transpose(1, 0, 2), f32(h_next))
    out['hp0'] = _abs(f64(dev['hp'])[:, 0], 0.0, 1e-30)         # slot (b, 0): h_0 = 0, untouched
    return out


def violations(errs, margin=1.0):
    """Names of the tensors whose figures are not within 1 / margin of their bounds."""
    bad = []
    for k, e in errs.items():
        ok = (e['err'] <= 1 and e['flips'] * margin <= e['cap']) if 'flips' in e else e['err'] * margin <= e['bound']
        if not ok:
            bad.append(k)
    return bad


def report(tag, errs):
    for k, e in errs.items():
        if 'flips' in e:
            print('%s %s: %d of %d not the rounded reference (cap %.2f %%), worst %d ulp' % (tag, k, e['n_flips'], e['n'], 100 * e['cap'], e['err']))
        else:
            print('%s %s: %.3e (bound %.3e, share %.3f) at %s' % (tag, k, e['err'], e['bound'], e['ratio'], e['where']))


# ------------------------------------------------------------------------------------------------ the stand-in device
def _mm32(a, w):
    return (torch.as_tensor(np.ascontiguousarray(a, np.float32)) @ torch.as_tensor(np.ascontiguousarray(w, np.float32))).numpy()


def _quarters(a, w, drop=None):
    """a [B,n] x w [n,m] in fp32, K summed in the four quarters of the padded 1664 (one per wave), then across them."""
    s = np.zeros((a.shape[0], w.shape[1]), np.float32)
    for q in range(4):
        if q != drop:
            s = (s + _mm32(a[:, q * KQ:(q + 1) * KQ], w[q * KQ:(q + 1) * KQ])).astype(np.float32)
    return s


def _sig32(v):
    v = np.asarray(v, np.float32)
    return (np.float32(1) / (np.float32(1) + np.exp(-v))).astype(np.float32)


def _bf(v):
    return bf16_rne(np.asarray(v, np.float32)).astype(np.float32)


def standin_xpre(x, p):
    """[B,T,1024,7,7] -> xpre [B,T,3,n] fp32 as forward_impl composes it: bf16 rows x bf16 projection + bias, stored bf16,
    flattened to 49*32, x bf16 x-side kernels + biases, fp32."""
    B, T = x.shape[:2]
    rows = np.ascontiguousarray(np.asarray(x).transpose(0, 1, 3, 4, 2)).reshape(-1, 1024)
    emb = _bf(_mm32(_bf(rows), _bf(p['proj_c3d_W'])) + np.asarray(p['proj_c3d_b'], np.float32)).reshape(B * T, NX)
    g, c = np.asarray(p['gates_kernel']), np.asarray(p['candidate_kernel'])
    gb, cb = np.asarray(p['gates_bias'], np.float32), np.asarray(p['candidate_bias'], np.float32)
    xu = _mm32(emb, _bf(g[:NX, N:])) + gb[N:]
    xr = _mm32(emb, _bf(g[:NX, :N])) + gb[:N]
    xc = _mm32(emb, _bf(c[:NX])) + cb
    return np.stack([xu, xr, xc], 1).reshape(B, T, 3, N).astype(np.float32)


def standin(x, p, fault=None):
    """The recurrence with fp32 products -> dev dict as check takes it.  fault: one of FAULTS."""
    assert fault is None or fault in FAULTS
    B, T = x.shape[:2]
    xpre = standin_xpre(x, p)
    wu, wr, wc = (w.astype(np.float32) for w in h_kernels(p))
    one = np.float32(1)
    h = np.zeros((B, N), np.float32)
    hp = np.zeros((B, T + 1, N), np.float32)
    dev = {k: [] for k in ('u', 'r', 'c', 'h', 'rh')}
    dev['h'].append(h)
    for t in range(T):
        xp = xpre[:, t].copy()
        if fault == 'next_clip_xpre':
            xp[0] = xpre[1 % B, t]
        if fault == 'next_step_xpre':
            xp = xpre[:, (t + 1) % T].copy()
        drop = 2 if fault == 'drop_k_quarter' else None
        su, sr = _quarters(hp[:, t], wu, drop), _quarters(hp[:, t], wr, drop)
        if fault == 'swap_ur':
            su, sr = sr, su
        u, r = _sig32(su + xp[:, 0]), _sig32(sr + xp[:, 1])
        if fault == 'rh_trunc':
            rh = bf16_trunc(r * h).astype(np.float32)
        elif fault == 'rh_from_bf16_h':
            rh = _bf(r * hp[:, t])
        else:
            rh = _bf(r * h)
        c = np.tanh((_quarters(rh, wc) + xp[:, 2]).astype(np.float32)).astype(np.float32)
        if fault == 'blend_swapped':
            hn = ((one - u) * h + u * c).astype(np.float32)
        else:
            hn = (u * h + (one - u) * c).astype(np.float32)
        row = _bf(hn)
        if fault == 'unit_shift':                                # member 5 publishes its 8 units one slot further on
            row = row.copy()
            row[:, 6 * UNITS:7 * UNITS] = row[:, 5 * UNITS:6 * UNITS]
            row[:, 5 * UNITS:6 * UNITS] = hp[:, t, 5 * UNITS:6 * UNITS]
        hp[:, t + 1] = row
        for k, v in (('u', u), ('r', r), ('c', c), ('h', hn), ('rh', rh)):
            dev[k].append(v)
        h = hn
    out = {k: np.stack(v, 0) for k, v in dev.items()}
    out['rh'] = np.ascontiguousarray(out['rh'].transpose(1, 0, 2))
    out['hp'], out['xpre'] = hp, xpre
    return out
