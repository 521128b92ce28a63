"""Float64 reference of the fc-GRU backward-through-time pass ON THE DEVICE'S OWN BUFFERS (test helper of
tests/test_fcgru_bptt_cpu.py and tests/test_fcgru_bptt_gpu.py), built on fcgru_local_ref.py.

Both BPTT paths of the library (per step: fc_bwd1_kernel, the b_c GEMM, fc_bwd2_kernel, the b_zr GEMM of
recurrent_gaze_prediction_amd/csrc/rgp_fcgru.hip; persistent: csrc/fcgru_bptt.hip.h) compose step t = T - 1 .. 0 as
    dh      = dh_head[t] + carry                       (carry = 0 at t = T - 1)
    du_pre  = bf16_rne(dh (h_{t-1} - c) u (1 - u))     dc_pre = bf16_rne(dh (1 - u) (1 - c^2))
    drh     = dc_pre W_c^T                             W_* = bf16(h-side kernels), fp32 accumulation
    dr_pre  = bf16_rne(drh h_{t-1} r (1 - r))
    carry   = dh u + drh r + du_pre W_u^T + dr_pre W_r^T
and leave carry behind step 0 as dh0 = d loss / d h_{-1}.  Buffers as FcGruEngine.read_buffer returns them: u, r, c [T,B,n],
h [T+1,B,n] (slot t = h_{t-1} of step t), dh_head [B,T,n], dxpre [B,T,3,n] parts [du_pre | dr_pre | dc_pre], dh0 [B,n].

1. The reference (bptt_reference).  At step t the two GEMM terms use the DEVICE'S OWN dxpre rows of that step (products of
bf16 operands are exact in float64), so an error in one step's rows does not spread to the reference of the others; only the
dh recursion (dh u, drh r) is carried, in float64.  It yields the pre-store value of all three parts of every step, and dh0.

2. The dxpre criterion (check), per part and step: an element must equal bf16_rne(reference); otherwise it is a flip.  At
most FLIP_CAP = 1e-3 of a part's elements may flip (the forward's cap, fcgru_local_ref.py), and every flipped element must
satisfy |dev - ref| <= 2^-8 |ref| + 2^-20 max|ref of that part and step|.  The floor is needed because elements near zero,
where dh cancels, sit many bf16 ordinals from the reference while being wrong by only a few fp32 roundings of the slab's
scale.  Measured on the stand-in below (fp32 products, K in four quarters) at (B, T) = (3,4), (17,3), (64,3) with
fcgru_local_ref.params / features: flip share at most 2.1e-4 (0.21 of the cap); excess over 2^-8 |ref| at most 8.8e-9 of the
slab maximum (0.0092 of the floor).  (The experiment the criterion was designed on found ordinal distances of up to 107 between
such elements and the reference -- which is why it is not "one ulp".)

3. The dh0 bound: |dh0 - ref| / max|ref| <= DH0_BOUND.  Not derived: measured.  The stand-in's worst figure over the three
shapes above is DH0_MEASURED (tests/test_fcgru_bptt_cpu.py prints it again on every run); the bound is 8 x that, rounded up
to a power of two.  The per-step path is the parent's arithmetic and is held to the same bound on the GPU.

Also here: the stand-in BPTT with a fault= argument (FAULTS), so that the CPU test can show that each mistake breaks a bound.
"""
import numpy as np

import fcgru_local_ref as fref
from fcgru_local_ref import FLIP_CAP, N, UNITS, _bf, _quarters, _mm32, h_kernels
from recurrence_local_ref import bf16_rne, bf16_trunc

REL = 2.0 ** -8                # a flipped element: within one bf16 ulp (2^-8 relative at worst) of the reference ...
FLOOR = 2.0 ** -20             # ... plus this share of the largest reference value of its part and step
DH0_MEASURED = 1.42e-7         # the stand-in's worst |dh0 - ref| / max|ref| over (3,4), (17,3), (64,3) (at 64 x 3): measure_dh0()
DH0_BOUND = 2.0 ** -19         # 8 x DH0_MEASURED = 1.14e-6, rounded up to a power of two (1.91e-6)
PARTS = ('du_pre', 'dr_pre', 'dc_pre')
BUFFERS = ('u', 'r', 'c', 'h', 'dh_head', 'dxpre', 'dh0')

FAULTS = ('drop_k_quarter', 'swap_ur', 'no_dh_u', 'no_drh_r', 'next_step_h', 'next_clip_dh_head', 'dc_trunc', 'unit_shift',
          'carry_not_cleared')


# ------------------------------------------------------------------------------------------------ 1. the reference
def bptt_reference(dev, p):
    """-> ({part: [T,B,n] float64 pre-store values}, dh0 [B,n] float64) from the device's own buffers."""
    f64 = lambda a: np.asarray(a, np.float64)
    wu, wr, wc = (f64(w) for w in h_kernels(p))
    u, r, c, h = f64(dev['u']), f64(dev['r']), f64(dev['c']), f64(dev['h'])
    dhh, dx = f64(dev['dh_head']), f64(dev['dxpre'])
    T, B = u.shape[:2]
    ref = {k: np.zeros((T, B, N)) for k in PARTS}
    carry = np.zeros((B, N))
    for t in range(T - 1, -1, -1):
        dh = dhh[:, t] + carry
        ref['du_pre'][t] = dh * (h[t] - c[t]) * u[t] * (1.0 - u[t])
        ref['dc_pre'][t] = dh * (1.0 - u[t]) * (1.0 - c[t] * c[t])
        drh = dx[:, t, 2] @ wc.T                              # on the device's own dc_pre rows
        ref['dr_pre'][t] = drh * h[t] * r[t] * (1.0 - r[t])
        carry = dh * u[t] + drh * r[t] + dx[:, t, 0] @ wu.T + dx[:, t, 1] @ wr.T
    return ref, carry


# ------------------------------------------------------------------------------------------------ 2. / 3. the criteria
def _part(got, ref):
    """One part of one step: got [B,n] (bf16 values), ref [B,n] float64 pre-store."""
    got = np.asarray(got, np.float64)
    want = np.asarray(bf16_rne(ref.astype(np.float32)), np.float64)
    flip = got != want
    top = float(np.abs(ref).max())
    # |dev - ref| <= REL |ref| + FLOOR top  <=>  the excess over REL |ref|, as a share of the slab maximum, is at most FLOOR.
    # (A flipped element sits near a rounding boundary, up to half a bf16 ulp = 2^-8 |ref| from the reference by construction:
    # the first term is no margin to take a share of; the excess is.)
    d = np.abs(got - ref)
    over = float(np.maximum(d - REL * np.abs(ref), 0.0)[flip].max() / max(top, 1e-300)) if flip.any() else 0.0
    return {'flips': float(flip.mean()), 'cap': FLIP_CAP, 'n_flips': int(flip.sum()), 'n': int(flip.size),
            'err': over, 'bound': FLOOR, 'top': top}


def check(dev, p):
    """dev: BUFFERS (numpy) -> {name: figures}: every part of every step ('du_pre[t]' ...), and 'dh0'."""
    ref, dh0 = bptt_reference(dev, p)
    T = dev['u'].shape[0]
    out = {}
    for t in range(T):
        for k, name in enumerate(PARTS):
            out['%s[%d]' % (name, t)] = _part(dev['dxpre'][:, t, k], ref[name][t])
    d = np.abs(np.asarray(dev['dh0'], np.float64) - dh0)
    top = max(float(np.abs(dh0).max()), 1e-300)
    i = np.unravel_index(int(np.argmax(d)), d.shape)
    out['dh0'] = {'err': float(d[i] / top), 'bound': DH0_BOUND, 'where': tuple(int(k) for k in i), 'top': top}
    return out


def violations(errs, margin=1.0):
    """Names of the entries whose figures are not within 1 / margin of their bounds."""
    bad = []
    for k, e in errs.items():
        ok = e['err'] * margin <= e['bound'] and (('flips' not in e) or e['flips'] * margin <= e['cap'])
        if not ok:
            bad.append(k)
    return bad


def shares(errs):
    """The largest share of each bound used: (flip share / cap, excess of a flipped element / floor, dh0 error / bound)."""
    parts = [e for e in errs.values() if 'flips' in e]
    return (max(e['flips'] / e['cap'] for e in parts), max(e['err'] / e['bound'] for e in parts),
            errs['dh0']['err'] / errs['dh0']['bound'])


def report(tag, errs):
    parts = {k: e for k, e in errs.items() if 'flips' in e}
    n_flips, n = sum(e['n_flips'] for e in parts.values()), sum(e['n'] for e in parts.values())
    s = shares(errs)
    worst = max(parts, key=lambda k: parts[k]['flips'])
    print('%s: dxpre %d of %d elements not the rounded reference; worst part (%s: %d of %d) %.3f of the flip cap; worst excess of a flipped element '
          'over 2^-8 |ref| %.2e of the slab maximum (%.4f of the floor); dh0 %.3e of max|ref| (%.3f of the bound)' %
          (tag, n_flips, n, worst, parts[worst]['n_flips'], parts[worst]['n'], s[0], max(e['err'] for e in parts.values()), s[1], errs['dh0']['err'], s[2]))
    for k in violations(errs):
        print('   VIOLATION %s: %s' % (k, errs[k]))


# ------------------------------------------------------------------------------------------------ the stand-in device
def standin_forward(x, p):
    """The forward stand-in of fcgru_local_ref plus a dh_head as backward_impl composes it: logits on the bf16 rows of h,
    d logits = bf16((softmax - labels) / F) against fixed labels, dh_head = d logits x bf16(W_out)^T in fp32."""
    dev = fref.standin(x, p)
    T, B = dev['u'].shape[:2]
    wout = _bf(np.asarray(p['proj_out_W'], np.float32))                       # [n, G]
    hrows = _bf(dev['h'][1:]).transpose(1, 0, 2).reshape(B * T, N)           # row b T + t
    z = _mm32(hrows, wout) + np.asarray(p['proj_out_b'], np.float32)
    z = z - z.max(1, keepdims=True)
    probs = np.exp(z) / np.exp(z).sum(1, keepdims=True)
    labels = np.random.RandomState(167).rand(*probs.shape).astype(np.float32)
    labels /= labels.sum(1, keepdims=True)
    dz = _bf((probs - labels) / np.float32(B * T))
    dev['dh_head'] = _mm32(dz, wout.T.copy()).reshape(B, T, N).astype(np.float32)
    return dev


def standin_bptt(fwd, p, fault=None):
    """The BPTT with fp32 products, K summed in four quarters as the kernel's four waves do, and the kernels' rounding sites
    -> fwd plus 'dxpre' and 'dh0'.  fault: one of FAULTS."""
    assert fault is None or fault in FAULTS
    wu, wr, wc = (np.ascontiguousarray(w.astype(np.float32).T) for w in h_kernels(p))     # transposed: [j, k]
    u, r, c, h, dhh = (np.asarray(fwd[k], np.float32) for k in ('u', 'r', 'c', 'h', 'dh_head'))
    T, B = u.shape[:2]
    one = np.float32(1)
    dx = np.zeros((B, T, 3, N), np.float32)
    carry = dhh[:, 0].copy() if fault == 'carry_not_cleared' else np.zeros((B, N), np.float32)
    for t in range(T - 1, -1, -1):
        head = dhh[:, t].copy()
        if fault == 'next_clip_dh_head':
            head[0] = dhh[1 % B, t]
        hp = h[min(t + 1, T)] if fault == 'next_step_h' else h[t]
        dh = (head + carry).astype(np.float32)
        du, dc = dh * (hp - c[t]), dh * (one - u[t])
        dup = _bf(du * u[t] * (one - u[t]))
        pre = dc * (one - c[t] * c[t])
        dcp = bf16_trunc(pre).astype(np.float32) if fault == 'dc_trunc' else _bf(pre)
        if fault == 'unit_shift':                                # member 5 publishes its 8 units one slot further on
            dup = dup.copy()
            dup[:, 6 * UNITS:7 * UNITS] = dup[:, 5 * UNITS:6 * UNITS]
            dup[:, 5 * UNITS:6 * UNITS] = 0
        drh = _quarters(dcp, wc, 2 if fault == 'drop_k_quarter' else None)
        carry = np.zeros_like(dh) if fault == 'no_dh_u' else (dh * u[t]).astype(np.float32)
        if fault != 'no_drh_r':
            carry = (carry + drh * r[t]).astype(np.float32)
        drp = _bf(drh * hp * r[t] * (one - r[t]))
        a, b_ = (wr, wu) if fault == 'swap_ur' else (wu, wr)
        s = np.zeros((B, N), np.float32)
        for q in range(4):                                       # a wave sums both halves of its K quarter, then the four are summed
            k = slice(q * fref.KQ, (q + 1) * fref.KQ)
            s = (s + (_mm32(dup[:, k], a[k]) + _mm32(drp[:, k], b_[k]))).astype(np.float32)
        carry = (carry + s).astype(np.float32)
        dx[:, t, 0], dx[:, t, 1], dx[:, t, 2] = dup, drp, dcp
    out = dict(fwd)
    out['dxpre'], out['dh0'] = dx, carry
    return out


def measure_dh0(shapes=((3, 4), (17, 3), (64, 3))):
    """The stand-in's worst |dh0 - ref| / max|ref| over `shapes`: the figure DH0_MEASURED records."""
    p = fref.params()
    worst = 0.0
    for B, T in shapes:
        errs = check(standin_bptt(standin_forward(fref.features(B, T), p), p), p)
        worst = max(worst, errs['dh0']['err'])
    return worst
