"""Float64 reference of the fc-GRU backward-through-time pass of F32 plans ON THE DEVICE'S OWN BUFFERS, and a numpy stand-in
of the f32 persistent BPTT kernel (csrc/fcgru_bptt_f32.hip.h): test helper of tests/test_fcgru_bptt_f32_cpu.py and
tests/test_fcgru_bptt_f32_gpu.py, built on fcgru_bptt_ref.py and fcgru_f32_local_ref.py.

Both f32 BPTT paths of the library (per step: fc_bwd1_kernel<float>, the b_c GEMM, fc_bwd2_kernel<float>, the b_zr GEMM of
recurrent_gaze_prediction_amd/csrc/rgp_fcgru.hip; persistent: csrc/fcgru_bptt_f32.hip.h) compose step t = T - 1 .. 0 as
    dh      = dh_head[t] + carry                       (carry = 0 at t = T - 1)
    du_pre  = dh (h_{t-1} - c) u (1 - u)               dc_pre = dh (1 - u) (1 - c^2)          stored as fp32: NO rounding site
    drh     = dc_pre W_c^T                             W_* = the fp32 h-side kernels, fp32 accumulation
    dr_pre  = drh h_{t-1} r (1 - r)
    carry   = dh u + drh r + du_pre W_u^T + dr_pre W_r^T
and leave carry behind step 0 as dh0.  Buffers as FcGruEngine.read_buffer returns them (fcgru_bptt_ref.BUFFERS).

1. The reference (bptt_reference): fcgru_bptt_ref.bptt_reference with UNROUNDED fp32 kernels.  At step t the two GEMM terms use
the DEVICE'S OWN dxpre rows of that step; only the dh recursion is carried, in float64.

2. The criteria.  There is no bf16 rounding, hence no flip criterion: per part and step
    max|dev - ref| / max|ref of that part and step| <= PART_BOUND,     and     |dh0 - ref| / max|ref| <= DH0_BOUND_F32.
Neither is derived: both are measured on the stand-in below (fp32 products; per K quarter the (chunk, component, fk) order of
the kernel's MFMAs; quarters ascending; fp32 gate math) at (B, T) = (3,4), (17,3), (64,3) with fcgru_local_ref.params /
features -- measure() -- and set to 8 x the stand-in's worst figure, rounded up to a power of two, as fcgru_bptt_ref.DH0_BOUND
was.  tests/test_fcgru_bptt_f32_cpu.py measures both again on every run.  On the GPU the yardstick is the per-step f32 BPTT
(the parent's arithmetic), held to the same bounds; the bounds are never set from the persistent kernel's own figures.

Also here: the stand-in BPTT with a fault= argument (FAULTS), so that the CPU test can show that each mistake breaks a bound.
"""
import numpy as np

import fcgru_f32_local_ref as f32ref
import fcgru_local_ref as fref
from fcgru_bptt_ref import BUFFERS, PARTS
from fcgru_f32_local_ref import N, UNITS, k_order

PART_MEASURED = 4.58e-7        # the stand-in's worst part figure over (3,4), (17,3), (64,3) (dr_pre[2] at 17 x 3): measure()
PART_BOUND = 2.0 ** -18        # 8 x PART_MEASURED = 3.66e-6, rounded up to a power of two (3.81e-6)
DH0_MEASURED_F32 = 1.49e-7     # the stand-in's worst |dh0 - ref| / max|ref| over the same shapes (at 64 x 3): measure()
DH0_BOUND_F32 = 2.0 ** -19     # 8 x DH0_MEASURED_F32 = 1.19e-6, rounded up to a power of two (1.91e-6)
SHAPES = ((3, 4), (17, 3), (64, 3))

FAULTS = ('drop_k_quarter', 'swap_ur', 'no_dh_u', 'no_drh_r', 'next_step_h', 'next_clip_dh_head', 'unit_shift',
          'carry_not_cleared', 'second_half_repeats', 'k_permutation_one_side')


def bound_from(measured):
    """8 x the measured figure, rounded up to a power of two."""
    return 2.0 ** np.ceil(np.log2(8 * measured))


# ------------------------------------------------------------------------------------------------ 1. the reference
def bptt_reference(dev, p):
    """-> ({part: [T,B,n] float64}, dh0 [B,n] float64) from the device's own buffers, unrounded kernels."""
    f64 = lambda a: np.asarray(a, np.float64)
    wu, wr, wc = f32ref.h_kernels64(p)
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


# ------------------------------------------------------------------------------------------------ 2. the criteria
def check(dev, p):
    """dev: BUFFERS (numpy) -> {name: {'err', 'bound', 'top'}}: every part of every step ('du_pre[t]' ...), and 'dh0'."""
    ref, dh0 = bptt_reference(dev, p)
    T = dev['u'].shape[0]
    out = {}
    for t in range(T):
        for k, name in enumerate(PARTS):
            want = ref[name][t]
            top = float(np.abs(want).max())
            d = float(np.abs(np.asarray(dev['dxpre'][:, t, k], np.float64) - want).max())
            out['%s[%d]' % (name, t)] = {'err': d / max(top, 1e-300), 'bound': PART_BOUND, 'top': top}
    d = np.abs(np.asarray(dev['dh0'], np.float64) - dh0)
    top = max(float(np.abs(dh0).max()), 1e-300)
    i = np.unravel_index(int(np.argmax(d)), d.shape)
    out['dh0'] = {'err': float(d[i] / top), 'bound': DH0_BOUND_F32, 'where': tuple(int(k) for k in i), 'top': top}
    return out


def violations(errs, margin=1.0):
    """Names of the entries whose figures are not within 1 / margin of their bounds (a NaN is a violation)."""
    return [k for k, e in errs.items() if not e['err'] * margin <= e['bound']]


def shares(errs):
    """The largest share of each bound used: (worst part error / PART_BOUND, dh0 error / DH0_BOUND_F32)."""
    return max(e['err'] / e['bound'] for k, e in errs.items() if k != 'dh0'), errs['dh0']['err'] / errs['dh0']['bound']


def report(tag, errs):
    parts = {k: e for k, e in errs.items() if k != 'dh0'}
    worst = max(parts, key=lambda k: parts[k]['err'])
    s = shares(errs)
    print('%s: worst part %s %.3e of its slab maximum (%.3f of the bound); dh0 %.3e of max|ref| (%.3f of the bound)' %
          (tag, worst, parts[worst]['err'], s[0], errs['dh0']['err'], s[1]))
    for k in violations(errs):
        print('   VIOLATION %s: %s' % (k, errs[k]))


# ------------------------------------------------------------------------------------------------ the stand-in device
def standin_forward(x, p):
    """The f32 forward stand-in of fcgru_f32_local_ref plus a dh_head as backward_impl<float> composes it: logits on the fp32 rows
    of h, d logits = (softmax - labels) / F against fixed labels, dh_head = d logits x W_out^T, all fp32."""
    dev = f32ref.standin(x, p)
    T, B = dev['u'].shape[:2]
    wout = np.asarray(p['proj_out_W'], np.float32)                           # [n, G]
    hrows = np.ascontiguousarray(dev['h'][1:].transpose(1, 0, 2)).reshape(B * T, N)
    z = fref._mm32(hrows, wout) + np.asarray(p['proj_out_b'], np.float32)
    z = z - z.max(1, keepdims=True)
    probs = np.exp(z) / np.exp(z).sum(1, keepdims=True)
    labels = np.random.RandomState(167).rand(*probs.shape).astype(np.float32)
    labels /= labels.sum(1, keepdims=True)
    dz = ((probs - labels) / np.float32(B * T)).astype(np.float32)
    dev['dh_head'] = fref._mm32(dz, wout.T.copy()).reshape(B, T, N).astype(np.float32)
    return dev


def _gemm_passes(passes, drop=None, a_flip=False):
    """One accumulator over several fcs32_gemm passes [(a [B,n], w [n(k), n(unit)]), ...] as the kernel sums them: per K quarter
    every pass in turn, each in the (chunk, component, fk) order, into ONE running fp32 sum; then the quarters ascending.
    a_flip: the A side reads component 3 - e where the B side reads e."""
    B = passes[0][0].shape[0]
    total = np.zeros((B, passes[0][1].shape[1]), np.float32)
    for q in range(4):
        if q == drop:
            continue
        s = np.zeros_like(total)
        for a, w in passes:
            a, w = np.asarray(a, np.float32), np.asarray(w, np.float32)
            for kb, ka in zip(k_order(q), k_order(q, flip_e=a_flip)):
                if ka < N and kb < N:
                    s += a[:, ka:ka + 1] * w[kb:kb + 1]
        total = total + s
    return total


def standin_bptt(fwd, p, fault=None):
    """The BPTT in the kernel's fp32 arithmetic -> fwd plus 'dxpre' and 'dh0'.  fault: one of FAULTS."""
    assert fault is None or fault in FAULTS
    # transposed: [k, unit j]
    wu, wr, wc = (np.ascontiguousarray(np.asarray(w, np.float32).T) for w in fref.h_kernels(p, rnd=lambda a: np.asarray(a, np.float32)))
    u, r, c, h, dhh = (np.asarray(fwd[k], np.float32) for k in ('u', 'r', 'c', 'h', 'dh_head'))
    T, B = u.shape[:2]
    one = np.float32(1)
    dx = np.zeros((B, T, 3, N), np.float32)
    carry = dhh[:, 0].copy() if fault == 'carry_not_cleared' else np.zeros((B, N), np.float32)
    m = slice(5 * UNITS, 6 * UNITS)                              # member 5's units, for the publishing mistakes
    flip = fault == 'k_permutation_one_side'
    for t in range(T - 1, -1, -1):
        head = dhh[:, t].copy()
        if fault == 'next_clip_dh_head':
            head[0] = dhh[1 % B, t]
        hp = h[min(t + 1, T)] if fault == 'next_step_h' else h[t]
        dh = (head + carry).astype(np.float32)
        du, dc = dh * (hp - c[t]), dh * (one - u[t])
        dup = (du * u[t] * (one - u[t])).astype(np.float32)
        dcp = (dc * (one - c[t] * c[t])).astype(np.float32)
        if fault == 'unit_shift':                                # member 5 publishes its 8 units one slot further on
            dup[:, 6 * UNITS:7 * UNITS] = dup[:, m]
            dup[:, m] = 0
        if fault == 'second_half_repeats':                       # its second 16-byte store repeats the first: units 4-7 = units 0-3
            dup[:, 5 * UNITS + 4:6 * UNITS] = dup[:, 5 * UNITS:5 * UNITS + 4]
        drh = _gemm_passes([(dcp, wc)], 2 if fault == 'drop_k_quarter' else None, flip)
        carry = np.zeros_like(dh) if fault == 'no_dh_u' else (dh * u[t]).astype(np.float32)
        if fault != 'no_drh_r':
            carry = (carry + drh * r[t]).astype(np.float32)
        drp = (drh * hp * r[t] * (one - r[t])).astype(np.float32)
        a, b_ = (wr, wu) if fault == 'swap_ur' else (wu, wr)
        carry = (carry + _gemm_passes([(dup, a), (drp, b_)], None, flip)).astype(np.float32)
        dx[:, t, 0], dx[:, t, 1], dx[:, t, 2] = dup, drp, dcp
    out = dict(fwd)
    out['dxpre'], out['dh0'] = dx, carry
    return out


def measure(shapes=SHAPES):
    """The stand-in's worst part figure and worst dh0 figure over `shapes`: what PART_MEASURED and DH0_MEASURED_F32 record."""
    p = fref.params()
    part = dh0 = 0.0
    for B, T in shapes:
        errs = check(standin_bptt(standin_forward(fref.features(B, T), p), p), p)
        part = max(part, max(e['err'] for k, e in errs.items() if k != 'dh0'))
        dh0 = max(dh0, errs['dh0']['err'])
    return part, dh0
