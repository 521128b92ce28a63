"""One-step float64 reference of the fc-GRU cell on supplied fp32 operands, and a numpy stand-in of the f32 persistent kernel
(csrc/fcgru_seq_f32.hip.h): test helper of tests/test_fcgru_persistent_f32_cpu.py and tests/test_fcgru_persistent_f32_gpu.py.

f32 plans keep fp32 operand rows and fp32 kernels, so the one-step reference of tests/fcgru_local_ref.py is taken on UNROUNDED
kernels (the f32 form of check_gates in tests/test_fcgru_stream_gpu.py), and the operand rows must be the fp32 values themselves:
    u = sigmoid(xpre_u + hp W_u),  r = sigmoid(xpre_r + hp W_r)        hp = the fp32 rows of h_{t-1}
    rh = fp32 r * fp32 h_{t-1}                                         ONE fp32 multiply, stored as it is: exact
    c = tanh(xpre_c + rh W_c)
    h_t = u h_{t-1} + (1 - u) c                                        from the device's own u, c, h_{t-1}
    hp[t+1] = h_t                                                      exact
Bounds: GATE_TOL = 5e-5 and BLEND_TOL = 2^-22 of tests/fcgru_local_ref.py; rh, hp and slot (b, 0) of hp exact.

The stand-in runs the kernel's arithmetic in fp32: K in four quarters (one per wave); within a quarter the 26 chunks of 16 in
ascending order, within a chunk component e = 0..3 (one MFMA each), within an MFMA the four k = 16 i + 4 fk + e, fk = 0..3, each
product rounded and added to the running sum; then the quarters in ascending order; fp32 gate math.  It can be told to make one of
the mistakes of FAULTS.
"""
import numpy as np

import fcgru_local_ref as ref
from recurrence_local_ref import sigmoid

GATE_TOL, BLEND_TOL = ref.GATE_TOL, ref.BLEND_TOL
N, NX, NP, UNITS, KQ = ref.N, ref.NX, ref.NP, ref.UNITS, ref.KQ
EXACT = 1e-30

FAULTS = ('swap_ur', 'drop_k_quarter', 'next_clip_xpre', 'next_step_xpre', 'blend_swapped', 'unit_shift', 'rh_from_new_h',
          'second_half_repeats', 'k_permutation_one_side')


def h_kernels64(p):
    return ref.h_kernels(p, rnd=lambda a: np.asarray(a, np.float64))


def check(dev, p, zero_state=True):
    """dev: the buffers FcGruEngine.read_buffer returns (numpy) -> {tensor: figures} over every gate of every step."""
    wu, wr, wc = h_kernels64(p)
    f32, f64 = (lambda a: np.asarray(a, np.float32)), (lambda a: np.asarray(a, np.float64))
    T = dev['u'].shape[0]
    hp = f64(dev['hp'])[:, :T].transpose(1, 0, 2)
    xp = f64(dev['xpre']).transpose(1, 0, 2, 3)
    h_prev, h_next = dev['h'][:-1], dev['h'][1:]
    rh = f64(dev['rh']).transpose(1, 0, 2)
    u, c = f64(dev['u']), f64(dev['c'])
    out = {'u': ref._abs(dev['u'], sigmoid(xp[:, :, 0] + hp @ wu), GATE_TOL),
           'r': ref._abs(dev['r'], sigmoid(xp[:, :, 1] + hp @ wr), GATE_TOL),
           'rh': ref._abs(rh, f64(f32(dev['r']) * f32(h_prev)), EXACT),
           'c': ref._abs(dev['c'], np.tanh(xp[:, :, 2] + rh @ wc), GATE_TOL),
           'h': ref._abs(h_next, u * f64(h_prev) + (1.0 - u) * c, BLEND_TOL),
           'hp': ref._abs(f64(dev['hp'])[:, 1:].transpose(1, 0, 2), f64(h_next), EXACT)}
    if zero_state:
        out['hp0'] = ref._abs(f64(dev['hp'])[:, 0], 0.0, EXACT)
    return out


violations, report = ref.violations, ref.report


# ------------------------------------------------------------------------------------------------ the stand-in device
def k_order(kq, flip_e=False):
    """The k indices of quarter kq in the order the kernel's MFMAs add them (the padded 1664: k >= N multiplies zeros)."""
    return [KQ * kq + 16 * i + 4 * fk + (3 - e if flip_e else e) for i in range(KQ // 16) for e in range(4) for fk in range(4)]


def _gemm(a, w, drop=None, a_flip=False):
    """a [B,n] x w [n,m] as the kernel sums it.  a_flip: the A side reads component 3 - e where the B side reads e."""
    a, w = np.asarray(a, np.float32), np.asarray(w, np.float32)
    total = np.zeros((a.shape[0], w.shape[1]), np.float32)
    for q in range(4):
        if q == drop:
            continue
        s = np.zeros_like(total)
        for kb, ka in zip(k_order(q), k_order(q, flip_e=a_flip)):
            if ka < N and kb < N:
                s += a[:, ka:ka + 1] * w[kb:kb + 1]
        total = total + s
    return total


def standin_xpre(x, p):
    """[B,T,1024,7,7] -> xpre [B,T,3,n] fp32: fp32 rows x fp32 projection + bias, flattened to 49*32, x fp32 x-side kernels + biases."""
    B, T = x.shape[:2]
    rows = np.ascontiguousarray(np.asarray(x, np.float32).transpose(0, 1, 3, 4, 2)).reshape(-1, 1024)
    emb = (ref._mm32(rows, p['proj_c3d_W']) + np.asarray(p['proj_c3d_b'], np.float32)).reshape(B * T, NX)
    g, c = np.asarray(p['gates_kernel'], np.float32), np.asarray(p['candidate_kernel'], np.float32)
    gb, cb = np.asarray(p['gates_bias'], np.float32), np.asarray(p['candidate_bias'], np.float32)
    xu = ref._mm32(emb, g[:NX, N:]) + gb[N:]
    xr = ref._mm32(emb, g[:NX, :N]) + gb[:N]
    xc = ref._mm32(emb, c[:NX]) + cb
    return np.stack([xu, xr, xc], 1).reshape(B, T, 3, N).astype(np.float32)


def standin(x, p, fault=None):
    """The recurrence in the kernel's fp32 arithmetic -> dev dict as check takes it.  fault: one of FAULTS."""
    assert fault is None or fault in FAULTS
    B, T = x.shape[:2]
    xpre = standin_xpre(x, p)
    wu, wr, wc = (np.asarray(w, np.float32) for w in ref.h_kernels(p, rnd=lambda a: np.asarray(a, np.float32)))
    one = np.float32(1)
    h = np.zeros((B, N), np.float32)
    hp = np.zeros((B, T + 1, N), np.float32)
    dev = {k: [] for k in ('u', 'r', 'c', 'h', 'rh')}
    dev['h'].append(h)
    m = slice(5 * UNITS, 6 * UNITS)                              # member 5's units, for the publishing mistakes
    for t in range(T):
        xp = xpre[:, t].copy()
        if fault == 'next_clip_xpre':
            xp[0] = xpre[1 % B, t]
        if fault == 'next_step_xpre':
            xp = xpre[:, (t + 1) % T].copy()
        drop = 2 if fault == 'drop_k_quarter' else None
        flip = fault == 'k_permutation_one_side'
        su, sr = _gemm(hp[:, t], wu, drop, flip), _gemm(hp[:, t], wr, drop, flip)
        if fault == 'swap_ur':
            su, sr = sr, su
        u, r = ref._sig32(su + xp[:, 0]), ref._sig32(sr + xp[:, 1])

        def cell(rh):
            c = np.tanh((_gemm(rh, wc) + xp[:, 2]).astype(np.float32)).astype(np.float32)
            if fault == 'blend_swapped':
                return c, ((one - u) * h + u * c).astype(np.float32)
            return c, (u * h + ((one - u) * c).astype(np.float32)).astype(np.float32)
        rh = (r * h).astype(np.float32)
        c, hn = cell(rh)
        if fault == 'rh_from_new_h':                             # the state behind the blend where the one in front of it belongs
            rh = (r * hn).astype(np.float32)
            c, hn = cell(rh)
        row = hn.copy()
        if fault == 'unit_shift':                                # member 5 publishes its 8 units one slot further on
            row[:, 6 * UNITS:7 * UNITS] = row[:, m]
            row[:, m] = hp[:, t, m]
        if fault == 'second_half_repeats':                       # its second 16-byte store repeats the first: units 4-7 = units 0-3
            row[:, 5 * UNITS + 4:6 * UNITS] = row[:, 5 * UNITS:5 * UNITS + 4]
        hp[:, t + 1] = row
        for k, v in (('u', u), ('r', r), ('c', c), ('h', hn), ('rh', rh)):
            dev[k].append(v)
        h = hn
    out = {k: np.stack(v, 0) for k, v in dev.items()}
    out['rh'] = np.ascontiguousarray(out['rh'].transpose(1, 0, 2))
    out['hp'], out['xpre'] = hp, xpre
    return out
