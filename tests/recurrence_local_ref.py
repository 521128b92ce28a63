"""One-step float64 references of the two conv-recurrent cells ON SUPPLIED OPERANDS (test helper of
tests/test_recurrence_local_cpu.py and tests/test_recurrence_local_gpu.py).

An end-to-end comparison of a bf16 recurrence with float64 has to allow for operand rounding that compounds over the steps.
Given the device's OWN h_{t-1} (and c_{t-1}), its own xpre / emb and its own gates, one step is a short float64 computation whose
only bf16 roundings are known exactly from the kernel source; products of bf16 operands are exact in fp32 and the kernels
accumulate in fp32, so a bf16 plan must agree with this reference as closely as an f32 plan agrees with float64: F32_TOL.

Each step restated as the kernels compose it (recurrent_gaze_prediction_amd/csrc):
  operand image of h_{t-1}   bf16 RNE of the fp32 state: publish_tile seq_group.hip.h:200 (f2bf, igemm.hip.h:39-42), the per-step
                             epilogues' store8<T> igemm.hip.h:301 / Elem<T>::to lstm_kernels.hip.h:45, and for a streaming call's
                             state seq_seed_kernel seq_group.hip.h:103,108; halo pixels and padding rows are zero (:144-150)
  K order                    tap * C + channel, tap = 3 ky + kx on the 9x9 padded image (a_frags_at seq_group.hip.h:166-170; the
                             packed filters rgp_grcn.hip:312-321 / :239-244): patches() below, filters as HWIO.reshape(9 C, N)
  ConvGRU (convgru_seq.hip.h; per step EpiGruZR / EpiGruC igemm.hip.h:250-305)
    u = sigmoid(xpre_z + U_z * hb), r likewise                  convgru_seq.hip.h:165-166, igemm.hip.h:260
    r.h = bf16_rne(fp32 r * fp32 h_{t-1})                        :167 (`rgs * h_prev`: the lane's fp32 state) then publish_tile;
                                                                igemm.hip.h:266-270
    c = tanh(xpre_c + U * (r.h))                                 :211, igemm.hip.h:295
    h = u h_{t-1} + (1 - u) c                                    :212, igemm.hip.h:296
    bn = bf16_rne(gamma[slot] (h inv_std) + beta[slot])          :228 with slot = (bn_phase + t) % T (:100,129-131;
                                                                rgp_grcn.hip:203-204), igemm.hip.h:297,303
  ConvLSTM (convlstm_seq.hip.h:152-161; per step EpiLstm lstm_kernels.hip.h:29-45): lstm_ref.lstm_cell(rnd=lstm_ref.bf16), which
    already rounds exactly h and the filters, takes the peepholes on the OLD c and g from W_hi.
  input side                 emb = bf16(x rows) @ bf16(proj_c3d_W) + b stored in bf16 (gaze_stages.h:121-136, EpiStore
                             igemm.hip.h:144-157); xpre = 3x3 convolutions of emb with bf16(W_z | W_r | W), fp32
                             (rgp_grcn.hip:106-111, :239-241)

All tensors are numpy [B, T, 49, C] (position 7 y + x); float64 unless noted.  bf16_rne goes through fp32 (a double rounding only
for values within 2^-24 of a bf16 tie: at most a one-ulp flip, which the bf16 comparisons count).

Also here, so that the CPU tests can validate bounds and sensitivity without a device: a stand-in "device" that runs the same
steps with fp32 products and fp32 accumulation (torch fp32 matmul) and can be told to make one of the mistakes of FAULTS.
"""
import numpy as np
import torch

import lstm_ref
from recurrent_gaze_prediction_amd import synthetic as syn

F32_TOL = 2e-5                 # the project's f32 bound (tests/test_grcn_gpu.py TOL['f32'], tests/test_lstm_gpu.py F32_TOL)
BLEND_TOL = 2.0 ** -22         # h = u h + (1-u) c, c' = f c + i g from the device's own gates: at most three fp32 roundings, with
#                                or without FMA contraction.  |h| < 1 always.  The cell state is not bounded by 1: for |c'| < 2 the
#                                roundings (of f c < 3, i g < 1 and the sum) add up to less than 2^-23 + 2^-24 + 2^-25, but for
#                                2 <= |c'| < 4 (f c < 5) only to less than 2^-22 + 2^-23 + 2^-25: blend_bound() doubles per binade
FLIP_CAP = {'bn': 1e-3, 'emb': 1e-2}     # share of bf16 elements that may sit one ulp from the rounded reference
BN_INV_STD = float(np.float32(1.0) / np.sqrt(np.float32(1.0) + np.float32(1e-3)))   # rgp_grcn.hip:149,205
S, P = 128, 512

GRU_FAULTS = ('drop_product', 'swap_taps', 'rh_trunc', 'rh_from_bf16_h', 'halo', 'next_clip_xpre', 'bn_slot')
LSTM_FAULTS = ('peephole_new_c', 'g_uses_whc')


# ------------------------------------------------------------------------------------------------ inputs of both test modules
def active_params(family, T):
    """Filter scales that keep the gates out of saturation on syn.c3d_features: recurrent filters N(0, 0.05) (a single
    (tap, cin) product is then ~1e-2 of a pre-activation), input filters a fifth / a quarter of that (pre-activations of std ~1);
    gaze_grcn's batch-norm rows random per timestep."""
    if family == 'grcn':
        p = syn.grcn_params(101, T, gru_std=0.05, random_bn=True)
        for k in ('GRU_Conv_Wz', 'GRU_Conv_Wr', 'GRU_Conv_W'):
            p[k] = (p[k] * np.float32(0.2)).astype(np.float32)
        return p
    p = syn.lstm_params(102, lstm_std=0.05)
    for k in ('ConvLSTM_Wxi', 'ConvLSTM_Wxf', 'ConvLSTM_Wxc', 'ConvLSTM_Wxo'):
        p[k] = (p[k] * np.float32(0.25)).astype(np.float32)
    return p


def features(B, T):
    return syn.c3d_features(103 + B, B, T)


def random_state(family, B, seed=107):
    """fp32 U(-1, 1), hence not bf16-representable: [B,49,S] for gaze_grcn, [2,B,49,S] = [h | c] for gaze_lstm."""
    rs = np.random.RandomState(seed + B)
    return rs.uniform(-1, 1, size=((B, 49, S) if family == 'grcn' else (2, B, 49, S))).astype(np.float32)


# ------------------------------------------------------------------------------------------------ roundings
def _t(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype)


def bf16_rne(a):
    """numpy -> float64 numpy of the bf16 (round to nearest even) values."""
    return _t(a, torch.float32).to(torch.bfloat16).to(torch.float64).numpy()


def bf16_trunc(a):
    """numpy -> float64 numpy of the bf16 values a truncating store would leave (seeded fault only)."""
    bits = np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32) & np.uint32(0xFFFF0000)
    return bits.view(np.float32).astype(np.float64)


def bf16_ordinal(a):
    """numpy of bf16-representable values -> int32 position on the bf16 number line (adjacent values differ by 1)."""
    bits = _t(a, torch.float32).to(torch.bfloat16).view(torch.int16).to(torch.int32).numpy()
    return np.where(bits < 0, -(bits & 0x7FFF), bits)


def same(v):
    return np.asarray(v, np.float64)


# ------------------------------------------------------------------------------------------------ the operators
def patches(img, dtype=torch.float64, halo=None, swap=None):
    """img [N,49,C] -> torch [N,49,9 C]: element tap * C + c of row 7 y + x is pixel (y + ky, x + kx) of the zero-padded 9x9
    image, tap = 3 ky + kx.  halo / swap: seeded faults (a value in halo pixel (0,0) of image 0; two taps exchanged)."""
    img = _t(img, dtype)
    n, _, c = img.shape
    pad = torch.zeros(n, 9, 9, c, dtype=dtype)
    pad[:, 1:8, 1:8] = img.reshape(n, 7, 7, c)
    if halo is not None:
        pad[0, 0, 0, :] = halo
    cols = [pad[:, ky:ky + 7, kx:kx + 7] for ky in range(3) for kx in range(3)]
    if swap is not None:
        cols[swap[0]], cols[swap[1]] = cols[swap[1]], cols[swap[0]]
    return torch.cat(cols, -1).reshape(n, 49, 9 * c)


def conv3x3(img, w_hwio, dtype=torch.float64, **kw):
    """tf.nn.conv2d SAME, stride 1, of [N,49,C] with [3,3,C,N_out] -> numpy [N,49,N_out] in `dtype` arithmetic."""
    w = _t(w_hwio, dtype)
    return (patches(img, dtype, **kw) @ w.reshape(-1, w.shape[-1])).numpy()


def sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def x_rows(x):
    """c3d_input [B,T,1024,7,7] -> [B*T*49, 1024] (gaze_grcn.py:239-242)."""
    return np.ascontiguousarray(np.asarray(x).transpose(0, 1, 3, 4, 2)).reshape(-1, 1024)


def projection(x, p, rnd=bf16_rne, dtype=torch.float64):
    """emb [B,T,49,P] BEFORE its store (float64, or fp32-accumulated for the stand-in)."""
    b, t = x.shape[:2]
    e = _t(rnd(x_rows(x)), dtype) @ _t(rnd(p['proj_c3d_W']), dtype) + _t(p['proj_c3d_b'], dtype)
    return e.numpy().reshape(b, t, 49, -1)


def gru_xpre(emb, p, rnd=bf16_rne, dtype=torch.float64):
    """[B,T,49,P] -> xpre [B,T,49,3 S] = W_z | W_r | W convolutions of emb."""
    b, t = emb.shape[:2]
    w = np.concatenate([rnd(p[k]) for k in ('GRU_Conv_Wz', 'GRU_Conv_Wr', 'GRU_Conv_W')], -1)
    return conv3x3(emb.reshape(b * t, 49, -1), w, dtype).reshape(b, t, 49, -1)


def gru_zr(xpre_t, hp, p, rnd=bf16_rne):
    """u, r of one step from the step's xpre [N,49,3 S] and the fp32 state h_{t-1} [N,49,S]."""
    w = np.concatenate([rnd(p['GRU_Conv_Uz']), rnd(p['GRU_Conv_Ur'])], -1)
    zr = conv3x3(rnd(hp), w)
    return sigmoid(xpre_t[..., :S] + zr[..., :S]), sigmoid(xpre_t[..., S:2 * S] + zr[..., S:])


def gru_rh(r, hp, rnd=bf16_rne):
    """The candidate convolution's operand: ONE IEEE fp32 multiply of the fp32 r and the fp32 state, then the store's rounding.
    With rounding switched off (rnd=same) the float64 product."""
    if rnd is same:
        return np.asarray(r, np.float64) * np.asarray(hp, np.float64)
    return rnd(np.asarray(r, np.float32) * np.asarray(hp, np.float32))


def gru_candidate(xpre_t, rh, p, rnd=bf16_rne):
    return np.tanh(xpre_t[..., 2 * S:] + conv3x3(rh, rnd(p['GRU_Conv_U'])))


def gru_blend(u, hp, c):
    u, hp, c = (np.asarray(v, np.float64) for v in (u, hp, c))
    return u * hp + (1.0 - u) * c


def gru_bn(h, p, slot, rnd=bf16_rne):
    g, b = np.asarray(p['bn_gamma'], np.float64)[slot], np.asarray(p['bn_beta'], np.float64)[slot]
    return rnd(g * (np.asarray(h, np.float64) * BN_INV_STD) + b)


def gru_step(xpre_t, hp, p, rnd=bf16_rne):
    """One step from its own gates (the chained form) -> dict(u, r, rh, c, h)."""
    u, r = gru_zr(xpre_t, hp, p, rnd)
    rh = gru_rh(r, hp, rnd)
    c = gru_candidate(xpre_t, rh, p, rnd)
    return {'u': u, 'r': r, 'rh': rh, 'c': c, 'h': gru_blend(u, hp, c)}


def lstm_params_t(p):
    return {k: _t(p[k]) for k in lstm_ref.KEYS}


def lstm_step(emb_t, c_prev, h_prev, pt, rnd=lstm_ref.bf16):
    """lstm_ref.lstm_cell on [N,49,.] numpy operands (emb as stored: bf16 values) -> dict of numpy [N,49,S]."""
    n = emb_t.shape[0]
    with torch.no_grad():
        out = lstm_ref.lstm_cell(_t(emb_t).reshape(n, 7, 7, -1), _t(c_prev).reshape(n, 7, 7, S), _t(h_prev).reshape(n, 7, 7, S), pt, rnd)
    return {k: v.numpy().reshape(n, 49, S) for k, v in out.items()}


# ------------------------------------------------------------------------------------------------ comparisons
def _abs(got, ref, bound, scale=1.0):
    """bound: a number, or one per element (the figures are then those of the element that comes closest to its bound)."""
    d = np.abs(np.asarray(got, np.float64) - ref) / scale
    b = np.broadcast_to(np.asarray(bound, np.float64), d.shape)
    i = np.unravel_index(int(np.argmax(d / b)), d.shape)
    return {'err': float(d[i]), 'bound': float(b[i]), 'where': tuple(int(k) for k in i), 'ratio': float(d[i] / b[i]),
            'f32': np.ndim(bound) == 0 and bound == F32_TOL}


def blend_bound(ref):
    """BLEND_TOL for |ref| < 2, doubled with every binade above (see BLEND_TOL)."""
    return BLEND_TOL * np.maximum(1.0, 2.0 ** (np.floor(np.log2(np.maximum(np.abs(ref), 1.0)))))


def _bf16(name, got, ref):
    """A bf16-stored tensor against the float64 reference BEFORE its store.  An element must equal bf16_rne(ref) or sit exactly
    one ulp from it (an fp32-evaluated expression can land on the other side of a rounding tie), and the elements that are not
    equal are capped at FLIP_CAP[name] of all.  One ulp is the whole allowance only where an ulp is large against the fp32
    evaluation's own error: where the terms cancel to a value near zero, the ulp of the result is smaller than the rounding
    errors of the terms (the stand-in shows ten ulps at |emb| ~ 1e-5).  There -- and it can only matter there -- an element
    further off must lie inside [bf16_rne(ref - eps), bf16_rne(ref + eps)], eps = F32_TOL max|ref|: the rounded image of the
    project's f32 bound on the value in front of the store (rounding is monotonic).  It still counts against the cap."""
    ref = np.asarray(ref, np.float64)
    eps = F32_TOL * np.abs(ref).max()
    o = bf16_ordinal(got).astype(np.int64)
    d = np.abs(o - bf16_ordinal(bf16_rne(ref)))
    inside = (o >= bf16_ordinal(bf16_rne(ref - eps))) & (o <= bf16_ordinal(bf16_rne(ref + eps)))
    far = (d > 1) & ~inside
    off = float((d >= 1).mean())
    worst = float(d[far].max()) if far.any() else float(min(d.max(), 1))
    return {'err': worst, 'bound': 1.0, 'flips': off, 'cap': FLIP_CAP[name], 'n_flips': int((d >= 1).sum()), 'n': int(d.size),
            'n_near_zero': int(((d > 1) & inside).sum()), 'ratio': max(worst if far.any() else 0.0, off / FLIP_CAP[name])}


def _prev(first, later):
    """[B,n,...] of the states in front of steps 0..n-1: `first` [B,...], then later[:, :n-1]."""
    return np.concatenate([first[:, None], later[:, :-1]], 1)


def check_gru(dev, x, p, state_in=None, bn_phase=0, n_steps=None, emb_ref=None):
    """dev: the device's emb, xpre, u, r, c, h, bn as [B,T,49,C] -> {tensor: figures} for the first n_steps steps (emb and xpre:
    every frame).  state_in [B,49,S] fp32: the state a streaming call started from; emb_ref: projection(x, p) if the caller has it."""
    B, T = dev['h'].shape[:2]
    n = T if n_steps is None else n_steps
    out = {'emb': _bf16('emb', dev['emb'], projection(x, p) if emb_ref is None else emb_ref)}
    xr = gru_xpre(np.asarray(dev['emb'], np.float64), p)
    out['xpre'] = _abs(dev['xpre'], xr, F32_TOL, np.abs(xr).max())
    h0 = np.zeros((B, 49, S), np.float32) if state_in is None else np.asarray(state_in, np.float32).reshape(B, 49, S)
    f = lambda a: np.asarray(a)[:, :n].reshape(B * n, 49, -1)
    hp = _prev(h0, np.asarray(dev['h'], np.float32)[:, :n]).reshape(B * n, 49, S)
    xp = f(dev['xpre']).astype(np.float64)
    u_ref, r_ref = gru_zr(xp, hp, p)
    c_ref = gru_candidate(xp, gru_rh(f(dev['r']), hp), p)
    out['u'] = _abs(f(dev['u']), u_ref, F32_TOL)
    out['r'] = _abs(f(dev['r']), r_ref, F32_TOL)
    out['c'] = _abs(f(dev['c']), c_ref, F32_TOL)
    out['h'] = _abs(f(dev['h']), gru_blend(f(dev['u']), hp, f(dev['c'])), BLEND_TOL)
    slots = (bn_phase + np.arange(n)) % T
    bn_ref = np.stack([gru_bn(np.asarray(dev['h'])[:, t], p, slots[t], rnd=same) for t in range(n)], 1)
    out['bn'] = _bf16('bn', np.asarray(dev['bn'])[:, :n], bn_ref)
    return out


def check_lstm(dev, x, p, state_in=None, n_steps=None, emb_ref=None):
    """dev: the device's emb [B,T,49,P] and i, f, g, o, c, h [B,T,49,S]; state_in [2,B,49,S] = [h | c]."""
    B, T = dev['h'].shape[:2]
    n = T if n_steps is None else n_steps
    out = {'emb': _bf16('emb', dev['emb'], projection(x, p) if emb_ref is None else emb_ref)}
    z = np.zeros((2, B, 49, S), np.float32) if state_in is None else np.asarray(state_in, np.float32).reshape(2, B, 49, S)
    f = lambda a: np.asarray(a)[:, :n].reshape(B * n, 49, -1)
    hp = _prev(z[0], np.asarray(dev['h'], np.float32)[:, :n]).reshape(B * n, 49, S)
    cp = _prev(z[1], np.asarray(dev['c'], np.float32)[:, :n]).reshape(B * n, 49, S)
    ref = lstm_step(f(dev['emb']), cp, hp, lstm_params_t(p))
    for k in 'ifgo':
        out[k] = _abs(f(dev[k]), ref[k], F32_TOL)
    d = {k: f(dev[k]).astype(np.float64) for k in 'ifgoc'}
    c_ref = d['f'] * cp + d['i'] * d['g']
    out['c'] = _abs(d['c'], c_ref, blend_bound(c_ref))
    out['h'] = _abs(f(dev['h']), np.tanh(d['c']) * d['o'], F32_TOL)      # the tanh(c') term: the gate bound
    return out


def activity(dev, gates, cands):
    """Share of gate values in (0.1, 0.9) and of candidate magnitudes below 0.9 (a saturated gate hides its operands)."""
    g = np.concatenate([np.asarray(dev[k]).ravel() for k in gates])
    c = np.concatenate([np.abs(np.asarray(dev[k])).ravel() for k in cands])
    return float(((g > 0.1) & (g < 0.9)).mean()), float((c < 0.9).mean())


def report(tag, errs):
    for k, e in errs.items():
        if 'flips' in e:
            print('%s %s: %d of %d not the rounded reference (%.4f %%, cap %.2f %%), %d of them by more than one ulp inside the f32 '
                  'bound near zero, worst outside it %d ulp' % (tag, k, e['n_flips'], e['n'], 100 * e['flips'], 100 * e['cap'],
                                                                e['n_near_zero'], e['err']))
        else:
            print('%s %s: %.3e (bound %.3e) at %s' % (tag, k, e['err'], e['bound'], e['where']))


def violations(errs, margin=1.0, cap_margin=1.0):
    """Names of the tensors whose figures are not within their bounds.  margin tightens the F32_TOL bounds, cap_margin the
    one-ulp caps; BLEND_TOL is a worst-case count of roundings and more than one bf16 ulp is a violation as it is."""
    bad = []
    for k, e in errs.items():
        if 'flips' in e:
            ok = e['err'] <= 1 and e['flips'] * cap_margin <= e['cap']
        else:
            ok = e['err'] * (margin if e['f32'] else 1.0) <= e['bound']
        if not ok:
            bad.append(k)
    return bad


# ------------------------------------------------------------------------------------------------ the stand-in device
def _f32(a):
    return np.asarray(a, np.float32)


def _sig32(v):
    v = _f32(v)
    return (np.float32(1) / (np.float32(1) + np.exp(-v))).astype(np.float32)


def _store_bf16(v):
    return bf16_rne(_f32(v)).astype(np.float32)


def standin_gru(x, p, state_in=None, bn_phase=0, fault=None):
    """The steps above with fp32 products and fp32 accumulation -> dev dict as check_gru takes it.  fault: one of GRU_FAULTS."""
    assert fault is None or fault in GRU_FAULTS
    B, T = x.shape[:2]
    f32 = torch.float32
    emb = _store_bf16(projection(x, p, dtype=f32))
    xpre = _f32(gru_xpre(emb, p, dtype=f32))
    w_zr = np.concatenate([bf16_rne(p['GRU_Conv_Uz']), bf16_rne(p['GRU_Conv_Ur'])], -1)
    w_c = bf16_rne(p['GRU_Conv_U'])
    gam, bet = _f32(p['bn_gamma']), _f32(p['bn_beta'])
    h = np.zeros((B, 49, S), np.float32) if state_in is None else _f32(state_in).reshape(B, 49, S).copy()
    dev = {k: [] for k in ('u', 'r', 'c', 'h', 'bn')}
    for t in range(T):
        xp = xpre[:, t].copy()
        if fault == 'next_clip_xpre':
            xp[0] = xpre[1, t]                                    # clip 0 reads the second slot's rows
        hb = _store_bf16(h)
        zr = _f32(conv3x3(hb, w_zr, f32, halo=0.5 if fault == 'halo' else None))
        if fault == 'drop_product':                               # centre tap, cin 5 -> u channel 7 at the corner (0, 0) of clip 0
            zr[0, 0, 7] -= np.float32(hb[0, 0, 5] * w_zr[1, 1, 5, 7])
        u, r = _sig32(zr[..., :S] + xp[..., :S]), _sig32(zr[..., S:] + xp[..., S:2 * S])
        if fault == 'rh_trunc':
            rh = bf16_trunc(r * h)
        elif fault == 'rh_from_bf16_h':
            rh = bf16_rne(r * hb)
        else:
            rh = bf16_rne(r * h)
        cc = _f32(conv3x3(rh, w_c, f32, swap=(0, 8) if fault == 'swap_taps' else None))
        c = np.tanh(_f32(cc + xp[..., 2 * S:])).astype(np.float32)
        hn = (u * h + (np.float32(1) - u) * c).astype(np.float32)
        slot = (bn_phase + t + (1 if fault == 'bn_slot' else 0)) % T
        bn = _store_bf16(gam[slot] * (hn * np.float32(BN_INV_STD)) + bet[slot])
        for k, v in (('u', u), ('r', r), ('c', c), ('h', hn), ('bn', bn)):
            dev[k].append(v)
        h = hn
    out = {k: np.stack(v, 1) for k, v in dev.items()}
    out['emb'], out['xpre'] = emb, xpre
    return out


def standin_lstm(x, p, state_in=None, fault=None):
    """gaze_lstm likewise -> dev dict as check_lstm takes it.  fault: one of LSTM_FAULTS."""
    assert fault is None or fault in LSTM_FAULTS
    B, T = x.shape[:2]
    f32 = torch.float32
    emb = _store_bf16(projection(x, p, dtype=f32))
    wx = np.concatenate([bf16_rne(p[k]) for k in ('ConvLSTM_Wxi', 'ConvLSTM_Wxf', 'ConvLSTM_Wxc', 'ConvLSTM_Wxo')], -1)
    xpre = _f32(conv3x3(emb.reshape(B * T, 49, -1), wx, f32)).reshape(B, T, 49, 4 * S)
    wh = np.concatenate([bf16_rne(p[k]) for k in ('ConvLSTM_Wxi_1', 'ConvLSTM_Wxf_1', 'ConvLSTM_Wxo_1', 'ConvLSTM_Whc')], -1)
    wci, wcf, wco = (_f32(p[k]).reshape(49, S) for k in ('ConvLSTM_Wci', 'ConvLSTM_Wcf', 'ConvLSTM_Wco'))
    st = np.zeros((2, B, 49, S), np.float32) if state_in is None else _f32(state_in).reshape(2, B, 49, S)
    h, c = st[0].copy(), st[1].copy()
    dev = {k: [] for k in 'ifgoch'}
    for t in range(T):
        s = _f32(conv3x3(_store_bf16(h), wh, f32))
        xi, xf, xg, xo = (xpre[:, t, :, k * S:(k + 1) * S] for k in range(4))
        si, sf, so, shc = (s[..., k * S:(k + 1) * S] for k in range(4))
        ig = _sig32(si + xi + wci * c)
        fg = _sig32(sf + xf + wcf * c)
        gg = np.tanh(_f32((shc if fault == 'g_uses_whc' else si) + xg)).astype(np.float32)
        cn = (fg * c + ig * gg).astype(np.float32)
        og = _sig32(so + xo + wco * (cn if fault == 'peephole_new_c' else c))
        hn = (np.tanh(cn) * og).astype(np.float32)
        for k, v in zip('ifgoch', (ig, fg, gg, og, cn, hn)):
            dev[k].append(v)
        h, c = hn, cn
    out = {k: np.stack(v, 1) for k, v in dev.items()}
    out['emb'] = emb
    return out
