"""Float64 references of every ShallowNet stage, forward and backward, ON SUPPLIED OPERANDS (test helper of
tests/test_shallownet_local_cpu.py and tests/test_shallownet_local_gpu.py).

tests/test_shallownet_gpu.py compares whole gradients of a piecewise-linear net with float64 autograd, so its bf16 bound has to
allow for pool windows and maxout pairs that bf16 resolves differently (cos > 0.95, rms < 0.35).  Given the device's OWN inputs
to a stage (rgp_shallownet_read_buffer) the stage is a short float64 computation whose only bf16 roundings are known from the
kernel source; products of bf16 operands are exact in fp32 and every kernel accumulates in fp32, so a bf16 plan must agree with
these references as closely as an f32 plan does (recurrence_local_ref.F32_TOL), and an arg-max or a maxout decision is
ambiguous only in the stage that takes it.

Each stage restated as the kernels compose it (recurrent_gaze_prediction_amd/csrc); T = the plan's operand type, round_T = the
identity (f32) or bf16 round-to-nearest-even (f2bf igemm.hip.h:39-42, Elem<T>::to):
  frames4     round_T(frames), a zero 4th channel                frame_prep_kernel kernels_misc.hip.h:424-433
  filters     round_T of the fp32 filters (PackBatch)            rgp_shallownet.hip:62-70; the dgrad packs :75-80
  pool1       round_T(relu(max2x2(conv5x5(frames4, w1)) + b1)); the 2x2 members are rows 2 dy + dx of a window
              (in_tab rgp_shallownet.hip:565-568), the maximum and amax1 (the FIRST maximum) are taken on the raw fp32 sums:
              pool_window_argmax igemm.hip.h:334-348 then EpiStore igemm.hip.h:144-157; the frame kernel (n >= 48, bf16,
              rgp_shallownet.hip:108) shallow_conv1.hip.h:98-112
  act2, act3  round_T(relu(conv3x3_valid(pool, w) + b))          EpiStore<T, true, true> rgp_shallownet.hip:121-134
  pool2/3     tf.nn.max_pool 3x3 / 2 SAME of the stored act: out = ceil(in / 2), pad_before = max((out - 1) 2 + 3 - in, 0) / 2
              (rgp_shallownet.hip:88-89), cells outside ignored; amax = place 3 a + b of the first maximum in scan order,
              counted from the window's corner: maxpool_same_kernel kernels_misc.hip.h:451-486
  mo1         round_T(max(a, b)), a = d1 relu(pool3 . W1[:, j] + b1[j]), b = d2 relu(... j + 2401 ...), d = keep byte ? 1 / keep : 0
              with the site on, else 1; mask1 = max(a, b) > 0 ? (a >= b ? 1 : 2) : 0 on the fp32 values
              EpiReluMaxout igemm.hip.h:189-212
  sal         the same in fp32 from mo1, mask2                   rgp_shallownet.hip:145-151
  sal7        mean of the 7x7 blocks, fp32                       avgpool7_kernel kernels_misc.hip.h:489-498
  dz2         round_T(d_sal) in the half mask2 names, 0 elsewhere        maxout_bwd_kernel train_kernels.hip.h:13-26
  dmo1        dz2 . W2^T (fp32)                                  b_fc2 rgp_shallownet.hip:302-307, :358-362
  dz1         round_T(dmo1 (1 / keep)) through mask1             rgp_shallownet.hip:365-366
  fc?_b       column sums of dz?                                 fc_bias_grad_kernel train_kernels.hip.h:30-46
  fc2_w, fc1_w   mo1^T . dz2, pool3^T . dz1                      fc_wgrad rgp_shallownet.hip:341-350
  dpool3      dz1 . W1^T (fp32)                                  rgp_shallownet.hip:371-375
  dy3, dy2    round_T(sum of dpool over the windows whose amax names this cell), 0 where act <= 0
              maxpool_same_bwd_kernel rgp_shallownet.hip:180-216
  conv?_b     sums of dy? over frames and the valid region       conv_bias_grad_kernel rgp_shallownet.hip:250-275
  conv?_w     correlation of the stage's input with dy           conv_wgrad rgp_shallownet.hip:377-389, conv1 :429-438
  dpool2/1    full correlation of dy3 / dy2 with the rotated, in/out-swapped filter (fp32)     dgrad3 rgp_shallownet.hip:290-299
  dy1         round_T(dpool1) at the member amax1 names, 0 where pool1 <= 0       unpool2x2_kernel rgp_shallownet.hip:220-245

All buffers are numpy in the layouts rgp_shallownet_read_buffer documents (NHWC, [n, units]).  Decisions taken on values the
plan does not store (amax1 on conv1's raw sums, mask1 / mask2 on the FC pre-activations) are checked wherever the float64
margin is decisive (more than F32_TOL max|stage|); the rest is excluded, capped at EXCLUDED_CAP of a buffer, and must still
name a near-tied candidate.  inputs() makes the maxout pairs of TIE_UNITS exact ties (equal columns, equal biases): tf.maximum
sends a tie to the first operand, and random weights never produce one.

Also here, so that the CPU test can validate bounds and sensitivity without a device: a stand-in "device" that runs the same
stages with fp32 products and fp32 accumulation and can be told to make one of the mistakes of FAULTS.
"""
import numpy as np
import torch
import torch.nn.functional as F

import recurrence_local_ref as rl
from recurrence_local_ref import F32_TOL, bf16_rne, bf16_trunc
from salicon_ref import with_biases
from recurrent_gaze_prediction_amd import synthetic as syn

GRAD_TOL = 1e-4               # filter and bias gradients: tests/test_c3d_backward_gpu.py's f32 operator-local bound
EXCLUDED_CAP = 1e-3           # share of a decision buffer whose float64 margin may be inside F32_TOL of the stage
SAL7_TOL = 50 * 2.0 ** -24    # 49 fp32 additions and one multiply of non-negative terms: at most 50 roundings of the mean
TIE_UNITS = (7, 1203, 2400)   # maxout pairs (j, j + 2401) of fc1 and fc2 made exact ties
KEEP = 0.4

FAULTS = ('pool_last_max', 'same_pad_after', 'argmax_after_relu', 'maxout_tie_second', 'mask_halves_swapped', 'no_inv_keep',
          'grad_to_gated', 'dgrad_not_rotated', 'dgrad_unswapped', 'bias_grad_halo', 'bf16_trunc_store')

FWD = ('frames4', 'pool1', 'amax1', 'act2', 'pool2', 'amax2', 'act3', 'pool3', 'amax3', 'mo1', 'mask1', 'sal', 'mask2', 'sal7')
BWD = ('dz2', 'fc2_b', 'fc2_w', 'dmo1', 'dz1', 'fc1_b', 'fc1_w', 'dpool3', 'dy3', 'dy3_gate', 'conv3_b', 'conv3_w', 'dpool2',
       'dy2', 'dy2_gate', 'conv2_b', 'conv2_w', 'dpool1', 'dy1', 'dy1_gate', 'conv1_b', 'conv1_w')
CONV1_STAGES = ('frames4', 'pool1', 'amax1', 'dy1', 'dy1_gate', 'conv1_w', 'conv1_b')
DROPOUT_STAGES = ('mo1', 'mask1', 'dz1', 'fc1_w', 'fc1_b', 'dpool3')
FORWARD_BUFFERS = ('frames4', 'pool1', 'act2', 'pool2', 'act3', 'pool3', 'mo1')
TRAINING_BUFFERS = ('amax1', 'amax2', 'amax3', 'mask1', 'mask2')
BACKWARD_BUFFERS = ('dz2', 'dz1', 'dmo1', 'dpool3', 'dy3', 'dy2', 'dpool2', 'dpool1', 'dy1')
PARAMS = ('conv1_w', 'conv1_b', 'conv2_w', 'conv2_b', 'conv3_w', 'conv3_b', 'fc1_w', 'fc1_b', 'fc2_w', 'fc2_b')


# ------------------------------------------------------------------------------------------------ geometry and inputs
def geom(hw):
    c1 = hw - 4
    p1 = c1 // 2
    c2 = p1 - 2
    p2 = (c2 + 1) // 2
    c3 = p2 - 2
    p3 = (c3 + 1) // 2
    return {'hw': hw, 'c1': c1, 'p1': p1, 'c2': c2, 'p2': p2, 'c3': c3, 'p3': p3, 'nflat': p3 * p3 * 32}


def shapes(hw, n):
    """{buffer: shape} of rgp_shallownet_read_buffer."""
    g = geom(hw)
    return {'frames4': (n, hw, hw, 3), 'pool1': (n, g['p1'], g['p1'], 32), 'act2': (n, g['c2'], g['c2'], 64),
            'pool2': (n, g['p2'], g['p2'], 64), 'act3': (n, g['c3'], g['c3'], 32), 'pool3': (n, g['nflat']), 'mo1': (n, 2401),
            'amax1': (n, g['p1'], g['p1'], 32), 'amax2': (n, g['p2'], g['p2'], 64), 'amax3': (n, g['p3'], g['p3'], 32),
            'mask1': (n, 2401), 'mask2': (n, 2401), 'dz2': (n, 4802), 'dz1': (n, 4802), 'dmo1': (n, 2401),
            'dpool3': (n, g['nflat']), 'dy3': (n, g['c3'], g['c3'], 32), 'dy2': (n, g['c2'], g['c2'], 64),
            'dpool2': (n, g['p2'], g['p2'], 64), 'dpool1': (n, g['p1'], g['p1'], 32), 'dy1': (n, g['c1'], g['c1'], 32)}


def same_pad(h):
    """pad_before of tf.nn.max_pool 3x3 / 2 SAME on h cells."""
    return max(((h + 1) // 2 - 1) * 2 + 3 - h, 0) // 2


def params(hw):
    """syn.shallownet_params with all biases non-zero and the pairs of TIE_UNITS tied in both FC layers."""
    p = with_biases(syn.shallownet_params(171, hw))
    for k in ('fc1', 'fc2'):
        w, b = p[k + '_w'].copy(), p[k + '_b'].copy()
        for j in TIE_UNITS:
            w[:, j + 2401] = w[:, j]
            b[j] = b[j + 2401] = abs(b[j]) + np.float32(0.01)
        p[k + '_w'], p[k + '_b'] = w, b
    return p


def inputs(hw, n):
    """(params, frames [n,hw,hw,3] fp32 in [0,1), d_sal [n,49,49] fp32, keep bytes [n,4802] for the dropout case)."""
    rs = np.random.RandomState(172 + hw + n)
    frames = rs.rand(n, hw, hw, 3).astype(np.float32)
    d_sal = rs.randn(n, 49, 49).astype(np.float32)
    drop = (rs.rand(n, 4802) < KEEP).astype(np.uint8)
    return params(hw), frames, d_sal, drop


# ------------------------------------------------------------------------------------------------ operators
def _t(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dt)


def _np(dt):
    return np.float64 if dt == torch.float64 else np.float32


def round_T(dtype):
    return bf16_rne if dtype == 'bf16' else (lambda a: np.asarray(a, np.float64))


def conv_valid(x, w, dt):
    """tf.nn.conv2d VALID of NHWC x with HWIO w -> NHWC, in dt arithmetic."""
    with torch.no_grad():
        y = F.conv2d(_t(x, dt).permute(0, 3, 1, 2), _t(w, dt).permute(3, 2, 0, 1))
    return y.permute(0, 2, 3, 1).contiguous().numpy()


def conv_wgrad(x, dy, k, dt):
    """Gradient of conv_valid(x, w) w.r.t. w (HWIO, k x k) for the output gradient dy."""
    xt, gt = _t(x, dt).permute(0, 3, 1, 2), _t(dy, dt).permute(0, 3, 1, 2)
    with torch.no_grad():
        g = torch.nn.grad.conv2d_weight(xt, (gt.shape[1], xt.shape[1], k, k), gt)
    return g.permute(2, 3, 1, 0).contiguous().numpy()


def conv_dgrad(dy, w, in_h, dt):
    """Gradient of conv_valid(x, w) w.r.t. x [n,in_h,in_h,Cin]."""
    gt, wt = _t(dy, dt).permute(0, 3, 1, 2), _t(w, dt).permute(3, 2, 0, 1)
    with torch.no_grad():
        g = torch.nn.grad.conv2d_input((gt.shape[0], wt.shape[1], in_h, in_h), wt, gt)
    return g.permute(0, 2, 3, 1).contiguous().numpy()


def matmul(a, b, dt):
    with torch.no_grad():
        return (_t(a, dt) @ _t(b, dt)).numpy()


def windows2x2(raw):
    """[n,2p,2p,C] -> [n,p,p,4,C], member 2 dy + dx."""
    n, h, _, c = raw.shape
    return np.ascontiguousarray(raw.reshape(n, h // 2, 2, h // 2, 2, c).transpose(0, 1, 3, 2, 4, 5)).reshape(n, h // 2, h // 2, 4, c)


def windows3x3(act, pad=None):
    """[n,H,H,C] -> [n,OH,OH,9,C]: place 3 a + b of window (oy, ox) is cell (2 oy - pad + a, 2 ox - pad + b), -inf outside."""
    n, h, _, c = act.shape
    oh = (h + 1) // 2
    pad = same_pad(h) if pad is None else pad
    full = np.full((n, 2 * oh + 1, 2 * oh + 1, c), -np.inf, act.dtype)
    hi = min(h, 2 * oh + 1 - pad)
    full[:, pad:pad + hi, pad:pad + hi] = act[:, :hi, :hi]
    return np.stack([full[:, a:a + 2 * oh:2, b:b + 2 * oh:2] for a in range(3) for b in range(3)], 3)


def unpool3x3(dpool, amax, act, pad=None, gate=True):
    """Scatter dpool [n,OH,OH,C] to the cell its window's amax names (windows overlap: sums), 0 where act <= 0."""
    n, h, _, c = act.shape
    oh = dpool.shape[1]
    pad = same_pad(h) if pad is None else pad
    code = np.asarray(amax).astype(np.int64)
    ni, oy, ox, ci = np.meshgrid(np.arange(n), np.arange(oh), np.arange(oh), np.arange(c), indexing='ij')
    y, x = 2 * oy - pad + code // 3, 2 * ox - pad + code % 3
    ok = (code >= 0) & (code < 9) & (y >= 0) & (y < h) & (x >= 0) & (x < h)
    lin = ((ni[ok] * h + y[ok]) * h + x[ok]) * c + ci[ok]
    out = np.bincount(lin, weights=np.asarray(dpool, np.float64)[ok], minlength=n * h * h * c).reshape(n, h, h, c)
    return out * (np.asarray(act) > 0) if gate else out


def unpool2x2(dpool, amax, pooled):
    """dpool [n,p,p,C] to member amax of its window, 0 where pooled <= 0 -> [n,2p,2p,C]."""
    n, ph, _, c = dpool.shape
    g = np.where(np.asarray(pooled) > 0, np.asarray(dpool, np.float64), 0.0)
    out = np.zeros((n, ph, 2, ph, 2, c))
    for q in range(4):
        out[:, :, q >> 1, :, q & 1, :] = np.where(np.asarray(amax) == q, g, 0.0)
    return out.reshape(n, 2 * ph, 2 * ph, c)


def fc_halves(pre, drop=None):
    """pre [n,4802] -> the two maxout operands' pre-activations [n,2401]; a dropped unit: -inf."""
    za, zb = pre[:, :2401].copy(), pre[:, 2401:].copy()
    if drop is not None:
        d = np.asarray(drop).reshape(pre.shape[0], 4802) != 0
        za[~d[:, :2401]] = -np.inf
        zb[~d[:, 2401:]] = -np.inf
    return za, zb


def route(v, mask):
    """[n,2401] values to the half of [n,4802] that mask names."""
    return np.concatenate([np.where(mask == 1, v, 0.0), np.where(mask == 2, v, 0.0)], 1)


# ------------------------------------------------------------------------------------------------ comparisons
def _exact(got, ref):
    bad = int((np.asarray(got, np.float64) != np.asarray(ref, np.float64)).sum())
    return {'kind': 'exact', 'bad': bad, 'n': int(np.size(ref))}


def _rel(got, ref, bound):
    ref = np.asarray(ref, np.float64)
    err = float(np.abs(np.asarray(got, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))
    return {'kind': 'tol', 'err': err, 'bound': bound}


def _stored(got, ref, dtype):
    """A buffer stored in T against the float64 value in front of its store: rl._bf16 (the rounded reference or one ulp from
    it, at most FLIP_CAP['emb'] not equal; further off only inside the rounded image of F32_TOL max|ref| around the reference,
    which can matter only next to zero) on bf16 plans, F32_TOL of the largest value on f32 plans."""
    return rl._bf16('emb', got, ref) if dtype == 'bf16' else _rel(got, ref, F32_TOL)


def _decision(got, want, margin, allowed, tol, forced=None):
    """got / want: recorded and float64 codes; margin: the float64 distance to another outcome; allowed: got is one of the
    candidates within tol.  forced: elements checked whatever their margin (ties by construction)."""
    got, want = np.asarray(got).astype(np.int64), np.asarray(want).astype(np.int64)
    decisive = margin > tol
    if forced is not None:
        decisive = decisive | forced
    return {'kind': 'decision', 'wrong': int(((got != want) & decisive).sum()), 'outside': int((~allowed & ~decisive).sum()),
            'excluded': float((~decisive).mean()), 'cap': EXCLUDED_CAP, 'n': int(got.size),
            'seen': sorted(int(v) for v in np.unique(want[decisive]))}


def _mask_check(got, pre, drop, tol):
    """Maxout decision on pre-activations [n,4802] (both operands carry the same 1 / keep, so margins are taken in front of it)."""
    za, zb = fc_halves(pre, drop)
    top = np.maximum(za, zb)
    want = np.where(top > 0, np.where(za >= zb, 1, 2), 0)
    with np.errstate(invalid='ignore'):
        gap = np.abs(np.maximum(za, 0) - np.maximum(zb, 0))
    margin = np.where(top > 0, np.minimum(top, gap), -top)
    got = np.asarray(got).astype(np.int64)
    allowed = np.where(got == 1, (za > -tol) & (za >= np.maximum(zb, 0) - tol),
                       np.where(got == 2, (zb > -tol) & (zb >= np.maximum(za, 0) - tol), (got == 0) & (top <= tol)))
    forced = np.zeros(want.shape, bool)
    tied = list(TIE_UNITS)
    forced[:, tied] = (za[:, tied] == zb[:, tied]) & (za[:, tied] > tol)          # an exact tie above zero: the first operand
    return _decision(got, want, margin, allowed, tol, forced)


def _gate(dy, act):
    return {'kind': 'exact', 'bad': int(((np.asarray(act) <= 0) & (np.asarray(dy) != 0)).sum()), 'n': int(np.size(dy))}


def check(dev, p, frames, d_sal, dtype, keep=None, drop=None, stages=FWD + BWD):
    """dev: the device's buffers (shapes()), 'sal' [n,2401], 'sal7' [n,49] and 'grads' {variable: gradient} -> {stage: figures},
    every stage from the device's own inputs to it.  keep / drop: the dropout site's keep probability and bytes [n,4802]."""
    rT = round_T(dtype)
    f64 = torch.float64
    W = {k: rT(p[k]) if k.endswith('_w') else np.asarray(p[k], np.float64) for k in PARAMS}
    n, hw = frames.shape[0], frames.shape[1]
    g = geom(hw)
    inv = 1.0 / keep if drop is not None else 1.0
    d = {k: np.asarray(v, np.float64) for k, v in dev.items() if k != 'grads'}
    grads = dev.get('grads', {})
    out = {}
    want = lambda k: k in stages
    if want('frames4'):
        out['frames4'] = _exact(d['frames4'], rT(frames))
    if want('pool1') or want('amax1'):
        win = windows2x2(conv_valid(d['frames4'], W['conv1_w'], f64))
        out['pool1'] = _stored(d['pool1'], np.maximum(win.max(3) + W['conv1_b'], 0.0), dtype)
        if 'amax1' in d and want('amax1'):
            tol = F32_TOL * np.abs(win).max()
            srt = np.sort(win, 3)
            code = np.clip(d['amax1'].astype(np.int64), 0, 3)
            chosen = np.take_along_axis(win, code[:, :, :, None, :], 3)[:, :, :, 0, :]
            out['amax1'] = _decision(d['amax1'], win.argmax(3), srt[:, :, :, 3] - srt[:, :, :, 2],
                                     (chosen >= srt[:, :, :, 3] - tol) & (code == d['amax1']), tol)
    for act, src, w, b, pool, amax in (('act2', 'pool1', 'conv2_w', 'conv2_b', 'pool2', 'amax2'),
                                       ('act3', 'pool2', 'conv3_w', 'conv3_b', 'pool3', 'amax3')):
        if want(act):
            out[act] = _stored(d[act], np.maximum(conv_valid(d[src].reshape(shapes(hw, n)[src]), W[w], f64) + W[b], 0.0), dtype)
        if want(pool) or want(amax):
            win = windows3x3(d[act])
            out[pool] = _exact(d[pool].reshape(n, -1), win.max(3).reshape(n, -1))
            if amax in d and want(amax):
                out[amax] = _exact(d[amax], win.argmax(3))
                out[amax]['seen'] = sorted(int(v) for v in np.unique(d[amax]))
    if want('mo1') or want('mask1'):
        pre = matmul(d['pool3'], W['fc1_w'], f64) + W['fc1_b']
        za, zb = fc_halves(pre, drop)
        out['mo1'] = _stored(d['mo1'], np.maximum(np.maximum(za, zb), 0.0) * inv, dtype)
        if 'mask1' in d and want('mask1'):
            out['mask1'] = _mask_check(d['mask1'], pre, drop, F32_TOL * np.abs(pre).max())
    if want('sal') or want('mask2'):
        pre = matmul(d['mo1'], W['fc2_w'], f64) + W['fc2_b']
        za, zb = fc_halves(pre)
        out['sal'] = _rel(d['sal'].reshape(n, 2401), np.maximum(np.maximum(za, zb), 0.0), F32_TOL)
        if 'mask2' in d and want('mask2'):
            out['mask2'] = _mask_check(d['mask2'], pre, None, F32_TOL * np.abs(pre).max())
    if want('sal7'):
        ref = d['sal'].reshape(n, 7, 7, 7, 7).mean(axis=(2, 4)).reshape(n, 49)
        err = np.abs(d['sal7'].reshape(n, 49) - ref) / np.maximum(ref, 1e-300)
        out['sal7'] = {'kind': 'tol', 'err': float(err.max()), 'bound': SAL7_TOL}
    # ---- backward
    if want('dz2'):
        out['dz2'] = _exact(d['dz2'], route(rT(d_sal).reshape(n, 2401), d['mask2']))
    if want('fc2_b'):
        out['fc2_b'] = _rel(grads['fc2_b'], d['dz2'].sum(0), GRAD_TOL)
    if want('fc2_w'):
        out['fc2_w'] = _rel(grads['fc2_w'], matmul(d['mo1'].T, d['dz2'], f64), GRAD_TOL)
    if want('dmo1'):
        out['dmo1'] = _rel(d['dmo1'], matmul(d['dz2'], W['fc2_w'].T, f64), F32_TOL)
    if want('dz1'):
        out['dz1'] = _stored(d['dz1'], route(d['dmo1'] * inv, d['mask1']), dtype)
    if want('fc1_b'):
        out['fc1_b'] = _rel(grads['fc1_b'], d['dz1'].sum(0), GRAD_TOL)
    if want('fc1_w'):
        out['fc1_w'] = _rel(grads['fc1_w'], matmul(d['pool3'].T, d['dz1'], f64), GRAD_TOL)
    if want('dpool3'):
        out['dpool3'] = _rel(d['dpool3'], matmul(d['dz1'], W['fc1_w'].T, f64), F32_TOL)
    for dy, dp, amax, act, src, w, b, dnext, in_h in (('dy3', 'dpool3', 'amax3', 'act3', 'pool2', 'conv3_w', 'conv3_b', 'dpool2', g['p2']),
                                                      ('dy2', 'dpool2', 'amax2', 'act2', 'pool1', 'conv2_w', 'conv2_b', 'dpool1', g['p1'])):
        if want(dy):
            out[dy] = _stored(d[dy], unpool3x3(d[dp].reshape(shapes(hw, n)[amax]), d[amax], d[act]), dtype)
        if want(dy + '_gate'):
            out[dy + '_gate'] = _gate(d[dy], d[act])
        if want(b):
            out[b] = _rel(grads[b], d[dy].sum(axis=(0, 1, 2)), GRAD_TOL)
        if want(w):
            out[w] = _rel(grads[w], conv_wgrad(d[src], d[dy], 3, f64), GRAD_TOL)
        if want(dnext):
            out[dnext] = _rel(d[dnext], conv_dgrad(d[dy], W[w], in_h, f64), F32_TOL)
    if want('dy1'):
        out['dy1'] = _stored(d['dy1'], unpool2x2(d['dpool1'], d['amax1'], d['pool1']), dtype)
    if want('dy1_gate'):
        out['dy1_gate'] = _gate(d['dy1'].reshape(n, g['p1'], 2, g['p1'], 2, 32), d['pool1'][:, :, None, :, None, :])
    if want('conv1_b'):
        out['conv1_b'] = _rel(grads['conv1_b'], d['dy1'].sum(axis=(0, 1, 2)), GRAD_TOL)
    if want('conv1_w'):
        out['conv1_w'] = _rel(grads['conv1_w'], conv_wgrad(d['frames4'], d['dy1'], 5, f64), GRAD_TOL)
    return out


def report(tag, errs):
    for k, e in errs.items():
        if 'flips' in e:
            print('%s %s: %d of %d not the rounded reference (%.5f %%, cap %.2f %%), %d of them by more than one ulp inside the f32 '
                  'bound near zero, worst outside it %d ulp' % (tag, k, e['n_flips'], e['n'], 100 * e['flips'], 100 * e['cap'],
                                                                e['n_near_zero'], e['err']))
        elif e['kind'] == 'exact':
            print('%s %s: %d of %d differ (exact)%s' % (tag, k, e['bad'], e['n'], ' codes seen %s' % e['seen'] if 'seen' in e else ''))
        elif e['kind'] == 'decision':
            print('%s %s: %d decisive wrong, %.5f %% of %d excluded (cap %.2f %%), %d of the excluded not a candidate, codes seen %s'
                  % (tag, k, e['wrong'], 100 * e['excluded'], e['n'], 100 * e['cap'], e['outside'], e['seen']))
        else:
            print('%s %s: %.3e (bound %.3e)' % (tag, k, e['err'], e['bound']))


def violations(errs, margin=1.0):
    """Names of the stages whose figures are not within their bounds; margin tightens every bound that is a tolerance, a flip
    cap or an excluded share (more than one bf16 ulp, an exact mismatch and a wrong decisive choice are violations as they are)."""
    bad = []
    for k, e in errs.items():
        if 'flips' in e:
            ok = e['err'] <= 1 and e['flips'] * margin <= e['cap']
        elif e['kind'] == 'exact':
            ok = e['bad'] == 0
        elif e['kind'] == 'decision':
            ok = e['wrong'] == 0 and e['outside'] == 0 and e['excluded'] * margin <= e['cap']
        else:
            ok = e['err'] * margin <= e['bound']
        if not ok:
            bad.append(k)
    return bad


# ------------------------------------------------------------------------------------------------ the stand-in device
def standin(p, frames, d_sal, dtype, keep=None, drop=None, fault=None):
    """The stages above, chained, with fp32 products and fp32 accumulation (torch fp32) -> dev dict as check() takes it.
    fault: one of FAULTS."""
    assert fault is None or fault in FAULTS
    f32, F = torch.float32, np.float32                               # F: numpy's fp32 from here on
    rT = round_T(dtype)
    store = lambda v: rT(np.asarray(v, F)).astype(F)
    W = {k: (rT(p[k]) if k.endswith('_w') else np.asarray(p[k])).astype(F) for k in PARAMS}
    n, hw = frames.shape[0], frames.shape[1]
    g = geom(hw)
    inv = F(1.0) / F(keep) if drop is not None else F(1.0)
    relu = lambda v: np.maximum(v, F(0))
    dev = {'frames4': store(frames)}
    win = windows2x2(conv_valid(dev['frames4'], W['conv1_w'], f32))
    dev['amax1'] = (relu(win + W['conv1_b']) if fault == 'argmax_after_relu' else win).argmax(3).astype(F)
    dev['pool1'] = store(relu(win.max(3) + W['conv1_b']))
    for act, src, w, b, pool, amax in (('act2', 'pool1', 'conv2_w', 'conv2_b', 'pool2', 'amax2'),
                                       ('act3', 'pool2', 'conv3_w', 'conv3_b', 'pool3', 'amax3')):
        v = relu(conv_valid(dev[src], W[w], f32) + W[b])
        dev[act] = bf16_trunc(v).astype(F) if fault == 'bf16_trunc_store' and act == 'act2' and dtype == 'bf16' else store(v)
        win = windows3x3(dev[act], 0 if fault == 'same_pad_after' else None)
        dev[pool] = win.max(3)
        dev[amax] = (8 - win[:, :, :, ::-1].argmax(3) if fault == 'pool_last_max' else win.argmax(3)).astype(F)
    dev['pool3'] = dev['pool3'].reshape(n, -1)

    def maxout(x, w, bias, drop, inv):
        za, zb = fc_halves(matmul(x, W[w], f32) + W[bias], drop)
        a, b = relu(za) * inv, relu(zb) * inv
        first = a > b if fault == 'maxout_tie_second' else a >= b
        mask = np.where(np.maximum(a, b) > 0, np.where(first, 1, 2), 0)
        if fault == 'mask_halves_swapped':
            mask = np.where(mask > 0, 3 - mask, 0)
        return np.maximum(a, b).astype(F), mask.astype(F)
    mo1, dev['mask1'] = maxout(dev['pool3'], 'fc1_w', 'fc1_b', drop, inv)
    dev['mo1'] = store(mo1)
    dev['sal'], dev['mask2'] = maxout(dev['mo1'], 'fc2_w', 'fc2_b', None, F(1.0))
    dev['sal7'] = dev['sal'].reshape(n, 7, 7, 7, 7).mean(axis=(2, 4), dtype=F).reshape(n, 49)
    # ---- backward
    gr = {}
    dev['dz2'] = route(store(d_sal).reshape(n, 2401), dev['mask2']).astype(F)
    gr['fc2_b'] = dev['dz2'].sum(0, dtype=F)
    gr['fc2_w'] = matmul(dev['mo1'].T, dev['dz2'], f32)
    dev['dmo1'] = matmul(dev['dz2'], W['fc2_w'].T, f32)
    dev['dz1'] = store(route(dev['dmo1'] * (F(1.0) if fault == 'no_inv_keep' else inv), dev['mask1']))
    gr['fc1_b'] = dev['dz1'].sum(0, dtype=F)
    gr['fc1_w'] = matmul(dev['pool3'].T, dev['dz1'], f32)
    dev['dpool3'] = matmul(dev['dz1'], W['fc1_w'].T, f32)
    pad = 0 if fault == 'same_pad_after' else None
    for dy, dp, amax, act, src, w, b, dnext, in_h in (('dy3', 'dpool3', 'amax3', 'act3', 'pool2', 'conv3_w', 'conv3_b', 'dpool2', g['p2']),
                                                      ('dy2', 'dpool2', 'amax2', 'act2', 'pool1', 'conv2_w', 'conv2_b', 'dpool1', g['p1'])):
        dev[dy] = store(unpool3x3(dev[dp].reshape(dev[amax].shape), dev[amax], dev[act], pad, gate=not (fault == 'grad_to_gated' and dy == 'dy3')))
        h = dev[dy].shape[1]
        gr[b] = (dev[dy][:, :h - 2, :h - 2] if fault == 'bias_grad_halo' and dy == 'dy3' else dev[dy]).sum(axis=(0, 1, 2), dtype=F)
        gr[w] = conv_wgrad(dev[src], dev[dy], 3, f32)
        wd = W[w]
        if fault == 'dgrad_not_rotated' and dy == 'dy3':
            wd = wd[::-1, ::-1]
        if fault == 'dgrad_unswapped' and dy == 'dy2':                   # the [ci][co] plane of every tap read as [co][ci]
            wd = np.ascontiguousarray(wd).reshape(3, 3, wd.shape[3], wd.shape[2]).transpose(0, 1, 3, 2)
        dev[dnext] = conv_dgrad(dev[dy], wd, in_h, f32)
    dev['dy1'] = store(unpool2x2(dev['dpool1'], dev['amax1'], dev['pool1']))
    gr['conv1_b'] = dev['dy1'].sum(axis=(0, 1, 2), dtype=F)
    gr['conv1_w'] = conv_wgrad(dev['frames4'], dev['dy1'], 5, f32)
    dev['grads'] = gr
    return dev
