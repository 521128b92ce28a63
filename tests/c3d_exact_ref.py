"""Operands for which the C3D forward has ONE right answer, and the float64 chain that computes it (test helper).

With integer video samples, filters of a few entries +-2^-2 per output channel and biases that are multiples of 2^-2, every
product and every partial sum of a layer is a multiple of `unit` = (smallest lsb among the layer's non-zero inputs) * 2^-2 and
no larger in magnitude than max(sum |a w| + |b|).  While log2 of that ratio -- the layer's HEADROOM, in bits -- stays below the
24 bits of an fp32 significand, any fp32 accumulation of the layer is exact whatever its summation order, tile shape or
kernel; the bf16 store (round to nearest even) is the one rounding left and it is deterministic.  A kernel then has to
reproduce the chain below bit for bit.

Layouts are the project's: video [n,16,H,W,3], filters DHWIO [3,3,3,Cin,Cout] with K index ((kd*3+kh)*3+kw)*Cin+ci,
activations NDHWC, rows [n*h*w, d*512+c], features [n,1024,h,w] with channel c*2+d.
"""
import functools
import os

import numpy as np
import torch

SPECS = (('conv1a', 3, 64, (1, 2)), ('conv2a', 64, 128, (2, 2)), ('conv3a', 128, 256, None), ('conv3b', 256, 256, (2, 2)),
         ('conv4a', 256, 512, None), ('conv4b', 512, 512, (2, 2)), ('conv5a', 512, 512, None), ('conv5b', 512, 512, None))
NAMES = tuple(s[0] for s in SPECS)
W_MAG = 0.25                   # every non-zero filter entry is +-2^-2; biases are multiples of it
VIDEO_MAX = 4                  # video samples: integers in [-VIDEO_MAX, VIDEO_MAX] (exact in bf16)
# Nominal standard deviation of each layer's pre-activation under this recipe, which only scales the bias draw
# N(0, 0.3 sd): measured once by calibrate_sd() on one 16x32x32 window of filter set 0, rounded to two digits.  The tests
# do not rely on these figures; they assert the zero fractions and the headroom of the chain they actually compare with.
PREACT_SD = {32: (3.5, 6.0, 8.3, 7.4, 8.8, 7.4, 7.4, 4.2), 16: (2.5, 3.0, 3.4, 2.3, 1.8, 1.1, 0.74, 0.29)}


def exact_params(set_id, nnz=32, sd=None):
    """{name_w: [3,3,3,Cin,Cout], name_b: [Cout]} fp32.  Output channel `cout` of a layer has its nnz non-zero entries at
    the K indices perm[(nnz*cout + j) % K], j < nnz, of ONE permutation of range(K): distinct within a channel, and every
    (tap, cin) is hit as soon as nnz*Cout >= K (all eight layers at nnz = 32).  Permutation and signs depend on set_id."""
    rs = np.random.RandomState(9000 + 17 * int(set_id) + nnz)
    sd = PREACT_SD[nnz] if sd is None else sd
    p = {}
    for i, (name, cin, cout, _) in enumerate(SPECS):
        k = 27 * cin
        m = min(nnz, k)
        perm = rs.permutation(k)
        pos = perm[(m * np.arange(cout)[:, None] + np.arange(m)[None, :]) % k]                    # [cout, m]
        w = np.zeros((k, cout), np.float32)
        w[pos, np.arange(cout)[:, None]] = rs.choice([-W_MAG, W_MAG], size=(cout, m)).astype(np.float32)
        p[name + '_w'] = w.reshape(3, 3, 3, cin, cout)
        p[name + '_b'] = (np.round(rs.randn(cout) * 0.3 * sd[i] * 4) / 4).astype(np.float32)
    return p


def exact_video(seed, n, frames=16, hw=112):
    """[n,frames,hw,hw,3] fp32, integers uniform in [-VIDEO_MAX, VIDEO_MAX]."""
    rs = np.random.RandomState(seed)
    return rs.randint(-VIDEO_MAX, VIDEO_MAX + 1, size=(n, frames, hw, hw, 3)).astype(np.float32)


def min_lsb_exp(x):
    """log2 of the smallest lsb (largest power of two dividing the value) among the non-zero elements of float64 x."""
    x = np.abs(np.asarray(x, np.float64)).ravel()
    x = x[x != 0]
    if x.size == 0:
        return 0
    m, e = np.frexp(x)
    mi = (m * 2.0 ** 53).astype(np.int64)
    low = (mi & -mi).astype(np.float64)
    return int((np.log2(low) + e - 53).min())


def bf16_rne(x):
    return x.float().bfloat16().double()


def bf16_trunc(x):
    """Chop the low 16 bits of the fp32 pattern (toward zero) -- the rounding a correct store must NOT use."""
    bits = x.float().contiguous().view(torch.int32) & -65536
    return bits.view(torch.float32).double()


def sparse_conv(xp, w, want_abs=True):
    """xp [Cin,n,D+2,H+2,W+2] float64 (zero halo included), w [3,3,3,Cin,Cout] -> (z [Cout,n,D,H,W] float64 without bias,
    max over all outputs of sum |a w|).  Sums one shifted slice of xp per non-zero filter entry."""
    cin, n, d, h, wd = xp.shape
    d, h, wd = d - 2, h - 2, wd - 2
    w = np.asarray(w, np.float64)
    cout = w.shape[-1]
    wk = w.reshape(27 * cin, cout)
    xa = xp.abs() if want_abs and bool((xp < 0).any()) else None
    z = torch.empty(cout, n, d, h, wd, dtype=torch.float64)
    pos, neg = torch.empty_like(z[0]), torch.empty_like(z[0])
    absmax = 0.0
    for co in range(cout):
        pos.zero_()
        neg.zero_()
        if xa is not None:
            acc = z[co].zero_()
        for k in np.flatnonzero(wk[:, co]):
            tap, ci = divmod(int(k), cin)
            kd, kh, kw = tap // 9, (tap // 3) % 3, tap % 3
            v = float(wk[k, co])
            if xa is None:      # inputs >= 0: positive and negative parts give the sum and the sum of magnitudes
                (pos if v > 0 else neg).add_(xp[ci, :, kd:kd + d, kh:kh + h, kw:kw + wd], alpha=abs(v))
            else:
                acc.add_(xp[ci, :, kd:kd + d, kh:kh + h, kw:kw + wd], alpha=v)
                pos.add_(xa[ci, :, kd:kd + d, kh:kh + h, kw:kw + wd], alpha=abs(v))
        if xa is None:
            torch.sub(pos, neg, out=z[co])
            if want_abs:
                absmax = max(absmax, float(pos.add_(neg).max()))
        else:
            absmax = max(absmax, float(pos.max()))
    return z, absmax


def pad_input(x_ndhwc):
    """[n,D,H,W,C] -> channel-major with the zero halo: [C,n,D+2,H+2,W+2] float64."""
    x = x_ndhwc.double().permute(4, 0, 1, 2, 3)
    return torch.nn.functional.pad(x, (1, 1, 1, 1, 1, 1)).contiguous()


def reference_chain(video, params, dtype='bf16', rounding='rne', halo=None, upto='conv5b'):
    """The float64 chain conv + bias + ReLU + max-pool per layer; for dtype 'bf16' each pooled output goes through fp32 and
    the bf16 store (`rounding`: 'rne', or 'trunc' for the sensitivity test) before it feeds the next layer, for 'f32'
    nothing rounds.  halo = (layer, (ci, window, z, y, x), value) overwrites one element of that layer's PADDED input
    (sensitivity test: a stale halo).

    -> dict: 'layers' (pooled outputs, NDHWC fp32 tensors), 'rows' [n*h*w, d*512+c] (bf16 or fp32), 'features'
    [n,1024,h,w] fp32 (channel c*2+d), and per layer 'headroom_bits', 'zero_frac', 'unit_exp', 'rne_trunc_differ' (how
    many stored elements RNE and truncation would store differently), 'exact_in_f32' (the pre-store values survive a
    cast to fp32; implied by headroom <= 24, asserted by the tests)."""
    x = torch.as_tensor(np.asarray(video), dtype=torch.float64)
    out = {'layers': [], 'headroom_bits': [], 'zero_frac': [], 'unit_exp': [], 'rne_trunc_differ': [], 'exact_in_f32': []}
    for i, (name, cin, cout, pool) in enumerate(SPECS):
        xp = pad_input(x)
        if halo is not None and halo[0] == i:
            xp[tuple(halo[1])] = halo[2]
        b = torch.as_tensor(np.asarray(params[name + '_b']), dtype=torch.float64)
        z, absmax = sparse_conv(xp, params[name + '_w'])
        unit_exp = min(min_lsb_exp(xp.numpy()), 0) + int(np.log2(W_MAG))
        out['unit_exp'].append(unit_exp)
        out['headroom_bits'].append(float(np.log2(absmax + float(b.abs().max()))) - unit_exp)
        z = torch.relu(z + b.view(-1, 1, 1, 1, 1))
        if pool is not None:
            z = torch.nn.functional.max_pool3d(z, (pool[0], pool[1], pool[1]))
        z = z.permute(1, 2, 3, 4, 0).contiguous()                                   # NDHWC
        out['exact_in_f32'].append(bool(torch.equal(z.float().double(), z)))
        if dtype == 'bf16':
            out['rne_trunc_differ'].append(int((bf16_rne(z) != bf16_trunc(z)).sum()))
            z = bf16_rne(z) if rounding == 'rne' else bf16_trunc(z)
        else:
            out['rne_trunc_differ'].append(0)
        out['zero_frac'].append(float((z == 0).double().mean()))
        out['layers'].append(z.float())
        x = z
        if name == upto:
            break
    if len(out['layers']) == 8:
        last = out['layers'][7]                                                     # [n,2,h,w,512]
        n, d, h, w, c = last.shape
        rows = last.permute(0, 2, 3, 1, 4).reshape(n * h * w, d * c)
        out['rows'] = rows.bfloat16() if dtype == 'bf16' else rows.contiguous()
        out['features'] = last.permute(0, 4, 1, 2, 3).reshape(n, c * d, h, w).contiguous()
    return out


def calibrate_sd(nnz, hw=32, seed=1):
    """How PREACT_SD was obtained: walk the layers, measuring each pre-activation's standard deviation before its bias
    is drawn.  Not used by the tests."""
    sd = [1.0] * 8
    video = exact_video(seed, 1, hw=hw)
    for i in range(8):
        p = exact_params(0, nnz, sd=sd)
        x = torch.as_tensor(video, dtype=torch.float64)
        if i:
            x = reference_chain(video, p, 'bf16' if nnz == 32 else 'f32', upto=NAMES[i - 1])['layers'][-1].double()
        sd[i] = float('%.2g' % float(sparse_conv(pad_input(x), p[NAMES[i] + '_w'], want_abs=False)[0].std()))
    return tuple(sd)


def probed_k(params, layer):
    """Boolean [K]: which (tap, cin) of `layer` at least one output channel multiplies."""
    w = np.asarray(params[NAMES[layer] + '_w'])
    return (w.reshape(-1, w.shape[-1]) != 0).any(1)


def first_mismatch(got, want, name, show=5):
    """None when got and want (same shape, [window, z, y, x, c] or anything else) are equal element for element, else a
    message: the layer, how many elements differ and the first few coordinates with both values."""
    got, want = torch.as_tensor(got).detach().cpu(), torch.as_tensor(want).detach().cpu()
    if got.shape != want.shape:
        return '%s: shape %s, expected %s' % (name, tuple(got.shape), tuple(want.shape))
    if got.dtype != want.dtype:
        got, want = got.double(), want.double()
    if torch.equal(got, want):
        return None
    idx = torch.nonzero(got != want)
    lines = ['%s: %d of %d elements differ; first at (%s):' % (name, idx.shape[0], got.numel(),
                                                                'window, z, y, x, c' if got.dim() == 5 else 'index')]
    for j in idx[:show].tolist():
        lines.append('  %s got %r want %r' % (tuple(j), float(got[tuple(j)]), float(want[tuple(j)])))
    return '\n'.join(lines)


# ---------------------------------------------------------------------------------------------------------------------
# The backward half: operands for which every GRADIENT of the conv stack has one right answer, and the float64 chain
# that computes it.  Two recipes (the forward recipe above does not serve: each +-2^-2 layer costs two bits of lsb on the
# way up and two on the way down, so a filter gradient of exact_params(0, 32) needs 24 ... 27 bits):
#   light_params         four entries +-1 per output channel, integer biases: with an integer upstream gradient nothing
#                        ever leaves the integers; every filter, bias and input gradient fits fp32 with bits to spare.
#   tap_complete_params  +-2^-2, one entry per (tap, cout): every tap of the rotated filter is multiplied by something and
#                        the bf16 store of the gradient images really rounds; its filter gradients are NOT exact.
# ---------------------------------------------------------------------------------------------------------------------
POOLED = tuple(i for i, s in enumerate(SPECS) if s[3] is not None)


def _covering_perm(rs, cin):
    """A permutation of range(27 * cin) (K index tap * cin + ci) made of 27 blocks of cin entries; block b holds every
    input channel once, channel ci with its b-th tap of a per-channel permutation of the 27 taps.  Any cin consecutive
    entries from a block boundary therefore name every input channel."""
    taps = np.stack([rs.permutation(27) for _ in range(cin)])                       # [cin, 27]
    blocks = []
    for b in range(27):
        order = rs.permutation(cin)
        blocks.append(taps[order, b] * cin + order)
    return np.concatenate(blocks)


def light_params(set_id, nnz=4, dense_from=8):
    """{name_w, name_b} fp32, nnz (even) entries +-1 per output channel, biases round(N(0, 1)).  nnz / 2 entries +1 sit at
    perm[(nnz/2 * cout + j) % K], j < nnz / 2, of ONE permutation (_covering_perm: nnz/2 * Cout >= Cin in every layer, so
    every input channel of every layer is multiplied by some filter); each has a partner -1 on the SAME input channel at
    the opposite tap 26 - tap (a central difference; every input channel is thereby read from two sides).
    Pairs, because from conv2a on the inputs are >= 0 and the channels' magnitudes drift apart with depth: a filter of
    independent +-1 entries takes the sign of its largest input nearly everywhere, and the channels it leaves dead or
    almost so are zero columns of the layer's filter gradient and zero channels of its gradient image, which no comparison
    can check.  A sum of differences of two shifts of one channel is positive at about half the positions whatever the
    sizes of its inputs.
    Layers dense_from ... 7 instead take every entry as +1 and biases >= 1: with inputs >= 0 all their outputs are positive
    (case_t: the small top layers with no zero anywhere, so that every entry of their filter gradients is reached)."""
    assert nnz % 2 == 0
    rs = np.random.RandomState(9500 + 17 * int(set_id) + nnz)
    p = {}
    m = nnz // 2
    for i, (name, cin, cout, _) in enumerate(SPECS):
        k = 27 * cin
        perm = _covering_perm(rs, cin)
        pos = perm[(m * np.arange(cout)[:, None] + np.arange(m)[None, :]) % k]                     # [cout, m]
        w = np.zeros((k, cout), np.float32)
        w[pos, np.arange(cout)[:, None]] = 1.0
        shift = rs.randint(1, 27, size=(cout, m))
        for co in range(cout):
            for j in range(m):
                tap, ci = divmod(int(pos[co, j]), cin)
                tap = 26 - tap if tap != 13 else (tap + shift[co, j]) % 27          # the opposite tap; the centre has none
                while w[tap * cin + ci, co] != 0:          # (taken by another entry of this filter)
                    tap = (tap + 1) % 27
                w[tap * cin + ci, co] = -1.0
        bias = np.round(rs.randn(cout))
        if i >= dense_from:
            assert i >= 1
            w, bias = np.abs(w), np.abs(bias) + 1
        p[name + '_w'] = w.reshape(3, 3, 3, cin, cout)
        p[name + '_b'] = bias.astype(np.float32)
    return p


def tap_complete_params(set_id):
    """{name_w, name_b} fp32: +-2^-2 at (tap, perm_tap[cout % Cin], cout) for every tap and cout -- 27 entries per filter,
    every (tap, cout) and (Cout >= Cin in every layer) every (tap, cin) non-zero somewhere.  Biases as exact_params."""
    rs = np.random.RandomState(9700 + 17 * int(set_id))
    p = {}
    for i, (name, cin, cout, _) in enumerate(SPECS):
        w = np.zeros((27, cin, cout), np.float32)
        for tap in range(27):
            ci = rs.permutation(cin)[np.arange(cout) % cin]
            w[tap, ci, np.arange(cout)] = rs.choice([-W_MAG, W_MAG], size=cout).astype(np.float32)
        p[name + '_w'] = w.reshape(3, 3, 3, cin, cout)
        p[name + '_b'] = (np.round(rs.randn(cout) * 0.3 * PREACT_SD[32][i] * 4) / 4).astype(np.float32)
    return p


def exact_upstream(seed, n, density=2.0 / 3.0, gmax=1, hw=7):
    """Gradient w.r.t. the features, [n,1024,hw,hw] fp32: non-zero with probability `density`, then uniform over the
    integers +-1 ... +-gmax.  The defaults are the dense {-1, 0, 1} draw."""
    rs = np.random.RandomState(seed)
    shape = (n, 1024, hw, hw)
    mag = rs.randint(1, gmax + 1, size=shape) * rs.choice([-1, 1], size=shape)
    return (mag * (rs.rand(*shape) < density)).astype(np.float32)


def _to_win(t, pd, ph):
    """[C,n,D,H,W] -> [C,n,D/pd,H/ph,W/ph,pd*ph*ph], members in (dz, dy, dx) order."""
    c, n, d, h, w = t.shape
    return t.reshape(c, n, d // pd, pd, h // ph, ph, w // ph, ph).permute(0, 1, 2, 4, 6, 3, 5, 7).reshape(
        c, n, d // pd, h // ph, w // ph, pd * ph * ph)


def _from_win(t, pd, ph):
    c, n, do, ho, wo, _ = t.shape
    return t.reshape(c, n, do, ho, wo, pd, ph, ph).permute(0, 1, 2, 5, 3, 6, 4, 7).reshape(c, n, do * pd, ho * ph, wo * ph)


def _store(x, dtype, rounding='rne'):
    if dtype != 'bf16':
        return x
    return bf16_rne(x) if rounding == 'rne' else bf16_trunc(x)


def _lsb(x):
    return min(min_lsb_exp(x.numpy() if isinstance(x, torch.Tensor) else x), 0)


def _bits(absmax, unit_exp):
    return float(np.log2(absmax)) - unit_exp if absmax > 0 else 0.0


def sparse_dgrad(dy, w, swap=None, want_abs=True):
    """dy [Cout,n,D,H,W] float64, w [3,3,3,Cin,Cout] -> (d loss / d input [Cin,n,D,H,W], max sum |dy w|): one shifted
    slice added per non-zero filter entry -- the transpose of sparse_conv.  swap = (t1, t2): the fault 'two taps swapped'."""
    cout, n, d, h, wd = dy.shape
    w = np.asarray(w, np.float64)
    cin = w.shape[3]
    wk = w.reshape(27 * cin, cout)
    dxp = torch.zeros(cin, n, d + 2, h + 2, wd + 2, dtype=torch.float64)
    axp = torch.zeros_like(dxp) if want_abs else None
    ady = dy.abs() if want_abs else None
    for k, co in zip(*(a.tolist() for a in np.nonzero(wk))):
        tap, ci = divmod(k, cin)
        if swap is not None and tap in swap:
            tap = swap[1] if tap == swap[0] else swap[0]
        kd, kh, kw = tap // 9, (tap // 3) % 3, tap % 3
        v = float(wk[k, co])
        dxp[ci, :, kd:kd + d, kh:kh + h, kw:kw + wd].add_(dy[co], alpha=v)
        if want_abs:
            axp[ci, :, kd:kd + d, kh:kh + h, kw:kw + wd].add_(ady[co], alpha=abs(v))
    inner = (slice(None), slice(None), slice(1, -1), slice(1, -1), slice(1, -1))
    return dxp[inner].contiguous(), float(axp[inner].max()) if want_abs else 0.0


def tap_wgrad(xp, dy, want_abs=True):
    """xp [Cin,n,D+2,H+2,W+2] float64 (zero halo), dy [Cout,n,D,H,W] float64 -> per window: (dW [27,Cin,Cout] float64,
    max over the entries of sum |x dy|), and how many entries have sum |x dy| = 0 over all windows together.  One matrix product per tap and window; the sums of magnitudes in fp32
    (they only feed log2 and a test for zero, and a sum of non-negative integers is zero in fp32 only if every term is)."""
    cin, n, d, h, wd = xp.shape
    d, h, wd = d - 2, h - 2, wd - 2
    cout = dy.shape[0]
    dyt = [dy[:, j].reshape(cout, -1).t().contiguous() for j in range(n)]
    ayt = [t.abs().float() for t in dyt]
    dws = [torch.empty(27, cin, cout, dtype=torch.float64) for _ in range(n)]
    amax, untouched = [0.0] * n, 0
    for tap in range(27):
        kd, kh, kw = tap // 9, (tap // 3) % 3, tap % 3
        total = 0
        for j in range(n):
            xt = xp[:, j, kd:kd + d, kh:kh + h, kw:kw + wd].reshape(cin, -1)
            torch.mm(xt, dyt[j], out=dws[j][tap])
            if want_abs:
                a = torch.mm(xt.abs().float(), ayt[j])
                amax[j] = max(amax[j], float(a.max()))
                total = total + a
        if want_abs:
            untouched += int((total == 0).sum())
    return dws, amax, untouched


def backward_chain(video, params, g, dtype='bf16', fault=None, bounds=True, stop_at=0):
    """Forward and backward of the conv stack in float64, layer by layer, as the kernels compose it: conv + bias + ReLU
    + max-pool with the bf16 store (RNE) of every pooled output; then from conv5b down the filter gradient (DHWIO) and
    bias gradient of the layer from its stored input and its gradient image dY, the input gradient, and the image of the
    layer below -- un-pooled: gated by (stored activation > 0) and stored (bf16 RNE); pooled: the dense pooled gradient
    stored (bf16 RNE) FIRST, then gated and routed to the first maximum in (dz, dy, dx) order of the float64 conv output.
    dtype 'f32': nothing rounds.  bounds=False skips the sums of magnitudes (headroom_bits, abs_max and untouched are then
    meaningless); stop_at: the lowest layer whose gradients are wanted (everything below stays None / absent).
    Gradients are kept PER WINDOW (they are linear in windows: combine_windows).

    fault (sensitivity tests only), a dict with any of: 'route': 'last'; 'gate': 'ge'; 'store': 'trunc';
    'swap_taps': (layer, t1, t2) of the input-gradient filter; 'drop_product': (layer, window) one x * dy product missing
    from one filter-gradient entry; 'bias_block': (layer, window, rows) the first `rows` positions missing from a bias sum.

    -> dict: 'dys' (eight [n,D,H,W,Cout] fp32, the layout of read_grad_image), 'layers' / 'features' (as reference_chain),
    'grads' (per window: {name_w: [3,3,3,Cin,Cout], name_b: [Cout]} float64), and per tensor name (name_w, name_b, name_dy)
    'headroom_bits' (all windows summed), 'abs_max' (per window, the numerator of the headroom), 'unit_exp', 'exact_in_f32',
    'untouched' (name_w only: entries whose sum |x dy| over all windows is zero -- no comparison can see a term missing
    from them), 'rounded_elems' (name_dy: elements of the image whose store changed the value; under fault 'store' those
    that RNE and truncation store differently); 'fwd_rounded_elems' (per layer: activations the forward's store changed);
    and per pooled layer name 'tied_frac' (windows with a positive maximum attained more than once) and 'code_hist'."""
    fault = fault or {}
    ge = fault.get('gate') == 'ge'
    on = (lambda a: a >= 0) if ge else (lambda a: a > 0)
    rounding = fault.get('store', 'rne')
    x = torch.as_tensor(np.asarray(video), dtype=torch.float64)
    n = x.shape[0]
    out = {'dys': [None] * 8, 'layers': [], 'grads': [dict() for _ in range(n)], 'headroom_bits': {}, 'abs_max': {}, 'untouched': {},
           'unit_exp': {}, 'exact_in_f32': {}, 'rounded_elems': {}, 'tied_frac': {}, 'code_hist': {}, 'fault_info': {}, 'fwd_rounded_elems': []}
    xps, codes = [], {}
    a = None                                                                        # channel-major activation [C,n,D,H,W]
    for i, (name, cin, cout, pool) in enumerate(SPECS):
        xp = pad_input(x) if i == 0 else torch.nn.functional.pad(a, (1, 1, 1, 1, 1, 1))
        xps.append(xp)
        z = sparse_conv(xp, params[name + '_w'], want_abs=False)[0]
        z += torch.as_tensor(np.asarray(params[name + '_b']), dtype=torch.float64).view(-1, 1, 1, 1, 1)
        if pool is not None:
            zw = _to_win(z, pool[0], pool[1])
            p_ = zw.shape[-1]
            m = zw.max(-1).values
            eq = zw == m.unsqueeze(-1)
            idx = torch.arange(p_).view(1, 1, 1, 1, 1, p_)
            if fault.get('route') == 'last':
                code = torch.where(eq, idx, torch.full_like(idx, -1)).max(-1).values
            else:
                code = torch.where(eq, idx, torch.full_like(idx, p_)).min(-1).values
            pos = m > 0
            out['tied_frac'][name] = float(((eq.sum(-1) > 1) & pos).sum()) / max(int(pos.sum()), 1)
            out['code_hist'][name] = torch.bincount(code[pos].flatten(), minlength=p_).tolist()
            codes[i] = code.to(torch.uint8)
            del zw, eq
            z = m
        z = torch.relu(z)
        a = _store(z, dtype)
        out['fwd_rounded_elems'].append(int((a != z).sum()))
        del z
        out['layers'].append(a.permute(1, 2, 3, 4, 0).contiguous().float())
    last = out['layers'][7]
    _, d5, h5, w5, c5 = last.shape
    out['features'] = last.permute(0, 4, 1, 2, 3).reshape(n, c5 * d5, h5, w5).contiguous()
    acts = [None] + [l.double().permute(4, 0, 1, 2, 3) for l in out['layers']]       # acts[i]: input of layer i, i >= 1

    g5 = torch.as_tensor(np.asarray(g), dtype=torch.float64).reshape(n, c5, d5, h5, w5).permute(1, 0, 2, 3, 4)
    gated = g5 * on(acts[8])
    dy = _store(gated, dtype, rounding)
    out['headroom_bits']['conv5b_dy'] = _bits(float(g5.abs().max()), _lsb(g5))
    out['abs_max']['conv5b_dy'], out['unit_exp']['conv5b_dy'] = float(g5.abs().max()), _lsb(g5)
    out['exact_in_f32']['conv5b_dy'] = True
    out['rounded_elems']['conv5b_dy'] = int((dy != gated).sum())
    for i in range(7, -1, -1):
        name, cin, cout, _ = SPECS[i]
        out['dys'][i] = dy.permute(1, 2, 3, 4, 0).contiguous().float()
        xp = xps[i]
        xps[i] = None
        # filter gradient
        dws, amax, untouched = tap_wgrad(xp, dy, bounds)
        unit = _lsb(xp) + _lsb(dy)
        if fault.get('drop_product', (None,))[0] == i:
            j = fault['drop_product'][1]
            co, z_, y_, x_ = [int(v) for v in torch.nonzero(dy[:, j])[0]]
            tap = next(t for t in range(27) if bool((xp[:, j, z_ + t // 9, y_ + (t // 3) % 3, x_ + t % 3] != 0).any()))
            src = xp[:, j, z_ + tap // 9, y_ + (tap // 3) % 3, x_ + tap % 3]
            ci = int(torch.nonzero(src)[0])
            dws[j][tap, ci, co] -= src[ci] * dy[co, j, z_, y_, x_]
            out['fault_info']['drop_product'] = (tap, ci, co)
        key = name + '_w'
        out['abs_max'][key], out['untouched'][key], out['unit_exp'][key] = amax, untouched, unit
        out['headroom_bits'][key] = _bits(sum(amax), unit)
        out['exact_in_f32'][key] = all(bool(torch.equal(t.float().double(), t)) for t in dws)
        # bias gradient
        key = name + '_b'
        flat = dy.reshape(cout, n, -1)
        dbs = [flat[:, j].sum(1) for j in range(n)]
        if fault.get('bias_block', (None,))[0] == i:
            _, j, rows = fault['bias_block']
            dbs[j] = dbs[j] - flat[:, j, :rows].sum(1)
        babs = [float(flat[:, j].abs().sum(1).max()) for j in range(n)]
        out['abs_max'][key], out['unit_exp'][key] = babs, _lsb(dy)
        out['headroom_bits'][key] = _bits(sum(babs), _lsb(dy))
        out['exact_in_f32'][key] = all(bool(torch.equal(t.float().double(), t)) for t in dbs)
        for j in range(n):
            out['grads'][j][name + '_w'] = dws[j].reshape(3, 3, 3, cin, cout)
            out['grads'][j][name + '_b'] = dbs[j]
        del xp, dws
        if i == stop_at:
            break
        # input gradient, and the gradient image of the layer below
        sw = fault.get('swap_taps')
        dx, absmax = sparse_dgrad(dy, params[name + '_w'], swap=sw[1:] if sw is not None and sw[0] == i else None, want_abs=bounds)
        lo, pool = SPECS[i - 1][0], SPECS[i - 1][3]
        key = lo + '_dy'
        unit = _lsb(dy) + _lsb(np.asarray(params[name + '_w'], np.float64))
        out['abs_max'][key], out['unit_exp'][key] = absmax, unit
        out['headroom_bits'][key] = _bits(absmax, unit)
        out['exact_in_f32'][key] = bool(torch.equal(dx.float().double(), dx))
        gate = on(acts[i])
        other = _store(dx, dtype, 'trunc' if rounding == 'rne' else 'rne') if 'store' in fault else dx
        stored = _store(dx, dtype, rounding)
        out['rounded_elems'][key] = int(((stored != other) & gate).sum())
        gated = stored * gate
        if pool is None:
            dy = gated
        else:
            p_ = pool[0] * pool[1] * pool[1]
            sel = codes[i - 1].long().unsqueeze(-1) == torch.arange(p_).view(1, 1, 1, 1, 1, p_)
            dy = _from_win(sel * gated.unsqueeze(-1), pool[0], pool[1])
            del sel
    return out


def combine_windows(chain, coeffs):
    """sum_j coeffs[j] * (gradients of window j) in float64 -> ({name: tensor}, {name: headroom bits of that combination}).
    The bound is the one of backward_chain with every window's sum of magnitudes scaled by its coefficient."""
    grads, bits = {}, {}
    for key in chain['grads'][0]:
        grads[key] = sum(float(c) * chain['grads'][j][key] for j, c in enumerate(coeffs) if c)
        bits[key] = _bits(sum(float(c) * chain['abs_max'][key][j] for j, c in enumerate(coeffs)), chain['unit_exp'][key])
    return grads, bits


# The cases of tests/test_c3d_exact_bwd_gpu.py, built once per process and shared (never modified); the CPU file asserts
# their premises on the same objects.
SEED_BWD_VIDEO, SEED_BWD_G, LIGHT_NNZ = 4343, 4344, 4


@functools.lru_cache(maxsize=None)
def case_w():
    """Light filters, windows A and B, dense upstream gradient in {-1, 0, 1}, bf16."""
    p = light_params(0, LIGHT_NNZ)
    video = exact_video(SEED_BWD_VIDEO, 2)
    g = exact_upstream(SEED_BWD_G, 2)
    return p, video, g, _with_threads(lambda: backward_chain(video, p, g, 'bf16'))


TOP = 4          # case T: conv4a, conv4b, conv5a, conv5b


@functools.lru_cache(maxsize=None)
def case_t():
    """Case W's filters below conv4b, all-positive filters and biases from conv4b up, upstream gradient +-1 everywhere; the
    backward only down to conv4b.  On the 14 x 14 and 7 x 7 layers case W's gates and routes leave a share of the filter-
    gradient entries without any contribution; here no activation and no upstream element is zero, so every entry of
    d conv4b_w, d conv5a_w and d conv5b_w has one, and the forward's bf16 store rounds (activations pass 256)."""
    p = light_params(0, LIGHT_NNZ, dense_from=TOP)
    video = exact_video(SEED_BWD_VIDEO, 2)
    g = exact_upstream(SEED_BWD_G + 2, 2, density=1.0)
    return p, video, g, _with_threads(lambda: backward_chain(video, p, g, 'bf16', stop_at=TOP))


@functools.lru_cache(maxsize=None)
def case_d():
    """Tap-complete filters, window A, upstream gradient of density 0.3 in {-2 ... 2}, bf16."""
    p = tap_complete_params(0)
    video = exact_video(SEED_BWD_VIDEO, 1)
    g = exact_upstream(SEED_BWD_G + 1, 1, density=0.3, gmax=2)
    return p, video, g, _with_threads(lambda: backward_chain(video, p, g, 'bf16'))


def _with_threads(fn, threads=16):
    old = torch.get_num_threads()
    torch.set_num_threads(min(threads, os.cpu_count() or 1))
    try:
        return fn()
    finally:
        torch.set_num_threads(old)


def describe_chain(chain):
    """One line per class of tensor: what the docstrings of the test files quote."""
    hb = chain['headroom_bits']
    rng = lambda suffix: '%.1f ... %.1f' % (min(v for k, v in hb.items() if k.endswith(suffix)), max(v for k, v in hb.items() if k.endswith(suffix)))
    return ('headroom bits: filter %s, bias %s, image %s; tied windows %s; image elements rounded by the store %s, activations '
            '%s; zeros %s; filter-gradient entries nothing contributes to %s' % (
                rng('_w'), rng('_b'), rng('_dy'), {k: '%.3f' % v for k, v in chain['tied_frac'].items()},
                [chain['rounded_elems'].get(nm + '_dy') for nm in NAMES], chain['fwd_rounded_elems'],
                ['%.2f' % float((l == 0).float().mean()) for l in chain['layers']], [chain['untouched'].get(nm + '_w') for nm in NAMES]))
