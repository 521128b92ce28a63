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
