"""GPU: the C3D conv-stack BACKWARD on operands whose sums are exact (tests/c3d_exact_ref.py: backward_chain) must EQUAL the
float64 chain, bit for bit: the eight gradient images, the sixteen filter and bias gradients and the saved activations, for
every kernel selection and window count below.  No tolerance anywhere in this file except where case D says so: with these
operands every product and partial sum of every gradient is representable in fp32 (the premise is asserted on the chain each
test compares with), so a result depends on no summation order, column partition, atomic order or kernel family, and the
bf16 store of the gradient images (round to nearest even) is deterministic.  One window's contribution missing from one
(tap, cin, cout), two swapped taps of a rotated filter, a bias sum short of one block, a truncating image store, a `>= 0`
gate or another member of a tied pooling window all change some element (tests/test_c3d_exact_bwd_cpu.py shows it on the
chain), and first_mismatch() says where.

All 15 cases are equal on the MI355X.  Measured there, at 112 x 112:
  case W (light filters: 4 entries per filter, a +1 and a -1 on the same input channel at opposite taps, twice; integer biases;
    windows A and B; upstream gradient dense in {-1, 0, 1}): headroom of the filter gradients 12.5 ... 17.3 bits, bias gradients
    7.1 ... 16.0, gradient images <= 4.8; 2 A + B 17.9, 3 A + 2 B 18.6, 34 A + 33 B 22.3 bits.  8.6 % / 10.0 % / 7.0 % / 5.5 % of
    the positive pooling windows of conv1a / conv2a / conv3b / conv4b have a tied maximum and every member code is used, so the
    kernels' tie rule (first maximum in (dz, dy, dx) order) is compared, in both families.  Zeros 2 % ... 57 % per layer: every
    gate has both sides.  Nothing leaves the integers below 256, so no store rounds, forward or backward, and the same chain
    serves the f32 plan.  Every entry of the filter gradients of conv1a ... conv3b has contributions; on the 14 x 14 and 7 x 7
    layers up to 19 % of them have none, which is what case T is for.
  case T (case W with all-positive filters and biases from conv4a up, upstream gradient +-1 everywhere, compared from conv4a
    up): no zero in any activation or gradient of those layers, every entry of their filter gradients reached; 15.3 ... 17.4
    bits, 34 A + 33 B 22.4; 6 307 / 48 912 / 77 950 saved activations of conv4b / conv5a / conv5b are values the bf16 store rounded.
  case D (tap-complete filters +-2^-2, window A, upstream gradient of density 0.3 in {-2 ... 2}): gradient images 1.0 ... 13.0 bits;
    RNE changes 1 230 825 / 127 583 / 791 stored elements of the images of conv1a / conv2a / conv3a.  Its filter gradients
    (24.2 ... 26.2 bits) and conv1a's bias gradient (24.7) are compared by the relative bound; its other seven bias gradients exactly.
Kernels covered: rows_grad_kernel (d_features and d_rows), wgrad_patch_bf16_kernel<64,128,56,16> / <128,256,28,8> /
<256,256,28,8> and its window-pair form <256,512,14,4> / <512,512,14,4> (with the bias gradients of conv3a and conv4a),
conv1a_wgrad_bf16_kernel, wgrad_kernel (bf16: conv5a / conv5b, every layer of the second family; f32: launch_wgrad<float> with
conv1a_unpack_grad_kernel), the patch and implicit-GEMM input gradients with and without the fused gate, unpool8_rows_kernel<128>
/ <256> / <512>, unpool_kernel<bf16> (conv1a's image on demand) and <float>, colsum_kernel.
Wall time: 5.7 s, 1.6 s and 4.7 s for the first case of W, T and D (they build the chains on the CPU), 0.06 ... 0.5 s for every
other case, 1.2 s and 0.7 s for the two 67-window runs of W and of T, 19 s for the file."""
import collections

import pytest
import torch

import c3d_exact_ref as ref
from test_c3d_backward_gpu import TOL_LOCAL, rel

pytestmark = pytest.mark.gpu
TOL_BITS = 23


def chain_w():
    """Case W (light filters, windows A and B) with its premises asserted -- on first use it builds the chain, afterwards
    it is the cached object."""
    p, video, g, chain = ref.case_w()
    hb = chain['headroom_bits']
    assert len(hb) == 24 and max(hb.values()) <= TOL_BITS and all(chain['exact_in_f32'].values()), hb
    for i in ref.POOLED:
        assert chain['tied_frac'][ref.NAMES[i]] > 0.05 and min(chain['code_hist'][ref.NAMES[i]]) > 0
    return p, torch.as_tensor(video), torch.as_tensor(g), chain


def chain_t():
    """Case T (case W with dense, all-positive layers from conv4a up; the backward down to conv4a only)."""
    p, video, g, chain = ref.case_t()
    assert max(chain['headroom_bits'].values()) <= TOL_BITS and all(chain['exact_in_f32'].values()), chain['headroom_bits']
    assert all(chain['untouched'][nm + '_w'] == 0 for nm in ref.NAMES[ref.TOP:]) and min(chain['fwd_rounded_elems'][ref.TOP + 1:]) > 0
    return p, torch.as_tensor(video), torch.as_tensor(g), chain


CASES = {'W': (chain_w, range(8)), 'T': (chain_t, range(ref.TOP, 8))}


def chain_d():
    """Case D (tap-complete filters, window A): gradient images exact and really rounded by their store."""
    p, video, g, chain = ref.case_d()
    hb = chain['headroom_bits']
    assert max(hb[nm + '_dy'] for nm in ref.NAMES) <= TOL_BITS and all(chain['exact_in_f32'][nm + '_dy'] for nm in ref.NAMES), hb
    assert all(chain['rounded_elems'][nm + '_dy'] > 0 for nm in ref.NAMES[:3]), chain['rounded_elems']
    return p, torch.as_tensor(video), torch.as_tensor(g), chain


def make_engine(gpu, plan, p, dtype='bf16', kernels='patch', stale_seed=None):
    """A training plan; stale_seed: a forward and backward on dense random data on ALL windows of the plan first, so a
    gradient or image element the exact run fails to write keeps a foreign value."""
    from recurrent_gaze_prediction_amd.engine import C3DEngine
    eng = C3DEngine(plan, dtype=dtype, device=gpu, save_for_backward=True, kernels=kernels)
    eng.set_weights(p)
    if stale_seed is not None:
        gen = torch.Generator(device=gpu)
        gen.manual_seed(stale_seed)
        eng.forward((torch.rand(plan, 16, 112, 112, 3, device=gpu, generator=gen) - 0.5) * 16)
        eng.backward(d_features=torch.randn(plan, 1024, 7, 7, device=gpu, generator=gen))
        for i in range(8):
            assert float(eng.read_grad_image(i, plan).abs().max()) > 0
    return eng


def run(eng, video, g, idx, gpu, **kw):
    sel = torch.as_tensor(idx)
    feats, _ = eng.forward(video[sel].to(gpu).contiguous())
    eng.backward(d_features=g[sel].to(gpu).contiguous(), **kw)
    return feats


def cmp(got, want, name):
    """first_mismatch, but equal tensors are settled on the device."""
    want = want.to(got.device)
    if got.shape == want.shape and got.dtype == want.dtype and torch.equal(got, want):
        return None
    return ref.first_mismatch(got, want, name)


def mismatches(eng, feats, chain, idx, tag, images=range(8), windows=None, grads=True):
    """Every tensor of the run on windows idx that differs from the chain -> list of first_mismatch messages."""
    n = len(idx) if windows is None else windows
    sel = torch.as_tensor(idx)[:n]
    bad = []
    if feats is not None:
        for i in range(7):
            want = chain['layers'][i][sel]
            bad.append(cmp(eng.read_layer(i, n).reshape(want.shape), want, '%s: saved %s' % (tag, ref.NAMES[i])))
        bad.append(cmp(feats[:n], chain['features'][sel], '%s: features [window, c*2+d, y, x]' % tag))
    for i in images:
        bad.append(cmp(eng.read_grad_image(i, n), chain['dys'][i][sel], '%s: dY %s' % (tag, ref.NAMES[i])))
    if grads:
        count = collections.Counter(idx)
        coeffs = [count.get(j, 0) for j in range(len(chain['grads']))]
        want, bits = ref.combine_windows(chain, coeffs)
        assert max(bits.values()) <= TOL_BITS, bits
        views = eng.grad_views()
        for k in want:
            v = views[k]
            assert torch.equal(want[k].float().double(), want[k])
            bad.append(cmp(v, want[k].float(), '%s: d %s %s' % (tag, k, '[kd, kh, kw, cin, cout]' if k.endswith('_w') else '')))
    return [b for b in bad if b is not None]


def require(bad):
    if bad:
        pytest.fail('\n'.join(bad))


@pytest.mark.parametrize('kernels', ['patch', 'igemm', 'igemm128'])
def test_exact_backward_case_w(gpu, kernels):
    """bf16, windows A and B on a plan of 3 after a dense run.  'patch': wgrad_patch (56 / 28 / window-pair 14x14),
    conv1a_wgrad, wgrad_kernel on conv5a/b, the patch input gradients, unpool8_rows, rows_grad; 'igemm' / 'igemm128':
    wgrad_kernel and the implicit-GEMM input gradients on every layer, colsum_kernel.  Then the d_rows entry point and
    accumulation into existing gradients."""
    p, video, g, chain = chain_w()
    eng = make_engine(gpu, 3, p, kernels=kernels, stale_seed=101)
    print(kernels, [eng.layer_kernel_name(i, 2) for i in range(8)])
    feats = run(eng, video, g, [0, 1], gpu)
    require(mismatches(eng, feats, chain, [0, 1], kernels))
    first = {k: v.clone() for k, v in eng.grad_views().items()}
    images = [eng.read_grad_image(i, 2) for i in range(1, 8)]
    # d_rows [n*49, d*512+c] is the same gradient in the rows layout: the same bits
    rows = g.reshape(2, 512, 2, 49).permute(0, 3, 2, 1).reshape(2 * 49, 1024).contiguous().to(gpu)
    eng.forward(video.to(gpu))
    eng.backward(d_rows=rows)
    bad = [ref.first_mismatch(v, first[k], 'd_rows: d ' + k) for k, v in eng.grad_views().items()]
    bad += [ref.first_mismatch(eng.read_grad_image(i, 2), images[i - 1], 'd_rows: dY ' + ref.NAMES[i]) for i in range(1, 8)]
    # a second backward into the same buffer: exactly twice (one more bit of headroom, inside the significand)
    assert max(ref.combine_windows(chain, [2, 2])[1].values()) <= TOL_BITS
    eng.backward(d_rows=rows, zero_grads=False)
    bad += [ref.first_mismatch(v, 2 * first[k], 'accumulated: d ' + k) for k, v in eng.grad_views().items()]
    require([b for b in bad if b is not None])


def test_exact_backward_families_agree(gpu):
    """The patch and implicit-GEMM families leave identical gradient images and gradients (both equal the chain above; here
    against each other, which also holds the tie rule of their pooling epilogues together)."""
    p, video, g, _ = chain_w()
    got = {}
    for kernels in ('patch', 'igemm'):
        eng = make_engine(gpu, 2, p, kernels=kernels)
        run(eng, video, g, [0, 1], gpu)
        got[kernels] = ([eng.read_grad_image(i, 2) for i in range(8)], {k: v.clone() for k, v in eng.grad_views().items()})
        del eng
    bad = [ref.first_mismatch(a, b, 'igemm against patch: dY ' + ref.NAMES[i]) for i, (a, b) in enumerate(zip(got['igemm'][0], got['patch'][0]))]
    bad += [ref.first_mismatch(got['igemm'][1][k], v, 'igemm against patch: d ' + k) for k, v in got['patch'][1].items()]
    require([b for b in bad if b is not None])


@pytest.mark.parametrize('kernels', ['patch', 'igemm'])
def test_exact_backward_case_t(gpu, kernels):
    """conv4a ... conv5b with no zero in any activation or gradient: every entry of their filter gradients has contributions
    (case W leaves up to 19 % of them without one), and the saved activations are bf16-rounded values."""
    p, video, g, chain = chain_t()
    eng = make_engine(gpu, 3, p, kernels=kernels, stale_seed=105)
    feats = run(eng, video, g, [0, 1], gpu)
    require(mismatches(eng, feats, chain, [0, 1], 'dense top, ' + kernels, images=range(ref.TOP, 8)))


def test_exact_backward_f32_plan(gpu):
    """fp32 operands and stores, window A: launch_wgrad<float>, conv1a_unpack_grad_kernel, unpool_kernel<float> on all four
    pooled layers, colsum_kernel, the fp32 implicit-GEMM input gradients.  Nothing rounds, forward or backward."""
    p, video, g, chain = chain_w()
    # no store of the bf16 chain changed a value, forward or backward (integers below 256): it is the f32 plan's chain too
    assert sum(chain['fwd_rounded_elems']) == 0 and all(v == 0 for v in chain['rounded_elems'].values())
    eng = make_engine(gpu, 2, p, dtype='f32', stale_seed=102)
    feats = run(eng, video, g, [0], gpu)
    require(mismatches(eng, feats, chain, [0], 'f32'))


@pytest.mark.parametrize('case', ['W', 'T'])
@pytest.mark.parametrize('idx', [[0, 1, 0], [0, 1, 0, 1, 0]], ids=['3 windows', '5 windows'])
def test_exact_backward_partition_edges(gpu, idx, case):
    """bf16 patch kernels at odd window counts: column ranges of unequal length, empty ranges, and on the 14 x 14 layers a
    last window pair that is half empty.  Gradients are linear in windows: the reference is 2 dW(A) + dW(B), 3 dW(A) + 2 dW(B),
    asserted to stay inside the significand; every replica's gradient images equal its original's."""
    p, video, g, chain = CASES[case][0]()
    eng = make_engine(gpu, len(idx), p, stale_seed=103)
    feats = run(eng, video, g, idx, gpu)
    require(mismatches(eng, feats, chain, idx, '%s, %d windows' % (case, len(idx)), images=CASES[case][1]))


@pytest.mark.parametrize('case', ['W', 'T'])
def test_exact_backward_67_windows(gpu, case):
    """The window count of the fine-tune benchmark's partition (odd, 34 window pairs with the last half empty, several
    persistent rounds), both families, one forward and backward each: dW = 34 dW(A) + 33 dW(B) exactly -- log2(33.5) = 5.1
    bits on top of the two-window headroom, asserted <= 23 -- and the gradient images of every replica from conv3a up, of the
    first pair on every layer."""
    p, video, g, chain = CASES[case][0]()
    n = 67
    idx = [j % 2 for j in range(n)]
    _, bits = ref.combine_windows(chain, [34, 33])
    print('67 windows, case %s: headroom bits up to %.1f' % (case, max(bits.values())))
    assert max(bits.values()) <= TOL_BITS
    for kernels in ('patch', 'igemm'):
        eng = make_engine(gpu, n, p, kernels=kernels)
        feats = run(eng, video, g, idx, gpu)
        tag = '%s, 67 windows, %s' % (case, kernels)
        bad = mismatches(eng, feats, chain, idx, tag, images=CASES[case][1], windows=2)
        bad += mismatches(eng, None, chain, idx, tag + ', every replica', images=[i for i in CASES[case][1] if i >= 2], grads=False)
        del eng
        require(bad)


@pytest.mark.parametrize('kernels', ['patch', 'igemm'])
def test_exact_backward_case_d(gpu, kernels):
    """Tap-complete filters: every tap of every rotated filter multiplies something and the bf16 store of the gradient
    images rounds (asserted on the chain): all eight images and the saved activations equal the chain.  A filter or bias
    gradient of this case is compared exactly only where its own headroom allows, otherwise by the bound of
    test_c3d_backward_gpu.py -- acceptable only because case W compares every one of them exactly, which is asserted."""
    p, video, g, chain = chain_d()
    fwd = ref.reference_chain(video.numpy(), p, 'bf16')              # the forward's own premise, and a second opinion on it
    assert max(fwd['headroom_bits']) <= TOL_BITS and all(fwd['exact_in_f32'])
    assert all(torch.equal(a, b) for a, b in zip(fwd['layers'], chain['layers']))
    w_bits = chain_w()[3]['headroom_bits']
    assert all(w_bits[k] <= TOL_BITS for k in w_bits)               # case W compared all sixteen gradients exactly
    eng = make_engine(gpu, 1, p, kernels=kernels, stale_seed=104)
    feats = run(eng, video, g, [0], gpu)
    bad = mismatches(eng, feats, chain, [0], 'tap-complete, ' + kernels, grads=False)
    fell_back = []
    for k, v in eng.grad_views().items():
        want = chain['grads'][0][k]
        if chain['headroom_bits'][k] <= TOL_BITS and chain['exact_in_f32'][k]:
            bad.append(ref.first_mismatch(v, want.float(), 'tap-complete, %s: d %s' % (kernels, k)))
        else:
            fell_back.append('%s (%.1f bits)' % (k, chain['headroom_bits'][k]))
            assert float(want.abs().max()) > 0
            assert rel(v.cpu().numpy(), want.numpy()) < TOL_LOCAL['bf16'], k
    print('compared by the relative bound, not exactly:', fell_back)
    require([b for b in bad if b is not None])
