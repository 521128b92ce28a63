"""GPU: the C3D forward on operands whose sums are exact (tests/c3d_exact_ref.py) must EQUAL the float64 chain, bit for bit:
every layer, every kernel selection, every window count.  No tolerance: with these operands each product and each partial
sum is representable in fp32 (the tests assert the headroom of the very chain they compare with), so the result does not
depend on summation order, tile shape or kernel family, and the bf16 store (round to nearest even) is deterministic.  One
wrong (tap, cin) product, a stale halo element, a truncating store, a bias missing from a few columns or two swapped K indices
all change some element, and first_mismatch() says where.

The one assumption the recipe could not settle on paper -- that the bf16 MFMA accumulates exactly when every partial sum is
representable -- holds on the MI355X: all 21 cases are equal.  Measured there, at 112 x 112 on windows A and B: headroom
6.9 / 9.8 / 12.4 / 14.2 / 16.5 / 18.4 / 20.5 / 20.2 bits (set 0), 6.9 / 9.8 / 12.1 / 14.1 / 16.4 / 18.3 / 20.3 / 20.9
(set 1), 6.0 ... 18.1 (f32 plan, 16 entries per filter); zeros 9 % ... 53 % per layer; RNE and truncation differ on
7 347 ... 335 362 stored elements of every layer from conv2a on.  Kernels covered: conv1a_pool_bf16_kernel<fused> and
<act0,argmax>, conv_patch_slab_bf16_kernel<64,128,56,16>, conv_patch_bf16_kernel<64,128,56,16> / <128,256,28,8> / <256,256,28,8>,
conv_patch14_bf16_kernel<256> / <512>, conv_patch7_bf16_kernel<image> / <rows>, igemm_kernel<128x128> / <64x64> (bf16 and f32),
igemm_stagger_kernel<256x128>, igemm_wide_kernel<512x128> / <256x256>.  Wall time: 1.9 s for the first case of a filter set
(it builds the shared chain), 0.02 ... 0.09 s for every other case, 6.6 s for the file.  A device run with one conv3a product
removed differed from the chain in 43 elements of that output channel, in both kernel families."""
import functools

import pytest
import torch

import c3d_exact_ref as ref

pytestmark = pytest.mark.gpu

SEED_A_B = 4242          # exact_video(SEED_A_B, 2): the two distinct windows A and B


@functools.lru_cache(maxsize=None)
def exact_chain(set_id, dtype='bf16', nnz=32):
    """(params, chain of windows A and B) -- built once per filter set and shared, never modified."""
    p = ref.exact_params(set_id, nnz)
    chain = ref.reference_chain(ref.exact_video(SEED_A_B, 2), p, dtype)
    print('exact chain set %d %s nnz %d: headroom bits %s zeros %s rne!=trunc %s' % (
        set_id, dtype, nnz, ['%.1f' % b for b in chain['headroom_bits']], ['%.2f' % z for z in chain['zero_frac']],
        chain['rne_trunc_differ']))
    # the premise of equality, checked on the chain actually used (112 x 112, both windows)
    assert all(chain['exact_in_f32']) and max(chain['headroom_bits']) <= 23, chain['headroom_bits']
    assert all(0.01 < z < 0.90 for z in chain['zero_frac']), chain['zero_frac']
    if dtype == 'bf16':
        assert max(chain['rne_trunc_differ']) > 0
    return p, chain


def video_of(idx, device):
    v = torch.as_tensor(ref.exact_video(SEED_A_B, 2), device=device)
    return v[torch.as_tensor(idx, device=device)].contiguous()


def require_equal(eng, feats, rows, chain, idx, layers_of=None):
    """read_layer(0..6), rows and features of a run on windows A/B[idx] against the chain; fails on the first layer that
    differs, with the coordinates.  layers_of: compare the layer images of the first `layers_of` windows only."""
    n = len(idx)
    m = n if layers_of is None else layers_of
    dev = feats.device
    sel = torch.as_tensor(idx)
    for i in range(7):
        want = chain['layers'][i][sel[:m]]
        got = eng.read_layer(i, m).reshape(want.shape)
        if not torch.equal(got, want.to(dev)):
            pytest.fail(ref.first_mismatch(got, want, ref.NAMES[i]))
    want = chain['rows'].reshape(2, 49, 1024)[sel]
    got = rows.reshape(n, 49, 1024)
    assert got.dtype == want.dtype
    if not torch.equal(got, want.to(dev)):
        as_image = lambda t: t.float().cpu().reshape(n, 7, 7, 2, 512).permute(0, 3, 1, 2, 4)      # (window, z, y, x, c)
        pytest.fail(ref.first_mismatch(as_image(got), as_image(want), 'conv5b (rows)'))
    want = chain['features'][sel]
    if not torch.equal(feats, want.to(dev)):
        pytest.fail(ref.first_mismatch(feats, want, 'features [window, c*2+d, y, x]'))


PATCH_NAMES = ('conv1a_pool_bf16_kernel<fused>', 'conv_patch_slab_bf16_kernel<64,128,56,16', 'conv_patch_bf16_kernel<128,256,28,8',
               'conv_patch_bf16_kernel<256,256,28,8', 'conv_patch14_bf16_kernel<256', 'conv_patch14_bf16_kernel<512',
               'conv_patch7_bf16_kernel<image>', 'conv_patch7_bf16_kernel<rows>')


def check_names(eng, n, kernels, save=False):
    names = [eng.layer_kernel_name(i, n) for i in range(8)]
    assert names[0] == ('conv1a_pool_bf16_kernel<act0,argmax>' if save else 'conv1a_pool_bf16_kernel<fused>'), names
    if kernels in ('patch', 'patch-rowwise'):
        want = list(PATCH_NAMES)
        if save or kernels == 'patch-rowwise':
            want[1] = 'conv_patch_bf16_kernel<64,128,56,16'
        assert all(nm.startswith(w) for nm, w in zip(names[1:], want[1:])), names
    elif kernels == 'igemm128':
        assert all(nm.startswith('igemm_kernel<') for nm in names[1:]), names                  # tile loops only
    else:
        assert all(nm.startswith('igemm_') for nm in names[1:]), names
        if n >= 2:
            assert names[1].startswith('igemm_stagger_kernel<256x128'), names                 # conv2a: >= 100 352 rows
    return names


def run_small(gpu, kernels, set_id, n, save=False):
    from recurrent_gaze_prediction_amd.engine import C3DEngine
    p, chain = exact_chain(set_id)
    idx = [0, 1, 0][:n]
    eng = C3DEngine(3, dtype='bf16', device=gpu, save_for_backward=save, kernels=kernels)
    eng.set_weights(p)
    print(kernels, n, check_names(eng, n, kernels, save))
    # stale data first: a dense video on all 3 windows of the plan, so an element the exact run fails to write (or a halo a
    # kernel wrongly wrote) keeps a value that is not the reference's
    g = torch.Generator(device=gpu)
    g.manual_seed(77 + n)
    stale = (torch.rand(3, 16, 112, 112, 3, device=gpu, generator=g) - 0.5) * 16
    eng.forward(stale, want_features=True, want_rows=True)
    feats, rows = eng.forward(video_of(idx, gpu), want_features=True, want_rows=True)
    require_equal(eng, feats, rows, chain, idx)


@pytest.mark.parametrize('n', [1, 2, 3])
@pytest.mark.parametrize('kernels,set_id', [('patch', 0), ('patch-rowwise', 0), ('igemm', 0), ('igemm128', 0), ('patch', 1)])
def test_exact_forward_small_counts(gpu, kernels, set_id, n):
    """Windows A / A,B / A,B,A on a plan of 3: the conv1a kernel, conv2a's slab ('patch') and row-wise ('patch-rowwise')
    kernels, the 28 x 28, 14 x 14 and 7 x 7 patch kernels, the implicit-GEMM tile loops ('igemm128') and what that family
    picks by size ('igemm'), after a run that left other data in every buffer."""
    run_small(gpu, kernels, set_id, n)


@pytest.mark.parametrize('kernels', ['patch', 'igemm'])
def test_exact_forward_training_plans(gpu, kernels):
    """save_for_backward plans: conv1a from the converted act0 image with arg-max recording, conv2a on the row-wise kernel,
    arg-max codes recorded by every pooling layer -- the stored activations are the same numbers."""
    run_small(gpu, kernels, 0, 2, save=True)


def run_at_scale(gpu, kernels, n):
    from recurrent_gaze_prediction_amd.engine import C3DEngine
    p, chain = exact_chain(0)
    eng = C3DEngine(n, dtype='bf16', device=gpu, kernels=kernels)
    eng.set_weights(p)
    names = [eng.layer_kernel_name(i, n) for i in range(8)]
    reps = (n + 1) // 2
    video = torch.as_tensor(ref.exact_video(SEED_A_B, 2), device=gpu).repeat(reps, 1, 1, 1, 1)[:n].contiguous()
    feats, rows = eng.forward(video, want_features=True, want_rows=True)
    # every replica of A and B, the last (partial) group included, on the device; then the layer images of the first pair
    want_rows = chain['rows'].reshape(2, 49 * 1024).to(gpu).repeat(reps, 1)[:n]
    want_feats = chain['features'].reshape(2, -1).to(gpu).repeat(reps, 1)[:n]
    got_rows, got_feats = rows.reshape(n, -1), feats.reshape(n, -1)
    if not (torch.equal(got_rows, want_rows) and torch.equal(got_feats, want_feats)):
        bad = torch.nonzero((got_rows != want_rows).any(1) | (got_feats != want_feats).any(1)).flatten().tolist()
        w = bad[0]
        as_image = lambda t: t.float().cpu().reshape(1, 7, 7, 2, 512).permute(0, 3, 1, 2, 4)
        pytest.fail('%d of %d windows differ (first %s); window %d: %s' % (
            len(bad), n, bad[:8], w, ref.first_mismatch(as_image(got_rows[w]), as_image(want_rows[w]), 'conv5b (rows)')
            or ref.first_mismatch(got_feats[w], want_feats[w], 'features')))
    require_equal(eng, feats[:2], rows[:2 * 49], chain, [0, 1], layers_of=2)
    return names


def test_exact_forward_patch_96_windows(gpu):
    """Several persistent rounds of the patch kernels."""
    names = run_at_scale(gpu, 'patch', 96)
    assert all(nm.startswith(w) for nm, w in zip(names, PATCH_NAMES)), names


def test_exact_forward_igemm_85_windows(gpu):
    """conv4a / conv4b: 66 640 rows = 260.3 row tiles of 256 on the persistent staggered kernel, ragged last tile."""
    names = run_at_scale(gpu, 'igemm', 85)
    assert names[4].startswith('igemm_stagger_kernel<256x128') and names[5].startswith('igemm_stagger_kernel<256x128'), names


def test_exact_forward_igemm_768_windows(gpu):
    """igemm_wide 512x128 (conv2a) and 256x256 (conv3a..conv4b), the staggered kernel on conv5a/b."""
    names = run_at_scale(gpu, 'igemm', 768)
    assert names[1].startswith('igemm_wide_kernel<512x128') and names[6].startswith('igemm_stagger_kernel<256x128'), names
    assert all(nm.startswith('igemm_wide_kernel<256x256') for nm in names[2:6]), names


def test_exact_forward_f32_plan(gpu):
    """fp32 operands and stores: nothing rounds, the lsb shrinks by two bits per layer; 16 entries per filter keep the sums
    inside the significand (asserted by exact_chain).  Equal to the float64 chain cast to fp32."""
    from recurrent_gaze_prediction_amd.engine import C3DEngine
    p, chain = exact_chain(0, 'f32', 16)
    eng = C3DEngine(1, dtype='f32', device=gpu)
    eng.set_weights(p)
    names = [eng.layer_kernel_name(i, 1) for i in range(8)]
    assert all(nm.startswith('igemm_') and ',f32,' in nm for nm in names), names
    feats, rows = eng.forward(video_of([0], gpu), want_features=True, want_rows=True)
    require_equal(eng, feats, rows, chain, [0])
