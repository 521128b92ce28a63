"""GPU: the plane-pure form of conv3a / conv3b + pool3 (conv_patch_pure_bf16_kernel of conv_patch.hip.h: block tile = a pair of
clip windows x one output plane x a band of 4 rows, conv3b pooled across two passes) computes bit for bit what the two-plane
block tile computes, which a plan created with RGP_C3D_CONV3_TWOPLANE (kernels='patch-twoplane') still runs."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _engines(gpu, capacity):
    from recurrent_gaze_prediction_amd import synthetic as syn
    from recurrent_gaze_prediction_amd.engine import C3DEngine
    p = syn.c3d_params(21, scale='he')                       # the weights of test_c3d_gpu.py's c3d_case
    out = []
    for kernels in ('patch', 'patch-twoplane'):
        eng = C3DEngine(capacity, dtype='bf16', device=gpu, kernels=kernels)
        eng.set_weights(p)
        out.append(eng)
    return out


def _video(gpu, seed, n):
    g = torch.Generator(device=gpu)
    g.manual_seed(seed)
    return torch.rand(n, 16, 112, 112, 3, device=gpu, generator=g) - 0.5


@pytest.mark.parametrize('n', [1, 2, 3, 19, 35])
def test_conv3_plane_pure_equals_two_plane_tile(gpu, n):
    """n = 1: a lone ragged pair; 2: one whole pair; 3: a whole pair and a ragged one; 19: a short chunk of the tile order (10 of
    16 pairs, the last one ragged) and several persistent rounds (10 pairs x 56 / 28 tiles over 256 workgroups); 35: a whole
    chunk followed by a short one of two pairs, the last one ragged.  Each engine first runs a DIFFERENT video, so an output position the
    tile walk never reaches keeps that run's value and shows up as a difference."""
    pure, two = _engines(gpu, n)
    assert pure.layer_kernel_name(2, n) == two.layer_kernel_name(2, n) == 'conv_patch_bf16_kernel<128,256,28,8,pool1>'
    assert pure.layer_kernel_name(3, n) == two.layer_kernel_name(3, n) == 'conv_patch_bf16_kernel<256,256,28,8,pool8>'
    stale, video = _video(gpu, 5200 + n, n), _video(gpu, 5300 + n, n)
    got = []
    for eng in (pure, two):
        eng.forward(stale, want_features=False, want_rows=True)
        before = eng.read_layer(3, n).clone()
        _, rows = eng.forward(video, want_features=False, want_rows=True)
        got.append((eng.read_layer(2, n), eng.read_layer(3, n), rows))
        assert not torch.equal(before, got[-1][1])
    torch.cuda.synchronize()
    (a2, a3, ar), (b2, b3, br) = got
    assert float(b3.abs().max()) > 0 and 0.05 < float((b3 == 0).float().mean()) < 0.95, 'degenerate activations'
    assert torch.equal(a2, b2), 'conv3a output differs'
    assert torch.equal(a3, b3), 'pooled conv3b output differs'
    assert torch.equal(ar, br), 'conv5b rows differ'


def test_conv3_plane_pure_leaves_windows_beyond_n_untouched(gpu):
    """An engine of capacity 8 run with 3 windows (one whole pair, one ragged pair): the activations of windows 3 .. 7 keep
    what a run of 8 other windows left there, and the rows buffer is written up to row 3 * 49 only."""
    cap, n = 8, 3
    pure, two = _engines(gpu, cap)
    stale, video = _video(gpu, 5401, cap), _video(gpu, 5402, n)
    got = []
    for eng in (pure, two):
        eng.forward(stale, want_features=False, want_rows=True)
        old2, old3 = eng.read_layer(2, cap).reshape(cap, -1).clone(), eng.read_layer(3, cap).reshape(cap, -1).clone()
        rows = torch.full((cap * 49, 1024), -7.0, dtype=eng.torch_dtype, device=gpu)
        eng.forward(video, want_features=False, want_rows=True, out_rows=rows)
        new2, new3 = eng.read_layer(2, cap).reshape(cap, -1), eng.read_layer(3, cap).reshape(cap, -1)
        assert torch.equal(new2[n:], old2[n:]) and torch.equal(new3[n:], old3[n:]), 'a window beyond n was written'
        assert not torch.equal(new2[:n], old2[:n]) and not torch.equal(new3[:n], old3[:n])
        assert bool((rows[n * 49:] == -7.0).all()), 'rows beyond n were written'
        got.append((new2[:n], new3[:n], rows[:n * 49]))
    torch.cuda.synchronize()
    for a, b in zip(*got):
        assert torch.equal(a, b)
