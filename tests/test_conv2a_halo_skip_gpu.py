"""GPU: conv2a's inference forward leaves out the tap groups that multiply the zero halo planes z = -1 and z = 16 (1/24 of
its MFMAs) and walks its tiles in the rotated (window, yp, zp) order of conv_patch.hip.h's decode()."""
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL_BF16 = 3e-2          # TOL['bf16'] of tests/test_c3d_gpu.py: max-abs error / max-abs of the reference tensor


def _rel(a, ref):
    return float((a.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-30))


@pytest.mark.parametrize('n', [1, 3, 17, 96])
def test_conv2a_halo_skip_matches_rowwise_and_unskipped_family(gpu, n):
    """n = 1: one window; 3: a ragged walk; 17: no multiple of the order's period (2 windows = 7 blocks of 32 tiles);
    96: several persistent rounds.

    * default plan (conv_patch_slab_bf16_kernel) and 'patch-rowwise' plan (conv_patch_bf16_kernel): the
      pooled conv2a output is EQUAL bit for bit.
    * every output position written exactly once: each engine first runs a DIFFERENT video, so a position decode() never
      reaches keeps that run's value, and the tile count is fixed, so a position written twice leaves another one
      unwritten.  Both patch plans share decode(); the implicit-GEMM family ('igemm') has its own row order and skips
      nothing, and the whole layer must agree with it within the bf16 tolerance.
    * pooled planes 0 and 7 (the tiles that skip), each on its own, agree with that family within the same tolerance: a
      dropped or misplaced tap group is an error of tens of per cent."""
    from recurrent_gaze_prediction_amd import synthetic as syn
    from recurrent_gaze_prediction_amd.engine import C3DEngine
    p = syn.c3d_params(21, scale='he')
    g = torch.Generator(device=gpu)
    g.manual_seed(4100 + n)
    stale = torch.rand(n, 16, 112, 112, 3, device=gpu, generator=g) - 0.5
    video = torch.rand(n, 16, 112, 112, 3, device=gpu, generator=g) - 0.5
    out = {}
    for kernels in ('patch', 'patch-rowwise', 'igemm'):
        eng = C3DEngine(n, dtype='bf16', device=gpu, kernels=kernels)
        eng.set_weights(p)
        name = eng.layer_kernel_name(1, n)
        assert name.startswith({'patch': 'conv_patch_slab_bf16_kernel<64,128,56,16', 'patch-rowwise': 'conv_patch_bf16_kernel<64,128,56,16',
                                'igemm': 'igemm_'}[kernels]), name
        eng.forward(stale, want_features=False, want_rows=True)
        before = eng.read_layer(1, n).clone()
        eng.forward(video, want_features=False, want_rows=True)
        out[kernels] = eng.read_layer(1, n).reshape(n, 8, 28, 28, 128)
        assert not torch.equal(before.reshape(out[kernels].shape), out[kernels])
        del eng
    torch.cuda.synchronize()
    a, b, ref = out['patch'], out['patch-rowwise'], out['igemm']
    assert float(ref.abs().max()) > 0 and 0.05 < float((ref == 0).float().mean()) < 0.95, 'degenerate activations'
    assert torch.equal(a, b), 'pooled conv2a output differs between the two fetch variants'
    for tag, got in (('slab', a), ('rowwise', b)):
        figures = [_rel(got, ref), _rel(got[:, 0], ref[:, 0]), _rel(got[:, 7], ref[:, 7])]
        # per window and pooled row pair as well: one stale 2 x 28 tile must not hide behind a large maximum elsewhere
        tiles = (got.double() - ref.double()).abs().reshape(n, 8, 14, -1).amax(-1) / ref.double().abs().reshape(n, 8, 14, -1).amax(-1).clamp_min(1e-30)
        figures.append(float(tiles.max()))
        print('conv2a %s n=%d: rel err whole %.3e, plane 0 %.3e, plane 7 %.3e, worst tile %.3e' % ((tag, n) + tuple(figures)))
        assert figures[0] < TOL_BF16 and figures[1] < TOL_BF16 and figures[2] < TOL_BF16
        assert figures[3] < 4 * TOL_BF16, 'a tile of the output is stale or misplaced'
