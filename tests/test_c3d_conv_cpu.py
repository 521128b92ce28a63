"""CPU: gaze_c3d_conv, the no-recurrence baseline -- the algebra its HIP path rests on (the whole network folds into one
1024 -> 384 filter and a bias plane, csrc/c3dconv_fused.hip.h), known answers of the graph, the helper's gradients, the
checkpoint mapping and the host-only side of the C ABI.  No kernel is launched here."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import c3d_conv_ref as ref
from recurrent_gaze_prediction_amd import _lib, checkpoint
from recurrent_gaze_prediction_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_params(seed, dim_proj):
    """Reference initialisers, the two biases and out_W widened so that no term hides behind another."""
    p = syn.c3d_conv_params(seed, dim_proj)
    rs = np.random.RandomState(seed + 1)
    p['proj_c3d_b'] = rs.uniform(-1, 1, size=p['proj_c3d_b'].shape).astype(np.float32)
    p['out_b'] = rs.uniform(-1, 1, size=1).astype(np.float32)
    return p


@pytest.mark.parametrize('dim_proj,B,T', [(512, 2, 3), (64, 1, 2)])
def test_fold_equals_the_staged_graph_in_float64(dim_proj, B, T):
    p = random_params(3, dim_proj)
    x = syn.c3d_features(4, B, T)
    staged = ref.forward_f64(x, p)
    folded = ref.folded_forward_numpy(x, p)
    assert np.abs(folded - staged).max() <= 1e-12 * np.abs(staged).max()


def test_fold_border_terms_corner_feature():
    """A frame whose features are non-zero only at a corner position: the map is the bias plane (whose border pixels
    gather fewer terms than the interior) plus one 19x19 patch cut by two borders."""
    p = random_params(5, 64)
    x = np.zeros((1, 2, 1024, 7, 7), np.float32)
    x[0, 0, :, 0, 0] = np.random.RandomState(6).rand(1024)
    x[0, 1, :, 6, 6] = np.random.RandomState(7).rand(1024)
    staged = ref.forward_f64(x, p)
    folded = ref.folded_forward_numpy(x, p)
    assert np.abs(folded - staged).max() <= 1e-12 * np.abs(staged).max()
    _, plane = ref.fold_numpy(p)
    assert np.abs(plane[0, 0] - plane[24, 24]) > 1e-3          # a plane, not a scalar
    far = staged[0, 0, 16:, :] - plane[16:, :]                 # position (0, 0) reaches rows -3 .. 15 only
    assert np.abs(far).max() <= 1e-12 * np.abs(staged).max()


def test_known_answers():
    p = {k: np.zeros_like(v) for k, v in syn.c3d_conv_params(1, 64).items()}
    x = syn.c3d_features(2, 1, 2)
    logits = ref.forward_f64(x, p)
    import torch
    maps = ref.softmax_maps(torch.tensor(logits)).numpy()
    assert np.allclose(maps, 1.0 / 2401, rtol=0, atol=1e-15)
    gt = syn.gaze_maps(3, 1, 2)[0].astype(np.float64)
    gt = gt / gt.reshape(1, 2, -1).sum(-1)[..., None, None]
    loss = float(ref.gaze_loss(torch.tensor(logits), torch.tensor(gt, dtype=torch.float64)))
    assert abs(loss - math.log(2401)) < 1e-9
    # proj_c3d_W = 0: every frame's logits are the bias plane, whatever the input
    q = random_params(8, 64)
    q['proj_c3d_W'][:] = 0
    _, plane = ref.fold_numpy(q)
    out = ref.forward_f64(x, q)
    assert np.abs(out - plane).max() <= 1e-12 * np.abs(plane).max()
    assert np.abs(out - ref.forward_f64(2 * x + 1, q)).max() == 0
    # a one-hot feature at position (m, n) responds only inside rows 6m-3 .. 6m+15 (and the same columns)
    r = random_params(9, 64)
    base = ref.forward_f64(np.zeros((1, 1, 1024, 7, 7), np.float32), r)
    for m, n in ((0, 0), (3, 2), (6, 6)):
        one = np.zeros((1, 1, 1024, 7, 7), np.float32)
        one[0, 0, 17, m, n] = 1.0
        d = ref.forward_f64(one, r)[0, 0] - base[0, 0]
        inside = np.zeros((49, 49), bool)
        inside[max(6 * m - 3, 0):min(6 * m + 16, 49), max(6 * n - 3, 0):min(6 * n + 16, 49)] = True
        assert np.abs(d[~inside]).max() <= 1e-14 and np.abs(d[inside]).max() > 1e-6


@pytest.mark.parametrize('loss_type', ['xentropy', 'l2'])
def test_helper_gradients_match_finite_differences(loss_type):
    import torch
    p = random_params(10, 64)
    x = syn.c3d_features(11, 1, 2)
    gt = syn.gaze_maps(12, 1, 2)[0].astype(np.float64)
    gt = gt / gt.reshape(1, 2, -1).sum(-1)[..., None, None]
    loss, _, grads = ref.loss_and_grads(x, gt, p, loss_type, want_input_grad=True)

    def f(params, xin):
        return float(ref.gaze_loss(torch.tensor(ref.forward_f64(xin, params)), torch.tensor(gt), loss_type))
    assert abs(f(p, x) - loss) < 1e-12 * max(1.0, abs(loss))
    rs = np.random.RandomState(13)
    eps = 1e-5
    for k in ref.KEYS:
        for _ in range(3):
            idx = tuple(rs.randint(0, s) for s in p[k].shape)
            hi = {kk: np.asarray(v, np.float64).copy() for kk, v in p.items()}
            lo = {kk: np.asarray(v, np.float64).copy() for kk, v in p.items()}
            hi[k][idx] += eps
            lo[k][idx] -= eps
            fd = (f(hi, x) - f(lo, x)) / (2 * eps)
            assert abs(fd - grads[k][idx]) <= 1e-6 * max(1.0, abs(fd)), (k, idx, fd, grads[k][idx])
    for _ in range(3):
        idx = tuple(rs.randint(0, s) for s in x.shape)
        hi, lo = x.astype(np.float64).copy(), x.astype(np.float64).copy()
        hi[idx] += eps
        lo[idx] -= eps
        fd = (f(p, hi) - f(p, lo)) / (2 * eps)
        assert abs(fd - grads['c3d_input'][idx]) <= 1e-6 * max(1.0, abs(fd))


def test_checkpoint_mapping_round_trips():
    p = syn.c3d_conv_params(14)
    tf_vars = checkpoint.export_model_variables('gaze_c3d_conv', p)
    assert sorted(tf_vars) == ['RGP/Upsampling/weight1', 'RGP/Upsampling/weight2', 'RGP/Upsampling/weight3',
                               'RGP/out_W', 'RGP/out_b', 'RGP/proj_c3d_W', 'RGP/proj_c3d_b']
    variants = [tf_vars, {k + ':0': v for k, v in tf_vars.items()}, {k[len('RGP/'):]: v for k, v in tf_vars.items()},
                {k[len('RGP/'):] + ':0': v for k, v in tf_vars.items()}]
    for v in variants:
        v = dict(v)
        v['RGP/out_W/Adam'] = np.zeros((12, 1), np.float32)        # optimizer slots and the step counter are not parameters
        v['global_step'] = np.zeros((), np.int64)
        back = checkpoint.import_model_variables('gaze_c3d_conv', v)
        assert sorted(back) == sorted(p)
        for k in p:
            assert back[k].dtype == np.float32 and np.array_equal(back[k], p[k]), k
    with pytest.raises(KeyError, match='weight2'):
        checkpoint.import_c3d_conv_variables({k: v for k, v in tf_vars.items() if 'weight2' not in k})


def test_plan_is_host_only_until_bound():
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.rgp_c3dconv_create(ctypes.byref(h), 64, 16, 512, _lib.RGP_BF16, 0) == 0, lib.rgp_last_error()
    assert lib.rgp_c3dconv_path(h) == b'fused'
    ws_fused = lib.rgp_c3dconv_workspace_bytes(h)
    assert ws_fused > 64 * 16 * 49 * 1024 * 2 + 2 * 384 * 1024 * 2          # the transposed input + the filter, twice
    assert lib.rgp_c3dconv_buffer_elems(h, b'folded_filter') == 384 * 1024
    assert lib.rgp_c3dconv_buffer_elems(h, b'bias_plane') == 2401
    assert lib.rgp_c3dconv_buffer_elems(h, b'c3d_embedded') == 0             # the fused kernel has no such intermediate
    assert lib.rgp_c3dconv_buffer_elems(h, b'nope') == 0
    assert lib.rgp_c3dconv_forward(h, None, None, None, None) == -3 and b'workspace' in lib.rgp_last_error()
    lib.rgp_c3dconv_destroy(h)
    assert lib.rgp_c3dconv_create(ctypes.byref(h), 64, 16, 512, _lib.RGP_BF16, _lib.RGP_C3DCONV_STAGED) == 0
    assert lib.rgp_c3dconv_path(h) == b'staged'
    assert lib.rgp_c3dconv_buffer_elems(h, b'c3d_embedded') == 64 * 16 * 49 * 512
    assert lib.rgp_c3dconv_workspace_bytes(h) - ws_fused > 64 * 16 * 49 * 384 * 4     # Z goes through memory here
    lib.rgp_c3dconv_destroy(h)
    assert lib.rgp_c3dconv_create(ctypes.byref(h), 2, 3, 512, _lib.RGP_F32, 0) == 0
    assert lib.rgp_c3dconv_path(h) == b'staged'
    lib.rgp_c3dconv_destroy(h)
    bad = ctypes.c_void_p()
    assert lib.rgp_c3dconv_create(ctypes.byref(bad), 2, 3, 512, _lib.RGP_F32, _lib.RGP_C3DCONV_FUSED) == -1
    assert b'bf16' in lib.rgp_last_error()
    assert lib.rgp_c3dconv_create(ctypes.byref(bad), 2, 3, 512, _lib.RGP_BF16, 6) == -1
    assert lib.rgp_c3dconv_create(ctypes.byref(bad), 2, 3, 512, _lib.RGP_BF16, 8) == -1 and b'flags' in lib.rgp_last_error()
    # training plans run the staged path, keep more, and refuse the fused kernel
    assert lib.rgp_c3dconv_create(ctypes.byref(h), 8, 35, 512, _lib.RGP_BF16, _lib.RGP_C3DCONV_SAVE_FOR_BACKWARD) == 0
    assert lib.rgp_c3dconv_path(h) == b'staged'
    ws_train = lib.rgp_c3dconv_workspace_bytes(h)
    assert lib.rgp_c3dconv_backward_input(h, ctypes.c_void_p(256), None) == -4 and b'backward' in lib.rgp_last_error()
    lib.rgp_c3dconv_destroy(h)
    assert lib.rgp_c3dconv_create(ctypes.byref(h), 8, 35, 512, _lib.RGP_BF16, _lib.RGP_C3DCONV_STAGED) == 0
    assert ws_train > lib.rgp_c3dconv_workspace_bytes(h) + 8 * 35 * 49 * 1024 * 2          # + at least the transposed input
    lib.rgp_c3dconv_destroy(h)
    assert lib.rgp_c3dconv_create(ctypes.byref(bad), 2, 3, 512, _lib.RGP_BF16,
                                  _lib.RGP_C3DCONV_SAVE_FOR_BACKWARD | _lib.RGP_C3DCONV_FUSED) == -1
    assert lib.rgp_c3dconv_create(ctypes.byref(bad), 0, 3, 512, _lib.RGP_BF16, 0) == -1
    assert lib.rgp_c3dconv_create(ctypes.byref(bad), 2, 3, 500, _lib.RGP_BF16, 0) == -1
    assert b'multiple of 64' in lib.rgp_last_error()


def test_header_section_compiles_as_c99(tmp_path):
    if shutil.which('gcc') is None:
        pytest.skip('no C compiler')
    src = tmp_path / 'abi.c'
    src.write_text(r'''
#include <string.h>
#include "rgp.h"
int main(void) {
  rgp_c3dconv_t* g = 0;
  rgp_c3dconv_weights w;
  memset(&w, 0, sizeof w);
  if (rgp_c3dconv_create(&g, 8, 35, 512, RGP_BF16, RGP_C3DCONV_STAGED) != RGP_OK) return 1;
  if (strcmp(rgp_c3dconv_path(g), "staged")) return 2;
  if (rgp_c3dconv_workspace_bytes(g) == 0) return 3;
  if (rgp_c3dconv_set_weights(g, &w, 0) != RGP_EWORKSPACE) return 4;
  if (rgp_c3dconv_buffer_elems(g, "bias_plane") != 2401u) return 5;
  rgp_c3dconv_destroy(g);
  if (rgp_c3dconv_create(&g, 8, 35, 512, RGP_F32, RGP_C3DCONV_FUSED) != RGP_EINVAL) return 6;
  return 0;
}
''')
    inc = os.path.join(ROOT, 'include')
    libdir = os.path.join(ROOT, 'recurrent_gaze_prediction_amd')
    r = subprocess.run(['gcc', '-std=c99', '-Wall', '-Wextra', '-pedantic', '-fsyntax-only', '-I', inc, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    exe = tmp_path / 'abi'
    r = subprocess.run(['gcc', '-std=c99', '-I', inc, str(src), '-o', str(exe), '-L', libdir, '-l:librgp_hip.so',
                        '-Wl,-rpath,' + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-1000:])
