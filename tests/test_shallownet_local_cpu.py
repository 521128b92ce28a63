"""Host-only: the stage references of tests/shallownet_local_ref.py are pinned to the oracle's ShallowNet, their bounds are
validated on a stand-in device (the same stages chained with fp32 products and fp32 accumulation), and every mistake the
checks are meant to catch is seeded into that stand-in and must fail the check named next to it.  Every test prints its
figures before it asserts (-s).

Measured on the stand-in (worst over CASES; each at most half its bound):
  pool1 / act2 / act3 / mo1 (bf16: not the rounded reference)   0.0033 % / 0.0033 % / 0.0036 % / 0.028 % of a buffer (cap 1 %; mo1
                                                                at 3 frames: 2 of 7203); at 49 frames 1 / 3 / 2 / 0 elements more
                                                                than one ulp off, all next to zero inside the rounded F32_TOL
                                                                image, none outside it
  dz1, dy3, dy2, dy1 (bf16)                                     every element the rounded reference
  pool1 / act2 / act3 / mo1, dy3 / dy2, dz1 / dy1 (f32)         4.8e-7 / 7.3e-7 / 9.9e-7 / 3.1e-7, 4.5e-8 / 5.8e-8, 0 (bound 2e-5)
  sal, dmo1, dpool3, dpool2, dpool1                             4.1e-7, 3.4e-7, 3.1e-7, 1.4e-7, 1.5e-7 (bound 2e-5)
  sal7                                                          2.0e-7 of an element (bound 50 x 2^-24 = 3.0e-6)
  fc2_b, fc2_w, fc1_b, fc1_w                                    7.0e-8, 6.3e-8, 5.7e-8, 9.5e-8 (bound 1e-4)
  conv3_b, conv3_w, conv2_b, conv2_w, conv1_b, conv1_w          4.8e-7, 3.7e-7, 8.2e-7, 1.0e-6, 4.9e-6, 2.5e-6 (bound 1e-4)
  excluded: amax1 / mask1 / mask2                               0.021 % / 0.014 % / 0.042 % of a buffer (cap 0.1 %; the masks of 3
                                                                frames have 7203 elements: 1 and 3 of them)
  frames4, pool2, pool3, amax2, amax3, dz2, the gating rule     exact
"""
import ctypes

import numpy as np
import pytest
import torch

import shallownet_local_ref as sl
from oracle import torch_ref

# (dtype, hw, n, dropout): the shapes of tests/test_shallownet_local_gpu.py's cases A, D and B (hw = 98)
CASES = [('f32', 98, 3, False), ('bf16', 98, 3, False), ('f32', 112, 3, False), ('bf16', 112, 3, False), ('bf16', 98, 3, True),
         ('bf16', 98, 49, False)]
_RUNS = {}


def run(dtype, hw, n, dropout, fault=None):
    """(inputs, stand-in buffers, figures), once per case."""
    key = (dtype, hw, n, dropout, fault)
    if key not in _RUNS:
        p, frames, d_sal, drop = sl.inputs(hw, n)
        keep, drop = (sl.KEEP, drop) if dropout else (None, None)
        dev = sl.standin(p, frames, d_sal, dtype, keep, drop, fault)
        _RUNS[key] = (dev, sl.check(dev, p, frames, d_sal, dtype, keep, drop))
    return _RUNS[key]


# ------------------------------------------------------------------------------------------------ 1. the stages are the net
@pytest.mark.parametrize('hw', [98, 112])
def test_chained_float64_stages_are_the_oracle_net(hw):
    """The forward stages without rounding, chained, against oracle.torch_ref.shallownet_forward; the backward stages, chained
    through the float64 decisions, against float64 autograd of it."""
    n = 2
    p, frames, d_sal, _ = sl.inputs(hw, n)
    g = sl.geom(hw)
    f64 = torch.float64
    W = {k: np.asarray(v, np.float64) for k, v in p.items()}
    win1 = sl.windows2x2(sl.conv_valid(frames, W['conv1_w'], f64))
    pool1, amax1 = np.maximum(win1.max(3) + W['conv1_b'], 0), win1.argmax(3)
    act2 = np.maximum(sl.conv_valid(pool1, W['conv2_w'], f64) + W['conv2_b'], 0)
    win2 = sl.windows3x3(act2)
    pool2, amax2 = win2.max(3), win2.argmax(3)
    act3 = np.maximum(sl.conv_valid(pool2, W['conv3_w'], f64) + W['conv3_b'], 0)
    win3 = sl.windows3x3(act3)
    pool3, amax3 = win3.max(3).reshape(n, -1), win3.argmax(3)

    def maxout(x, k):
        za, zb = sl.fc_halves(sl.matmul(x, W[k + '_w'], f64) + W[k + '_b'])
        return np.maximum(np.maximum(za, zb), 0), np.where(np.maximum(za, zb) > 0, np.where(za >= zb, 1, 2), 0)
    mo1, mask1 = maxout(pool3, 'fc1')
    sal, mask2 = maxout(mo1, 'fc2')
    pt = {k: torch.tensor(v, dtype=f64, requires_grad=True) for k, v in p.items()}
    ref = torch_ref.shallownet_forward(torch.tensor(frames, dtype=f64), pt)
    err = np.abs(sal - ref.detach().numpy().reshape(n, 2401)).max()
    print('chained forward stages against the oracle, %d: %.3e' % (hw, err))
    assert err < 1e-12
    (ref * torch.tensor(d_sal, dtype=f64)).sum().backward()
    got = {}
    dz2 = sl.route(d_sal.reshape(n, 2401).astype(np.float64), mask2)
    got['fc2_b'], got['fc2_w'] = dz2.sum(0), mo1.T @ dz2
    dz1 = sl.route(dz2 @ W['fc2_w'].T, mask1)
    got['fc1_b'], got['fc1_w'] = dz1.sum(0), pool3.T @ dz1
    dy3 = sl.unpool3x3((dz1 @ W['fc1_w'].T).reshape(amax3.shape), amax3, act3)
    got['conv3_b'], got['conv3_w'] = dy3.sum(axis=(0, 1, 2)), sl.conv_wgrad(pool2, dy3, 3, f64)
    dy2 = sl.unpool3x3(sl.conv_dgrad(dy3, W['conv3_w'], g['p2'], f64), amax2, act2)
    got['conv2_b'], got['conv2_w'] = dy2.sum(axis=(0, 1, 2)), sl.conv_wgrad(pool1, dy2, 3, f64)
    dy1 = sl.unpool2x2(sl.conv_dgrad(dy2, W['conv2_w'], g['p1'], f64), amax1, pool1)
    got['conv1_b'], got['conv1_w'] = dy1.sum(axis=(0, 1, 2)), sl.conv_wgrad(frames, dy1, 5, f64)
    # torch.maximum halves the gradient of an exact tie where tf.maximum sends it to the first operand: the tied columns
    # are equal, so everything behind them agrees, and only those columns of the FC gradients are left out here
    tied = [j + h for j in sl.TIE_UNITS for h in (0, 2401)]
    for k in sl.PARAMS:
        want = pt[k].grad.numpy().copy()
        if k.startswith('fc'):
            got[k][..., tied] = want[..., tied] = 0
        e = np.abs(got[k] - want).max() / np.abs(want).max()
        print('chained backward stages against autograd, %d %s: %.3e' % (hw, k, e))
        assert e < 1e-11, k


def test_rounding_switch_and_tied_pairs():
    p = sl.params(98)
    for k in ('fc1', 'fc2'):
        for j in sl.TIE_UNITS:
            assert np.array_equal(p[k + '_w'][:, j], p[k + '_w'][:, j + 2401]) and p[k + '_b'][j] == p[k + '_b'][j + 2401] > 0
    assert all(np.abs(p[k]).min() > 0 for k in sl.PARAMS if k.endswith('_b'))
    v = np.float32([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -9])
    assert np.array_equal(sl.round_T('bf16')(v), [1.0, 1.0 + 2.0 ** -7]) and np.array_equal(sl.round_T('f32')(v), v)


# ------------------------------------------------------------------------------------------------ 2. the bounds hold with margin
@pytest.mark.parametrize('dtype,hw,n,dropout', CASES)
def test_fp32_stand_in_passes_every_check_at_half_its_bound(dtype, hw, n, dropout):
    """fp32 products and fp32 accumulation of the same operands: every tolerance, every flip cap and every excluded share at
    most half used, every exact check exact -- the references' own precision does not use the bounds up -- and the decisions
    are not degenerate: every pool place, every 2x2 member and every mask value occurs among the checked elements."""
    dev, errs = run(dtype, hw, n, dropout)
    sl.report('stand-in %s %d n=%d%s' % (dtype, hw, n, ' dropout' if dropout else ''), errs)
    assert set(errs) == set(sl.FWD + sl.BWD)
    assert sl.violations(errs, margin=2.0) == []
    assert errs['amax1']['seen'] == [0, 1, 2, 3]
    assert errs['amax2']['seen'] == errs['amax3']['seen'] == list(range(9))
    assert errs['mask1']['seen'] == errs['mask2']['seen'] == [0, 1, 2]
    tied = list(sl.TIE_UNITS)
    assert (dev['mask1'][:, tied] == 1).any() and (dev['mask2'][:, tied] == 1).any()      # a tie above zero is among them


# ------------------------------------------------------------------------------------------------ 3. seeded faults are caught
CAUGHT_BY = {'pool_last_max': 'amax2', 'same_pad_after': 'pool2', 'argmax_after_relu': 'amax1', 'maxout_tie_second': 'mask1',
             'mask_halves_swapped': 'mask2', 'no_inv_keep': 'dz1', 'grad_to_gated': 'dy3_gate', 'dgrad_not_rotated': 'dpool2',
             'dgrad_unswapped': 'dpool1', 'bias_grad_halo': 'conv3_b', 'bf16_trunc_store': 'act2'}


@pytest.mark.parametrize('fault,caught_by', sorted(CAUGHT_BY.items()))
def test_seeded_fault_fails_its_check(fault, caught_by):
    """One mistake in the stand-in (bf16, 98, 3 frames, the dropout site on), everything else as above.  The checks are local,
    so the stages behind the faulty one still see consistent operands: what fails is the check of the stage that is wrong."""
    _, errs = run('bf16', 98, 3, True, fault)
    bad = sl.violations(errs)
    sl.report('fault %s' % fault, {k: errs[k] for k in bad})
    assert caught_by in bad, bad


def test_every_fault_has_a_check():
    assert set(CAUGHT_BY) == set(sl.FAULTS) and set(CAUGHT_BY.values()) <= set(sl.FWD + sl.BWD)


# ------------------------------------------------------------------------------------------------ 4. the read-back ABI, host side
def test_buffer_elems_host_only():
    """rgp_shallownet_buffer_elems before any forward: max_frames of every buffer's un-padded shape; 0 for an unknown name and for
    training-plan buffers of an inference plan; read_buffer without a workspace is refused."""
    from recurrent_gaze_prediction_amd import _lib
    lib = _lib.load()
    for hw in (98, 112):
        shp = sl.shapes(hw, 5)
        train, infer = ctypes.c_void_p(), ctypes.c_void_p()
        assert lib.rgp_shallownet_create_ex(ctypes.byref(train), 5, hw, _lib.RGP_BF16, 1) == 0
        assert lib.rgp_shallownet_create_ex(ctypes.byref(infer), 5, hw, _lib.RGP_F32, 0) == 0
        assert set(shp) == set(sl.FORWARD_BUFFERS + sl.TRAINING_BUFFERS + sl.BACKWARD_BUFFERS)
        for k, s in shp.items():
            assert lib.rgp_shallownet_buffer_elems(train, k.encode()) == int(np.prod(s)), k
            assert lib.rgp_shallownet_buffer_elems(infer, k.encode()) == (int(np.prod(s)) if k in sl.FORWARD_BUFFERS else 0), k
        assert lib.rgp_shallownet_buffer_elems(train, b'nope') == 0
        assert lib.rgp_shallownet_read_buffer(train, b'pool1', None, None) == -1
        lib.rgp_shallownet_destroy(train)
        lib.rgp_shallownet_destroy(infer)
