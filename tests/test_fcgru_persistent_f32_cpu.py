"""CPU: what the f32 persistent fc-GRU recurrence (RGP_FCGRU_PERSISTENT_F32, csrc/fcgru_seq_f32.hip.h) can show without a device.

1. Flag arithmetic of rgp_fcgru_create_flags on unbound plans: every refusal that depends on the arguments comes before the
   library asks the device for its CU count (an accepted create needs that count: tests/test_fcgru_persistent_f32_gpu.py).
2. The one-step float64 reference on unrounded kernels (tests/fcgru_f32_local_ref.py) against a numpy stand-in of the kernel's
   arithmetic: the stand-in stays within HALF of every bound at (B, T) = (3, 4) and (17, 3), and each seeded mistake breaks one.
"""
import ctypes

import numpy as np
import pytest

import fcgru_local_ref as ref
import fcgru_f32_local_ref as ref32
from recurrent_gaze_prediction_amd import _lib

RGP_EINVAL = -1                                    # include/rgp.h
P32 = getattr(_lib, 'RGP_FCGRU_PERSISTENT_F32', 16)
SAVE, PER_STEP, PERSISTENT = _lib.RGP_FCGRU_SAVE_FOR_BACKWARD, _lib.RGP_FCGRU_PER_STEP, _lib.RGP_FCGRU_PERSISTENT


def _create(batch, dtype, flags, n_steps=4):
    lib = _lib.load()
    h = ctypes.c_void_p()
    rc = lib.rgp_fcgru_create_flags(ctypes.byref(h), batch, n_steps, 7, 7, dtype, flags)
    return lib, h, rc, lib.rgp_last_error().decode()


def test_the_flag_is_bit_16():
    assert _lib.RGP_FCGRU_PERSISTENT_F32 == 16


@pytest.mark.parametrize('batch,dtype,flags,word,n_steps', [
    (3, _lib.RGP_BF16, P32, 'f32', 4),
    (3, _lib.RGP_BF16, P32 | SAVE, 'f32', 4),
    (65, _lib.RGP_F32, P32, 'batch', 4),
    (65, _lib.RGP_F32, P32 | SAVE, 'batch', 4),
    (3, _lib.RGP_F32, P32 | PER_STEP, 'both', 4),
    (3, _lib.RGP_F32, P32 | PERSISTENT, 'both', 4),
    (3, _lib.RGP_BF16, P32 | PERSISTENT, 'both', 4),
    # 32-bit byte offsets into the fp32 exchange rows: 64 rows x T x 1664 x 4 bytes < 2^32 is T <= 10081, rounded down to 8192
    (1, _lib.RGP_F32, P32, 'n_steps', 8193),
    (64, _lib.RGP_F32, P32 | SAVE, 'n_steps', 10082),
])
def test_create_flags_refusals_name_the_argument(batch, dtype, flags, word, n_steps):
    lib, h, rc, msg = _create(batch, dtype, flags, n_steps)
    assert rc == RGP_EINVAL and word in msg and 'unknown' not in msg, (rc, msg)


def test_the_older_flags_keep_refusing_f32():
    for flags in (PERSISTENT, _lib.RGP_FCGRU_BPTT_PERSISTENT | SAVE, _lib.RGP_FCGRU_BPTT_PERSISTENT | SAVE | P32):
        lib, h, rc, msg = _create(3, _lib.RGP_F32, flags)
        assert rc == RGP_EINVAL and 'dtype' in msg, (flags, rc, msg)


def test_the_step_limit_is_the_kernels_offset_range():
    assert 64 * 8192 * 1664 * 4 < 2 ** 32 and 64 * 10081 * 1664 * 4 < 2 ** 32 <= 64 * 10083 * 1664 * 4
    # a training plan's seeded rows are (T + 1) steps apart
    assert 64 * (8192 + 1) * 1664 * 4 < 2 ** 32


def test_per_step_f32_plans_have_no_persistent_workgroups():
    for flags in (0, PER_STEP, SAVE, SAVE | PER_STEP):
        lib, h, rc, msg = _create(65, _lib.RGP_F32, flags, 8193)
        assert rc == 0, msg
        assert lib.rgp_fcgru_persistent_workgroups(h) == 0
        lib.rgp_fcgru_destroy(h)


# ------------------------------------------------------------------------------------------------ reference vs stand-in
SHAPES = [(3, 4), (17, 3)]


@pytest.fixture(scope='module')
def weights():
    return ref.params()


@pytest.fixture(scope='module', params=SHAPES, ids=lambda s: '%dx%d' % s)
def inputs(request, weights):
    B, T = request.param
    return ref.features(B, T), weights


def test_k_order_is_a_permutation_of_each_quarter():
    for q in range(4):
        ks = ref32.k_order(q)
        assert sorted(ks) == list(range(416 * q, 416 * q + 416))
        assert ks[:8] == [416 * q + k for k in (0, 4, 8, 12, 1, 5, 9, 13)]          # MFMA (0, 0): fk = 0..3, then MFMA (0, 1)
        assert sorted(ref32.k_order(q, flip_e=True)) == sorted(ks) and ref32.k_order(q, flip_e=True) != ks


def test_standin_is_within_half_of_every_bound(inputs):
    x, p = inputs
    dev = ref32.standin(x, p)
    errs = ref32.check(dev, p)
    ref32.report('f32 stand-in %dx%d' % x.shape[:2], errs)
    assert ref32.violations(errs, margin=2.0) == [], errs
    # the inputs exercise the gates: neither saturated nor stuck at the bias
    g = np.concatenate([dev['u'].ravel(), dev['r'].ravel()])
    assert ((g > 0.1) & (g < 0.9)).mean() > 0.5 and (np.abs(dev['c']) < 0.9).mean() > 0.5
    assert np.abs(dev['h'][-1]).max() > 0.1


@pytest.mark.parametrize('fault', ref32.FAULTS)
def test_each_seeded_mistake_breaks_a_bound(weights, fault):
    x = ref.features(3, 4)
    errs = ref32.check(ref32.standin(x, weights, fault=fault), weights)
    bad = ref32.violations(errs)
    ref32.report(fault, {k: errs[k] for k in bad})
    assert bad, (fault, errs)
