"""CPU: what the persistent fc-GRU BPTT (RGP_FCGRU_BPTT_PERSISTENT, csrc/fcgru_bptt.hip.h) can show without a device.

1. The library's interface: the constant and the prototype in _lib, and the refusals of rgp_fcgru_create_flags that depend on
   the ARGUMENTS (the flag without SAVE_FOR_BACKWARD, f32, batch > 64, batch x n_steps past the 32-bit offsets), which come
   before the library asks the device for its CU count; an accepted create needs that count (tests/test_fcgru_bptt_gpu.py).
2. The float64 BPTT reference of tests/fcgru_bptt_ref.py against its own fp32 stand-in: the stand-in stays within HALF of every
   bound at (3,4), (17,3) and (64,3), and each seeded mistake breaks one.  The dh0 figure the bound was set from is measured
   again and printed.
3. The model's recovery from an RGP_ETIMEOUT that a BPTT-persistent engine reports, on a stand-in engine.
"""
import ctypes

import numpy as np
import pytest
import torch

import fcgru_bptt_ref as ref
import fcgru_local_ref as fref
from recurrent_gaze_prediction_amd import _lib

RGP_EINVAL = -1                                    # include/rgp.h
SHAPES = [(3, 4), (17, 3), (64, 3)]


# ------------------------------------------------------------------------------------------------ 1. interface
def test_lib_declares_the_constant_and_the_prototype():
    assert _lib.RGP_FCGRU_BPTT_PERSISTENT == 8
    lib = _lib.load()
    fn = lib.rgp_fcgru_bptt_persistent_workgroups
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == [ctypes.c_void_p]
    assert fn(None) == 0
    # a plan without the flag reports 0; the three names of the backward have their sizes on training plans only
    h = ctypes.c_void_p()
    assert lib.rgp_fcgru_create_flags(ctypes.byref(h), 5, 4, 7, 7, _lib.RGP_BF16, _lib.RGP_FCGRU_SAVE_FOR_BACKWARD) == 0
    assert fn(h) == 0
    assert lib.rgp_fcgru_buffer_elems(h, b'dxpre') == 5 * 4 * 3 * 1617
    assert lib.rgp_fcgru_buffer_elems(h, b'dh_head') == 5 * 4 * 1617 and lib.rgp_fcgru_buffer_elems(h, b'dh0') == 5 * 1617
    lib.rgp_fcgru_destroy(h)
    assert lib.rgp_fcgru_create_flags(ctypes.byref(h), 5, 4, 7, 7, _lib.RGP_BF16, 0) == 0
    assert lib.rgp_fcgru_buffer_elems(h, b'dxpre') == 0
    lib.rgp_fcgru_destroy(h)


SAVE, BPTT = _lib.RGP_FCGRU_SAVE_FOR_BACKWARD, getattr(_lib, 'RGP_FCGRU_BPTT_PERSISTENT', 8)


@pytest.mark.parametrize('batch,n_steps,dtype,flags,word', [
    (3, 4, _lib.RGP_BF16, BPTT, 'SAVE_FOR_BACKWARD'),                      # the flag without SAVE
    (3, 4, _lib.RGP_BF16, BPTT | _lib.RGP_FCGRU_PERSISTENT, 'SAVE_FOR_BACKWARD'),
    (3, 4, _lib.RGP_F32, BPTT | SAVE, 'bf16'),
    (65, 4, _lib.RGP_BF16, BPTT | SAVE, 'batch'),
    # (B T + 1) * 3 * 1664 * 2 bytes < 2^32: at 64 clips 6721 steps pass the check, 6722 do not
    (64, 6722, _lib.RGP_BF16, BPTT | SAVE, '2^32'),
    (1, 430186, _lib.RGP_BF16, BPTT | SAVE, '2^32'),
    # the rows >= B of the last 16-clip fragment must land behind the buffer, not wrap: batch rounded up to 16
    (1, 26887, _lib.RGP_BF16, BPTT | SAVE, '2^32'),
])
def test_create_flags_refusals_name_the_reason(batch, n_steps, dtype, flags, word):
    lib = _lib.load()
    h = ctypes.c_void_p()
    rc = lib.rgp_fcgru_create_flags(ctypes.byref(h), batch, n_steps, 7, 7, dtype, flags)
    msg = lib.rgp_last_error().decode()
    assert rc == RGP_EINVAL and word in msg and 'BPTT' in msg, (rc, msg)


def test_the_offset_limit_is_the_stated_one():
    assert (64 * 6721 + 1) * 3 * 1664 * 2 < 2 ** 32 <= (64 * 6722 + 1) * 3 * 1664 * 2


# ------------------------------------------------------------------------------------------------ 2. reference vs stand-in
@pytest.fixture(scope='module')
def forwards():
    p = fref.params()
    return p, {(B, T): ref.standin_forward(fref.features(B, T), p) for B, T in SHAPES}


def test_standin_is_within_half_of_every_bound(forwards):
    p, fwd = forwards
    worst_dh0 = 0.0
    for (B, T), f in fwd.items():
        dev = ref.standin_bptt(f, p)
        errs = ref.check(dev, p)
        ref.report('stand-in %dx%d' % (B, T), errs)
        assert ref.violations(errs, margin=2.0) == [], {k: errs[k] for k in ref.violations(errs, margin=2.0)}
        worst_dh0 = max(worst_dh0, errs['dh0']['err'])
        # the inputs exercise every term: no part is all zero (dr_pre of step 0 is: h_{-1} = 0), the carry reaches step 0
        assert all(np.abs(dev['dxpre'][:, 1:, k]).max() > 0 for k in range(3)) and np.abs(dev['dh0']).max() > 0
        assert not np.any(dev['dxpre'][:, 0, 1])
    # the figure DH0_BOUND was set from: 8 x, rounded up to a power of two
    print('stand-in worst |dh0 - ref| / max|ref| = %.3e (recorded %.3e, bound %.3e)' % (worst_dh0, ref.DH0_MEASURED, ref.DH0_BOUND))
    assert ref.DH0_BOUND == 2.0 ** np.ceil(np.log2(8 * ref.DH0_MEASURED))
    assert 8 * worst_dh0 <= ref.DH0_BOUND                  # (the host's BLAS summation order may move the figure's last digits)


@pytest.mark.parametrize('fault', ref.FAULTS)
def test_each_seeded_mistake_breaks_a_bound(forwards, fault):
    p, fwd = forwards
    errs = ref.check(ref.standin_bptt(fwd[(3, 4)], p, fault=fault), p)
    bad = ref.violations(errs)
    print(fault, bad)
    assert bad, (fault, errs)


def test_reference_uses_the_devices_own_rows():
    """A wrong dc_pre row of ONE step shows in that step's dc_pre and nowhere in the reference of the others: its GEMM terms
    are taken from the device's rows."""
    p = fref.params()
    dev = ref.standin_bptt(ref.standin_forward(fref.features(3, 4), p), p)
    dev['dxpre'] = dev['dxpre'].copy()
    dev['dxpre'][:, 2, 2] = fref._bf(dev['dxpre'][:, 2, 2] * np.float32(1.5))
    bad = ref.violations(ref.check(dev, p))
    # dr_pre[2] and everything downstream was computed from the ORIGINAL row: inconsistent with the altered one
    assert 'dc_pre[2]' in bad and 'dc_pre[3]' not in bad and 'du_pre[3]' not in bad and 'dr_pre[3]' not in bad


# ------------------------------------------------------------------------------------------------ 3. model recovery
class _Dropout(object):
    """engine.DropoutSite's state: keep probability, Philox key and the draw counter."""
    keep_prob, seed, draws = 1.0, 0, 0

    def configure(self, keep_prob, seed=0):
        self.keep_prob, self.seed, self.draws = float(keep_prob), int(seed), 0

    def off(self):
        pass


class _StandInEngine(object):
    """What GazePredictionGRU touches of FcGruEngine; the backward of a BPTT-persistent instance loses a member once: status()
    then reports RGP_ETIMEOUT once."""
    made = []

    def __init__(self, batch, n_steps, gazemap_hw=(49, 49), dtype='f32', device='cpu', save_for_backward=False, per_step=False,
                 persistent=False, bptt_persistent=False):
        self.B, self.T, self.GH, self.GW = batch, n_steps, gazemap_hw[0], gazemap_hw[1]
        self.dtype, self.device, self.save_for_backward, self.per_step = dtype, device, save_for_backward, per_step
        self.persistent, self.bptt_persistent = bool(persistent), bool(bptt_persistent)
        self.will_lose, self.lost = self.bptt_persistent, False
        self.weights = None
        self.adam_m = self.adam_v = None
        self.dropout = _Dropout()
        self.forwards = self.backwards = self.steps = self.status_calls = 0
        _StandInEngine.made.append(self)

    def set_weights(self, params):
        self.weights = {k: torch.as_tensor(np.asarray(v)).clone() for k, v in params.items()}

    def status(self):
        self.status_calls += 1
        if self.lost:
            self.lost = False
            e = _lib.RgpError('lost member')
            e.code = _lib.RGP_ETIMEOUT
            raise e

    def forward(self, x, want_probs=True, **kw):
        self.forwards += 1
        z = torch.zeros(self.B, self.T, self.GH, self.GW)
        return z, torch.softmax(z.reshape(self.B, self.T, -1), -1).reshape(z.shape)

    def backward(self, logits, probs, labels, loss_type='xentropy'):
        self.backwards += 1
        if self.will_lose:
            self.will_lose, self.lost = False, True
        self.grad_is_nan = self.lost

    def adam_step(self, step, lr, max_grad_norm=10.0, **kw):
        assert not self.grad_is_nan                            # the optimizer never sees the poisoned gradients
        self.steps += 1
        return torch.zeros(1)


@pytest.mark.parametrize('fwd_path', [None, 'per_step', 'persistent'])
def test_model_rebuilds_the_engine_per_step_when_the_bptt_times_out(monkeypatch, tmp_path, fwd_path):
    from recurrent_gaze_prediction_amd import engine
    from recurrent_gaze_prediction_amd.models.base import Session
    from recurrent_gaze_prediction_amd.models import gaze_rnn, gaze_rnn77
    monkeypatch.setattr(engine, 'FcGruEngine', _StandInEngine)
    for module, hw in ((gaze_rnn, (7, 7)), (gaze_rnn77, None)):
        _StandInEngine.made = []
        cfg = module.GRUModelConfig()
        assert cfg.fcgru_bptt_path is None                     # the default: the library's choice, per step
        cfg.batch_size, cfg.n_lstm_steps, cfg.train_dir = 2, 3, str(tmp_path)
        cfg.fcgru_path, cfg.fcgru_bptt_path, cfg.loss_type = fwd_path, 'persistent', 'xentropy'
        kw = {} if hw is None else {'gazemap_height': hw[0], 'gazemap_width': hw[1]}
        model = module.GazePredictionGRU(Session('cpu'), None, cfg, **kw)
        first = model.engine
        assert first.bptt_persistent and first.persistent == (fwd_path == 'persistent') and first.per_step == (fwd_path == 'per_step')
        first.adam_m = torch.arange(4.0)
        site = first.dropout
        site.draws = 11                                        # eleven training steps so far
        maps = model.predict(np.zeros((2, 3, 1024, 7, 7), np.float32), train=True)
        assert model.engine is first and first.status_calls == 1          # a BPTT-persistent plan is asked for its status
        labels = torch.zeros_like(maps)
        step0 = model.global_step
        model.train_op(model.predicted_gazemaps_logit, model.predicted_gazemaps, labels)
        new = model.engine
        assert new is not first and len(_StandInEngine.made) == 2
        assert new.per_step and not new.persistent and not new.bptt_persistent
        assert cfg.fcgru_path == 'per_step' and cfg.fcgru_bptt_path == 'per_step'
        # the step was computed again on the new engine, and only its gradients reached the optimizer
        assert (first.forwards, first.backwards, first.steps) == (1, 1, 0)
        assert (new.forwards, new.backwards, new.steps) == (1, 1, 1) and model.global_step == step0 + 1
        assert all(torch.equal(new.weights[k], first.weights[k]) for k in first.weights)
        assert torch.equal(new.adam_m, first.adam_m) and new.adam_m is not first.adam_m
        # the dropout site goes on where it was: key and draw counter, not a restart from the seed
        now = new.dropout
        assert now is not site and (now.keep_prob, now.seed, now.draws) == (site.keep_prob, site.seed, 11)
        assert not model._recover_from_timeout()               # already the fall-back
