"""CPU: what the persistent f32 fc-GRU BPTT (RGP_FCGRU_BPTT_PERSISTENT_F32, csrc/fcgru_bptt_f32.hip.h) can show without a device.

1. The library's interface: the constant, and the refusals of rgp_fcgru_create_flags that depend on the ARGUMENTS (the flag
   without SAVE_FOR_BACKWARD, a plan that is not f32, batch > 64, the flag together with RGP_FCGRU_BPTT_PERSISTENT, batch16 x
   n_steps past the 32-bit offsets), which come before the library asks the device for its CU count.  RGP_FCGRU_BPTT_PERSISTENT
   on an f32 plan stays refused.
2. The float64 BPTT reference of tests/fcgru_f32_bptt_ref.py against its own fp32 stand-in: the stand-in stays within HALF of
   every bound at (3,4), (17,3) and (64,3), and each seeded mistake breaks one.  The figures the bounds were set from are
   measured again and printed.
3. The model's plumbing on a stand-in engine: which keyword each compute_dtype names, and the recovery from an RGP_ETIMEOUT that
   an engine whose f32 BPTT was persistent reports.
"""
import ctypes

import numpy as np
import pytest
import torch

import fcgru_f32_bptt_ref as ref
import fcgru_local_ref as fref
from recurrent_gaze_prediction_amd import _lib

RGP_EINVAL = -1                                    # include/rgp.h
SAVE, BPTT = _lib.RGP_FCGRU_SAVE_FOR_BACKWARD, _lib.RGP_FCGRU_BPTT_PERSISTENT
BPTT32 = getattr(_lib, 'RGP_FCGRU_BPTT_PERSISTENT_F32', 32)
ROW = 3 * 1664 * 4                                 # bytes per fp32 dxpre row


# ------------------------------------------------------------------------------------------------ 1. interface
def test_lib_declares_the_constant():
    assert _lib.RGP_FCGRU_BPTT_PERSISTENT_F32 == 32
    assert (_lib.RGP_FCGRU_PERSISTENT, _lib.RGP_FCGRU_BPTT_PERSISTENT, _lib.RGP_FCGRU_PERSISTENT_F32) == (4, 8, 16)


@pytest.mark.parametrize('batch,n_steps,dtype,flags,word', [
    (3, 4, _lib.RGP_F32, BPTT32, 'SAVE_FOR_BACKWARD'),                     # the flag without SAVE
    (3, 4, _lib.RGP_F32, BPTT32 | _lib.RGP_FCGRU_PERSISTENT_F32, 'SAVE_FOR_BACKWARD'),
    (3, 4, _lib.RGP_F32, BPTT32 | _lib.RGP_FCGRU_PER_STEP, 'SAVE_FOR_BACKWARD'),
    (3, 4, _lib.RGP_BF16, BPTT32 | SAVE, 'f32 plans'),                     # a plan that is not f32
    (65, 4, _lib.RGP_F32, BPTT32 | SAVE, 'batch'),
    (3, 4, _lib.RGP_F32, BPTT32 | BPTT | SAVE, 'RGP_FCGRU_BPTT_PERSISTENT_F32 with RGP_FCGRU_BPTT_PERSISTENT'),
    (3, 4, _lib.RGP_BF16, BPTT32 | BPTT | SAVE, 'RGP_FCGRU_BPTT_PERSISTENT_F32 with RGP_FCGRU_BPTT_PERSISTENT'),
    # (B16 T + 1) * 3 * 1664 * 4 bytes < 2^32: at 64 clips 3360 steps pass the check, 3361 do not
    (64, 3361, _lib.RGP_F32, BPTT32 | SAVE, '2^32'),
    # the rows >= B of the last 16-clip fragment must land behind the buffer, not wrap: batch rounded up to 16
    (1, 13444, _lib.RGP_F32, BPTT32 | SAVE, '2^32'),
    (49, 3361, _lib.RGP_F32, BPTT32 | SAVE, '2^32'),
])
def test_create_flags_refusals_name_the_reason(batch, n_steps, dtype, flags, word):
    """(On the parent commit every one of these says "unknown flags".)"""
    lib = _lib.load()
    h = ctypes.c_void_p()
    rc = lib.rgp_fcgru_create_flags(ctypes.byref(h), batch, n_steps, 7, 7, dtype, flags)
    msg = lib.rgp_last_error().decode()
    assert rc == RGP_EINVAL and word in msg and 'BPTT' in msg and 'unknown flags' not in msg, (rc, msg)


def test_the_offset_limit_is_the_stated_one():
    assert (64 * 3360 + 1) * ROW < 2 ** 32 <= (64 * 3361 + 1) * ROW
    assert (16 * 13443 + 1) * ROW < 2 ** 32 <= (16 * 13444 + 1) * ROW      # batch 1 is addressed as a whole 16-row fragment


def test_flag_8_on_an_f32_plan_still_refuses():
    lib = _lib.load()
    h = ctypes.c_void_p()
    rc = lib.rgp_fcgru_create_flags(ctypes.byref(h), 3, 4, 7, 7, _lib.RGP_F32, BPTT | SAVE)
    msg = lib.rgp_last_error().decode()
    assert rc == RGP_EINVAL and 'bf16' in msg and 'BPTT' in msg, (rc, msg)


def test_unknown_bits_are_still_refused():
    lib = _lib.load()
    h = ctypes.c_void_p()
    rc = lib.rgp_fcgru_create_flags(ctypes.byref(h), 3, 4, 7, 7, _lib.RGP_F32, 64 | SAVE)
    assert rc == RGP_EINVAL and 'unknown flags' in lib.rgp_last_error().decode()


# ------------------------------------------------------------------------------------------------ 2. reference vs stand-in
@pytest.fixture(scope='module')
def forwards():
    p = fref.params()
    return p, {(B, T): ref.standin_forward(fref.features(B, T), p) for B, T in ref.SHAPES}


def test_standin_is_within_half_of_every_bound(forwards):
    p, fwd = forwards
    worst_part = worst_dh0 = 0.0
    for (B, T), f in fwd.items():
        dev = ref.standin_bptt(f, p)
        errs = ref.check(dev, p)
        ref.report('f32 stand-in %dx%d' % (B, T), errs)
        assert ref.violations(errs, margin=2.0) == [], {k: errs[k] for k in ref.violations(errs, margin=2.0)}
        worst_part = max(worst_part, max(e['err'] for k, e in errs.items() if k != 'dh0'))
        worst_dh0 = max(worst_dh0, errs['dh0']['err'])
        # the inputs exercise every term: no part is all zero (dr_pre of step 0 is: h_{-1} = 0), the carry reaches step 0
        assert all(np.abs(dev['dxpre'][:, 1:, k]).max() > 0 for k in range(3)) and np.abs(dev['dh0']).max() > 0
        assert not np.any(dev['dxpre'][:, 0, 1])
    # the figures the bounds were set from: 8 x, rounded up to a power of two
    print('f32 stand-in worst part figure %.3e (recorded %.3e, bound %.3e); worst |dh0 - ref| / max|ref| %.3e (recorded %.3e, bound %.3e)' %
          (worst_part, ref.PART_MEASURED, ref.PART_BOUND, worst_dh0, ref.DH0_MEASURED_F32, ref.DH0_BOUND_F32))
    assert ref.PART_BOUND == ref.bound_from(ref.PART_MEASURED) and ref.DH0_BOUND_F32 == ref.bound_from(ref.DH0_MEASURED_F32)
    # (the host's BLAS summation order in the forward stand-in may move the figures' last digits)
    assert 8 * worst_part <= ref.PART_BOUND and 8 * worst_dh0 <= ref.DH0_BOUND_F32


@pytest.mark.parametrize('fault', ref.FAULTS)
def test_each_seeded_mistake_breaks_a_bound(forwards, fault):
    p, fwd = forwards
    errs = ref.check(ref.standin_bptt(fwd[(3, 4)], p, fault=fault), p)
    bad = ref.violations(errs)
    print(fault, bad)
    assert bad, (fault, errs)


def test_there_are_at_least_nine_seeded_mistakes():
    assert len(set(ref.FAULTS)) >= 9


def test_reference_uses_the_devices_own_rows(forwards):
    """A wrong dc_pre row of ONE step shows in that step and nowhere in the reference of the later ones: the GEMM terms of a
    step are taken from the device's rows."""
    p, fwd = forwards
    dev = ref.standin_bptt(fwd[(3, 4)], p)
    dev['dxpre'] = dev['dxpre'].copy()
    dev['dxpre'][:, 2, 2] = dev['dxpre'][:, 2, 2] * np.float32(1.5)
    bad = ref.violations(ref.check(dev, p))
    assert 'dc_pre[2]' in bad and 'dc_pre[3]' not in bad and 'du_pre[3]' not in bad and 'dr_pre[3]' not in bad


# ------------------------------------------------------------------------------------------------ 3. model plumbing
class _Dropout(object):
    """engine.DropoutSite's state: keep probability, Philox key and the draw counter."""
    keep_prob, seed, draws = 1.0, 0, 0

    def configure(self, keep_prob, seed=0):
        self.keep_prob, self.seed, self.draws = float(keep_prob), int(seed), 0

    def off(self):
        pass


class _StandInEngine(object):
    """What GazePredictionGRU touches of FcGruEngine, with the keyword of the f32 BPTT; it records the keywords it was NAMED
    with.  The backward of a BPTT-persistent instance loses a member once: status() then reports RGP_ETIMEOUT once."""
    made = []

    def __init__(self, batch, n_steps, gazemap_hw=(49, 49), dtype='f32', device='cpu', save_for_backward=False, per_step=False,
                 persistent=False, **kw):
        assert set(kw) <= {'bptt_persistent', 'bptt_persistent_f32'}, kw
        self.named = dict(kw)
        self.B, self.T, self.GH, self.GW = batch, n_steps, gazemap_hw[0], gazemap_hw[1]
        self.dtype, self.device, self.save_for_backward, self.per_step = dtype, device, save_for_backward, per_step
        self.persistent = bool(persistent)
        # (the library refuses bptt_persistent on f32 plans and bptt_persistent_f32 on bf16 plans)
        assert not (kw.get('bptt_persistent') and dtype == 'f32') and not (kw.get('bptt_persistent_f32') and dtype != 'f32')
        self.bptt_persistent = bool(kw.get('bptt_persistent') or kw.get('bptt_persistent_f32'))
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


def _model(monkeypatch, tmp_path, module, hw, dtype, fwd_path, bptt_path):
    from recurrent_gaze_prediction_amd import engine
    from recurrent_gaze_prediction_amd.models.base import Session
    monkeypatch.setattr(engine, 'FcGruEngine', _StandInEngine)
    _StandInEngine.made = []
    cfg = module.GRUModelConfig()
    cfg.batch_size, cfg.n_lstm_steps, cfg.train_dir, cfg.compute_dtype = 2, 3, str(tmp_path), dtype
    cfg.fcgru_path, cfg.fcgru_bptt_path, cfg.loss_type = fwd_path, bptt_path, 'xentropy'
    kw = {} if hw is None else {'gazemap_height': hw[0], 'gazemap_width': hw[1]}
    return cfg, module.GazePredictionGRU(Session('cpu'), None, cfg, **kw)


def test_the_keyword_follows_the_compute_dtype(monkeypatch, tmp_path):
    from recurrent_gaze_prediction_amd.models import gaze_rnn, gaze_rnn77
    for module, hw in ((gaze_rnn, (7, 7)), (gaze_rnn77, None)):
        _, model = _model(monkeypatch, tmp_path, module, hw, 'f32', None, 'persistent')
        assert model.engine.named == {'bptt_persistent_f32': True}
        _, model = _model(monkeypatch, tmp_path, module, hw, 'bf16', None, 'persistent')
        assert model.engine.named == {'bptt_persistent': True}
        for dtype in ('f32', 'bf16'):                          # named only when asked for
            for path in (None, 'per_step'):
                _, model = _model(monkeypatch, tmp_path, module, hw, dtype, None, path)
                assert model.engine.named == {} and not model.engine.bptt_persistent


@pytest.mark.parametrize('fwd_path', [None, 'per_step', 'persistent'])
def test_model_rebuilds_the_engine_per_step_when_the_f32_bptt_times_out(monkeypatch, tmp_path, fwd_path):
    from recurrent_gaze_prediction_amd.models import gaze_rnn, gaze_rnn77
    for module, hw in ((gaze_rnn, (7, 7)), (gaze_rnn77, None)):
        cfg, model = _model(monkeypatch, tmp_path, module, hw, 'f32', fwd_path, 'persistent')
        first = model.engine
        assert first.named == {'bptt_persistent_f32': True} and first.dtype == 'f32'
        assert first.persistent == (fwd_path == 'persistent') and first.per_step == (fwd_path == 'per_step')
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
        # the new engine takes neither persistent path, and is an f32 plan as the old one was
        assert new.per_step and not new.persistent and not new.bptt_persistent and new.named == {} and new.dtype == 'f32'
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
