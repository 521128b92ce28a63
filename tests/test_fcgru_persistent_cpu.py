"""CPU: what the persistent fc-GRU recurrence (RGP_FCGRU_PERSISTENT, csrc/fcgru_seq.hip.h) can show without a device.

1. Flag arithmetic of rgp_fcgru_create_flags on unbound plans.  The refusals that depend on the ARGUMENTS (f32, batch > 64,
   both path flags, an unknown bit) come before the library asks the device for its CU count, so they are checked here; an
   accepted persistent create needs that count and is covered by tests/test_fcgru_persistent_gpu.py.
2. The one-step float64 reference of tests/fcgru_local_ref.py against its own fp32 stand-in: the stand-in stays within HALF
   of every bound on the test inputs, and each seeded mistake breaks one.
3. The model's recovery from RGP_ETIMEOUT, on a stand-in engine.
"""
import ctypes

import numpy as np
import pytest
import torch

import fcgru_local_ref as ref
from recurrent_gaze_prediction_amd import _lib

B, T = 3, 4
RGP_EINVAL, RGP_ESTATE = -1, -4                    # include/rgp.h


# ------------------------------------------------------------------------------------------------ 1. flags
def _create(batch, dtype, flags, n_steps=4):
    """-> (lib, plan, return code, rgp_last_error())."""
    lib = _lib.load()
    h = ctypes.c_void_p()
    rc = lib.rgp_fcgru_create_flags(ctypes.byref(h), batch, n_steps, 7, 7, dtype, flags)
    return lib, h, rc, lib.rgp_last_error().decode()


@pytest.mark.parametrize('batch,dtype,flags,word,n_steps', [
    (3, _lib.RGP_F32, _lib.RGP_FCGRU_PERSISTENT, 'dtype', 4),
    (65, _lib.RGP_BF16, _lib.RGP_FCGRU_PERSISTENT, 'batch', 4),
    (65, _lib.RGP_BF16, _lib.RGP_FCGRU_PERSISTENT | _lib.RGP_FCGRU_SAVE_FOR_BACKWARD, 'batch', 4),
    (3, _lib.RGP_BF16, _lib.RGP_FCGRU_PERSISTENT | _lib.RGP_FCGRU_PER_STEP, 'both', 4),
    (3, _lib.RGP_BF16, 8, 'flags', 4),
    (3, _lib.RGP_BF16, 1 << 20, 'flags', 4),
    # 32-bit byte offsets into the exchange rows (64 rows x T x 1664 x 2 bytes < 2^32): at most 16384 steps
    (1, _lib.RGP_BF16, _lib.RGP_FCGRU_PERSISTENT, 'n_steps', 16385),
    (64, _lib.RGP_BF16, _lib.RGP_FCGRU_PERSISTENT | _lib.RGP_FCGRU_SAVE_FOR_BACKWARD, 'n_steps', 20000),
])
def test_create_flags_refusals_name_the_argument(batch, dtype, flags, word, n_steps):
    lib, h, rc, msg = _create(batch, dtype, flags, n_steps)
    assert rc == RGP_EINVAL and word in msg, (rc, msg)


def test_refusals_of_the_four_persistent_kinds_come_in_one_order():
    """The order of the refusals that rgp_fcgru_create_flags takes from its table of the four persistent kinds (flag, noun,
    dtype, training plan or not): at batch 65, n_steps 2 every one of them is refused for an ARGUMENT, with RGP_EINVAL, before
    the device is asked for its CU count (this runs without a device: a device error would be RGP_EHIP).  The two BPTT flags are
    given with RGP_FCGRU_SAVE_FOR_BACKWARD, which they need ahead of everything else; without it that is what the message names."""
    L = _lib
    save = L.RGP_FCGRU_SAVE_FOR_BACKWARD
    kinds = [(L.RGP_FCGRU_PERSISTENT, L.RGP_BF16, 0), (L.RGP_FCGRU_PERSISTENT_F32, L.RGP_F32, 0),
             (L.RGP_FCGRU_BPTT_PERSISTENT, L.RGP_BF16, save), (L.RGP_FCGRU_BPTT_PERSISTENT_F32, L.RGP_F32, save)]
    for flag, flag_dtype, needs in kinds:
        for dtype in (L.RGP_BF16, L.RGP_F32):
            lib, h, rc, msg = _create(65, dtype, flag | needs, 2)
            # the right dtype: the batch; the wrong one: the dtype, which comes first
            assert rc == RGP_EINVAL and ('batch' if dtype == flag_dtype else 'dtype') in msg, (flag, dtype, rc, msg)
            assert ('batch' in msg) == (dtype == flag_dtype), (flag, dtype, msg)
            if needs:
                lib, h, rc, msg = _create(65, dtype, flag, 2)
                assert rc == RGP_EINVAL and 'SAVE_FOR_BACKWARD' in msg and 'batch' not in msg, (flag, dtype, rc, msg)
    # two flags for one pass: refused as naming both, whatever else is wrong with the call
    for pair in (4 | 16, 2 | 16, 2 | 4, 8 | 32):
        for dtype in (L.RGP_BF16, L.RGP_F32):
            lib, h, rc, msg = _create(65, dtype, pair | save, 2)
            assert rc == RGP_EINVAL and 'both' in msg, (pair, dtype, rc, msg)


def test_per_step_plans_take_any_number_of_steps():
    lib, h, rc, msg = _create(1, _lib.RGP_BF16, _lib.RGP_FCGRU_PER_STEP, 16385)        # the limit is the persistent kernel's
    assert rc == 0, msg
    lib.rgp_fcgru_destroy(h)


def test_per_step_plans_have_no_persistent_workgroups_and_inference_plans_no_buffers():
    for flags in (0, _lib.RGP_FCGRU_PER_STEP, _lib.RGP_FCGRU_SAVE_FOR_BACKWARD, _lib.RGP_FCGRU_SAVE_FOR_BACKWARD | _lib.RGP_FCGRU_PER_STEP):
        for dtype in (_lib.RGP_BF16, _lib.RGP_F32):
            lib, h, rc, msg = _create(65, dtype, flags)
            assert rc == 0, msg
            assert lib.rgp_fcgru_persistent_workgroups(h) == 0
            train = bool(flags & _lib.RGP_FCGRU_SAVE_FOR_BACKWARD)
            assert lib.rgp_fcgru_buffer_elems(h, b'h') == (5 * 65 * 1617 if train else 0)
            assert lib.rgp_fcgru_buffer_elems(h, b'xpre') == (65 * 4 * 3 * 1617 if train else 0)
            assert lib.rgp_fcgru_buffer_elems(h, b'nope') == 0
            dst = (ctypes.c_float * 4)()
            assert lib.rgp_fcgru_read_buffer(h, b'nope', dst, None) == RGP_EINVAL and b'nope' in lib.rgp_last_error()
            # an inference plan has no such buffers; a training plan none before its first forward
            assert lib.rgp_fcgru_read_buffer(h, b'rh', dst, None) == RGP_ESTATE
            assert (b'SAVE_FOR_BACKWARD' in lib.rgp_last_error()) == (not train)
            lib.rgp_fcgru_destroy(h)
    lib = _lib.load()
    assert lib.rgp_fcgru_persistent_workgroups(None) == 0


def test_create_and_create_ex_mean_flags_0_and_save():
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.rgp_fcgru_create(ctypes.byref(h), 2, 3, 7, 7, _lib.RGP_BF16) == 0
    ws0 = lib.rgp_fcgru_workspace_bytes(h)
    assert lib.rgp_fcgru_buffer_elems(h, b'u') == 0
    lib.rgp_fcgru_destroy(h)
    assert lib.rgp_fcgru_create_flags(ctypes.byref(h), 2, 3, 7, 7, _lib.RGP_BF16, 0) == 0
    assert lib.rgp_fcgru_workspace_bytes(h) == ws0             # the default plan takes nothing for the persistent path
    lib.rgp_fcgru_destroy(h)
    assert lib.rgp_fcgru_create_ex(ctypes.byref(h), 2, 3, 7, 7, _lib.RGP_BF16, 1) == 0
    assert lib.rgp_fcgru_buffer_elems(h, b'u') == 3 * 2 * 1617 and lib.rgp_fcgru_workspace_bytes(h) > ws0
    lib.rgp_fcgru_destroy(h)


# ------------------------------------------------------------------------------------------------ 2. reference vs stand-in
@pytest.fixture(scope='module')
def inputs():
    return ref.features(B, T), ref.params()


def test_standin_is_within_half_of_every_bound(inputs):
    x, p = inputs
    dev = ref.standin(x, p)
    errs = ref.check(dev, p)
    ref.report('stand-in', errs)
    assert ref.violations(errs, margin=2.0) == [], errs
    # the inputs exercise the gates: neither saturated nor stuck at the bias
    g = np.concatenate([dev['u'].ravel(), dev['r'].ravel()])
    assert ((g > 0.1) & (g < 0.9)).mean() > 0.5 and (np.abs(dev['c']) < 0.9).mean() > 0.5
    assert np.abs(dev['h'][-1]).max() > 0.1


@pytest.mark.parametrize('fault', ref.FAULTS)
def test_each_seeded_mistake_breaks_a_bound(inputs, fault):
    x, p = inputs
    errs = ref.check(ref.standin(x, p, fault=fault), p)
    bad = ref.violations(errs)
    ref.report(fault, {k: errs[k] for k in bad})
    assert bad, (fault, errs)


# ------------------------------------------------------------------------------------------------ 3. model recovery
class _Dropout(object):
    """engine.DropoutSite's state: keep probability, Philox key and the draw counter."""
    keep_prob, seed, draws = 1.0, 0, 0

    def configure(self, keep_prob, seed=0):
        self.keep_prob, self.seed, self.draws = float(keep_prob), int(seed), 0

    def off(self):
        pass


class _StandInEngine(object):
    """What GazePredictionGRU touches of FcGruEngine; a persistent instance reports RGP_ETIMEOUT once and returns NaN maps."""
    made = []

    def __init__(self, batch, n_steps, gazemap_hw=(49, 49), dtype='f32', device='cpu', save_for_backward=False, per_step=False,
                 persistent=False):
        self.B, self.T, self.GH, self.GW = batch, n_steps, gazemap_hw[0], gazemap_hw[1]
        self.dtype, self.device, self.save_for_backward, self.per_step = dtype, device, save_for_backward, per_step
        self.persistent = bool(persistent)
        self.lost = self.persistent
        self.weights = None
        self.adam_m = self.adam_v = None
        self.dropout = _Dropout()
        self.forwards = 0
        _StandInEngine.made.append(self)

    def set_weights(self, params):
        self.weights = {k: torch.as_tensor(np.asarray(v)).clone() for k, v in params.items()}

    def status(self):
        if self.lost:
            self.lost = False
            e = _lib.RgpError('lost member')
            e.code = _lib.RGP_ETIMEOUT
            raise e

    def forward(self, x, want_probs=True, **kw):
        self.forwards += 1
        z = torch.full((self.B, self.T, self.GH, self.GW), float('nan') if self.lost else 0.0)
        return z, torch.softmax(z.reshape(self.B, self.T, -1), -1).reshape(z.shape)


def test_model_switches_to_per_step_on_timeout(monkeypatch, tmp_path):
    from recurrent_gaze_prediction_amd import engine
    from recurrent_gaze_prediction_amd.models.base import Session
    from recurrent_gaze_prediction_amd.models import gaze_rnn, gaze_rnn77
    monkeypatch.setattr(engine, 'FcGruEngine', _StandInEngine)
    for module, hw in ((gaze_rnn, (7, 7)), (gaze_rnn77, None)):
        _StandInEngine.made = []
        cfg = module.GRUModelConfig()
        assert cfg.fcgru_path is None                          # the default: the library's choice, per step
        cfg.batch_size, cfg.n_lstm_steps, cfg.train_dir, cfg.fcgru_path = 2, 3, str(tmp_path), 'persistent'
        cfg.loss_type = 'xentropy'                             # (gaze_rnn77's own is l2: predict() then returns raw maps)
        kw = {} if hw is None else {'gazemap_height': hw[0], 'gazemap_width': hw[1]}
        model = module.GazePredictionGRU(Session('cpu'), None, cfg, **kw)
        first = model.engine
        assert first.persistent and not first.per_step
        first.adam_m = torch.arange(4.0)
        site = first.dropout
        assert site.keep_prob == cfg.train_keep_prob and site.seed != 0
        site.draws = 11                                        # eleven training steps so far
        maps = model.predict(np.zeros((2, 3, 1024, 7, 7), np.float32))
        assert model.engine is not first and model.engine.per_step and not model.engine.persistent
        assert cfg.fcgru_path == 'per_step'
        assert first.forwards == 1 and model.engine.forwards == 1          # the batch was computed again on the new engine
        assert torch.isfinite(maps).all() and torch.allclose(maps.reshape(6, -1).sum(-1), torch.ones(6))
        assert all(torch.equal(model.engine.weights[k], first.weights[k]) for k in first.weights)
        assert torch.equal(model.engine.adam_m, first.adam_m) and model.engine.adam_m is not first.adam_m
        # the dropout site goes on where it was: key and draw counter, not a restart from the seed
        now = model.engine.dropout
        assert now is not site and (now.keep_prob, now.seed, now.draws) == (site.keep_prob, site.seed, 11)
        assert len(_StandInEngine.made) == 2
        assert not model._recover_from_timeout()                           # already the fall-back
        # a per-step engine is never asked for its status (no host wait on the default path)
        model.engine.lost = True
        model.predict(np.zeros((2, 3, 1024, 7, 7), np.float32))
        assert model.engine.lost and len(_StandInEngine.made) == 2
