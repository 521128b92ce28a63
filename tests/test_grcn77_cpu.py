"""CPU: gaze_grcn77 / gaze_rnn77 -- the float64 helper against a second statement of the read-out, the checkpoint name
mapping, the synthetic initialisers, and the two model modules' constants and configuration defaults."""
import numpy as np
import pytest
import torch

import grcn77_ref as ref
from recurrent_gaze_prediction_amd import checkpoint
from recurrent_gaze_prediction_amd import synthetic as syn


def test_helper_head_matches_plain_numpy_loops():
    p = syn.grcn77_params(3)
    x = syn.c3d_features(4, 1, 2)
    logits, states, emb = ref.forward_f64(x, p)
    assert logits.shape == (1, 2, 7, 7) and states.shape == (1, 2, 7, 7, 128) and emb.shape == (1, 2, 7, 7, 512)
    assert np.abs(states).max() > 0.1 and np.abs(states[:, 1] - states[:, 0]).max() > 1e-3      # the recurrence carries signal
    again = ref.head_numpy(states, p['out_W'], p['out_b'])
    assert np.abs(again - logits).max() < 1e-13 * max(1.0, np.abs(logits).max())
    # the projection, written out for one row: pixel (y, x) of frame (b, t) is the 1024 channels at that position
    row = x[0, 1, :, 3, 5].astype(np.float64) @ p['proj_c3d_W'].astype(np.float64) + p['proj_c3d_b']
    assert np.abs(row - emb[0, 1, 3, 5]).max() < 1e-12
    probs = ref.softmax49(logits)
    assert np.allclose(probs.reshape(2, 49).sum(-1), 1.0, atol=1e-14)
    assert np.abs(probs - ref.softmax_maps(torch.tensor(logits)).numpy()).max() < 1e-15


def test_helper_loss_is_over_49_pixels():
    p = syn.grcn77_params(5)
    x = syn.c3d_features(6, 1, 2)
    g = ref.normalized_labels(7, 1, 2)
    assert np.allclose(g.reshape(2, 49).sum(-1), 1.0, atol=1e-6)
    for loss_type in ('xentropy', 'l2'):
        ls, logits, grads, dx = ref.loss_and_grads(x, g, p, loss_type)
        z, gg = logits.reshape(2, 49), g.reshape(2, 49).astype(np.float64)
        want = (-(gg * np.log(ref.softmax49(logits).reshape(2, 49))).sum() if loss_type == 'xentropy' else 0.5 * ((z - gg) ** 2).sum()) / 2
        assert abs(ls - want) < 1e-12 * max(1.0, abs(want))
        assert set(grads) == set(ref.KEYS) and dx.shape == x.shape
        assert all(grads[k].shape == p[k].shape for k in ref.KEYS)


def test_grcn77_params_shapes_and_initialisers():
    p = syn.grcn77_params(11)
    assert set(p) == set(ref.KEYS)
    assert p['proj_c3d_W'].shape == (1024, 512) and p['proj_c3d_b'].shape == (512,)
    for k in ('Wz', 'Wr', 'W'):
        assert p['GRU_Conv_' + k].shape == (3, 3, 512, 128)
    for k in ('Uz', 'Ur', 'U'):
        assert p['GRU_Conv_' + k].shape == (3, 3, 128, 128)
    assert p['out_W'].shape == (128, 1) and p['out_b'].shape == (1,)
    for k in ('proj_c3d_W', 'proj_c3d_b', 'out_W', 'out_b'):           # uniform +-0.1 (gaze_grcn77.py:152-153,183-184)
        assert p[k].dtype == np.float32 and np.abs(p[k]).max() <= 0.1
    assert np.abs(p['out_W']).max() > 0.09
    assert np.abs(p['GRU_Conv_U']).max() <= 2 * 0.05 + 1e-7            # truncated normal
    assert abs(np.abs(syn.grcn77_params(11, gru_std=1e-4)['GRU_Conv_U']).max() - 2e-4) < 1e-5
    assert all(np.array_equal(p[k], syn.grcn77_params(11)[k]) for k in p)


def test_checkpoint_names_round_trip():
    p = syn.grcn77_params(12)
    tf_vars = checkpoint.export_model_variables('gaze_grcn77', p)
    assert set(tf_vars) == {'proj_c3d_W', 'proj_c3d_b', 'RCNBottom/out_W', 'RCNBottom/out_b'} | {
        'RCNBottom/GRU_Conv_' + g for g in ('Wz', 'Uz', 'Wr', 'Ur', 'W', 'U')}
    for v in (tf_vars, {k + ':0': a for k, a in tf_vars.items()}):
        extra = dict(v)
        extra['RCNBottom/out_W/Adam'] = np.zeros(1)
        extra['global_step'] = np.zeros(1)
        back = checkpoint.import_model_variables('gaze_grcn77', extra)
        assert set(back) == set(p)
        for k in p:
            assert back[k].dtype == np.float32 and np.array_equal(back[k], p[k]), k
    with pytest.raises(KeyError, match='GRU_Conv_Ur, out_W'):
        checkpoint.import_model_variables('gaze_grcn77', {k: v for k, v in tf_vars.items() if not k.endswith(('Ur', 'out_W'))})
    # gaze_grcn's names (scope RGP, batch-norm, up-sampling) are another model's
    with pytest.raises(KeyError):
        checkpoint.import_model_variables('gaze_grcn77', checkpoint.export_model_variables('gaze_grcn', syn.grcn_params(1, 2)))


def test_rnn77_checkpoint_mapping_is_the_fc_gru_s():
    p = syn.fcgru_params(13, 7, 7)
    assert p['proj_out_W'].shape == (1617, 49) and p['proj_out_b'].shape == (49,)
    back = checkpoint.import_model_variables('gaze_rnn77', checkpoint.export_model_variables('gaze_rnn77', p))
    assert set(back) == set(p) and all(np.array_equal(back[k], p[k]) for k in p)


def test_model_modules_constants_and_config_defaults():
    from recurrent_gaze_prediction_amd.models import gaze_grcn77, gaze_rnn, gaze_rnn77
    c = gaze_grcn77.CONSTANTS
    assert (c.image_width, c.image_height, c.gazemap_width, c.gazemap_height) == (98, 98, 7, 7)
    assert issubclass(gaze_grcn77.GazePredictionGRCN, gaze_rnn.GazePredictionGRU)
    assert gaze_grcn77.GRUModelConfig is gaze_rnn.GRUModelConfig          # gaze_grcn77.py:35 imports the parent's
    assert (gaze_grcn77.GazePredictionGRCN.DIM_CNN_PROJ, gaze_grcn77.GazePredictionGRCN.RNN_STATE_SIZE) == (512, 128)
    assert 'inert' in gaze_grcn77.GazePredictionGRCN.__doc__
    c = gaze_rnn77.CONSTANTS
    assert (c.image_width, c.image_height, c.gazemap_width, c.gazemap_height) == (98, 98, 7, 7)
    assert (c.saliencymap_width, c.saliencymap_height) == (49, 49)
    cfg = gaze_rnn77.GRUModelConfig()
    assert (cfg.n_lstm_steps, cfg.batch_size, cfg.loss_type, cfg.optimization_method) == (35, 7, 'l2', 'adam')
    assert (cfg.dim_feature, cfg.dim_sal, cfg.dim_sal_proj) == (1024, 1024 * 49, 1024)
    assert issubclass(gaze_rnn77.GazePredictionGRU, gaze_rnn.GazePredictionGRU)
    assert gaze_rnn.CONSTANTS.gazemap_height == 49                         # the parent's stay as they are


def test_engine_tables_and_abi_constants():
    from recurrent_gaze_prediction_amd import _lib, engine
    assert tuple(engine.GRCN77_PARAM_TO_FIELD) == ref.KEYS
    assert tuple(engine.GRCN77_PARAM_TO_FIELD.values()) == _lib.Grcn77Weights.FIELDS
    assert (_lib.RGP_GRCN77_SAVE_FOR_BACKWARD, _lib.RGP_GRCN77_PER_STEP) == (_lib.RGP_GRCN_SAVE_FOR_BACKWARD, _lib.RGP_GRCN_PER_STEP)
    assert 'rgp_grcn77_inject_fault' not in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.rgp_version() >= 102


def test_synthetic_dataset_hands_out_7x7_maps():
    ds = syn.SyntheticDataSet(4, 3, seed=2, gazemap_hw=7)
    images, maps, fix, c3d, _, _ = ds.next_batch(2)
    assert maps.shape == (2, 3, 7, 7) and fix.shape == (2, 3, 7, 7) and c3d.shape == (2, 3, 512, 2, 7, 7)
    assert (maps.reshape(6, -1).sum(-1) > 0).all() and (fix.reshape(6, -1).sum(-1) >= 1).all()
    assert syn.SyntheticDataSet(4, 3, seed=2).next_batch(2)[1].shape == (2, 3, 49, 49)
