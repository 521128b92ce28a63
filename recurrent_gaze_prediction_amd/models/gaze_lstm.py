"""Mirror of /root/reference/models/gaze_lstm.py: LSTM_RCN_Cell and GazePredictionLSTM, the ConvLSTM member of the gaze
family (the recurrent baseline the paper's ConvGRU is compared against), executed by the HIP path (rgp_lstm_*)."""
import numpy as np

from .. import synthetic
from ..engine import LSTM_PARAM_TO_FIELD, LSTM_UNTRAINED, LstmEngine  # noqa: F401
from .gaze_rnn import CONSTANTS, GazePredictionGRU, GRUModelConfig  # noqa: F401  (re-exported, gaze_lstm.py:35-45)


class LSTM_RCN_Cell(object):
    """gaze_lstm.py:48-148: eleven variables (truncated-normal stddev 1e-4) and the geometry of the convolutional LSTM.
    The step, as the reference writes it (:114-131) --

        i = sigmoid(W_xi*x + W_hi*h + W_ci.c)      f = sigmoid(W_xf*x + W_hf*h + W_cf.c)
        new_c = f.c + i.tanh(W_xc*x + W_hi*h)      (:125 reuses W_hi; W_hc is never read)
        o = sigmoid(W_xo*x + W_ho*h + W_co.c)      (:130 the OLD c)
        new_h = tanh(new_c).o

    -- runs in csrc/convlstm_seq.hip.h (one launch for all steps) or in the ``EpiLstm`` epilogue of the per-step GEMM.
    The state is concat([c, h]) (:133): state_size = 2 * num_units."""

    def __init__(self, num_units, dim_feature, spatial_shape=(7, 7), kernel_spatial_shape=(3, 3), seed=0, stddev=1e-4):
        self.spatial_H, self.spatial_W = spatial_shape
        assert self.spatial_H > 0 and self.spatial_W > 0
        assert tuple(spatial_shape) == (7, 7) and tuple(kernel_spatial_shape) == (3, 3), \
            'HIP path is built for the 3x3 cell on 7x7 maps (gaze_lstm.py:261)'
        assert (num_units, dim_feature) == (128, 512), 'HIP path is built for the reference widths (gaze_lstm.py:210,215)'
        self._num_units, self.dim_feature = num_units, dim_feature
        p = synthetic.lstm_params(seed, lstm_std=stddev, peephole_std=stddev)
        self.W_xi, self.W_hi, self.W_ci = p['ConvLSTM_Wxi'], p['ConvLSTM_Wxi_1'], p['ConvLSTM_Wci']
        self.W_xf, self.W_hf, self.W_cf = p['ConvLSTM_Wxf'], p['ConvLSTM_Wxf_1'], p['ConvLSTM_Wcf']
        self.W_xc, self.W_hc = p['ConvLSTM_Wxc'], p['ConvLSTM_Whc']
        self.W_xo, self.W_ho, self.W_co = p['ConvLSTM_Wxo'], p['ConvLSTM_Wxo_1'], p['ConvLSTM_Wco']

    @property
    def input_size(self):
        return self._num_units      # gaze_lstm.py:92, as written

    @property
    def output_size(self):
        return self._num_units

    @property
    def state_size(self):
        return 2 * self._num_units  # LSTM: [c, h]

    def zero_state(self, batch_size, dtype=np.float32):
        return np.zeros([batch_size, self.spatial_H, self.spatial_W, self.state_size], dtype)


class GazePredictionLSTM(GazePredictionGRU):
    """gaze_lstm.py:154-353."""

    DIM_CNN_PROJ = 512      # gaze_lstm.py:210
    RNN_STATE_SIZE = 128    # gaze_lstm.py:215
    STREAMS = True
    STATE_PARTS = 2         # [h | c]

    def __init__(self, session, data_sets, config=None):
        super(GazePredictionLSTM, self).__init__(session, data_sets, config=config)

    @staticmethod
    def create_gazeprediction_network(frame_images, c3d_input, dropout_keep_prob=1.0, net=None, model=None):
        """gaze_lstm.py:178-353.  Returns the device engine that evaluates the graph; ``net`` receives the variables.
        frame_images is only shape-checked by the reference.  Both tf.nn.dropout sites (:246-247, :342) are inert there:
        __init__ (:161-175) builds the graph through the parent on placeholder_with_default(1.0) and rebinds
        self.dropout_keep_prob to an orphan placeholder afterwards, so no dropout is built here.
        config.convlstm_path ('persistent' / 'per_step', default None = the library's choice) selects the recurrence path,
        config.convlstm_bptt_path (the same values; the library's choice is per step) that of the backward-through-time pass."""
        assert model is not None, 'pass the owning model (B, T, dtype, device come from its config)'
        if net is None:
            net = {}
        path = getattr(model.config, 'convlstm_path', None)
        assert path in (None, 'persistent', 'per_step'), path
        bptt_path = getattr(model.config, 'convlstm_bptt_path', None)
        assert bptt_path in (None, 'persistent', 'per_step'), bptt_path
        engine = LstmEngine(model.batch_size, model.n_lstm_steps, dtype=getattr(model.config, 'compute_dtype', 'bf16'),
                            save_for_backward=getattr(model.config, 'trainable', True), device=model.session.device,
                            per_step=path == 'per_step', persistent=path == 'persistent',
                            bptt_persistent=bptt_path == 'persistent')
        model.variables = synthetic.lstm_params(getattr(model.config, 'init_seed', 0), lstm_std=1e-4, peephole_std=1e-4)
        engine.set_weights(model.variables)
        net['variables'] = model.variables
        return engine

    def _has_dropout(self):
        return False

    def _recover_from_timeout(self):
        """A persistent ConvLSTM launch (forward or BPTT) lost a group member (include/rgp.h): continue on a plan that runs
        the recurrence and its BPTT as per-timestep launches (RGP_LSTM_PER_STEP, no RGP_LSTM_BPTT_PERSISTENT).  A new engine
        object in this process; master weights and optimizer slots move over device to device (engine.move_training_state);
        the caller recomputes the poisoned batch."""
        from ..engine import move_training_state
        old = self.engine
        if getattr(old, 'per_step', False) and not getattr(old, 'bptt_persistent', False):
            return False
        log = __import__('logging').getLogger('rgp')
        log.warning('persistent ConvLSTM launch timed out (RGP_ETIMEOUT): switching this model to per-timestep launches')
        new = LstmEngine(old.B, old.T, dtype=old.dtype, save_for_backward=old.save_for_backward, device=old.device, per_step=True,
                         bptt_persistent=False)
        move_training_state(old, new)
        self.engine = new
        self.config.convlstm_path = 'per_step'
        self.config.convlstm_bptt_path = 'per_step'
        return True

    # ---- variables (TF names without the RGP/ and RCNBottom/ scopes), for checkpoints and exported weights ----------
    def state_dict(self):
        return {k: v.detach().cpu().numpy().copy() for k, v in self.engine.weights.items()}

    def load_state_dict(self, state):
        missing = [k for k in LSTM_PARAM_TO_FIELD if k not in state]
        assert not missing, 'missing variables: %s' % missing
        self.variables = {k: np.asarray(state[k], np.float32) for k in LSTM_PARAM_TO_FIELD}
        self.engine.set_weights(self.variables)
