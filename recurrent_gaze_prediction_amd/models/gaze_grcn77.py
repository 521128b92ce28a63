"""Mirror of /root/reference/models/gaze_grcn77.py: the ConvGRU gaze model that predicts 7x7 maps, executed by the HIP
path (rgp_grcn77_*): gaze_grcn's projection and GRU_RCN_Cell, then a per-pixel 128 -> 1 read-out on the state."""
from types import SimpleNamespace

import numpy as np

from .. import synthetic
from ..engine import GRCN77_PARAM_TO_FIELD, Grcn77Engine
from .gaze_grcn import GRU_RCN_Cell  # noqa: F401  (gaze_grcn77.py:46)
from .gaze_rnn import GazePredictionGRU, GRUModelConfig  # noqa: F401  (re-exported, gaze_grcn77.py:35)

CONSTANTS = SimpleNamespace(image_width=98, image_height=98, gazemap_width=7, gazemap_height=7)     # gaze_grcn77.py:39-43


class GazePredictionGRCN(GazePredictionGRU):
    """gaze_grcn77.py:52-218.  Maps, labels, the softmax and the loss are over 7 x 7 = 49 pixels (create_loss_and_summary
    takes its sizes from the tensors).  No batch-norm, no up-sampling.

    Dropout: both tf.nn.dropout sites of the reference graph (:160-161 on the projected features, :209 on the logits) are
    inert -- the parent's __init__ builds the graph on placeholder_with_default(1.0), and this class rebinds
    dropout_keep_prob to an orphan placeholder only afterwards (:72-74), so the 0.5 that single_step feeds reaches
    nothing (as in models/gaze_c3d_conv.py).  No dropout is built here."""

    DIM_CNN_PROJ = 512      # gaze_grcn77.py:109
    RNN_STATE_SIZE = 128    # gaze_grcn77.py:114
    STREAMS = True

    def __init__(self, session, data_sets, config=None):
        super(GazePredictionGRCN, self).__init__(session, data_sets, config=config,
                                                 gazemap_height=CONSTANTS.gazemap_height,
                                                 gazemap_width=CONSTANTS.gazemap_width)

    @staticmethod
    def create_gazeprediction_network(frame_images, c3d_input, dropout_keep_prob=1.0, net=None, model=None):
        """gaze_grcn77.py:77-218.  Returns the device engine that evaluates the graph; ``net`` receives the variables.
        frame_images is only shape-checked by the reference.  config.convgru_per_step selects per-timestep launches for
        the recurrence and its BPTT, as in models/gaze_grcn.py."""
        assert model is not None, 'pass the owning model (B, T, dtype, device come from its config)'
        if net is None:
            net = {}
        engine = Grcn77Engine(model.batch_size, model.n_lstm_steps, dtype=getattr(model.config, 'compute_dtype', 'bf16'),
                              save_for_backward=getattr(model.config, 'trainable', True), device=model.session.device,
                              per_step=bool(getattr(model.config, 'convgru_per_step', False)))
        # reference initialisers (gaze_grcn77.py:152-153,183-184; the cell's: gaze_grcn.py:64-81)
        model.variables = synthetic.grcn77_params(getattr(model.config, 'init_seed', 0), gru_std=1e-4)
        engine.set_weights(model.variables)
        net['variables'] = model.variables
        return engine

    def _has_dropout(self):
        return False

    def _recover_from_timeout(self):
        """A persistent ConvGRU launch lost a group member (include/rgp.h): continue on a plan that runs the recurrence
        and its BPTT as per-timestep launches (RGP_GRCN77_PER_STEP).  A new engine object in this process; master
        weights and optimizer slots move over device to device (engine.move_training_state); the caller recomputes the
        poisoned batch."""
        from ..engine import move_training_state
        old = self.engine
        if getattr(old, 'per_step', False):
            return False
        log = __import__('logging').getLogger('rgp')
        log.warning('persistent ConvGRU launch timed out (RGP_ETIMEOUT): switching this model to per-timestep launches')
        new = Grcn77Engine(old.B, old.T, dtype=old.dtype, save_for_backward=old.save_for_backward, device=old.device,
                           per_step=True)
        move_training_state(old, new)
        self.engine = new
        self.config.convgru_per_step = True
        return True

    # ---- variables (TF names without the RCNBottom/ scope), for checkpoints and exported weights ----------
    def state_dict(self):
        return {k: v.detach().cpu().numpy().copy() for k, v in self.engine.weights.items()}

    def load_state_dict(self, state):
        missing = [k for k in GRCN77_PARAM_TO_FIELD if k not in state]
        assert not missing, 'missing variables: %s' % missing
        self.variables = {k: np.asarray(state[k], np.float32) for k in GRCN77_PARAM_TO_FIELD}
        self.engine.set_weights(self.variables)


GazePredictionGRCN77 = GazePredictionGRCN     # the name the module's class goes by next to models/gaze_grcn.py's
