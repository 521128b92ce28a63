"""Mirror of /root/reference/models/gaze_c3d_conv.py: GazePredictionConv, the no-recurrence baseline of the gaze family
(gaze_grcn's projection and up-sampling head with the ConvGRU taken out), executed by the HIP path (rgp_c3dconv_*)."""
import numpy as np

from .. import synthetic
from ..engine import C3DCONV_PARAM_TO_FIELD, C3dConvEngine
from .gaze_rnn import CONSTANTS, GazePredictionGRU, GRUModelConfig  # noqa: F401  (re-exported, gaze_c3d_conv.py:35-42)


class GazePredictionConv(GazePredictionGRU):
    """gaze_c3d_conv.py:45-218."""

    DIM_CNN_PROJ = 512      # gaze_c3d_conv.py:96

    def __init__(self, session, data_sets, config=None):
        super(GazePredictionConv, self).__init__(session, data_sets, config=config)

    @staticmethod
    def create_gazeprediction_network(frame_images, c3d_input, dropout_keep_prob=1.0, net=None, model=None):
        """gaze_c3d_conv.py:65-218.  Returns the device engine that evaluates the graph; ``net`` receives the variables.
        frame_images is only shape-checked by the reference.  Both tf.nn.dropout sites (:132-133, :207) are inert there:
        __init__ (:47-61) rebinds dropout_keep_prob to an orphan placeholder after the parent has built the graph on
        placeholder_with_default(1.0), so no dropout is built here and training and inference run the same function.
        config.c3d_conv_path ('fused' / 'staged', default None = the library's choice) selects the inference path."""
        assert model is not None, 'pass the owning model (B, T, dtype, device come from its config)'
        if net is None:
            net = {}
        P = GazePredictionConv.DIM_CNN_PROJ
        engine = C3dConvEngine(model.batch_size, model.n_lstm_steps, P, dtype=getattr(model.config, 'compute_dtype', 'bf16'),
                               save_for_backward=getattr(model.config, 'trainable', True), device=model.session.device,
                               path=getattr(model.config, 'c3d_conv_path', None))
        model.variables = synthetic.c3d_conv_params(getattr(model.config, 'init_seed', 0), P)
        engine.set_weights(model.variables)
        net['variables'] = model.variables
        return engine

    def _has_dropout(self):
        return False

    # ---- variables (TF names without the RGP/ scope), for checkpoints and for loading exported weights ----------
    def state_dict(self):
        return {k: v.detach().cpu().numpy().copy() for k, v in self.engine.weights.items()}

    def load_state_dict(self, state):
        missing = [k for k in C3DCONV_PARAM_TO_FIELD if k not in state]
        assert not missing, 'missing variables: %s' % missing
        self.variables = {k: np.asarray(state[k], np.float32) for k in C3DCONV_PARAM_TO_FIELD}
        self.engine.set_weights(self.variables)
