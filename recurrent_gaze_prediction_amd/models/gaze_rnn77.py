"""Mirror of /root/reference/models/gaze_rnn77.py: the fc-GRU of gaze_rnn predicting 7x7 maps.  Configuration only: the
graph and the HIP path (rgp_fcgru_*) are the parent's."""
from types import SimpleNamespace

from .gaze_rnn import GazePredictionGRU as GazePredictionGRU4949
from .gaze_rnn import GRUModelConfig as _GRUModelConfig4949

CONSTANTS = SimpleNamespace(image_width=98, image_height=98, gazemap_width=7, gazemap_height=7,
                            saliencymap_width=49, saliencymap_height=49)        # gaze_rnn77.py:35-41


class GRUModelConfig(_GRUModelConfig4949):
    """gaze_rnn77.py:45-60: 35 steps, batch 7, l2 loss (the other fields are the parent's)."""

    def __init__(self):
        super(GRUModelConfig, self).__init__()
        self.n_lstm_steps = 35
        self.batch_size = 7
        self.loss_type = 'l2'


class GazePredictionGRU(GazePredictionGRU4949):
    """gaze_rnn77.py:65-101.

    Quirk of the reference: as written the class cannot run.  It sets gazemap_height / _width to 7 only after the
    parent's __init__ has built the graph, and the inherited create_gazeprediction_network reads gaze_rnn's own CONSTANTS
    (49 x 49) for the read-out, against a ground-truth placeholder the file means to be 7 x 7.  What is implemented here
    is the evident intent: the parent's graph with a 7 x 7 read-out, proj_out_W [1617, 49], proj_out_b [49]."""

    def __init__(self, session, data_sets, config=None):
        super(GazePredictionGRU, self).__init__(session, data_sets, config=config if config is not None else GRUModelConfig(),
                                                gazemap_height=CONSTANTS.gazemap_height,
                                                gazemap_width=CONSTANTS.gazemap_width)
