"""Mirror of the reference's models/action_classification.py: the action classifier on gaze-attended C3D features.

A gaze map weights the 1024x7x7 C3D features as spatial attention and a classifier on the weighted features predicts the
13 Hollywood2 action labels (action_classification.py:210-292).  The graph runs in librgp_hip (engine.ActionEngine,
csrc/rgp_action.hip); this module is the reference's host side: hyper-parameters, the Classifier with its train / predict
/ evaluate loop, the multi-label metrics, and -- in place of create_tfrecords.load_data and the TFRecord files -- a
generator of batches straight from a gaze model's ``generate``.

Quirks kept as the reference writes them: no non-linearity between the three NN layers (use_relu=False); the SVM's labels
stay {0, 1}, so a zero label adds a constant to the hinge sum and no gradient; ``evaluate`` scores ``np.sign(pred)`` (for
sigmoid outputs: all ones) and spells its third key 'average-pecision'."""
import logging

import numpy as np
import torch

from .. import synthetic
from ..engine import ActionEngine, action_learning_rate

log = logging.getLogger('rgp')


class HParams(dict):
    """tf.contrib.training.HParams as far as the reference uses it: attribute access to a dictionary."""
    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name)

    __setattr__ = dict.__setitem__


def create_standard_hparams():
    """action_classification.py:50-71, the reference's values."""
    return HParams(
        feat_dimensions=[1024, 7, 7], label_dimensions=[13], batch_size=10, num_classes=13,
        max_iter=2001, num_epochs=3, frame_width=98, frame_height=98, channels=3,
        gazemap_width=49, gazemap_height=49, saliencymap_width=49, saliencymap_height=49,
        learning_rate=0.002, dataset='h2', use_gazemap=False)


def _binary_ap(y_true, score):
    """sklearn.metrics.average_precision_score on flat binary labels: sum over the distinct score thresholds (descending)
    of (recall_k - recall_{k-1}) precision_k; tied scores enter together."""
    y_true, score = np.asarray(y_true, np.float64).reshape(-1), np.asarray(score, np.float64).reshape(-1)
    order = np.argsort(-score, kind='mergesort')
    y, s = y_true[order], score[order]
    last = np.r_[np.where(np.diff(s))[0], y.size - 1]          # last index of each run of equal scores
    tp = np.cumsum(y)[last]
    precision = tp / (last + 1.0)
    recall = tp / max(tp[-1], 1e-300) if tp[-1] > 0 else np.full_like(tp, np.nan)
    return float(np.sum(np.diff(np.r_[0.0, recall]) * precision))


def evaluate_helper(pred, true, binarize='sign'):
    """Classifier.evaluate (action_classification.py:363-373) in plain numpy, restated from the published definitions:
    'Hamming' = fraction of wrong labels, 'zero-one' = fraction of samples with any wrong label, both on np.sign(pred) as the
    reference does (binarize='round': on np.round(pred), the reference's unused y_pred_class); 'average-pecision' (the
    reference's spelling) = micro average precision over the flattened arrays, on the raw scores."""
    pred, true = np.asarray(pred, np.float64), np.asarray(true, np.float64)
    hard = {'sign': np.sign, 'round': np.round}[binarize](pred)
    wrong = hard != true
    return {'Hamming': float(wrong.mean()), 'zero-one': float(wrong.reshape(len(true), -1).any(axis=1).mean()),
            'average-pecision': _binary_ap(true.reshape(-1), pred.reshape(-1))}


def batches_from_gaze_model(model, dataset, labels, batch_size=10, max_instances=50):
    """Replaces create_tfrecords.load_data + the TFRecord files: runs ``model.generate(dataset, max_instances)`` and yields
    (c3d [B,1024,49], gt_gazemap [B,49,49], pred_gazemap [B,49,49], labels [B,13]) float32 batches over its frames; a ragged
    last batch is dropped.  labels: [frames, 13], or [clips, 13] (repeated over each clip's timesteps)."""
    ret = model.generate(dataset, max_instances)
    c3d = np.asarray(ret['c3d_list'], np.float32).reshape(-1, 1024, 49)
    gt = np.asarray(ret['gt_gazemap_list'], np.float32).reshape(-1, 49, 49)
    pred = np.asarray(ret['pred_gazemap_list'], np.float32).reshape(-1, 49, 49)
    labels = np.asarray(labels, np.float32).reshape(-1, 13)
    if len(labels) != len(c3d):
        assert len(c3d) % len(labels) == 0, 'labels: one row per frame or per clip'
        labels = np.repeat(labels, len(c3d) // len(labels), axis=0)
    for i in range(0, len(c3d) - batch_size + 1, batch_size):
        sl = slice(i, i + batch_size)
        yield c3d[sl], gt[sl], pred[sl], labels[sl]


class Classifier(object):
    """action_classification.py:150-292.  ``build_model('NN' | 'SVM')`` creates the engine and the initial variables;
    ``single_step`` is one optimizer step, ``predict`` the forward, ``fit`` the training loop over an iterable of batches."""

    def __init__(self, hparams, device='cuda:0', dtype='bf16', seed=0, unfused=False):
        self.hparams = hparams
        self.batch_size = int(hparams.batch_size)
        self.num_classes = int(hparams.num_classes)
        self.dim_feature = int(hparams.feat_dimensions[0])
        self.use_gazemap = bool(hparams.use_gazemap)
        self.max_iter = int(hparams.max_iter)
        self.num_epochs = int(hparams.num_epochs)
        self.device, self.dtype, self.seed, self.unfused = torch.device(device), dtype, seed, unfused
        self.global_step = 0
        self.engine = self.model = None
        self.batch_score = {}

    def build_model(self, model):
        if model not in ('NN', 'SVM'):
            raise NotImplementedError(model)                       # (the reference returns NotImplementedError)
        self.model = model
        self.engine = ActionEngine(self.batch_size, self.dim_feature, model, self.use_gazemap, self.dtype, save_for_backward=True,
                                   device=self.device, unfused=self.unfused)
        self.engine.set_weights(synthetic.action_params(self.seed, model, self.use_gazemap, self.dim_feature))
        self.global_step = 0

    @property
    def learning_rate(self):
        if self.model == 'SVM':
            return 0.01
        return action_learning_rate(self.global_step, self.hparams.learning_rate)

    def _dev(self, x):
        return None if x is None else torch.as_tensor(np.asarray(x, np.float32) if not torch.is_tensor(x) else x).to(
            self.device, torch.float32).contiguous()

    def single_step(self, c3d, gazemap, labels):
        """One training step on a batch; returns the loss before the update (float)."""
        loss = self.engine.train_step(self._dev(c3d), self._dev(gazemap) if self.use_gazemap else None, self._dev(labels),
                                      self.global_step, self.learning_rate)
        self.global_step += 1
        return float(loss.item())

    def predict(self, c3d, gazemap=None):
        """-> y_pred [B, 13] device tensor (NN: sigmoid(logits); SVM: the margins)."""
        return self.engine.forward(self._dev(c3d), self._dev(gazemap) if self.use_gazemap else None)[1]

    def get_weights(self):
        return {k: v.cpu().numpy() for k, v in self.engine.get_weights().items()}

    def set_weights(self, params):
        self.engine.set_weights(params)

    def fit(self, batches, gaze='gt', log_every=100):
        """Trains on (c3d, gt_gazemap, pred_gazemap, labels) batches (batches_from_gaze_model) until they run out or max_iter
        steps are done; gaze: which of the two maps is the attention ('gt' as the reference feeds it, or 'pred').
        Returns the losses."""
        losses = []
        for c3d, gt, pred, labels in batches:
            if self.global_step >= self.max_iter:
                break
            losses.append(self.single_step(c3d, gt if gaze == 'gt' else pred, labels))
            if log_every and self.global_step % log_every == 0:
                log.info(' [action %s step %4d] loss %.5f (lr=%.3g)', self.model, self.global_step, losses[-1], self.learning_rate)
        return losses

    def evaluate(self, pred_class, true_class):
        self.batch_score = evaluate_helper(pred_class, true_class)
        return self.batch_score
