"""Mirror of /root/reference/models/saliency_shallownet.py: SaliencyModel, the pre-training of the ShallowNet on
SALICON whose result the cascade takes as its frozen branch (gaze_rnn.py:412-433, initialize_pretrained_shallownet).

The graph (:74-216) is the ShallowNet plan with its dropout site on relu(fc1) switched on (keep 0.4 when training, :330);
the loss (:246-250) is the Euclidean loss normalised by the map size and the CONFIGURED batch size plus 1e-7 times the
l2 loss of every variable; a training batch mirrors a random half of its samples (:306-311).  On the HIP path the step is
rgp_salicon_batch (a set resident on the device) or an upload (a host set) -> rgp_shallownet_forward ->
rgp_euclid_loss_fwd_bwd -> rgp_shallownet_backward -> rgp_l2_reg -> clip + optimizer."""
import logging
import time
from itertools import chain

import numpy as np
import torch

from .. import synthetic
from ..engine import ShallowNetEngine, clip_step_multi, euclid_loss_fwd_bwd, l2_reg, OPTIMIZERS
from ..evaluation_metrics import AVAILABLE_METRICS, saliency_score
from .base import BaseModelConfig, ModelBase, Session

log = logging.getLogger('rgp')

TRAIN_KEEP_PROB = 0.4       # saliency_shallownet.py:330
L2_REG = 1e-7               # :247


class SaliencyModelConfig(BaseModelConfig):
    """The configuration self_test builds (saliency_shallownet.py:453-462) as defaults, and what the HIP path adds."""

    def __init__(self):
        super(SaliencyModelConfig, self).__init__()
        self.batch_size = 128
        self.use_flip_batch = True
        self.initial_learning_rate = 0.00003
        self.optimization_method = 'adam'
        self.steps_per_evaluation = 7000
        # constants of the reference's graph, and additions (not in the reference)
        self.train_keep_prob = TRAIN_KEEP_PROB
        self.l2_reg = L2_REG
        self.image_hw = 98
        self.compute_dtype = 'bf16'      # MFMA operand dtype; the master weights, the loss and the optimizer are fp32
        self.max_frames = None           # frames one step may hold ([B, T, ...] batches are concatenated); None: batch_size
        self.init_seed = 0
        self.flip_seed = None            # None: derived from init_seed and the rank, recorded in the log / checkpoint


class SaliencyModel(ModelBase):
    """saliency_shallownet.py:34-411."""

    def __init__(self, session, data_sets, config=None):
        self.session = session if session is not None else Session()
        self.data_sets = data_sets
        self.config = config if config is not None else SaliencyModelConfig()
        super(SaliencyModel, self).__init__(self.config)
        self.batch_size = self.config.batch_size
        self.initial_learning_rate = self.config.initial_learning_rate
        self.max_grad_norm = self.config.max_grad_norm
        # the reference flips with numpy's GLOBAL RNG (:309); as in the gaze models each rank owns a seeded stream that
        # rides in the checkpoint (models/base.py)
        from .. import dist as rdist
        rank = rdist.env_world()[0]
        cfg_seed = getattr(self.config, 'flip_seed', None)
        self.flip_seed = int(cfg_seed) if cfg_seed is not None else \
            (int(getattr(self.config, 'init_seed', 0)) * 1000003 + 7919 * rank + 54321) & 0x7fffffff
        self.flip_rng = np.random.RandomState(self.flip_seed)
        log.info('flip-augmentation RNG: rank %d seed %d', rank, self.flip_seed)
        self.loss = self.target_loss = self.reg_loss = None
        self.grad_norm = None
        self.train_forward = True         # what engine.forward gets as `train` in a training step; 'keep': a mask set by
        self.build_model()                # engine.dropout.use() stays (parity tests)
        self.build_train_op()
        self.prepare_data()

    # ------------------------------------------------------------------ graph
    def build_model(self):
        from .gaze_rnn import dropout_seed
        cfg = self.config
        hw = int(getattr(cfg, 'image_hw', 98))
        frames = int(getattr(cfg, 'max_frames', None) or self.batch_size)
        self.engine = ShallowNetEngine(frames, hw, dtype=getattr(cfg, 'compute_dtype', 'bf16'), device=self.session.device,
                                       save_for_backward=getattr(cfg, 'trainable', True), dropout=True)
        self.variables = synthetic.shallownet_params(getattr(cfg, 'init_seed', 0), hw)
        self.engine.set_weights(self.variables)
        self.engine.dropout.configure(getattr(cfg, 'train_keep_prob', TRAIN_KEEP_PROB), seed=dropout_seed(cfg, 0x1b873593))
        self.saliency_output = None        # device tensor [n, 49, 49] of the last forward

    def build_train_op(self):
        if self.config.optimization_method not in OPTIMIZERS:
            raise ValueError('Invalid optimization method!')          # base.py:274

    def prepare_data(self):
        train = getattr(self.data_sets, 'train', None)
        self.n_train_instances = len(train) if train is not None else 0

    def state_dict(self):
        return {k: v.detach().cpu().numpy().copy() for k, v in self.engine.weights.items()}

    def load_state_dict(self, state):
        self.variables = {k: np.asarray(state[k], np.float32) for k in self.variables}
        self.engine.set_weights(self.variables)

    # ------------------------------------------------------------------ execution
    def _device_images(self, images):
        x = images if torch.is_tensor(images) else torch.as_tensor(np.ascontiguousarray(images, np.float32))
        return x.to(self.session.device, torch.float32).contiguous()

    def _batch(self, dataset, train_mode):
        """One batch as device tensors (images [n,H,W,3], maps [n,49,49]): :297-311.  A set resident on the device makes
        it there; a host set is gathered and flipped with numpy and uploaded."""
        flipping = train_mode and self.config.use_flip_batch
        if getattr(dataset, 'on_device', False):
            flip = None
            if flipping:
                flip = np.zeros(self.batch_size, np.uint8)
                flip[self.flip_rng.choice(self.batch_size, self.batch_size // 2, replace=False)] = 1
            return dataset.next_batch_device(self.batch_size, flip)[:2]
        batch_images, batch_maps = dataset.next_batch(self.batch_size)[:2]
        if len(batch_images[0].shape) == 4:            # [B, T, H, W, 3]: every frame on its own (:299-304)
            batch_images, batch_maps = np.concatenate(batch_images), np.concatenate(batch_maps)
        if flipping:
            batch_images, batch_maps = np.array(batch_images), np.array(batch_maps)
            n = len(batch_images)
            indices = self.flip_rng.choice(n, n // 2, replace=False)        # Python-2 integer division in the reference
            batch_images[indices] = batch_images[indices][:, :, ::-1, :]
            batch_maps[indices] = batch_maps[indices][:, :, ::-1]
        return self._device_images(batch_images), self._device_images(batch_maps)

    def train_step(self, images, maps, train_mode=True):
        """The device part of a step on a batch already there -> (target_loss, reg_loss) 1-element device tensors."""
        e = self.engine
        if len(images) > e.max_frames:
            raise ValueError('%d frames in one step: the plan holds %d (config.max_frames)' % (len(images), e.max_frames))
        sal, _ = e.forward(images, train=self.train_forward if train_mode else False)
        self.saliency_output = sal
        target, d_sal = euclid_loss_fwd_bwd(sal, maps.reshape(sal.shape), self.batch_size)
        coeff = float(getattr(self.config, 'l2_reg', L2_REG))
        if not train_mode:
            return target, l2_reg(e.flat_params, None, coeff)
        e.backward(d_sal)
        reg = l2_reg(e.flat_params, e.flat_grads, coeff)          # before the clip: the gradient of the total loss is clipped
        self.grad_norm = clip_step_multi([e], self._global_step, self.current_learning_rate, self.max_grad_norm,
                                         self.config.optimization_method)
        self._global_step += 1
        return target, reg

    def single_step(self, train_mode=True, dataset=None):
        """saliency_shallownet.py:291-366."""
        _start_time = time.time()
        if dataset is None:
            dataset = self.data_sets.train if train_mode else self.data_sets.valid
        images, maps = self._batch(dataset, train_mode)
        target, reg = self.train_step(images, maps, train_mode)
        self.target_loss, self.reg_loss = float(target.item()), float(reg.item())
        self.loss = self.reg_loss + self.target_loss
        if train_mode and not np.isfinite(self.loss):
            raise FloatingPointError('non-finite training loss %r at step %d' % (self.loss, self.current_step))
        step = self.current_step
        dt = time.time() - _start_time
        if (not train_mode) or step % max(1, self.config.steps_per_logprint) == 0:
            epoch = float(step * self.batch_size) / max(1, self.n_train_instances)
            log.info(" [%5s epoch %.1f / step %4d]  batch total-loss: %.5f, target-loss: %.5f (%.3f sec/batch, "
                     "%.3f instances/sec)", 'train' if train_mode else 'val', epoch, step, self.loss, self.target_loss, dt,
                     self.batch_size / dt)
        return step

    def predict(self, images):
        """images [n,H,W,3] float32 in [0,1] (numpy or tensor) -> numpy [n,49,49], dropout off (:389-395)."""
        x = self._device_images(images)
        out = []
        for i in range(0, len(x), self.engine.max_frames):
            out.append(self.engine.forward(x[i:i + self.engine.max_frames].contiguous(), train=False)[0])
        return torch.cat(out).cpu().numpy()

    def generate(self, dataset, max_instances=None):
        """The loop of evaluate (:369-402): len(dataset) // batch_size batches (at most max_instances samples) through the
        network -> {'pred_maps', 'gt_maps', 'fixation_maps'}, per image."""
        n = len(dataset) if max_instances is None else min(len(dataset), max_instances)
        num_steps = n // self.batch_size
        gt_maps, pred_maps, fixation_maps = [], [], []
        for v in range(num_steps):
            if v % 10 == 0:
                log.info('Evaluating step %d ...', v)
            batch_images, batch_maps, batch_fix = dataset.next_batch(self.batch_size)[:3]
            if len(batch_images[0].shape) == 4:
                batch_images, batch_maps = np.concatenate(batch_images), np.concatenate(batch_maps)
                batch_fix = list(chain(*batch_fix))
            pred = self.predict(batch_images).reshape(-1, 49, 49)
            assert len(pred) == len(batch_maps)
            gt_maps.extend(batch_maps)
            pred_maps.extend(pred)
            fixation_maps.extend(batch_fix)
        return {'pred_maps': pred_maps, 'gt_maps': gt_maps, 'fixation_maps': fixation_maps}

    def evaluate(self, dataset, scorer='host', seed=0, max_instances=None):
        """saliency_shallownet.py:369-411 -> {metric: score}.  scorer: 'host' (evaluation_metrics, frame by frame on the
        CPU) or 'device' (evaluation_metrics_gpu: one launch per metric, the fixation maps at their raw scale stay
        sparse and the maps are upsized inside the kernel; draws made on the device from ``seed``)."""
        ret = self.generate(dataset, max_instances)
        pred, gt, fix = ret['pred_maps'], ret['gt_maps'], ret['fixation_maps']
        log.info('Validation on total %d images', len(pred))
        if scorer == 'host':
            score = saliency_score
        elif scorer == 'device':
            from functools import partial
            from .. import evaluation_metrics_gpu as emg
            dev = self.session.device
            pred, gt = (torch.as_tensor(np.asarray(emg.stack_maps(m, name))).to(dev) for m, name in ((pred, 'pred'), (gt, 'gt')))
            score = partial(emg.saliency_score, draws='device', seed=seed)
        else:
            raise ValueError("scorer must be 'host' or 'device', got %r" % (scorer,))
        batch_scores = {}
        for metric in AVAILABLE_METRICS:
            batch_scores[metric] = score(metric, pred, gt, fix)
            log.info('Saliency %s : %f', metric, batch_scores[metric])
        self.report_evaluate_summary(batch_scores)
        return batch_scores

    def generate_and_evaluate(self, dataset, scorer='host', seed=0, max_instances=None):
        """What ModelBase.fit calls every steps_per_evaluation steps (base.py:330-358)."""
        return self.evaluate(dataset, scorer=scorer, seed=seed, max_instances=max_instances)


__all__ = ['SaliencyModelConfig', 'SaliencyModel', 'TRAIN_KEEP_PROB', 'L2_REG']
