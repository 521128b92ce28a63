"""Device-side engines: thin owners of a librgp_hip plan + its workspace.

PyTorch is plumbing only here (device memory, streams); all arithmetic happens in
the HIP kernels behind the C ABI (include/rgp.h).  These classes play the role of
the reference's ``tf.Session`` + graph for the gaze path (models/gaze_rnn.py:523-531).

Layout: every engine class stands on _PlanEngine, the plan owner (library, device, the family's resolved entry points
``_f``, handle, workspace, destroy; the flat fp32 master buffer with its per-variable views, the lazily created gradient
buffer, the weights struct, adam_step).  What only some families' C ABI has lives in one mixin each, and a class lists
exactly those its family exports (tests/test_engine_tables_cpu.py holds the classes to _lib.SIGNATURES): _Buffers
(buffer_elems), _Streaming (state_elems, forward_stream), _Persistent (status, persistent_workgroups), _BpttPersistent,
_FaultHook (inject_fault), _StreamBackward (backward_stream).  The models probe engines with hasattr / getattr, so a
member an ABI lacks must stay absent.  DESIGN.md section 37.
"""
import ctypes

import numpy as np
import torch

from . import _lib

GRCN_PARAM_TO_FIELD = {   # reference TF variable name -> rgp_grcn_weights field
    'proj_c3d_W': 'proj_c3d_W', 'proj_c3d_b': 'proj_c3d_b',
    'GRU_Conv_Wz': 'gru_Wz', 'GRU_Conv_Uz': 'gru_Uz', 'GRU_Conv_Wr': 'gru_Wr', 'GRU_Conv_Ur': 'gru_Ur',
    'GRU_Conv_W': 'gru_W', 'GRU_Conv_U': 'gru_U', 'bn_gamma': 'bn_gamma', 'bn_beta': 'bn_beta',
    'weight1': 'up_weight1', 'weight2': 'up_weight2', 'weight3': 'up_weight3', 'out_W': 'out_W', 'out_b': 'out_b',
}
C3D_LAYER_NAMES = ('conv1a', 'conv2a', 'conv3a', 'conv3b', 'conv4a', 'conv4b', 'conv5a', 'conv5b')
C3D_EXTENTS = ((16, 112), (16, 56), (8, 28), (8, 28), (4, 14), (4, 14), (2, 7), (2, 7))     # conv output D, H (= W)
C3D_CHANNELS = ((3, 64), (64, 128), (128, 256), (256, 256), (256, 512), (512, 512), (512, 512), (512, 512))


def _stream_ptr(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _require_gpu(device):
    if not torch.cuda.is_available():
        raise _lib.RgpError('no HIP device visible: the gaze path runs only on the GPU (no CPU fallback)')
    return torch.device(device)


def _as_dev_f32(x, device):
    t = torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x)
    return t.to(device=device, dtype=torch.float32).contiguous()


OPTIMIZERS = ('adam', 'rmsprop', 'sgd')      # create_train_op (base.py:268-273)


def _opt_slots(e, method):
    """Optimizer slot buffers of one engine, created on first use with TF's initial values."""
    if method == 'adam':
        if getattr(e, 'adam_m', None) is None:
            e.adam_m, e.adam_v = torch.zeros_like(e.flat_params), torch.zeros_like(e.flat_params)
    elif method == 'rmsprop':
        if getattr(e, 'rms_ms', None) is None:       # RMSPropOptimizer: rms slot starts at ones, momentum at zeros
            e.rms_ms, e.rms_mom = torch.ones_like(e.flat_params), torch.zeros_like(e.flat_params)
    elif method == 'sgd':
        if getattr(e, 'mom_accum', None) is None:
            e.mom_accum = torch.zeros_like(e.flat_params)
    else:
        raise ValueError('Invalid optimization method!')          # base.py:274


OPT_STATE_KEYS = ('adam_m', 'adam_v', 'rms_ms', 'rms_mom', 'mom_accum')


def optimizer_state(engine):
    """{slot name: cpu tensor} of the slots that exist (what tf.train.Saver(tf.all_variables()) also saves,
    base.py:236-251: a resumed run must not restart Adam's moments at zero)."""
    return {k: getattr(engine, k).detach().cpu().clone() for k in OPT_STATE_KEYS if getattr(engine, k, None) is not None}


def load_optimizer_state(engine, state):
    for k, v in (state or {}).items():
        if k in OPT_STATE_KEYS:
            setattr(engine, k, torch.as_tensor(v).to(engine.device, torch.float32).contiguous().clone())


def move_training_state(old, new):
    """What a model's fallback engine takes over from the one it replaces (the models' _recover_from_timeout): the master
    weights, the optimizer slots that exist and, where both engines have a dropout site, the site's key AND its draw
    counter: the mask sequence goes on where it was (the recomputed batch draws the mask after the one the poisoned forward
    used), it does not start again from the seed."""
    new.set_weights(old.weights)
    for k in OPT_STATE_KEYS:
        if getattr(old, k, None) is not None:
            setattr(new, k, getattr(old, k).clone())
    if getattr(old, 'dropout', None) is not None and getattr(new, 'dropout', None) is not None:
        new.dropout.configure(old.dropout.keep_prob, seed=old.dropout.seed)
        new.dropout.draws = old.dropout.draws


def clip_step_multi(engines, step, lr, max_grad_norm=10.0, method='adam', beta1=0.9, beta2=0.999, eps=1e-8,
                    momentum=0.9, rms_decay=0.9, rms_eps=1e-10):
    """tf.clip_by_global_norm over the gradients of ALL engines (base.py:286-292) + the chosen optimizer
    (base.py:268-273; TF defaults) on each engine's flat buffers, then repack.
    engines: objects with flat_params / flat_grads.  Returns a 1-element device tensor with the pre-clip norm."""
    lib, dev = engines[0].lib, engines[0].device
    npart = _lib.RGP_SQNORM_PARTIALS
    partials = torch.zeros(npart * len(engines), dtype=torch.float32, device=dev)
    gnorm = torch.zeros(1, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        for i, e in enumerate(engines):
            _lib.check(lib.rgp_global_sqnorm(_ptr(e.flat_grads), e.flat_grads.numel(), _ptr(partials[i * npart:]),
                                             _stream_ptr(dev)))
        for e in engines:
            _opt_slots(e, method)
            n = e.flat_params.numel()
            if method == 'adam':
                _lib.check(lib.rgp_adam_clip_step_ext(_ptr(e.flat_params), _ptr(e.flat_grads), _ptr(e.adam_m), _ptr(e.adam_v),
                                                      n, _ptr(partials), partials.numel(), int(step), float(lr), beta1,
                                                      beta2, eps, float(max_grad_norm), _ptr(gnorm), _stream_ptr(dev)))
            elif method == 'rmsprop':
                _lib.check(lib.rgp_rmsprop_clip_step(_ptr(e.flat_params), _ptr(e.flat_grads), _ptr(e.rms_ms), _ptr(e.rms_mom),
                                                     n, _ptr(partials), partials.numel(), float(lr), rms_decay, momentum,
                                                     rms_eps, float(max_grad_norm), _ptr(gnorm), _stream_ptr(dev)))
            else:
                _lib.check(lib.rgp_momentum_clip_step(_ptr(e.flat_params), _ptr(e.flat_grads), _ptr(e.mom_accum), n,
                                                      _ptr(partials), partials.numel(), float(lr), momentum,
                                                      float(max_grad_norm), _ptr(gnorm), _stream_ptr(dev)))
            e.repack()
    return gnorm


def adam_clip_step_multi(engines, step, lr, max_grad_norm=10.0, beta1=0.9, beta2=0.999, eps=1e-8):
    return clip_step_multi(engines, step, lr, max_grad_norm, 'adam', beta1, beta2, eps)


def l2_loss(maps, labels, frames):
    """sum 0.5 (maps - labels)^2 / frames (gaze_rnn.py:387-389) -> 1-element device tensor."""
    lib = _lib.load()
    assert maps.is_cuda and maps.dtype == torch.float32 and maps.is_contiguous()
    assert labels.is_cuda and labels.dtype == torch.float32 and labels.is_contiguous() and labels.numel() == maps.numel()
    ws = torch.empty(_lib.RGP_SQNORM_PARTIALS, dtype=torch.float32, device=maps.device)
    loss = torch.empty(1, dtype=torch.float32, device=maps.device)
    with torch.cuda.device(maps.device):
        _lib.check(lib.rgp_l2_loss_fwd(_ptr(maps), _ptr(labels), maps.numel(), int(frames), _ptr(ws), _ptr(loss),
                                       _stream_ptr(maps.device)))
    return loss


def euclid_loss_fwd_bwd(maps, labels, batch_size, d_maps=None):
    """Target loss of saliency_shallownet.py:248-249 and its gradient in one pass (rgp_euclid_loss_fwd_bwd):
    2 l2_loss(maps - labels) / 2401 / batch_size with the CONFIGURED batch size, whatever the number of frames.
    -> (1-element device tensor, d_maps shaped like maps)."""
    lib = _lib.load()
    assert maps.is_cuda and maps.dtype == torch.float32 and maps.is_contiguous()
    assert labels.is_cuda and labels.dtype == torch.float32 and labels.is_contiguous() and labels.numel() == maps.numel()
    if d_maps is None:
        d_maps = torch.empty_like(maps)
    assert d_maps.is_cuda and d_maps.dtype == torch.float32 and d_maps.is_contiguous() and d_maps.numel() == maps.numel()
    ws = torch.empty(_lib.RGP_SQNORM_PARTIALS, dtype=torch.float32, device=maps.device)
    loss = torch.empty(1, dtype=torch.float32, device=maps.device)
    scale = 2.0 / (2401.0 * int(batch_size))
    with torch.cuda.device(maps.device):
        _lib.check(lib.rgp_euclid_loss_fwd_bwd(_ptr(maps), _ptr(labels), maps.numel(), scale, _ptr(ws), _ptr(loss),
                                               _ptr(d_maps), _stream_ptr(maps.device)))
    return loss, d_maps


def l2_reg(params, grads, coeff):
    """coeff * sum of tf.nn.l2_loss over a flat parameter buffer (saliency_shallownet.py:247); grads += coeff * params
    in place (rgp_l2_reg); grads None: the value alone.  -> 1-element device tensor with the regulariser's value."""
    lib = _lib.load()
    for t in (params, grads):
        assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous())
    assert grads is None or params.numel() == grads.numel()
    ws = torch.empty(_lib.RGP_SQNORM_PARTIALS, dtype=torch.float32, device=params.device)
    reg = torch.empty(1, dtype=torch.float32, device=params.device)
    with torch.cuda.device(params.device):
        _lib.check(lib.rgp_l2_reg(_ptr(params), _ptr(grads), params.numel(), float(coeff), _ptr(ws), _ptr(reg),
                                  _stream_ptr(params.device)))
    return reg


class SaliconBatcher(object):
    """Owner of the status word of rgp_salicon_batch for one resident image set: images_u8 [N,H,W,3] and maps_u8
    [N,49,49] uint8 device tensors -> batches gathered, mirrored and scaled by 1 / 255 in one launch."""

    def __init__(self, images_u8, maps_u8):
        self.lib = _lib.load()
        for t in (images_u8, maps_u8):
            assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
        assert images_u8.dim() == 4 and images_u8.shape[3] == 3 and maps_u8.dim() == 3 and len(maps_u8) == len(images_u8)
        self.images_u8, self.maps_u8, self.device = images_u8, maps_u8, images_u8.device
        self.workspace = torch.zeros(self.lib.rgp_salicon_workspace_bytes(), dtype=torch.uint8, device=self.device)

    def batch(self, index, flip=None, check=True):
        """index: [B] int32 device tensor (or anything torch.as_tensor takes); flip: [B] uint8 / bool or None.
        -> (images [B,H,W,3], maps [B,49,49]) fp32 device tensors.  check: wait for the launch and raise if an index
        was refused (RgpError, code RGP_EINVAL); a caller that knows its indices skips the wait."""
        dev = self.device
        index = torch.as_tensor(index).to(dev, torch.int32).contiguous()
        B = index.numel()
        if flip is not None:
            flip = torch.as_tensor(np.asarray(flip).astype(np.uint8) if not torch.is_tensor(flip) else flip)
            flip = flip.to(dev, torch.uint8).contiguous()
            assert flip.numel() == B
        N, H, W = self.images_u8.shape[:3]
        images = torch.empty(B, H, W, 3, dtype=torch.float32, device=dev)
        maps = torch.empty((B,) + tuple(self.maps_u8.shape[1:]), dtype=torch.float32, device=dev)
        a = _lib.SaliconBatchArgs(images_u8=self.images_u8.data_ptr(), maps_u8=self.maps_u8.data_ptr(), n=N, h=H, w=W,
                                  map_h=self.maps_u8.shape[1], map_w=self.maps_u8.shape[2],
                                  index=index.data_ptr() if B else self.workspace.data_ptr(),     # empty tensors have no address
                                  flip=flip.data_ptr() if flip is not None and B else None, batch=B,
                                  images=images.data_ptr() if B else self.workspace.data_ptr(),
                                  maps=maps.data_ptr() if B else self.workspace.data_ptr(),
                                  workspace=self.workspace.data_ptr(), workspace_bytes=self.workspace.numel())
        with torch.cuda.device(dev):
            _lib.check(self.lib.rgp_salicon_batch(ctypes.byref(a), _stream_ptr(dev)))
            if check and B:
                self.status()
        return images, maps

    def status(self):
        """Waits for the stream; raises RgpError if the last batch refused a sample, returns 0 otherwise."""
        refused = ctypes.c_int(0)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.rgp_salicon_status(_ptr(self.workspace), ctypes.byref(refused), _stream_ptr(self.device)))
        return refused.value


class DropoutSite(object):
    """Keep-mask owner of one tf.nn.dropout site: draws a fresh Philox mask per training step on the device
    (rgp_dropout_mask), or takes the caller's bytes (parity tests feed the oracle the same mask)."""

    def __init__(self, lib, device, n_elems, setter):
        self.lib, self.device, self.n, self._set = lib, device, int(n_elems), setter
        self.mask = torch.ones(self.n, dtype=torch.uint8, device=device)
        self.keep_prob, self.seed, self.draws = 1.0, 0, 0

    def configure(self, keep_prob, seed=0):
        self.keep_prob, self.seed, self.draws = float(keep_prob), int(seed), 0

    def off(self):
        _lib.check(self._set(ctypes.c_float(1.0), None))

    def arm(self, train):
        """The site for one forward: True = draw a fresh mask (if configured), 'keep' = leave the mask use() installed as it
        is, False = site off."""
        if train == 'keep':
            return
        self.draw() if train else self.off()

    def draw(self):
        """New mask for this step (counter offset advances by ceil(n/4) blocks per draw)."""
        if self.keep_prob >= 1.0:
            return self.off()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.rgp_dropout_mask(_ptr(self.mask), self.n, self.keep_prob, self.seed,
                                                 self.draws * ((self.n + 3) // 4), _stream_ptr(self.device)))
        self.draws += 1
        _lib.check(self._set(ctypes.c_float(self.keep_prob), _ptr(self.mask)))

    def use(self, mask, keep_prob):
        """Fixed mask (uint8 / bool array of n elements, reference order)."""
        m = torch.as_tensor(np.asarray(mask).astype(np.uint8) if not torch.is_tensor(mask) else mask)
        assert m.numel() == self.n, (m.numel(), self.n)
        self.mask.copy_(m.reshape(-1).to(self.device, torch.uint8))
        self.keep_prob = float(keep_prob)
        _lib.check(self._set(ctypes.c_float(self.keep_prob), _ptr(self.mask)))


def _flat_layout(names, shapes, untrained=()):
    """[(name, offset, numel)] of a flat fp32 buffer holding `names` in order, those in `untrained` left out."""
    out, off = [], 0
    for k in names:
        if k in untrained:
            continue
        n = int(np.prod(shapes[k]))
        out.append((k, off, n))
        off += n
    return out


def _flat_views(names, like, device, untrained=()):
    """One flat fp32 buffer + per-variable views (one all-reduce bucket, one optimizer launch).  like: {name: tensor of
    the variable's shape}.  Variables in `untrained` get zeros of their own OUTSIDE the flat buffer.
    Returns (flat, {name: view} in the order of names)."""
    shapes = {k: tuple(like[k].shape) for k in names}
    layout = _flat_layout(names, shapes, untrained)
    flat = torch.zeros(sum(n for _, _, n in layout), dtype=torch.float32, device=device)
    views = {k: flat[off:off + n].view(shapes[k]) for k, off, n in layout}
    for k in untrained:
        views[k] = torch.zeros(shapes[k], dtype=torch.float32, device=device)
    return flat, {k: views[k] for k in names}


def _struct(struct_cls, fields, views):
    """struct_cls with the device pointers of views; fields: {name in views: field of the struct}."""
    st = struct_cls()
    for k, f in fields.items():
        setattr(st, f, views[k].data_ptr())
    return st


class _PlanEngine(object):
    """The plan owner under every engine class: one rgp_<family>_ plan, its workspace, and the flat fp32 master buffers.

    A subclass names PREFIX (the family's C prefix), CREATE (its create entry behind the prefix), WEIGHTS (the struct of
    set_weights / backward), PARAM_TO_FIELD ({variable name: field of WEIGHTS} in the flat buffer's order; None = every
    field of WEIGHTS under its own name) and UNTRAINED (variables kept out of the flat buffers), and calls _create_plan()
    from its __init__.  Hooks for what is a family's own: _param_fields, _check_shapes, _struct_of."""
    PREFIX = WEIGHTS = PARAM_TO_FIELD = None
    CREATE = 'create'
    UNTRAINED = ()

    def _create_plan(self, device, *create_args):
        """create_args: the arguments of the create entry behind the plan pointer."""
        self.lib = _lib.load()
        self.device = _require_gpu(device)
        self.flat_params = self.flat_grads = self.grads = self.weights = self.adam_m = self.adam_v = None
        self._fields = self._param_fields()
        # the family's entry points by their name behind the prefix (resolved once: the training step is host-bound)
        self._f = {k[len(self.PREFIX):]: getattr(self.lib, k) for k in _lib.SIGNATURES if k.startswith(self.PREFIX)}
        self._h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self._f[self.CREATE](ctypes.byref(self._h), *create_args))
            nbytes = self._f['workspace_bytes'](self._h)
            self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            _lib.check(self._f['bind_workspace'](self._h, _ptr(self.workspace), nbytes, _stream_ptr(self.device)))

    def __del__(self):
        h, self._h = getattr(self, '_h', None), None
        if h:
            self._f['destroy'](h)

    def _call(self, entry, *args):
        """rgp_<family>_<entry>(plan, *args, stream) on the current stream of the plan's device, checked."""
        with torch.cuda.device(self.device):
            _lib.check(self._f[entry](self._h, *(args + (_stream_ptr(self.device),))))

    def _forward(self, entry, n_valid, *args):
        """_call for the forward entries.  The one place that notes how many steps the last forward of this object defined
        (backward_stream's default divisor)."""
        self._call(entry, *args)
        self._last_n_valid = n_valid

    def _dropout_site(self, n_elems):
        """The tf.nn.dropout site of a plan with a set_dropout entry; off until a training step draws a mask."""
        return DropoutSite(self.lib, self.device, n_elems, lambda keep, mask: self._f['set_dropout'](self._h, keep, mask))

    def _param_fields(self):
        """Hook: {variable name: field of WEIGHTS} of THIS plan, in the order of the flat buffers."""
        return self.PARAM_TO_FIELD or {k: k for k in self.WEIGHTS.FIELDS}

    def _check_shapes(self, src):
        """Hook: assert what the plan's geometry fixes about the parameters' shapes."""

    def _struct_of(self, views):
        """Hook: WEIGHTS with the device pointers of views (the master weights or the gradients)."""
        return _struct(self.WEIGHTS, self._fields, views)

    def _copy_in(self, values):
        """{variable: array/tensor} -> the flat fp32 master buffer (created on the first call) through its views."""
        src = {k: _as_dev_f32(values[k], self.device) for k in self._fields}
        self._check_shapes(src)
        if self.weights is None:
            self.flat_params, self.weights = _flat_views(self._fields, src, self.device, self.UNTRAINED)
        for k in self._fields:
            self.weights[k].copy_(src[k])

    def set_weights(self, params):
        """params: dict keyed by the variables' names (the reference's TF names, scope stripped) -> array/tensor (fp32).
        The values are copied into the engine's flat fp32 master buffer, then packed / folded (repack)."""
        self._copy_in(params)
        self.repack()

    def repack(self):
        """Re-pack the master weights into MFMA operand form (after set_weights / an optimizer step)."""
        st = self._struct_of(self.weights)      # the plan keeps raw pointers to biases / BN: views stay alive
        self._call('set_weights', ctypes.byref(st))

    def _grad_struct(self):
        """WEIGHTS over the gradient views; flat_grads / grads are created by the first backward and reused."""
        if self.grads is None:
            self.flat_grads, self.grads = _flat_views(self._fields, self.weights, self.device, self.UNTRAINED)
        return self._struct_of(self.grads)

    def adam_step(self, step, lr, max_grad_norm=10.0, method='adam'):
        """clip_by_global_norm + the chosen optimizer of base.py:268-273 on the flat buffers (the trained variables
        only), then repack."""
        return clip_step_multi([self], step, lr, max_grad_norm, method)


class _Buffers(object):
    """rgp_<family>_buffer_elems / _read_buffer: the intermediates of a plan by name, flat fp32."""

    def read_buffer_elems(self, name):
        """fp32 elements read_buffer(name) returns; 0 = this plan has no such intermediate."""
        return int(self._f['buffer_elems'](self._h, name.encode()))

    def read_buffer(self, name):
        n = self.read_buffer_elems(name)
        if n == 0:
            raise _lib.RgpError('unknown intermediate %r' % name)
        out = torch.empty(n, dtype=torch.float32, device=self.device)
        self._call('read_buffer', name.encode(), _ptr(out))
        return out


class _Streaming(object):
    """rgp_<family>_state_elems / _forward_stream: a recurrent state carried across calls."""
    STREAM_BN_PHASE = False     # the family's forward_stream takes a batch-norm phase (gaze_grcn: one BN layer per timestep)

    @property
    def state_elems(self):
        """fp32 elements of the recurrent state forward_stream carries (rgp_<family>_state_elems; the fc-GRU: B * 1617, h per
        clip; the cascade: per clip the bottom state 49*256, then the top state 49*49*3, each part [B, ...])."""
        return int(self._f['state_elems'](self._h))

    def _stream_call(self, B, T, c3d_input, state, n_valid, args, rows=None):
        """What the forward_stream methods share: c3d_input (or rows, as forward_rows takes them) and state are checked,
        n_valid defaults to T, new_state is allocated and rgp_<family>_forward_stream(plan, *args(state, new_state,
        n_valid), stream) is called and checked.  Returns new_state."""
        x = c3d_input
        if x is not None:
            assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
            assert tuple(x.shape) == (B, T, 1024, 7, 7), tuple(x.shape)
        if rows is not None:
            assert rows.is_cuda and rows.dtype == self.torch_dtype and rows.is_contiguous()
            assert rows.numel() == B * T * 49 * 1024
        n_valid = T if n_valid is None else int(n_valid)
        if state is not None:
            assert state.is_cuda and state.dtype == torch.float32 and state.is_contiguous()
            assert state.numel() == self.state_elems, (state.numel(), self.state_elems)
        new_state = torch.empty(self.state_elems, dtype=torch.float32, device=self.device)
        self._forward('forward_stream', n_valid, *args(_ptr(state), _ptr(new_state), n_valid))
        return new_state


class _Persistent(_Streaming):
    """... and rgp_<family>_status / _persistent_workgroups: a recurrence that may run as one persistent launch (gaze_grcn,
    gaze_grcn77, gaze_lstm, the fc-GRU; gaze_c3d_conv has none, and the models ask an engine for `status` / `persistent` with
    getattr)."""

    def status(self):
        """Wait for the current stream and raise RgpError (RGP_ETIMEOUT) if a persistent launch of this plan lost a
        group member since the last check (its outputs are NaN)."""
        self._call('status')

    @property
    def persistent_workgroups(self):
        """CUs a persistent sequence launch of this plan occupies (0: the recurrence runs as per-timestep launches)."""
        with torch.cuda.device(self.device):
            return int(self._f['persistent_workgroups'](self._h))

    @property
    def persistent(self):
        return self.persistent_workgroups > 0


class _BpttPersistent(object):
    """rgp_<family>_bptt_persistent_workgroups (gaze_lstm, the fc-GRU)."""

    @property
    def bptt_persistent_workgroups(self):
        """CUs the persistent BPTT launch of this plan's backward occupies (0: per-timestep launches)."""
        with torch.cuda.device(self.device):
            return int(self._f['bptt_persistent_workgroups'](self._h))

    @property
    def bptt_persistent(self):
        return self.bptt_persistent_workgroups > 0


class _FaultHook(object):
    """rgp_<family>_inject_fault (gaze_grcn, gaze_lstm)."""

    def inject_fault(self, kind='seq'):
        """Test hook (rgp_<family>_inject_fault): the next persistent launch of the forward ('seq') or of the BPTT
        ('bptt') loses a group member."""
        with torch.cuda.device(self.device):
            _lib.check(self._f['inject_fault'](self._h, {'seq': _lib.RGP_FAULT_SEQ_LOST_MEMBER,
                                                         'bptt': _lib.RGP_FAULT_BPTT_LOST_MEMBER}[kind]))


class _StreamBackward(object):
    """rgp_<family>_backward_stream (gaze_grcn, the fc-GRU): training across the carried state.  A class says what shape its
    d_state_in has (_state_shape)."""

    def backward_stream(self, logits, probs, labels, d_state=None, loss_frames=None, loss_type='xentropy', want_d_state=True):
        """The backward of the last forward of either kind (rgp_<family>_backward_stream): behind forward_stream(state,
        n_valid[, bn_phase]) the first n_valid steps of that call, the recurrence started at `state` (gaze_grcn: step t
        through batch-norm slot (bn_phase + t) % T); behind forward() / forward_rows() all T steps from the zero state.
        The loss is backward()'s, summed over the valid frames and divided by loss_frames (default B * n_valid of the last
        forward THIS OBJECT ran: a Python-side copy of what the plan keeps, used for this default alone; name loss_frames
        when the C entries are driven beside the engine), so the gradients of a film's chunks add up to the gradient of the
        mean over the film.  d_state: fp32, state_elems elements (gaze_grcn [B, 7, 7, S], the fc-GRU [B, 1617]), the gradient
        w.r.t. the new_state the forward returned, or None = zeros (truncated BPTT, the last chunk); never modified.
        The inputs of the forward must be finite over all T steps.
        Returns (grads, d_state_in): {variable: gradient view} (flat_grads, written, not accumulated) and a fresh tensor
        shaped like the state with d loss / d state (None with want_d_state=False)."""
        assert self.save_for_backward, 'create the engine with save_for_backward=True'
        assert labels.is_cuda and labels.dtype == torch.float32 and labels.is_contiguous()
        if d_state is not None:
            assert d_state.is_cuda and d_state.dtype == torch.float32 and d_state.is_contiguous()
            assert d_state.numel() == self.state_elems, (d_state.numel(), self.state_elems)
        if loss_frames is None:
            loss_frames = self.B * getattr(self, '_last_n_valid', self.T)
        st = self._grad_struct()
        d_in = torch.empty(self._state_shape(), dtype=torch.float32, device=self.device) if want_d_state else None
        self._call('backward_stream', _ptr(logits), _ptr(probs), _ptr(labels), _ptr(d_state), _ptr(d_in), int(loss_frames),
                   ctypes.byref(st), {'xentropy': 0, 'l2': 1}[loss_type])
        return self.grads, d_in


class _GazeEngine(_Buffers, _PlanEngine):
    """What the gaze-family engines on conv5b rows share (gaze_grcn, gaze_c3d_conv, gaze_lstm, gaze_grcn77): plans at fixed
    (B, T, dtype), forward from features or rows, the reference loss's backward."""

    def _create(self, batch, n_steps, dtype, save_for_backward, device, *create_args):
        """Common part of __init__; create_args: the arguments of rgp_<family>_create behind the plan pointer."""
        self.B, self.T = int(batch), int(n_steps)
        self.dtype = dtype
        self.save_for_backward = bool(save_for_backward)
        self.torch_dtype = torch.bfloat16 if _lib.DTYPES[dtype] == _lib.RGP_BF16 else torch.float32
        self._create_plan(device, *create_args)

    def backward(self, logits, probs, labels, loss_type='xentropy'):
        """Gradients of the reference loss (gaze_rnn.py:363-408) w.r.t. every variable, after a
        forward() on the same inputs.  labels: normalised gt maps [B,T,49,49] fp32 device tensor.
        Returns {TF variable name: fp32 gradient view}; the flat buffer is self.flat_grads."""
        # (GrcnEngine used to leave this check, and the contiguity of forward_rows' rows, to the library: no caller relied on it)
        assert self.save_for_backward, 'create the engine with save_for_backward=True'
        assert labels.is_cuda and labels.dtype == torch.float32 and labels.is_contiguous()
        st = self._grad_struct()
        self._call('backward', _ptr(logits), _ptr(probs), _ptr(labels), ctypes.byref(st), {'xentropy': 0, 'l2': 1}[loss_type])
        return self.grads

    def grad_buckets(self):
        """[(slice of flat_grads, ready)]: one bucket, complete when backward() returns on the launch stream."""
        return [(self.flat_grads, lambda stream: stream.wait_stream(torch.cuda.current_stream(self.device)))]

    def backward_input(self, out=None):
        """After backward(): d loss / d input as conv5b rows [B*T*49, 1024] fp32 (column d*512+c), the
        gradient C3DEngine.backward(d_rows=...) consumes when the conv stack is fine-tuned."""
        d = out if out is not None else torch.empty(self.B * self.T * 49, 1024, device=self.device)
        self._call('backward_input', _ptr(d))
        return d

    def _outputs(self, want_probs, out_logits, out_probs):
        logits = out_logits if out_logits is not None else torch.empty(self.B, self.T, 49, 49, device=self.device)
        probs = None
        if want_probs:
            probs = out_probs if out_probs is not None else torch.empty_like(logits)
        return logits, probs

    def forward(self, c3d_input, want_probs=True, out_logits=None, out_probs=None):
        """c3d_input [B,T,1024,7,7] fp32 device tensor -> (logits, probs) [B,T,49,49]."""
        x = c3d_input
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
        assert tuple(x.shape) == (self.B, self.T, 1024, 7, 7), tuple(x.shape)
        logits, probs = self._outputs(want_probs, out_logits, out_probs)
        self._forward('forward', self.T, _ptr(x), _ptr(logits), _ptr(probs))
        return logits, probs

    def forward_rows(self, rows, want_probs=True, out_logits=None, out_probs=None):
        """rows: conv5b rows from C3DEngine.forward (operand dtype, [B*T*49, 1024], column d*512+c)."""
        assert rows.is_cuda and rows.dtype == self.torch_dtype and rows.is_contiguous()
        assert rows.numel() == self.B * self.T * 49 * 1024
        logits, probs = self._outputs(want_probs, out_logits, out_probs)
        self._forward('forward_rows', self.T, _ptr(rows), _ptr(logits), _ptr(probs))
        return logits, probs


class _PersistentEngine(_Persistent, _GazeEngine):
    """... with a ConvGRU / ConvLSTM recurrence that streams and may run as a persistent launch (gaze_grcn, gaze_grcn77,
    gaze_lstm)."""

    def forward_stream(self, c3d_input=None, rows=None, state=None, n_valid=None, bn_phase=0, want_probs=True):
        """One call of a stream (rgp_<family>_forward_stream): the graph of forward() / forward_rows() started from
        `state` instead of zeros.  Exactly one of c3d_input [B,T,1024,7,7] fp32 and rows (as forward_rows) is given, always at
        the full plan size; the recurrence is defined for the first n_valid (default T) steps, later outputs are unspecified.
        state: fp32 device tensor of state_elems elements from an earlier call, or None = the zero state; never modified.
        bn_phase: step t uses batch-norm slot (bn_phase + t) % T (gaze_grcn only; the others have no per-timestep BN).
        Returns (logits, probs, new_state); new_state is a fresh tensor on every call: the state behind step n_valid."""
        assert (c3d_input is None) != (rows is None), 'exactly one of c3d_input and rows'
        assert self.STREAM_BN_PHASE or bn_phase == 0, 'this family has no per-timestep batch-norm'
        logits, probs = self._outputs(want_probs, None, None)
        phase = (int(bn_phase),) if self.STREAM_BN_PHASE else ()
        new_state = self._stream_call(self.B, self.T, c3d_input, state, n_valid, lambda si, so, nv: (
            _ptr(c3d_input), _ptr(rows), si, so, nv) + phase + (_ptr(logits), _ptr(probs)), rows=rows)
        return logits, probs, new_state


class GrcnEngine(_StreamBackward, _FaultHook, _PersistentEngine):
    """gaze_grcn graph (models/gaze_grcn.py:173-376) at fixed (B, T, P, S, dtype)."""
    PREFIX, PARAM_TO_FIELD, WEIGHTS = 'rgp_grcn_', GRCN_PARAM_TO_FIELD, _lib.GrcnWeights
    STREAM_BN_PHASE = True

    def __init__(self, batch, n_steps, dim_proj=512, dim_state=128, dtype='bf16', save_for_backward=False,
                 device='cuda:0', per_step=False, unfolded_head=False):
        """per_step=True: the recurrence (and its BPTT) as per-timestep launches even where the persistent
        kernels apply (RGP_GRCN_PER_STEP): the library's second implementation, used for cross-checks.
        unfolded_head=True: an inference plan that runs the three transposed convolutions one by one
        (RGP_GRCN_UNFOLDED_HEAD) instead of their exact fold into one GEMM (csrc/head_fold.hip.h); training plans
        always do."""
        self.P, self.S, self.per_step = int(dim_proj), int(dim_state), bool(per_step)
        flags = (_lib.RGP_GRCN_SAVE_FOR_BACKWARD if save_for_backward else 0) | (_lib.RGP_GRCN_PER_STEP if per_step else 0) | \
            (_lib.RGP_GRCN_UNFOLDED_HEAD if unfolded_head else 0)
        self._create(batch, n_steps, dtype, save_for_backward, device, int(batch), int(n_steps), self.P, self.S,
                     _lib.DTYPES[dtype], flags)

    def _check_shapes(self, src):
        assert tuple(src['bn_gamma'].shape) == (self.T, self.S), 'one batch-norm layer per timestep (SURVEY 9-Q1)'

    # gradient groups in the order the backward finishes them (rgp_grcn_wait_grads); each is one contiguous slice of
    # flat_grads because GRCN_PARAM_TO_FIELD lists the variables in this order
    GRAD_GROUPS = ((_lib.RGP_GRCN_GRADS_TOP, 'bn_gamma', 'out_b'),
                   (_lib.RGP_GRCN_GRADS_GRU, 'GRU_Conv_Wz', 'GRU_Conv_U'),
                   (_lib.RGP_GRCN_GRADS_PROJ, 'proj_c3d_W', 'proj_c3d_b'))

    def grad_buckets(self):
        """[(slice of flat_grads, ready)] in completion order: `ready(stream)` makes a torch.cuda.Stream wait until the
        last backward() has finished that slice (data-parallel training: the all-reduce of the upsampling / output
        gradients runs under the BPTT, that of the ConvGRU filters under the projection's filter gradient)."""
        names = list(GRCN_PARAM_TO_FIELD)
        offs, off = {}, 0
        for k in names:
            offs[k] = (off, off + self.grads[k].numel())
            off += self.grads[k].numel()
        out = []
        for group, first, last in self.GRAD_GROUPS:
            assert names.index(first) <= names.index(last)
            lo, hi = offs[first][0], offs[last][1]
            out.append((self.flat_grads[lo:hi],
                        lambda stream, group=group: _lib.check(self.lib.rgp_grcn_wait_grads(
                            self._h, group, ctypes.c_void_p(stream.cuda_stream)))))
        assert sum(b.numel() for b, _ in out) == self.flat_grads.numel()
        return out

    def adam_step(self, step, lr, max_grad_norm=10.0, beta1=0.9, beta2=0.999, eps=1e-8, method='adam'):
        """clip_by_global_norm + TF AdamOptimizer on the flat buffers (base.py:286-297), then repack.
        Returns a 1-element device tensor holding the pre-clip global gradient norm.
        method 'rmsprop' / 'sgd': the other two optimizers of base.py:268-273."""
        if method != 'adam':
            return clip_step_multi([self], step, lr, max_grad_norm, method)
        if getattr(self, 'adam_m', None) is None or getattr(self, '_opt_ws', None) is None:
            if getattr(self, 'adam_m', None) is None:       # (slots restored from a checkpoint are kept)
                self.adam_m = torch.zeros_like(self.flat_params)
                self.adam_v = torch.zeros_like(self.flat_params)
            self._opt_ws = torch.zeros(256, dtype=torch.float32, device=self.device)
            self._gnorm = torch.zeros(1, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.rgp_adam_clip_step(_ptr(self.flat_params), _ptr(self.flat_grads), _ptr(self.adam_m),
                                                   _ptr(self.adam_v), self.flat_params.numel(), _ptr(self._opt_ws),
                                                   int(step), float(lr), beta1, beta2, eps, float(max_grad_norm),
                                                   _ptr(self._gnorm), _stream_ptr(self.device)))
        self.repack()
        return self._gnorm

    def _state_shape(self):
        return (self.B, 7, 7, self.S)

    @property
    def grads_top_early(self):
        """Whether the first gradient bucket (grad_buckets()[0]) is released before the BPTT launch (include/rgp.h: only
        when that launch leaves RGP_RCCL_CU_RESERVE CUs to the collective) or behind it."""
        with torch.cuda.device(self.device):
            return bool(self.lib.rgp_grcn_grads_top_early(self._h))

    def profile(self, enable=True):
        _lib.check(self.lib.rgp_grcn_profile_enable(self._h, int(enable)))

    def profile_read(self):
        """{stage: (total_ms, launch_groups)} since the last read (HIP events on the launch stream)."""
        n = len(_lib.GRCN_STAGES)
        ms, calls = (ctypes.c_double * n)(), (ctypes.c_longlong * n)()
        _lib.check(self.lib.rgp_grcn_profile_read(self._h, ms, calls))
        return {k: (ms[i], calls[i]) for i, k in enumerate(_lib.GRCN_STAGES)}


C3DCONV_PARAM_TO_FIELD = {   # reference TF variable name (without scope) -> rgp_c3dconv_weights field
    'proj_c3d_W': 'proj_c3d_W', 'proj_c3d_b': 'proj_c3d_b',
    'weight1': 'up_weight1', 'weight2': 'up_weight2', 'weight3': 'up_weight3', 'out_W': 'out_W', 'out_b': 'out_b',
}


class C3dConvEngine(_GazeEngine):
    """gaze_c3d_conv graph (models/gaze_c3d_conv.py:105-218), the no-recurrence baseline, at fixed (B, T, P, dtype).

    path=None: the library's choice (bf16 inference plans: the fused kernel, one launch from rows to softmax; everything
    else the staged path); 'fused' / 'staged' force one (RGP_C3DCONV_FUSED / RGP_C3DCONV_STAGED).  Training plans
    (save_for_backward=True) run the staged path; their backward uses no float atomics (bit-reproducible gradients,
    flat_grads fully overwritten).  repack() folds the master weights into the 1024 -> 384 filter and the bias plane (and
    the staged path's operands).  read_buffer: 'c3d_embedded' [B*T*49, P] (staged plans), 'folded_filter' [384, 1024],
    'bias_plane' [49, 49] as fp32."""
    PREFIX, PARAM_TO_FIELD, WEIGHTS = 'rgp_c3dconv_', C3DCONV_PARAM_TO_FIELD, _lib.C3dConvWeights

    def __init__(self, batch, n_steps, dim_proj=512, dtype='bf16', save_for_backward=False, device='cuda:0', path=None):
        self.P = int(dim_proj)
        flags = {None: 0, 'staged': _lib.RGP_C3DCONV_STAGED, 'fused': _lib.RGP_C3DCONV_FUSED}[path]
        flags |= _lib.RGP_C3DCONV_SAVE_FOR_BACKWARD if save_for_backward else 0
        self._create(batch, n_steps, dtype, save_for_backward, device, int(batch), int(n_steps), self.P, _lib.DTYPES[dtype], flags)
        self.path = self.lib.rgp_c3dconv_path(self._h).decode()

    def _check_shapes(self, src):
        assert tuple(src['proj_c3d_W'].shape) == (1024, self.P) and tuple(src['weight1'].shape) == (5, 5, 64, self.P)


LSTM_PARAM_TO_FIELD = {   # TF variable name under RGP/ and RGP/RCNBottom/ (scope stripped) -> rgp_lstm_weights field.  TF
    # uniquifies the repeated name= of gaze_lstm.py:64-87: the second 'ConvLSTM_Wxi' is W_hi, and so on (unpinned: no TF here)
    'proj_c3d_W': 'proj_c3d_W', 'proj_c3d_b': 'proj_c3d_b',
    'ConvLSTM_Wxi': 'W_xi', 'ConvLSTM_Wxi_1': 'W_hi', 'ConvLSTM_Wci': 'W_ci',
    'ConvLSTM_Wxf': 'W_xf', 'ConvLSTM_Wxf_1': 'W_hf', 'ConvLSTM_Wcf': 'W_cf',
    'ConvLSTM_Wxc': 'W_xc', 'ConvLSTM_Whc': 'W_hc',
    'ConvLSTM_Wxo': 'W_xo', 'ConvLSTM_Wxo_1': 'W_ho', 'ConvLSTM_Wco': 'W_co',
    'weight1': 'up_weight1', 'weight2': 'up_weight2', 'weight3': 'up_weight3', 'out_W': 'out_W', 'out_b': 'out_b',
}
# gaze_lstm.py:80: W_hc is a graph variable with no path to the loss.  tf.gradients gives None for it, and
# clip_by_global_norm / apply_gradients (base.py:278-297) skip None: it is in checkpoints, never in the norm or the update.
LSTM_UNTRAINED = ('ConvLSTM_Whc',)


def lstm_flat_layout(shapes):
    """[(name, offset, numel)] of the flat fp32 buffer the clip norm and the optimizer see: every variable of
    LSTM_PARAM_TO_FIELD in order EXCEPT LSTM_UNTRAINED.  shapes: {name: shape}.  Host logic only."""
    return _flat_layout(LSTM_PARAM_TO_FIELD, shapes, LSTM_UNTRAINED)


class LstmEngine(_BpttPersistent, _FaultHook, _PersistentEngine):
    """gaze_lstm graph (models/gaze_lstm.py:178-353) at fixed (B, T, dtype): projection, ConvLSTM, up-sampling head.

    per_step=True: the recurrence as one launch per timestep (RGP_LSTM_PER_STEP), the library's second implementation;
    otherwise bf16 plans of at most 64 clips run all T steps in one persistent launch (csrc/convlstm_seq.hip.h).
    bptt_persistent=True: the backward-through-time pass of backward() as one persistent launch as well
    (RGP_LSTM_BPTT_PERSISTENT, csrc/convlstm_bptt.hip.h; bf16 training plans of at most 64 clips), whatever the forward runs.
    flat_params / flat_grads hold the 17 trained variables; W_hc (LSTM_UNTRAINED) lives outside them: backward() returns
    zeros for it.  read_buffer: 'h', 'c' (training plans also 'i', 'f', 'g', 'o' and, after a backward, 'd_i', 'd_f', 'd_g',
    'd_o') [B,T,7,7,128]; 'emb' [B*T*49, 512]; fp32."""
    PREFIX, PARAM_TO_FIELD, WEIGHTS, UNTRAINED = 'rgp_lstm_', LSTM_PARAM_TO_FIELD, _lib.LstmWeights, LSTM_UNTRAINED

    def __init__(self, batch, n_steps, dtype='bf16', save_for_backward=False, device='cuda:0', per_step=False, persistent=False,
                 bptt_persistent=False):
        """persistent=True asks for the persistent kernel by name (RGP_LSTM_PERSISTENT: refused for plans it cannot run);
        with both False the library chooses.  bptt_persistent=False is the library's choice for the BPTT (per step)."""
        self.P, self.S, self.per_step = 512, 128, bool(per_step)
        flags = (_lib.RGP_LSTM_SAVE_FOR_BACKWARD if save_for_backward else 0) | (_lib.RGP_LSTM_PER_STEP if per_step else 0) | \
            (_lib.RGP_LSTM_PERSISTENT if persistent else 0) | (_lib.RGP_LSTM_BPTT_PERSISTENT if bptt_persistent else 0)
        self._create(batch, n_steps, dtype, save_for_backward, device, int(batch), int(n_steps), _lib.DTYPES[dtype], flags)

    def _check_shapes(self, src):
        assert tuple(src['ConvLSTM_Wxi'].shape) == (3, 3, self.P, self.S) and tuple(src['ConvLSTM_Wci'].shape) == (7, 7, self.S)


GRCN77_PARAM_TO_FIELD = {   # TF variable name (scope RCNBottom/ stripped, gaze_grcn77.py:152-153,174-184) -> rgp_grcn77_weights field
    'proj_c3d_W': 'proj_c3d_W', 'proj_c3d_b': 'proj_c3d_b',
    'GRU_Conv_Wz': 'gru_Wz', 'GRU_Conv_Uz': 'gru_Uz', 'GRU_Conv_Wr': 'gru_Wr', 'GRU_Conv_Ur': 'gru_Ur',
    'GRU_Conv_W': 'gru_W', 'GRU_Conv_U': 'gru_U', 'out_W': 'out_W', 'out_b': 'out_b',
}


class Grcn77Engine(_PersistentEngine):
    """gaze_grcn77 graph (models/gaze_grcn77.py:77-218) at fixed (B, T, dtype): gaze_grcn's projection and ConvGRU, then a
    per-pixel 128 -> 1 read-out on the fp32 state and a 49-way softmax (csrc/head_point.hip.h).  Maps are [B,T,7,7].

    per_step=True: the recurrence and its BPTT as per-timestep launches (RGP_GRCN77_PER_STEP); otherwise bf16 plans of at
    most 64 clips run them as persistent launches, as GrcnEngine does.  read_buffer: 'c3d_embedded' [B,T,7,7,512],
    'rcn_outputs' [B,T,7,7,128] and, after a backward, 'd_rcn_outputs' [B,T,7,7,128]; fp32."""
    PREFIX, PARAM_TO_FIELD, WEIGHTS = 'rgp_grcn77_', GRCN77_PARAM_TO_FIELD, _lib.Grcn77Weights

    def __init__(self, batch, n_steps, dtype='bf16', save_for_backward=False, device='cuda:0', per_step=False):
        self.P, self.S, self.per_step = 512, 128, bool(per_step)
        flags = (_lib.RGP_GRCN77_SAVE_FOR_BACKWARD if save_for_backward else 0) | (_lib.RGP_GRCN77_PER_STEP if per_step else 0)
        self._create(batch, n_steps, dtype, save_for_backward, device, int(batch), int(n_steps), _lib.DTYPES[dtype], flags)

    def _check_shapes(self, src):
        assert tuple(src['GRU_Conv_Wz'].shape) == (3, 3, self.P, self.S) and tuple(src['out_W'].shape) == (self.S, 1)

    def _outputs(self, want_probs, out_logits, out_probs):
        logits = out_logits if out_logits is not None else torch.empty(self.B, self.T, 7, 7, device=self.device)
        probs = None
        if want_probs:
            probs = out_probs if out_probs is not None else torch.empty_like(logits)
        return logits, probs

    def head_forward(self, states=None, want_probs=True):
        """The read-out alone (rgp_grcn77_head_fwd): on the plan's own states of the last forward, or on the caller's
        fp32 device tensor [B,T,7,7,128] -> (logits, probs) [B,T,7,7]."""
        if states is not None:
            assert states.is_cuda and states.dtype == torch.float32 and states.is_contiguous()
            assert tuple(states.shape) == (self.B, self.T, 7, 7, self.S), tuple(states.shape)
        logits, probs = self._outputs(want_probs, None, None)
        self._call('head_fwd', _ptr(states), _ptr(logits), _ptr(probs))
        return logits, probs

    def inject_fault(self, kind='seq'):
        raise NotImplementedError('rgp_grcn77 exports no fault hook: the time-out path is the ConvGRU plan\'s (GrcnEngine)')


def softmax_xent(logits, labels=None, want_probs=True):
    """Per-frame softmax / cross entropy (model_util.py:61-72; gaze_rnn.py:390-407).
    logits [..., H, W] fp32 device tensor -> (probs, frame_loss, loss)."""
    lib = _lib.load()
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.is_contiguous()
    npix = logits.shape[-1] * logits.shape[-2]
    frames = logits.numel() // npix
    probs = torch.empty_like(logits) if want_probs else None
    frame_loss = loss = None
    if labels is not None:
        assert labels.shape == logits.shape and labels.dtype == torch.float32 and labels.is_contiguous()
        frame_loss = torch.empty(frames, device=logits.device)
        loss = torch.empty(1, device=logits.device)
    with torch.cuda.device(logits.device):
        _lib.check(lib.rgp_softmax_xent_fwd(_ptr(logits), _ptr(labels), _ptr(probs), _ptr(frame_loss), _ptr(loss),
                                            frames, npix, _stream_ptr(logits.device)))
    return probs, frame_loss, loss


class FcGruEngine(_StreamBackward, _BpttPersistent, _Persistent, _PlanEngine):
    """fc-GRU gaze model (models/gaze_rnn.py:211-360, BASELINE config 2) at fixed (B, T, GH, GW).

    per_step=True names the per-timestep recurrence (RGP_FCGRU_PER_STEP: two launches per step), persistent=True the
    one-launch recurrence with resident kernels: RGP_FCGRU_PERSISTENT for bf16 plans (csrc/fcgru_seq.hip.h),
    RGP_FCGRU_PERSISTENT_F32 for f32 plans (csrc/fcgru_seq_f32.hip.h: fp32 MFMAs on the plan's fp32 rows); plans of at
    most 64 clips on a device with at least 203 CUs, refused otherwise.  With both False the library chooses (per step).
    bptt_persistent=True: the backward-through-time pass of backward() as one persistent launch as well
    (RGP_FCGRU_BPTT_PERSISTENT, csrc/fcgru_bptt.hip.h; bf16 training plans of at most 64 clips), whatever the forward runs;
    False is the library's choice (four launches per step).  On an f32 plan that keyword is refused by the library;
    bptt_persistent_f32=True is the same pass for f32 training plans (RGP_FCGRU_BPTT_PERSISTENT_F32,
    csrc/fcgru_bptt_f32.hip.h: fp32 MFMAs on the plan's fp32 gate-gradient rows; at most 64 clips), behind any forward path.
    The bptt_persistent / bptt_persistent_workgroups properties report either.
    read_buffer (training plans, after a forward; fp32): 'xpre' [B,T,3,1617], 'h' [T+1,B,1617], 'u', 'r', 'c'
    [T,B,1617], 'hp' [B,T+1,1617], 'rh' [B,T,1617]; after a backward also 'dxpre' [B,T,3,1617] (the gate-gradient operand
    rows, parts u, r, c), 'dh_head' [B,T,1617] and 'dh0' [B,1617] (the final carry)."""

    BUFFER_SHAPES = {'xpre': lambda B, T: (B, T, 3, 1617), 'h': lambda B, T: (T + 1, B, 1617), 'u': lambda B, T: (T, B, 1617),
                     'r': lambda B, T: (T, B, 1617), 'c': lambda B, T: (T, B, 1617), 'hp': lambda B, T: (B, T + 1, 1617),
                     'rh': lambda B, T: (B, T, 1617), 'dxpre': lambda B, T: (B, T, 3, 1617), 'dh_head': lambda B, T: (B, T, 1617),
                     'dh0': lambda B, T: (B, 1617)}
    PREFIX, CREATE, WEIGHTS = 'rgp_fcgru_', 'create_flags', _lib.FcGruWeights

    def __init__(self, batch, n_steps, gazemap_hw=(49, 49), dtype='f32', device='cuda:0', save_for_backward=False,
                 per_step=False, persistent=False, bptt_persistent=False, bptt_persistent_f32=False):
        self.B, self.T, self.GH, self.GW = int(batch), int(n_steps), int(gazemap_hw[0]), int(gazemap_hw[1])
        self.dtype = dtype
        self.save_for_backward = bool(save_for_backward)
        self.per_step = bool(per_step)
        flags = (_lib.RGP_FCGRU_SAVE_FOR_BACKWARD if save_for_backward else 0) | (_lib.RGP_FCGRU_PER_STEP if per_step else 0) | \
            ((_lib.RGP_FCGRU_PERSISTENT_F32 if dtype == 'f32' else _lib.RGP_FCGRU_PERSISTENT) if persistent else 0) | \
            (_lib.RGP_FCGRU_BPTT_PERSISTENT if bptt_persistent else 0) | \
            (_lib.RGP_FCGRU_BPTT_PERSISTENT_F32 if bptt_persistent_f32 else 0)
        self._create_plan(device, self.B, self.T, self.GH, self.GW, _lib.DTYPES[dtype], flags)
        # tf.nn.dropout on c3d_embedded [B*T*49, 32] (gaze_rnn.py:302-303): off until a training step draws a mask
        self.dropout = self._dropout_site(self.B * self.T * 49 * 32)

    def _state_shape(self):
        return (self.B, 1617)

    def backward(self, logits, probs, labels, loss_type='xentropy'):
        """Gradients of the loss of gaze_rnn.py:363-408 w.r.t. the 8 variables after forward() on the same
        inputs; returns {field: gradient view}, the flat buffer is flat_grads."""
        assert self.save_for_backward, 'create the engine with save_for_backward=True'
        assert labels.is_cuda and labels.dtype == torch.float32 and labels.is_contiguous()
        st = self._grad_struct()
        self._call('backward', _ptr(logits), _ptr(probs), _ptr(labels), ctypes.byref(st), {'xentropy': 0, 'l2': 1}[loss_type])
        return self.grads

    def read_buffer(self, name):
        """An intermediate of the last forward (or backward) of a training plan (rgp_fcgru_read_buffer), fp32, shaped as the class
        docstring lists."""
        if name not in self.BUFFER_SHAPES:
            raise _lib.RgpError('unknown intermediate %r' % name)
        shape = self.BUFFER_SHAPES[name](self.B, self.T)
        out = torch.empty(shape, dtype=torch.float32, device=self.device)
        self._call('read_buffer', name.encode(), _ptr(out))
        return out

    def forward(self, c3d_input, want_probs=True, train=False):
        """train=True draws a fresh dropout mask when dropout.configure(keep < 1) was called (single_step feeds
        keep 0.5 in training, gaze_rnn.py:529); train=False runs with the site off, as every evaluation does."""
        x = c3d_input
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
        assert tuple(x.shape) == (self.B, self.T, 1024, 7, 7), tuple(x.shape)
        self.dropout.arm(train)
        logits = torch.empty(self.B, self.T, self.GH, self.GW, device=self.device)
        probs = torch.empty_like(logits) if want_probs else None
        self._forward('forward', self.T, _ptr(x), _ptr(logits), _ptr(probs))
        return logits, probs

    def forward_stream(self, c3d_input, state=None, n_valid=None, want_probs=True, train=False):
        """One call of a stream (rgp_fcgru_forward_stream): the graph of forward() started from `state` instead of zeros, on
        either recurrence path and on inference and training plans (backward() is refused behind it until a plain forward;
        backward_stream() differentiates it).
        c3d_input [B,T,1024,7,7] fp32 at the full plan size; the recurrence is defined for the first n_valid (default T)
        steps, later outputs are unspecified.  state: fp32 device tensor of state_elems elements ([B, 1617], one slot of
        read_buffer('h')) from an earlier call, or None = the zero state; never modified.  train: the dropout site, as
        forward(train=...) arms it (the site is frame-local); off by default.
        Returns (logits, probs, new_state); new_state is a fresh tensor on every call: h behind step n_valid."""
        self.dropout.arm(train)
        logits = torch.empty(self.B, self.T, self.GH, self.GW, device=self.device)
        probs = torch.empty_like(logits) if want_probs else None
        new_state = self._stream_call(self.B, self.T, c3d_input, state, n_valid,
                                      lambda si, so, nv: (_ptr(c3d_input), si, so, nv, _ptr(logits), _ptr(probs)))
        return logits, probs, new_state


class ShallowNetEngine(_Buffers, _PlanEngine):
    """Frame-wise ShallowNet (models/saliency_shallownet.py:74-216, BASELINE config 1)."""

    PREFIX, CREATE, WEIGHTS = 'rgp_shallownet_', 'create_ex', _lib.ShallowNetWeights

    def __init__(self, max_frames, image_hw=98, dtype='f32', device='cuda:0', save_for_backward=False, dropout=False):
        self.max_frames, self.image_hw, self.dtype = int(max_frames), int(image_hw), dtype
        self.save_for_backward = bool(save_for_backward)
        self._create_plan(device, self.max_frames, self.image_hw, _lib.DTYPES[dtype], int(self.save_for_backward))
        # tf.nn.dropout on relu(fc1) [n, 4802] before the maxout (saliency_shallownet.py:152-158): only SaliencyModel has
        # the site; the gaze models build the net with dropout off, and their checkpoints hold no site for it
        self.dropout = self._dropout_site(self.max_frames * 4802) if dropout else None

    def backward(self, d_saliency):
        """d loss / d saliency [n,49,49] fp32 (frames of the last forward) -> {field: gradient view} for all ten
        variables (FramewiseShallowNet trains them all, gaze_framewise_shallownet.py:43-57)."""
        assert self.save_for_backward, 'create the engine with save_for_backward=True'
        d = d_saliency
        assert d.is_cuda and d.dtype == torch.float32 and d.is_contiguous() and tuple(d.shape[1:]) == (49, 49)
        st = self._grad_struct()
        self._call('backward', d.shape[0], _ptr(d), ctypes.byref(st))
        return self.grads

    def read_buffer(self, name):
        """Flat fp32 copy of an intermediate of the last forward / backward (names and layouts: rgp_shallownet_read_buffer,
        include/rgp.h).  Raises RgpError for an unknown name (RGP_EINVAL) and for a buffer this plan does not hold yet
        (RGP_ESTATE: a training-plan buffer of an inference plan, a gradient before a backward)."""
        out = torch.empty(max(self.read_buffer_elems(name), 1), dtype=torch.float32, device=self.device)
        self._call('read_buffer', name.encode(), _ptr(out))
        return out

    def forward(self, frames, want_7x7=False, train=False):
        """frames [n,H,W,3] fp32 device tensor -> (saliency [n,49,49], saliency7 [n,7,7] or None).
        train (engines created with dropout=True): True = draw a dropout mask (if configured), 'keep' = leave the mask
        dropout.use() installed (row f of its [max_frames, 4802] bytes belongs to frame f), False = site off."""
        assert frames.is_cuda and frames.dtype == torch.float32 and frames.is_contiguous()
        n = frames.shape[0]
        assert tuple(frames.shape[1:]) == (self.image_hw, self.image_hw, 3) and n <= self.max_frames
        if self.dropout is None:
            assert not train, 'create the engine with dropout=True'
        else:
            self.dropout.arm(train)
        sal = torch.empty(n, 49, 49, device=self.device)
        sal7 = torch.empty(n, 7, 7, device=self.device) if want_7x7 else None
        self._call('forward', _ptr(frames), n, _ptr(sal), _ptr(sal7))
        return sal, sal7


class CascadeEngine(_Streaming, _PlanEngine):
    """Two-level cascade (models/gaze_grcn_cascade.py:188-423, BASELINE config 5), forward."""

    # rgp_cascade_weights field -> key of the parameter dictionary (TF variable names)
    KEYS = (('proj_c3d_W', 'proj_c3d_W'), ('proj_c3d_b', 'proj_c3d_b'),
            ('bottom_Wz', 'RCNBottom/GRU_Conv_Wz'), ('bottom_Uz', 'RCNBottom/GRU_Conv_Uz'),
            ('bottom_Wr', 'RCNBottom/GRU_Conv_Wr'), ('bottom_Ur', 'RCNBottom/GRU_Conv_Ur'),
            ('bottom_W', 'RCNBottom/GRU_Conv_W'), ('bottom_U', 'RCNBottom/GRU_Conv_U'),
            ('upsampling_weight', 'Upsampling/weight'),
            ('top_Wz', 'RCNGaze/GRU_Conv_Wz'), ('top_Uz', 'RCNGaze/GRU_Conv_Uz'),
            ('top_Wr', 'RCNGaze/GRU_Conv_Wr'), ('top_Ur', 'RCNGaze/GRU_Conv_Ur'),
            ('top_W', 'RCNGaze/GRU_Conv_W'), ('top_U', 'RCNGaze/GRU_Conv_U'),
            ('fc1_w', 'LastProjection/fc1_w'), ('fc1_b', 'LastProjection/fc1_b'),
            ('fc2_w', 'LastProjection/fc2_w'), ('fc2_b', 'LastProjection/fc2_b'))

    PREFIX, CREATE, WEIGHTS = 'rgp_cascade_', 'create_ex', _lib.CascadeWeights

    def __init__(self, batch, n_steps, image_hw=98, dtype='bf16', device='cuda:0', save_for_backward=False):
        self.batch, self.n_steps, self.image_hw, self.dtype = int(batch), int(n_steps), int(image_hw), dtype
        self.save_for_backward = bool(save_for_backward)
        self._create_plan(device, self.batch, self.n_steps, self.image_hw, _lib.DTYPES[dtype], int(self.save_for_backward))
        # tf.nn.dropout on relu(fc1) [B*T, 4802] before the maxout (gaze_grcn_cascade.py:401-402)
        self.dropout = self._dropout_site(self.batch * self.n_steps * 4802)

    def _struct_of(self, views):
        st = _struct(self.WEIGHTS, self._fields, views)
        for k in _lib.ShallowNetWeights.FIELDS:                 # frozen (learning rate 0, base.py:264-265)
            setattr(st.shallownet, k, self.weights['shallownet.' + k].data_ptr())
        return st

    def set_weights(self, params):
        """The 19 trainable arrays live in one flat fp32 master buffer (one all-reduce bucket, one Adam launch);
        the ShallowNet's arrays are separate and frozen."""
        self._copy_in({field: params[key] for field, key in self.KEYS})
        for k in _lib.ShallowNetWeights.FIELDS:
            self.weights['shallownet.' + k] = _as_dev_f32(params['ShallowNet'][k], self.device)
        self.repack()

    def backward(self, maps, gt, want_d_rows=False):
        """Gradients of the l2 loss (gaze_grcn_cascade.py:428-441) after forward() on the same inputs.
        Returns ({rgp_cascade_weights field: gradient view}, d_rows or None); the flat buffer is flat_grads."""
        assert self.save_for_backward, 'create the engine with save_for_backward=True'
        assert gt.is_cuda and gt.dtype == torch.float32 and gt.is_contiguous() and gt.numel() == maps.numel()
        st = self._grad_struct()
        d_rows = torch.empty(self.batch * self.n_steps * 49, 1024, device=self.device) if want_d_rows else None
        self._call('backward', _ptr(maps), _ptr(gt), ctypes.byref(st), _ptr(d_rows))
        return self.grads, d_rows

    def forward(self, frame_images, c3d_input, train=False):
        """frame_images [B,T,H,W,3], c3d_input [B,T,1024,7,7] fp32 device tensors -> maps [B,T,49,49].
        train: True = draw a dropout mask (if configured), 'keep' = leave an installed mask, False = site off."""
        B, T = self.batch, self.n_steps
        self.dropout.arm(train)
        assert frame_images.is_cuda and frame_images.dtype == torch.float32 and frame_images.is_contiguous()
        assert c3d_input.is_cuda and c3d_input.dtype == torch.float32 and c3d_input.is_contiguous()
        assert tuple(frame_images.shape) == (B, T, self.image_hw, self.image_hw, 3), tuple(frame_images.shape)
        assert tuple(c3d_input.shape) == (B, T, 1024, 7, 7), tuple(c3d_input.shape)
        maps = torch.empty(B, T, 49, 49, device=self.device)
        self._call('forward', _ptr(frame_images), _ptr(c3d_input), _ptr(maps))
        return maps

    def forward_stream(self, frame_images, c3d_input, state=None, n_valid=None, train=False):
        """One call of a stream (rgp_cascade_forward_stream): the graph of forward() with both recurrent states started
        from `state` instead of zeros.  Inputs as for forward(), always at the full plan size; the recurrence is defined for
        the first n_valid (default T) steps, later maps are unspecified.  state: fp32 device tensor of state_elems elements
        from an earlier call, or None = the zero state; never modified.  Returns (maps, new_state); new_state is a fresh
        tensor on every call: both states behind step n_valid."""
        B, T = self.batch, self.n_steps
        self.dropout.arm(train)
        assert frame_images.is_cuda and frame_images.dtype == torch.float32 and frame_images.is_contiguous()
        assert tuple(frame_images.shape) == (B, T, self.image_hw, self.image_hw, 3), tuple(frame_images.shape)
        maps = torch.empty(B, T, 49, 49, device=self.device)
        new_state = self._stream_call(B, T, c3d_input, state, n_valid,
                                      lambda si, so, nv: (_ptr(frame_images), _ptr(c3d_input), si, so, nv, _ptr(maps)))
        return maps, new_state

    BUFFERS = {'frm_sal': lambda B, T: (B, T, 49, 49), 'rcn_outputs': lambda B, T: (B, T, 7, 7, 256),
               'rcn_upsampled_outputs': lambda B, T: (B, T, 49, 49, 64), 'gaze_rcn_outputs': lambda B, T: (B, T, 49, 49, 3)}

    def read_buffer(self, name):
        out = torch.empty(self.BUFFERS[name](self.batch, self.n_steps), device=self.device)
        self._call('read_buffer', name.encode(), _ptr(out))
        return out


class C3DEngine(_PlanEngine):
    """C3D conv1a..conv5b (prototxt:22-342) for up to max_windows windows per launch chain."""
    PREFIX, CREATE, WEIGHTS = 'rgp_c3d_', 'create_ex', _lib.C3DWeights

    KERNELS = {'patch': 0, 'igemm': _lib.RGP_C3D_KERNELS_IGEMM,
               'igemm128': _lib.RGP_C3D_KERNELS_IGEMM | _lib.RGP_C3D_KERNELS_TILE128,
               'patch-rowwise': _lib.RGP_C3D_CONV2A_ROWWISE, 'patch-twoplane': _lib.RGP_C3D_CONV3_TWOPLANE}

    def __init__(self, max_windows, dtype='bf16', device='cuda:0', save_for_backward=False, kernels='patch'):
        """kernels: 'patch' (default: the layer-specific kernels for conv2a..conv4b), 'igemm' (the general
        implicit-GEMM / filter-gradient kernels for every layer, tile by problem size) or 'igemm128' (the same on
        the 128x128 tile loop only), 'patch-rowwise' (the patch kernels with conv2a's inference forward on
        conv_patch_bf16_kernel instead of conv_patch_slab_bf16_kernel: RGP_C3D_CONV2A_ROWWISE),
        'patch-twoplane' (the patch kernels with conv3a's / conv3b's inference forward on the two-plane block tile
        instead of the plane-pure one: RGP_C3D_CONV3_TWOPLANE) -- rgp_c3d_create_ex flags; the alternatives exist
        for cross-checks."""
        self.max_windows = int(max_windows)
        self.dtype = dtype
        self.kernels = kernels
        self.save_for_backward = bool(save_for_backward)
        self.torch_dtype = torch.bfloat16 if _lib.DTYPES[dtype] == _lib.RGP_BF16 else torch.float32
        self._create_plan(device, self.max_windows, _lib.DTYPES[dtype], int(self.save_for_backward) | self.KERNELS[kernels])
        # fp32 master parameters in one flat vector, layout w[0], b[0], w[1], b[1], ... (= rgp_c3d_backward's grads)
        n = self.lib.rgp_c3d_param_elems(self._h)
        self.flat_params = torch.zeros(n, device=self.device)
        self.flat_grads = torch.zeros(n, device=self.device) if self.save_for_backward else None
        self.weights = self._views(self.flat_params)
        self.weights_set = False

    def _param_fields(self):
        return None         # the master layout is the library's (rgp_c3d_param_offset), not a struct of named fields

    def _views(self, flat):
        """{name: view into flat} with the shapes of the parameters, at the library's offsets."""
        out = {}
        for i, name in enumerate(C3D_LAYER_NAMES):
            cin, cout = C3D_CHANNELS[i]
            ow, ob = self.lib.rgp_c3d_param_offset(self._h, i, 0), self.lib.rgp_c3d_param_offset(self._h, i, 1)
            out[name + '_w'] = flat[ow:ow + 27 * cin * cout].view(3, 3, 3, cin, cout)
            out[name + '_b'] = flat[ob:ob + cout]
        return out

    def grad_views(self):
        """{name: view into flat_grads} with the shapes of the parameters."""
        return self._views(self.flat_grads)

    def set_weights(self, params):
        """params: {'conv1a_w': [3,3,3,Cin,Cout], 'conv1a_b': [Cout], ...} fp32 -> master copy + packed operands."""
        for name in C3D_LAYER_NAMES:
            for suffix in ('_w', '_b'):
                self.weights[name + suffix].copy_(_as_dev_f32(params[name + suffix], self.device).reshape(
                    self.weights[name + suffix].shape))
        self.repack()

    def repack(self):
        """Re-derive the packed (and, for training, rotated) operand filters from the master parameters."""
        st = _lib.C3DWeights()
        for i, name in enumerate(C3D_LAYER_NAMES):
            st.w[i] = self.weights[name + '_w'].data_ptr()
            st.b[i] = self.weights[name + '_b'].data_ptr()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.rgp_c3d_set_weights(self._h, ctypes.byref(st), _stream_ptr(self.device)))
        self.weights_set = True

    def backward(self, d_features=None, d_rows=None, zero_grads=True):
        """Gradient of the last forward (<= max_windows windows) w.r.t. every conv filter and bias, given the
        gradient w.r.t. conv5b as d_features [n,1024,7,7] or d_rows [n*49,1024] (fp32); fills flat_grads."""
        assert self.save_for_backward, 'create the engine with save_for_backward=True'
        g = d_features if d_features is not None else d_rows
        assert (d_features is None) != (d_rows is None) and g.is_cuda and g.dtype == torch.float32 and g.is_contiguous()
        n = g.shape[0] if d_features is not None else g.shape[0] // 49
        if zero_grads:
            self.flat_grads.zero_()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.rgp_c3d_backward(self._h, _ptr(d_features), _ptr(d_rows), n, _ptr(self.flat_grads),
                                                 _stream_ptr(self.device)))
        return self.flat_grads

    def forward(self, video, want_features=True, want_rows=False, out_rows=None):
        """video [n,16,112,112,3] fp32 device tensor -> (features [n,1024,7,7] fp32, rows)."""
        assert video.is_cuda and video.dtype == torch.float32 and video.is_contiguous()
        assert tuple(video.shape[1:]) == (16, 112, 112, 3), tuple(video.shape)
        n = video.shape[0]
        feats = torch.empty(n, 1024, 7, 7, device=self.device) if want_features else None
        rows = out_rows
        if want_rows and rows is None:
            rows = torch.empty(n * 49, 1024, dtype=self.torch_dtype, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.rgp_c3d_forward(self._h, _ptr(video), n, _ptr(feats), _ptr(rows), _stream_ptr(self.device)))
        return feats, rows

    def layer_grad_slice(self, layer):
        """View of flat_grads holding layer's filter then bias gradient (contiguous: one all-reduce bucket)."""
        cin, cout = C3D_CHANNELS[layer]
        ow = self.lib.rgp_c3d_param_offset(self._h, layer, 0)
        return self.flat_grads[ow:ow + 27 * cin * cout + cout]

    def wait_layer_grads(self, layer, stream):
        """Make `stream` (a torch.cuda.Stream) wait until the last backward() has finished layer's gradient slice."""
        _lib.check(self.lib.rgp_c3d_wait_layer_grads(self._h, int(layer), ctypes.c_void_p(stream.cuda_stream)))

    def read_grad_image(self, layer, n_windows):
        """After backward(): d loss / d (conv output of `layer` before ReLU and pooling), [n,D,H,W,Cout] fp32."""
        d, h = C3D_EXTENTS[layer]
        out = torch.empty(n_windows, d, h, h, C3D_CHANNELS[layer][1], device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.rgp_c3d_read_grad_image(self._h, layer, n_windows, _ptr(out), _stream_ptr(self.device)))
        return out

    def _frames_args(self, frames, window_starts, mean_cube):
        assert frames.is_cuda and frames.dtype == torch.uint8 and frames.is_contiguous() and frames.dim() == 4
        assert frames.shape[3] == 3, tuple(frames.shape)
        starts = [int(v) for v in window_starts]
        arr = (ctypes.c_int * len(starts))(*starts)
        if mean_cube is not None:
            assert mean_cube.is_cuda and mean_cube.dtype == torch.float32 and mean_cube.is_contiguous()
            assert tuple(mean_cube.shape) == (3, 16, 128, 171), tuple(mean_cube.shape)
        return arr, len(starts)

    def forward_frames(self, frames, window_starts, mean_cube=None, want_features=True, want_rows=False, out_rows=None):
        """frames [N,H,W,3] uint8 device tensor, window_starts: first frame of each 16-frame window
        -> (features [n,1024,7,7] fp32, rows): the VIDEO_DATA layer + conv1a..conv5b."""
        arr, n = self._frames_args(frames, window_starts, mean_cube)
        feats = torch.empty(n, 1024, 7, 7, device=self.device) if want_features else None
        rows = out_rows
        if want_rows and rows is None:
            rows = torch.empty(n * 49, 1024, dtype=self.torch_dtype, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.rgp_c3d_forward_frames(self._h, _ptr(frames), frames.shape[0], frames.shape[1],
                                                       frames.shape[2], arr, n, _ptr(mean_cube), _ptr(feats), _ptr(rows),
                                                       _stream_ptr(self.device)))
        return feats, rows

    def frames_to_video(self, frames, window_starts, mean_cube=None):
        """The VIDEO_DATA step alone -> video [n,16,112,112,3] fp32 (the input of forward())."""
        arr, n = self._frames_args(frames, window_starts, mean_cube)
        video = torch.empty(n, 16, 112, 112, 3, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.rgp_c3d_frames_to_video(self._h, _ptr(frames), frames.shape[0], frames.shape[1],
                                                        frames.shape[2], arr, n, _ptr(mean_cube), _ptr(video),
                                                        _stream_ptr(self.device)))
        return video

    def layer_kernel_name(self, layer, n_windows):
        """Kernel instantiation that runs layer's forward at n_windows windows per launch (as a profiler names it)."""
        return self.lib.rgp_c3d_layer_kernel_name(self._h, int(layer), int(n_windows)).decode()

    def read_layer(self, layer, n_windows):
        n = self.lib.rgp_c3d_layer_elems(self._h, layer, n_windows)
        out = torch.empty(n, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.rgp_c3d_read_layer(self._h, layer, n_windows, _ptr(out), _stream_ptr(self.device)))
        return out

    def profile(self, enable=True):
        _lib.check(self.lib.rgp_c3d_profile_enable(self._h, int(enable)))

    def profile_read(self):
        """{stage: (total_ms, launch_groups)} since the last read (HIP events on the launch stream)."""
        n = len(_lib.C3D_STAGES)
        ms, calls = (ctypes.c_double * n)(), (ctypes.c_longlong * n)()
        _lib.check(self.lib.rgp_c3d_profile_read(self._h, ms, calls))
        return {k: (ms[i], calls[i]) for i, k in enumerate(_lib.C3D_STAGES)}


ACTION_PARAM_TO_FIELD = {      # state-dict name -> rgp_action_weights field, in the struct's order (= the flat buffer's)
    'NN': {'W1': 'W1', 'Wg': 'Wg', 'b1': 'b1', 'W2': 'W2', 'b2': 'b2', 'W3': 'W3', 'b3': 'b3'},
    'SVM': {'W1': 'W1', 'Wg': 'Wg', 'b1': 'b1'},
}


def action_learning_rate(step, lr0=0.002, decay=0.96, decay_steps=10):
    """tf.train.exponential_decay(lr0, step, 10, 0.96), staircase=False: the exponent is continuous
    (action_classification.py:282-283)."""
    return float(lr0) * float(decay) ** (float(step) / float(decay_steps))


class ActionEngine(_Buffers, _PlanEngine):
    """Owner of one rgp_action_ plan (action_classification.py:210-292), its workspace, the flat fp32 master buffer
    (W1 first, then Wg / b1 / W2 / b2 / W3 / b3: the small variables lie back to back, one optimizer launch) and, for NN
    training plans, Adam's slots adam_m / adam_v in the same layout.  A training step (train_step: the plan's own fused
    optimizer, no flat_grads) updates flat_params in place.  set_weights takes {name: array} (synthetic.action_params /
    checkpoint.import_action_*_variables) and leaves Adam's slots as they are (zero on first use)."""

    PREFIX, WEIGHTS = 'rgp_action_', _lib.ActionWeights
    PARAM_TO_FIELD = ACTION_PARAM_TO_FIELD['NN']       # every variable of the struct; a plan's own list: _param_fields

    def __init__(self, batch, dim_feat=1024, mode='NN', use_gazemap=False, dtype='bf16', save_for_backward=False,
                 device='cuda:0', unfused=False):
        self.B, self.C, self.K = int(batch), int(dim_feat), 49 * int(dim_feat)
        self.mode, self.use_gazemap, self.dtype = mode, bool(use_gazemap), dtype
        self.N = 256 if mode == 'NN' else 13
        self.save_for_backward, self.unfused = bool(save_for_backward), bool(unfused)
        self.torch_dtype = torch.bfloat16 if _lib.DTYPES[dtype] == _lib.RGP_BF16 else torch.float32
        self.names = tuple(k for k in ACTION_PARAM_TO_FIELD[mode] if k != 'Wg' or self.use_gazemap)
        flags = (_lib.RGP_ACTION_USE_GAZEMAP if use_gazemap else 0) | (_lib.RGP_ACTION_SAVE_FOR_BACKWARD if save_for_backward else 0) \
            | (_lib.RGP_ACTION_UNFUSED if unfused else 0)
        self._create_plan(device, self.B, self.C, {'NN': _lib.RGP_ACTION_NN, 'SVM': _lib.RGP_ACTION_SVM}[mode],
                          _lib.DTYPES[dtype], flags)

    def _param_fields(self):
        return {k: ACTION_PARAM_TO_FIELD[self.mode][k] for k in self.names}

    def shapes(self):
        s = {'W1': (self.K, self.N), 'Wg': (2401, 49), 'b1': (self.N,), 'W2': (256, 256), 'b2': (256,), 'W3': (256, 13), 'b3': (13,)}
        return {k: s[k] for k in self.names}

    def _check_shapes(self, src):
        for k, shp in self.shapes().items():
            assert tuple(src[k].shape) == shp, (k, tuple(src[k].shape), shp)

    def get_weights(self):
        """{name: device tensor}: copies made by the library (rgp_action_get_weights)."""
        flat, views = _flat_views(self.names, self.weights, self.device)
        st = self._struct_of(views)
        self._call('get_weights', ctypes.byref(st))
        return views

    def slots(self):
        """Adam's m and v as {name: view} (NN training plans; created as zeros and bound on first use)."""
        if self.adam_m is None:
            self.adam_m, self.adam_v = torch.zeros_like(self.flat_params), torch.zeros_like(self.flat_params)
        if getattr(self, '_bound_m', None) is not self.adam_m or self._bound_v is not self.adam_v:   # (load_optimizer_state swaps them)
            layout = _flat_layout(self.names, self.shapes())
            self._mv = tuple({k: buf[off:off + n].view(self.shapes()[k]) for k, off, n in layout} for buf in (self.adam_m, self.adam_v))
            _lib.check(self._f['bind_slots'](self._h, ctypes.byref(self._struct_of(self._mv[0])), ctypes.byref(self._struct_of(self._mv[1]))))
            self._bound_m, self._bound_v = self.adam_m, self.adam_v
        return self._mv

    def _check_inputs(self, c3d, gazemap, labels=None):
        assert c3d.is_cuda and c3d.dtype == torch.float32 and c3d.is_contiguous() and c3d.numel() == self.B * self.K, tuple(c3d.shape)
        if self.use_gazemap:
            assert gazemap is not None and gazemap.is_cuda and gazemap.dtype == torch.float32 and gazemap.is_contiguous()
            assert gazemap.numel() == self.B * 2401, tuple(gazemap.shape)
        if labels is not None:
            assert labels.is_cuda and labels.dtype == torch.float32 and labels.is_contiguous() and labels.numel() == self.B * 13

    def _gm(self, gazemap):
        return _ptr(gazemap) if self.use_gazemap else None

    def forward(self, c3d, gazemap=None):
        """c3d [B,C,49] (or [B,C,7,7]) fp32, gazemap [B,49,49] fp32 device tensors -> (logits, y_pred) [B,13]."""
        self._check_inputs(c3d, gazemap)
        logits = torch.empty(self.B, 13, device=self.device)
        y_pred = torch.empty_like(logits)
        self._call('forward', _ptr(c3d), self._gm(gazemap), _ptr(logits), _ptr(y_pred))
        return logits, y_pred

    def forward_rows(self, rows, gazemap=None):
        """rows: conv5b rows of C3DEngine.forward for B windows (operand dtype, [B*49, 1024], column d*512+c)."""
        assert rows.is_cuda and rows.dtype == self.torch_dtype and rows.is_contiguous() and rows.numel() == self.B * 49 * 1024
        logits = torch.empty(self.B, 13, device=self.device)
        y_pred = torch.empty_like(logits)
        self._call('forward_rows', _ptr(rows), self._gm(gazemap), _ptr(logits), _ptr(y_pred))
        return logits, y_pred

    def loss(self, labels):
        """The loss of the last forward's batch -> 1-element device tensor."""
        assert labels.is_cuda and labels.dtype == torch.float32 and labels.is_contiguous() and labels.numel() == self.B * 13
        out = torch.empty(1, device=self.device)
        self._call('loss', _ptr(labels), _ptr(out))
        return out

    def train_step(self, c3d, gazemap, labels, step, lr=None):
        """One optimizer step; lr None = the reference's (NN: 0.002 * 0.96^(step/10); SVM: 0.01).  Returns the loss
        before the update (1-element device tensor)."""
        self._check_inputs(c3d, gazemap, labels)
        if lr is None:
            lr = action_learning_rate(step) if self.mode == 'NN' else 0.01
        if self.mode == 'NN':
            self.slots()
        out = torch.empty(1, device=self.device)
        self._call('train_step', _ptr(c3d), self._gm(gazemap), _ptr(labels), int(step), float(lr), _ptr(out))
        return out

    # ---- the stages of a step (tests)
    def fc1_fwd(self, c3d, gazemap=None):
        self._check_inputs(c3d, gazemap)
        self._call('fc1_fwd', _ptr(c3d), self._gm(gazemap))

    def tail(self, labels=None):
        self._call('tail', _ptr(labels))

    def fc1_update(self, c3d, gazemap, d_h1, step, lr):
        self._check_inputs(c3d, gazemap)
        assert d_h1.is_cuda and d_h1.dtype == torch.float32 and d_h1.is_contiguous() and d_h1.numel() == self.B * self.N
        if self.mode == 'NN':
            self.slots()
        self._call('fc1_update', _ptr(c3d), self._gm(gazemap), _ptr(d_h1), int(step), float(lr))
