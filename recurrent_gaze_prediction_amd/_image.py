"""What the wrappers of the image-side launches (frames, overlay, gazemaps, models/extract_map) do alike: the refusals
the host can make about an array or tensor, its way to the device, the status workspace, and the launch itself --
entry, then status, then ``_lib.check`` with the outputs attached to the error (csrc/image_shared.hip.h has the C side)."""
import numpy as np
import torch

from . import _lib


def pick_device(device, *xs):
    """``device`` if given ('cuda' meaning cuda:0), else the device of the first device tensor among ``xs``, else cuda:0."""
    if device is not None:
        device = torch.device(device)
        return torch.device('cuda', 0 if device.index is None else device.index) if device.type == 'cuda' else device
    for x in xs:
        if torch.is_tensor(x) and x.is_cuda:
            return x.device
    return torch.device('cuda:0')


def own_device(x, device):
    """A device tensor's own device; for anything else ``device`` (None: cuda:0) as it is given."""
    return x.device if torch.is_tensor(x) and x.is_cuda else torch.device('cuda:0' if device is None else device)


def host_check(x, what, dtype, ndim, last=None, text=None):
    """The refusals the host can make about an array or tensor; -> its shape.  ``text``: the caller's own words for a
    wrong dtype or number of axes."""
    want = {torch.uint8: np.uint8, torch.float32: np.float32, torch.int32: np.int32}[dtype]
    if torch.is_tensor(x):
        ok = x.dtype == dtype
        if x.is_cuda and not x.is_contiguous():
            raise ValueError('a device tensor of %s must be contiguous' % what)
    else:
        ok = np.asarray(x).dtype == want
    shape = tuple(int(v) for v in x.shape)
    if not ok or len(shape) != ndim or (last is not None and shape[-1] != last):
        raise ValueError(text or '%s must be %s with %d axes%s'
                         % (what, np.dtype(want).name, ndim, '' if last is None else ', the last of %d' % last))
    return shape


def to_device(x, dev):
    """A contiguous tensor on ``dev``: a tensor that is there already as it is, anything else (a host tensor, numpy, a
    tensor on another device) copied there."""
    if torch.is_tensor(x):
        return x if x.device == dev else x.contiguous().to(dev)
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def ptr(t):
    return t.data_ptr() if t is not None else None


def workspace(n_bytes, dev):
    """The workspace of an entry, the status area at its head: at least 64 bytes."""
    return torch.empty(max(int(n_bytes), 64), dtype=torch.uint8, device=dev)


def check(rc, outputs):
    """``_lib.check``; an error carries what the device did compute as ``.outputs``."""
    try:
        _lib.check(rc)
    except _lib.RgpError as err:
        err.outputs = outputs
        raise


def launch(dev, entry, status, outputs):
    """``entry(stream)`` and, if it was queued, ``status(stream)`` (which waits: the workspace may go on return) on
    ``dev``'s current stream, then :func:`check`."""
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        rc = entry(stream)
        if rc == 0:
            rc = status(stream)
    check(rc, outputs)
