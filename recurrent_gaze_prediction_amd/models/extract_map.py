"""Mirror of the reference's models/extract_map.py: the gaze-map export, on the GPU.

The reference writes, per clip, ``<clip>.gazemap.49.npy`` (the model's maps) and ``<clip>.gazemap.npy``, the 7 x 7 maps
the action classifier reads.  Its ``avg_pool()`` (extract_map.py:35-41) is no average: it is
``scipy.misc.imresize(a[i], (7, 7))`` -- scipy's ``bytescale`` to 8 bits, then Pillow's two-pass 8-bit bilinear
resample -- followed by ``p /= p.sum()`` in float64.  :func:`avg_pool` does that to maps that are already on the device
in one launch (csrc/rgp_mapexport.hip, ``rgp_mapexport`` in include/rgp.h), bit for bit: the same bytes, and float64
quotients of the same integers.  A map whose resized bytes sum to 0 (a constant map, a very peaked one) comes back as
NaN, as the reference's 0 / 0 does.  :func:`bytescale_maps` returns the 8-bit maps alone, the pixels
``scipy.misc.imsave`` encodes (evaluate_gaze.py:148-152); :func:`bytescale` is the same arithmetic in numpy for arrays of
any shape (frame images).  :func:`export_clips` is the export loop of extract_map.py:148-238.

scipy.misc.imresize, imsave and bytescale left scipy in 1.3; the arithmetic is that of scipy <= 1.2 under a NumPy before
NEP 50 (a float64 scalar does not promote an fp32 array), written with explicit casts.

Not covered: maps above 64 x 64, upscaling, ``interp='nearest'``, more than one channel (that is ``frames.frame_images``),
the LSMDC folder scan with its hard-coded paths.  Those raise ``ValueError``; there is no host fallback.
"""
import ctypes
import logging
import os

import numpy as np
import torch

from .. import _image, _lib
from ..frames import FILTER_SUPPORT, _device_tables

log = logging.getLogger('rgp')
MAX_SIDE, MAX_KSIZE = _lib.RGP_MAPEXPORT_MAX_SIDE, _lib.RGP_MAPEXPORT_MAX_KSIZE


def bytescale(data):
    """scipy.misc.bytescale(data) (cmin / cmax from the data, high = 255, low = 0) on the host, for an fp32 array of any
    shape (uint8 goes through unchanged, as scipy returns it): the oracle's formulation, see the module docstring."""
    data = np.asarray(data)
    if data.dtype == np.uint8:
        return data
    a = data.astype(np.float32)
    cmin, cmax = np.float32(a.min()), np.float32(a.max())
    with np.errstate(all='ignore'):
        cscale = np.float32(cmax - cmin)
        if cscale == 0:
            cscale = np.float32(1)
        scale = np.float32(255.0 / float(cscale))
        b = np.multiply(np.subtract(a, cmin, dtype=np.float32), scale, dtype=np.float32)
        t = np.add(np.clip(b, np.float32(0), np.float32(255)), np.float32(0.5), dtype=np.float32)
        t = np.where(np.isnan(t), np.float32(0), t)             # 0 * inf: byte 0, the x86 conversion's result
    return np.trunc(t).astype(np.uint8)


def _check_maps(maps, device):
    """-> (torch.device, (n, h, w)); every refusal the host can make about the maps themselves."""
    n, h, w = _image.host_check(maps, 'maps', torch.float32, 3, text='maps must be float32 [n, H, W]')
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError('maps of %d x %d: both sides must be in [1, RGP_MAPEXPORT_MAX_SIDE = %d]' % (h, w, MAX_SIDE))
    return _image.own_device(maps, device), (n, h, w)


def _export(maps, out_shape, interp, want, device):
    """One launch of rgp_mapexport.  want: a subset of ('pooled', 'pooled_u8', 'bytes') -> {name: device tensor}."""
    dev, (n, h, w) = _check_maps(maps, device)
    resize = 'pooled' in want or 'pooled_u8' in want
    oh, ow, ksh, ksv = h, w, 0, 0
    if resize:
        if interp not in FILTER_SUPPORT:
            raise ValueError('interp = %r: choose from %s' % (interp, sorted(FILTER_SUPPORT)))
        oh, ow = (int(v) for v in out_shape)
        if not (1 <= oh <= h and 1 <= ow <= w):
            raise ValueError('out_shape = %s: each side must be in [1, the map\'s = %s]' % ((oh, ow), (h, w)))
        for size, out in ((w, ow), (h, oh)):
            ksize = int(np.ceil(FILTER_SUPPORT[interp] * max(float(size) / out, 1.0))) * 2 + 1
            if size != out and ksize > MAX_KSIZE:
                raise ValueError('%d -> %d with the %s filter: %d taps, above RGP_MAPEXPORT_MAX_KSIZE = %d'
                                 % (size, out, interp, ksize, MAX_KSIZE))
    # every refusal the host can make is above this line: from here on the device is used
    kh = bh = kv = bv = None
    if resize and w != ow:
        kh, bh, ksh = _device_tables(dev, w, ow, interp)
    if resize and h != oh:
        kv, bv, ksv = _device_tables(dev, h, oh, interp)
    x = _image.to_device(maps, dev)
    out = {}
    if 'pooled' in want:
        out['pooled'] = torch.empty((n, oh, ow), dtype=torch.float64, device=dev)
    if 'pooled_u8' in want:
        out['pooled_u8'] = torch.empty((n, oh, ow), dtype=torch.uint8, device=dev)
    if 'bytes' in want:
        out['bytes'] = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
    if n == 0:
        return out
    lib = _lib.load()
    ws, ptr = _image.workspace(lib.rgp_mapexport_workspace_bytes(), dev), _image.ptr
    args = _lib.MapExportArgs(maps=x.data_ptr(), n=n, h=h, w=w, out_h=oh, out_w=ow, kh=ptr(kh), bh=ptr(bh), ksize_h=ksh,
                              kv=ptr(kv), bv=ptr(bv), ksize_v=ksv, pooled=ptr(out.get('pooled')),
                              pooled_u8=ptr(out.get('pooled_u8')), bytes=ptr(out.get('bytes')), workspace=ws.data_ptr(),
                              workspace_bytes=ws.numel())
    _image.launch(dev, lambda s: lib.rgp_mapexport(ctypes.byref(args), s),
                  lambda s: lib.rgp_mapexport_status(ws.data_ptr(), None, s), out)
    return out


def _like(maps, t):
    return t if torch.is_tensor(maps) and maps.is_cuda else t.cpu().numpy()


def avg_pool(maps, out_shape=(7, 7), interp='bilinear', return_bytes=False, device=None):
    """extract_map.py:35-41.  maps fp32 [n, H, W] (a contiguous device tensor, or numpy / a host tensor, which is
    uploaded) -> float64 [n, out_h, out_w]: imresize(a[i], out_shape, interp) / its sum, NaN where the sum is 0.  A device
    tensor gives device tensors, anything else numpy.  ``return_bytes=True``: (pooled, the uint8 maps [n, H, W] that
    bytescale makes, the pixels imresize resamples).  ``interp``: 'bilinear' (scipy's default), 'lanczos' or 'bicubic'.
    One launch.  ValueError for what the kernel does not cover; ``_lib.RgpError`` if the device refused a map that holds a
    NaN or an Inf (NaN / 0 in that map's outputs, the others computed; the error carries the device tensors as
    ``.outputs``)."""
    out = _export(maps, out_shape, interp, ('pooled', 'bytes') if return_bytes else ('pooled',), device)
    if return_bytes:
        return _like(maps, out['pooled']), _like(maps, out['bytes'])
    return _like(maps, out['pooled'])


def bytescale_maps(maps, device=None):
    """scipy.misc.bytescale per map, maps fp32 [n, H, W] -> uint8 [n, H, W] (device tensor in, device tensor out;
    otherwise numpy): what scipy.misc.imsave encodes.  One launch; errors as :func:`avg_pool`."""
    return _like(maps, _export(maps, None, None, ('bytes',), device)['bytes'])


def export_clips(model, clips, out_dir, out_shape=(7, 7), interp='bilinear'):
    """extract_map.py:148-238.  clips: an iterable of (name, c3d) or (name, c3d, frames), c3d [len, 1024, 7, 7] (or
    [len, 512, 2, 7, 7]) and frames [len, 98, 98, 3] in [0, 1] for the models that read them.  B = model.batch_size clips
    go through one ``model.predict`` of T = model.n_lstm_steps steps: a shorter clip is padded with zeros, a longer one
    cut to T (with a warning, as the reference).  Per clip, ``out_dir/name/name.gazemap.49.npy`` (fp32, the first
    ``length`` maps as the model made them) and ``out_dir/name/name.gazemap.npy`` (float64, :func:`avg_pool` of those maps)
    are written.  A clip whose folder exists is skipped before it is loaded into a batch.  The pooling runs on the device
    tensor ``predict`` returns; only the two results are copied to the host.  -> the names written, in order."""
    B, T = int(model.batch_size), int(model.n_lstm_steps)
    written = []

    def flush(names, lengths, batch_c3d, batch_frames, use_frames):
        gazes = model.predict(batch_c3d, batch_frames if use_frames else None)
        gazes = gazes if torch.is_tensor(gazes) else torch.as_tensor(np.asarray(gazes))
        gazes = gazes.reshape((B, T) + tuple(gazes.shape[-2:])).to(torch.float32)
        rows = torch.as_tensor([b * T + t for b, n in enumerate(lengths) for t in range(n)], dtype=torch.long, device=gazes.device)
        valid = gazes.reshape((B * T,) + tuple(gazes.shape[-2:])).index_select(0, rows).contiguous()
        pooled = avg_pool(valid, out_shape, interp)
        maps49 = valid.cpu().numpy()
        pooled = pooled.cpu().numpy() if torch.is_tensor(pooled) else np.asarray(pooled)
        at = 0
        for name, n in zip(names, lengths):
            folder = os.path.join(out_dir, name)
            os.makedirs(folder, exist_ok=True)
            np.save(os.path.join(folder, '%s.gazemap.49.npy' % name), maps49[at:at + n])
            np.save(os.path.join(folder, '%s.gazemap.npy' % name), pooled[at:at + n])
            log.info('%s : saved length = %d', name, n)
            written.append(name)
            at += n

    names, lengths, use_frames = [], [], False
    batch_c3d = np.zeros((B, T, 1024, 7, 7), np.float32)
    batch_frames = None
    for i, clip in enumerate(clips):
        name, c3d = clip[0], clip[1]
        frames = clip[2] if len(clip) > 2 else None
        if os.path.exists(os.path.join(out_dir, name)):
            log.warning('Skipped - already exists %s', os.path.join(out_dir, name))
            continue
        c3d = np.asarray(c3d, np.float32).reshape(len(c3d), 1024, 7, 7)
        if frames is not None and len(frames) != len(c3d):
            raise ValueError('%d : %s length differs (%d frames != %d c3d steps)' % (i, name, len(frames), len(c3d)))
        n = len(c3d)
        if n > T:
            log.warning('%d %s : Too long. c3d_len = %d, rnn steps = %d', i, name, n, T)
            n = T
        b = len(names)
        batch_c3d[b] = 0
        batch_c3d[b, :n] = c3d[:n]
        if frames is not None:
            frames = np.asarray(frames, np.float32)
            if batch_frames is None:
                batch_frames = np.zeros((B, T) + frames.shape[1:], np.float32)
            batch_frames[b] = 0
            batch_frames[b, :n] = frames[:n]
            use_frames = True
        elif batch_frames is not None:
            batch_frames[b] = 0
        names.append(name)
        lengths.append(n)
        if len(names) == B:
            flush(names, lengths, batch_c3d, batch_frames, use_frames)
            names, lengths, use_frames = [], [], False
    if names:
        batch_c3d[len(names):] = 0           # the reference leaves the previous batch's clips here; their maps are not saved
        if batch_frames is not None:
            batch_frames[len(names):] = 0
        flush(names, lengths, batch_c3d, batch_frames, use_frames)
    return written


__all__ = ['avg_pool', 'bytescale_maps', 'bytescale', 'export_clips']
