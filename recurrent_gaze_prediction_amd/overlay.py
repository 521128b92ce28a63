"""Frame overlays on the GPU: a gaze map drawn over its video frame, in the bytes the host libraries give.

``overlay_maps`` takes uint8 RGB frames [n_src, H, W, 3] and fp32 maps [n, h, w] and returns uint8 [n, H, W, 3], made
where the maps and the frames already are (csrc/rgp_overlay.hip, ``rgp_overlay`` in include/rgp.h): the maps go to the
frames' size with ``evaluation_metrics.resize`` (scipy's order-3 spline; the identity at equal shapes), to bytes with
scipy's ``bytescale`` (models/extract_map.py), through a 256-entry colour table -- what
``matplotlib.colormaps[name](u8, bytes=True)[..., :3]`` returns -- and over the frame with ``PIL.Image.blend``.  The
frame-size floats (1.2 GB for 1024 maps at 405 x 720) are never stored.  ``overlay_clip`` pairs maps and frames of a
clip the way the loader does (every fifth frame from the fifteenth on, crc_input_data_seq.py:186).

Not covered: maps above 4096 pixels that need a resize, frames above RGP_METRICS_SCALED_MAX_PIX pixels, ``alpha`` outside
[0, 1] (Pillow extrapolates and clips there), RGBA.  Those raise ``ValueError``; there is no host fallback.
"""
import ctypes

import numpy as np
import torch

from . import _image, _lib
from ._image import host_check as _host_check, to_device as _to_device

MAX_PIX, SCALED_MAX_PIX = _lib.RGP_METRICS_MAX_PIX, _lib.RGP_METRICS_SCALED_MAX_PIX

# matplotlib's segment data of the two built-in tables: rows of (x, y below x, y from x on) per channel
_JET = {'red': ((0.00, 0, 0), (0.35, 0, 0), (0.66, 1, 1), (0.89, 1, 1), (1.00, 0.5, 0.5)),
        'green': ((0.000, 0, 0), (0.125, 0, 0), (0.375, 1, 1), (0.640, 1, 1), (0.910, 0, 0), (1.000, 0, 0)),
        'blue': ((0.00, 0.5, 0.5), (0.11, 1, 1), (0.34, 1, 1), (0.65, 0, 0), (1.00, 0, 0))}
_GRAY = {c: ((0.0, 0, 0), (1.0, 1, 1)) for c in ('red', 'green', 'blue')}
BUILTIN = {'jet': _JET, 'gray': _GRAY}


def _segment_channel(data, N=256):
    """matplotlib.colors._create_lookup_table(N, data, gamma=1): the float64 channel values in [0, 1]."""
    adata = np.array(data, dtype=np.float64)
    x, y0, y1 = adata[:, 0] * (N - 1), adata[:, 1], adata[:, 2]
    xind = (N - 1) * np.linspace(0, 1, N)
    ind = np.searchsorted(x, xind)[1:-1]
    distance = (xind[1:-1] - x[ind - 1]) / (x[ind] - x[ind - 1])
    lut = np.concatenate([[y1[0]], distance * (y0[ind] - y1[ind - 1]) + y1[ind - 1], [y0[-1]]])
    return np.clip(lut, 0.0, 1.0)


def colormap_lut(name_or_table):
    """-> uint8 [256, 3]: the bytes ``matplotlib.colormaps[name](np.arange(256, dtype=np.uint8), bytes=True)[:, :3]``
    returns.  'jet' and 'gray' are built here from the colormap's segment data (no matplotlib needed); a uint8 [256, 3]
    array is passed through; any other name resolves through matplotlib if it can be imported."""
    if not isinstance(name_or_table, str):
        table = name_or_table.cpu().numpy() if torch.is_tensor(name_or_table) else np.asarray(name_or_table)
        if table.dtype != np.uint8 or table.shape != (256, 3):
            raise ValueError('a colour table must be uint8 [256, 3], got %s %s' % (table.dtype, table.shape))
        return np.ascontiguousarray(table)
    if name_or_table in BUILTIN:
        seg = BUILTIN[name_or_table]
        lut = np.stack([_segment_channel(seg[c]) for c in ('red', 'green', 'blue')], axis=1)
        return (lut * 255).astype(np.uint8)
    try:
        import matplotlib
    except ImportError:
        raise ValueError("colormap %r needs matplotlib, which cannot be imported; built in: 'jet' and 'gray'" % (name_or_table,))
    try:
        cmap = matplotlib.colormaps[name_or_table]
    except KeyError:
        raise ValueError("unknown colormap %r (built in: 'jet' and 'gray'; others by matplotlib's names)" % (name_or_table,))
    return np.ascontiguousarray(cmap(np.arange(256, dtype=np.uint8), bytes=True)[:, :3])


def overlay_maps(frames, maps, alpha=0.4, colormap='jet', frame_idx=None, limits=None, want_heat=False, device=None,
                 out=None, want_out=True):
    """frames uint8 [n_src, H, W, 3] (RGB) and maps fp32 [n, h, w], each a contiguous device tensor or numpy / a host tensor
    (uploaded) -> uint8 device tensor [n, H, W, 3]: ``Image.blend(frame, colour, alpha)`` with colour =
    ``colormap_lut(colormap)[bytescale(resize(map, (H, W)))]``.  ``want_heat=True``: (overlays, the bytescaled maps uint8
    [n, H, W]); ``want_out=False`` with it: the heat bytes alone.

    ``frame_idx``: int32 [n], the frame of each map (default: map i on frame i); repeats and any order are allowed.
    ``limits``: None -- every map scaled between its own min and max; 'clip' -- one (cmin, cmax) for the call, the min and
    max over all resized maps; or fp32 [n, 2] (or one pair), scipy's ``bytescale(data, cmin=, cmax=)``: values outside
    are clipped.  ``out``: a contiguous uint8 device tensor [n, H, W, 3] to write into (it must not overlap ``frames``).

    ValueError for what the kernel does not cover, before the device is used.  ``_lib.RgpError`` if the device refused
    maps (a NaN or an Inf in the map, limits that are not finite or descend, a frame index outside the clip): their
    frames come back unchanged, their heat is 0, the other maps are computed; the error carries the tensors as
    ``.outputs``."""
    n_src, H, W, _ = _host_check(frames, 'frames', torch.uint8, 4, 3)
    n, h, w = _host_check(maps, 'maps', torch.float32, 3)
    alpha = float(alpha)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError('alpha = %r must be in [0, 1]' % (alpha,))
    if not (want_out or want_heat):
        raise ValueError('want_out and want_heat are both False: nothing to compute')
    lut = colormap_lut(colormap)
    if H < 1 or W < 1 or H * W > SCALED_MAX_PIX:
        raise ValueError('frames of %d x %d pixels: at least 1 and at most RGP_METRICS_SCALED_MAX_PIX = %d' % (H, W, SCALED_MAX_PIX))
    if (h, w) != (H, W) and (h < 2 or w < 2 or h * w > MAX_PIX):
        raise ValueError('maps of %d x %d pixels that need a resize: sides of at least 2 and at most RGP_METRICS_MAX_PIX = %d pixels'
                         % (h, w, MAX_PIX))
    if frame_idx is None:
        if n_src < n:
            raise ValueError('%d maps for %d frames and no frame_idx' % (n, n_src))
    else:
        if not torch.is_tensor(frame_idx):
            frame_idx = np.asarray(frame_idx)
            if frame_idx.dtype.kind in 'iu':
                frame_idx = frame_idx.astype(np.int32)
        if _host_check(frame_idx, 'frame_idx', torch.int32, 1) != (n,):
            raise ValueError('frame_idx must hold one entry per map (%d)' % n)
    flags = 0
    if isinstance(limits, str):
        if limits != 'clip':
            raise ValueError("limits must be None, 'clip' or an array [n, 2], got %r" % (limits,))
        limits, flags = None, _lib.RGP_OVERLAY_SHARED_LIMITS
    elif limits is not None:
        if not torch.is_tensor(limits):
            limits = np.ascontiguousarray(np.broadcast_to(np.asarray(limits, np.float32), (n, 2)))
        if _host_check(limits, 'limits', torch.float32, 2, 2) != (n, 2):
            raise ValueError('limits must be [n, 2] = [%d, 2]' % n)
    dev = _image.pick_device(device, frames, maps)
    if out is not None:
        if not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
                and tuple(out.shape) == (n, H, W, 3)):
            raise ValueError('out must be a contiguous uint8 device tensor [%d, %d, %d, 3]' % (n, H, W))
        if not want_out:
            raise ValueError('out is given and want_out is False')
    # every refusal the host can make is above this line: from here on the device is used
    frames_d, maps_d = _to_device(frames, dev), _to_device(maps, dev)
    idx_d = None if frame_idx is None else _to_device(frame_idx, dev)
    lim_d = None if limits is None else _to_device(limits, dev)
    lut_d = torch.from_numpy(np.array(lut)).to(dev)
    res = {}
    if want_out:
        res['out'] = out if out is not None else torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
    if want_heat:
        res['heat'] = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
    if n > 0:
        lib = _lib.load()
        ws, ptr = _image.workspace(lib.rgp_overlay_workspace_bytes(n, h, w, H, W), dev), _image.ptr
        args = _lib.OverlayArgs(frames=frames_d.data_ptr(), frame_idx=ptr(idx_d), maps=maps_d.data_ptr(), limits=ptr(lim_d),
                                lut=lut_d.data_ptr(), alpha=alpha, flags=flags, out=ptr(res.get('out')), heat_u8=ptr(res.get('heat')),
                                n=n, n_src=n_src, h=h, w=w, H=H, W=W)
        _image.launch(dev, lambda s: lib.rgp_overlay(ctypes.byref(args), ws.data_ptr(), ws.numel(), s),
                      lambda s: lib.rgp_overlay_status(ws.data_ptr(), None, s), res)
    if want_out and want_heat:
        return res['out'], res['heat']
    return res['out'] if want_out else res['heat']


def clip_frame_index(n_maps, first=15, step=5):
    """The frames of a clip the loader pairs with its maps (crc_input_data_seq.py:186, ``filepaths[15::5]``): int32 [n_maps]."""
    if first < 0 or step < 1:
        raise ValueError('first = %d must not be negative and step = %d must be positive' % (first, step))
    return (first + step * np.arange(int(n_maps), dtype=np.int64)).astype(np.int32)


def overlay_clip(clip, maps, first=15, step=5, **kw):
    """Maps of a clip over its frames: map i on frame ``first + i * step`` of ``clip`` (uint8 [n_frames, H, W, 3]), the
    loader's pairing.  Keyword arguments and the result as :func:`overlay_maps`.  ValueError if the clip is too short."""
    idx = clip_frame_index(len(maps), first, step)
    if len(idx) and int(idx[-1]) >= len(clip):
        raise ValueError('%d maps from frame %d every %d need %d frames, the clip has %d' % (len(maps), first, step, int(idx[-1]) + 1, len(clip)))
    return overlay_maps(clip, maps, frame_idx=idx, **kw)


__all__ = ['colormap_lut', 'overlay_maps', 'overlay_clip', 'clip_frame_index']
