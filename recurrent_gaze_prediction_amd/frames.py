"""The loader's frame images on the GPU: Pillow's antialiased resize, bit for bit, and the scale by 1 / 255.

The ShallowNet branch of the family (``ShallowNetEngine.forward``, ``CascadeEngine.forward``) takes ``frame_images``
[n, 98, 98, 3] fp32 in [0, 1].  The reference's loader makes them from the decoded video frames
(crc_input_data_seq.py:186-209): every fifth frame from 15 on, ``Image.resize((w, h), Image.ANTIALIAS)`` -- Pillow's
two-pass 8-bit Lanczos resample, whose support grows with the downscale -- and ``np.multiply(images.astype(np.float32),
1.0 / 255.0)``.  :func:`frame_images` does that to a uint8 clip that is already on the device (the C3D branch reads the
same clip: ``C3DFeatureExtractor.extract``) in one launch (csrc/rgp_frames.hip, ``rgp_frame_images`` in include/rgp.h).
The arithmetic is integer up to the final multiply, so the images equal Pillow's byte for byte.

Host side (numpy, float64): :func:`resample_coeffs` builds Pillow's weight and bounds tables in 22-bit fixed point and
checks that the int32 accumulator of a pass cannot overflow; the device computes no weight.
:func:`video_inputs` makes both inputs of the cascade -- conv5b features and frame images -- from one uploaded clip.

Not covered: more or fewer than 3 channels, an output side above 256, a filter of more than 128 taps (a downscale
beyond about 21x with Lanczos), frames wider than 2040 pixels.  Those raise ``ValueError``; there is no host fallback.
``extract_map.py``'s 49 -> 7 ``scipy.misc.imresize`` export -- one channel, scipy's bytescale in front, a float64
normalisation behind -- is ``models/extract_map.py``'s (csrc/rgp_mapexport.hip), with the tables made here.
"""
import ctypes

import numpy as np
import torch

from . import _image, _lib

PRECISION_BITS = 22
FILTER_SUPPORT = {'lanczos': 3.0, 'bilinear': 1.0, 'bicubic': 2.0}
OUTPUTS = ('float32', 'uint8', 'both')
MAX_OUT, MAX_KSIZE, MAX_IN_W, MAX_BYTES = (_lib.RGP_FRAMES_MAX_OUT, _lib.RGP_FRAMES_MAX_KSIZE, _lib.RGP_FRAMES_MAX_IN_W,
                                           _lib.RGP_FRAMES_MAX_BYTES)
LOADER_FIRST_FRAME, LOADER_FRAME_STEP = 15, 5
_tables = {}        # (device, in, out, filter) -> (k, bounds, ksize) on the device


def _filter(name, x):
    """Pillow's lanczos_filter / bilinear_filter / bicubic_filter (a = -0.5) on a float64 array."""
    if name == 'lanczos':
        inside = (x >= -3.0) & (x < 3.0)
        px = x * np.pi
        with np.errstate(invalid='ignore', divide='ignore'):
            a = np.where(x == 0.0, 1.0, np.sin(px) / px)
            x3 = x / 3
            p3 = x3 * np.pi
            b = np.where(x3 == 0.0, 1.0, np.sin(p3) / p3)
        return np.where(inside, a * b, 0.0)
    x = np.abs(x)
    if name == 'bilinear':
        return np.where(x < 1.0, 1.0 - x, 0.0)
    a = -0.5
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def resample_coeffs(in_size, out_size, filter='lanczos'):
    """-> (k int32 [out, ksize], bounds int32 [out, 2] = (xmin, n), ksize): Pillow's tables of one axis (precompute_coeffs
    and normalize_coeffs_8bpc of Resample.c).  Output xx is clamp((2^21 + sum_{x < n} pixel[xmin + x] k[xx, x]) >> 22, 0,
    255); entries past n are 0.  Raises ValueError for a geometry whose int32 accumulator could overflow
    (255 sum|k| + 2^21 >= 2^31 in some row), an unknown filter or a size below 1."""
    if filter not in FILTER_SUPPORT:
        raise ValueError('filter = %r: choose from %s' % (filter, sorted(FILTER_SUPPORT)))
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError('in_size = %d and out_size = %d must be at least 1' % (in_size, out_size))
    scale = float(in_size) / out_size
    fs = max(scale, 1.0)
    support = FILTER_SUPPORT[filter] * fs
    ksize = int(np.ceil(support)) * 2 + 1
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)            # (int): truncation, of values above -1 here
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size)
    n = xmax - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    valid = x < n[:, None]
    w = np.where(valid, _filter(filter, (x + xmin[:, None] - center[:, None] + 0.5) * (1.0 / fs)), 0.0)
    ww = np.zeros(out_size, np.float64)
    for j in range(ksize):                                                      # the sum in Pillow's order
        ww = ww + w[:, j]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    one = float(1 << PRECISION_BITS)
    k = np.where(w < 0, np.trunc(-0.5 + w * one), np.trunc(0.5 + w * one)).astype(np.int64)
    worst = int(np.abs(k).sum(axis=1).max())
    if 255 * worst + (1 << (PRECISION_BITS - 1)) >= 1 << 31 or int(np.abs(k).max()) >= 1 << 23:
        raise ValueError('%d -> %d with the %s filter: sum|k| = %.4f x 2^22 in some row, the int32 accumulator of a pass could '
                         'overflow' % (in_size, out_size, filter, worst / one))
    return k.astype(np.int32), np.stack([xmin, n], axis=1).astype(np.int32), ksize


def loader_frame_index(n_frames):
    """The frames the loader keeps (crc_input_data_seq.py:186): every fifth from 15 on."""
    return np.arange(LOADER_FIRST_FRAME, max(int(n_frames), LOADER_FIRST_FRAME), LOADER_FRAME_STEP, dtype=np.int64)


def band_plan(in_hw, out_hw, ksize_hw, n_out, bands=None):
    """The banding ``rgp_frame_images`` uses: -> (list of (r0, r1) output-row ranges, LDS bytes of a workgroup, the input
    rows a band's LDS image holds).  ``ksize_hw``: (ksize of the horizontal tables, of the vertical ones), 0 for a
    skipped pass.  ``bands``: the least count (None: the library's choice).  Host arithmetic only; ValueError if no
    banding fits."""
    (fh, fw), (oh, ow), (ksh, ksv) = in_hw, out_hw, ksize_hw
    lds, mid = ctypes.c_int(0), ctypes.c_int(0)
    nb = _lib.load().rgp_frames_plan(int(fh), int(fw), int(oh), int(ow), int(ksh), int(ksv), int(n_out), int(bands or 0),
                                     ctypes.byref(lds), ctypes.byref(mid))
    if nb <= 0:
        raise ValueError('%s -> %s with ksize %s, bands = %r: beyond the limits of rgp_frame_images, or not even one output row '
                         'per band fits RGP_FRAMES_LDS_BYTES = %d' % (in_hw, out_hw, ksize_hw, bands, _lib.RGP_FRAMES_LDS_BYTES))
    return [(b * oh // nb, (b + 1) * oh // nb) for b in range(nb)], lds.value, mid.value


def _ksize(in_size, out_size, filter):
    ksize = int(np.ceil(FILTER_SUPPORT[filter] * max(float(in_size) / out_size, 1.0))) * 2 + 1
    if ksize > MAX_KSIZE:
        raise ValueError('%d -> %d with the %s filter: %d taps, above RGP_FRAMES_MAX_KSIZE = %d'
                         % (in_size, out_size, filter, ksize, MAX_KSIZE))
    return ksize


def _device_tables(dev, in_size, out_size, filter):
    key = (str(dev), in_size, out_size, filter)
    if key not in _tables:
        k, b, ksize = resample_coeffs(in_size, out_size, filter)
        _tables[key] = (torch.from_numpy(k).to(dev), torch.from_numpy(b).to(dev), ksize)
    return _tables[key]


def frame_images(frames, out_hw=(98, 98), frame_index=None, filter='lanczos', out='float32', bands=None, device=None):
    """uint8 frames [N, H, W, 3] (numpy, or a contiguous device tensor) -> the loader's images of the frames
    ``frame_index`` selects (None: all, in order; repeats and any order are fine), on the device:
    ``out='float32'``: [n, oh, ow, 3] fp32 in [0, 1]; ``'uint8'``: the resized bytes; ``'both'``: (fp32, uint8).
    One launch.  ``bands``: the least number of bands of output rows per frame (None: the library's choice); the result
    does not depend on it.  Raises ValueError for what the kernel does not cover and ``_lib.RgpError`` if the device
    refused a frame (an index outside [0, N): NaN / 0 in that image; the error carries the outputs as ``.outputs``)."""
    if out not in OUTPUTS:
        raise ValueError('out = %r: choose from %s' % (out, OUTPUTS))
    if filter not in FILTER_SUPPORT:
        raise ValueError('filter = %r: choose from %s' % (filter, sorted(FILTER_SUPPORT)))
    oh, ow = (int(v) for v in out_hw)
    N, H, W, C = _image.host_check(frames, 'frames', torch.uint8, 4, text='frames must be uint8 [N, H, W, 3]')
    dev = _image.own_device(frames, device)
    if C != 3:
        raise ValueError('frames of %d channels: the kernel covers 3' % C)
    if not (1 <= oh <= MAX_OUT and 1 <= ow <= MAX_OUT):
        raise ValueError('out_hw = %s: both sides must be in [1, RGP_FRAMES_MAX_OUT = %d]' % ((oh, ow), MAX_OUT))
    if H < 1 or W < 1 or W > MAX_IN_W:
        raise ValueError('frames of %d x %d: the width must be in [1, RGP_FRAMES_MAX_IN_W = %d], the height at least 1' % (H, W, MAX_IN_W))
    if N * H * W * 3 >= MAX_BYTES:
        raise ValueError('%d frames of %d x %d x 3 bytes: RGP_FRAMES_MAX_BYTES = 2^40 or more' % (N, H, W))
    if bands is not None and not 1 <= int(bands) <= oh:
        raise ValueError('bands = %r must be in [1, out_h = %d]' % (bands, oh))
    if frame_index is None:
        idx, n = None, N
    else:
        idx = torch.as_tensor(frame_index).reshape(-1)
        if idx.numel() and (idx.dtype.is_floating_point or idx.dtype == torch.bool):
            raise ValueError('frame_index must hold integers')
        if idx.numel() and (int(idx.max()) >= 2 ** 31 or int(idx.min()) < -2 ** 31):
            raise ValueError('frame_index does not fit int32')
        n = int(idx.numel())
    if n * oh * ow * 3 >= MAX_BYTES:
        raise ValueError('%d images of %d x %d x 3: RGP_FRAMES_MAX_BYTES = 2^40 or more' % (n, oh, ow))
    kh = bh = kv = bv = None
    ksh = _ksize(W, ow, filter) if W != ow else 0
    ksv = _ksize(H, oh, filter) if H != oh else 0
    if n:
        band_plan((H, W), (oh, ow), (ksh, ksv), n, bands)          # ValueError if no banding fits
    # every refusal the host can make is above this line: from here on the device is used
    if W != ow:
        kh, bh, ksh = _device_tables(dev, W, ow, filter)
    if H != oh:
        kv, bv, ksv = _device_tables(dev, H, oh, filter)
    x = _image.to_device(frames, dev)
    f32 = torch.empty((n, oh, ow, 3), dtype=torch.float32, device=dev) if out in ('float32', 'both') else None
    u8 = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=dev) if out in ('uint8', 'both') else None
    result = f32 if out == 'float32' else u8 if out == 'uint8' else (f32, u8)
    if n == 0:
        return result
    d_idx = idx.to(torch.int32).to(dev).contiguous() if idx is not None else None
    lib = _lib.load()
    ws, ptr = _image.workspace(lib.rgp_frames_workspace_bytes(), dev), _image.ptr
    args = _lib.FramesArgs(frames=x.data_ptr(), n_frames=N, fh=H, fw=W, frame_index=ptr(d_idx), n_out=n, out_h=oh, out_w=ow,
                           kh=ptr(kh), bh=ptr(bh), ksize_h=ksh, kv=ptr(kv), bv=ptr(bv), ksize_v=ksv, bands=int(bands or 0),
                           images=ptr(f32), images_u8=ptr(u8), workspace=ws.data_ptr(), workspace_bytes=ws.numel())
    _image.launch(dev, lambda s: lib.rgp_frame_images(ctypes.byref(args), s),
                  lambda s: lib.rgp_frames_status(ws.data_ptr(), None, s), result)
    return result


def video_inputs(frames, extractor, image_hw=98):
    """One uint8 clip [N, H, W, 3] -> (starts, conv5b features [n, 1, 512, 2, 7, 7], frame_images [n, hw, hw, 3] fp32 on
    the device): the two inputs of the cascade from one upload.  The windows start every 5 frames
    (``window_starts(N, stride=5)``) and window i is paired with frame ``starts[i] + 15``, the pairing
    extract_map.py:183-187 asserts.  ``extractor``: a ``C3DFeatureExtractor``; its ``extract`` is used as it is."""
    from .c3d_frontend import window_starts
    dev = extractor.engine.device
    x = frames if torch.is_tensor(frames) else torch.from_numpy(np.ascontiguousarray(np.asarray(frames, np.uint8)))
    x = x.to(dev).contiguous()
    starts = window_starts(int(x.shape[0]), stride=LOADER_FRAME_STEP)
    starts, feats = extractor.extract(x, starts)
    index = np.asarray(starts, np.int64) + LOADER_FIRST_FRAME
    images = frame_images(x, (int(image_hw), int(image_hw)), frame_index=index)
    return starts, feats, images


__all__ = ['FILTER_SUPPORT', 'OUTPUTS', 'resample_coeffs', 'loader_frame_index', 'band_plan', 'frame_images', 'video_inputs']
