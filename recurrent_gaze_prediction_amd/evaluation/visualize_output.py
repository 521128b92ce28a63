"""Mirror of the reference's evaluation/visualize_output.py, with the part it left as ``Not implemented Yet :(`` (:54).

``tile_grid`` is ``imshow_grid``'s arithmetic (:22-51) -- images padded at the bottom and the right, the set padded to a
full grid, tiled row-major -- returning the sheet instead of handing it to ``plt.imshow``; on device tensors it runs as
torch operations.  ``visualize_outputs`` makes one contact sheet per call, a column per frame holding the frame, the
prediction drawn over it and the ground truth drawn over it (overlay.overlay_maps: one launch pair for each of the two).
matplotlib figures and the TensorFlow session wrapper (:87-150) are not reproduced.
"""
import math

import numpy as np
import torch

from ..overlay import overlay_maps


def tile_grid(data, height=None, width=None, padsize=1, padval=0):
    """[N, H, W] or [N, H, W, C] (tensor on any device, or numpy) -> the grid [height * (H + padsize), width * (W + padsize)(, C)]
    of the same kind.  Without ``height`` and ``width`` the grid is near-square; with ``width`` alone it has the rows N needs."""
    is_np = not torch.is_tensor(data)
    t = torch.as_tensor(np.asarray(data)) if is_np else data
    if t.dim() < 3:
        raise ValueError('data must be [N, H, W] or [N, H, W, C]')
    N = int(t.shape[0])
    if height is None:
        height = int(math.ceil(math.sqrt(N))) if width is None else int(math.ceil(N / float(width)))
    if width is None:
        width = int(math.ceil(N / float(height)))
    if height * width < N:
        raise ValueError('a grid of %d x %d holds fewer than %d images' % (height, width, N))
    rest = tuple(t.shape[3:])
    full = torch.full((height * width, t.shape[1] + padsize, t.shape[2] + padsize) + rest, padval, dtype=t.dtype, device=t.device)
    full[:N, :t.shape[1], :t.shape[2]] = t
    full = full.reshape((height, width) + tuple(full.shape[1:]))
    full = full.permute((0, 2, 1, 3) + tuple(range(4, full.dim())))
    sheet = full.reshape((height * full.shape[1], width * full.shape[3]) + rest)
    return sheet.numpy() if is_np else sheet


def frame_bytes(images):
    """Frames as uint8: uint8 goes through, the loader's float images in [0, 1] come back as ``rint(img * 255)``."""
    if torch.is_tensor(images):
        if images.dtype == torch.uint8:
            return images
        images = images.cpu().numpy()
    images = np.asarray(images)
    if images.dtype == np.uint8:
        return images
    return np.rint(images.astype(np.float32) * np.float32(255.0)).clip(0, 255).astype(np.uint8)


def visualize_outputs(images, gt_gazemap, pred_gazemap, alpha=0.4, colormap='jet', limits=None, padsize=1, padval=0, device=None):
    """images [n, H, W, 3] (uint8, or float in [0, 1]), gt_gazemap and pred_gazemap [n, h, w] -> the contact sheet, a uint8
    device tensor [3 * (H + padsize), n * (W + padsize), 3]: row 0 the frames, row 1 the predictions over them, row 2 the
    ground truth over them."""
    frames = frame_bytes(images)
    if not (torch.is_tensor(frames) and frames.is_cuda):              # uploaded once, read by both calls and by the sheet
        dev = torch.device('cuda:0' if device is None else device)
        frames = (frames if torch.is_tensor(frames) else torch.from_numpy(np.ascontiguousarray(frames))).contiguous().to(dev)

    def maps32(m):
        return m.to(torch.float32).contiguous() if torch.is_tensor(m) else np.ascontiguousarray(np.asarray(m), np.float32)
    pred = overlay_maps(frames, maps32(pred_gazemap), alpha=alpha, colormap=colormap, limits=limits, device=frames.device)
    gt = overlay_maps(frames, maps32(gt_gazemap), alpha=alpha, colormap=colormap, limits=limits, device=frames.device)
    n = int(pred.shape[0])
    return tile_grid(torch.cat([frames[:n], pred, gt]), height=3, width=max(n, 1), padsize=padsize, padval=padval)


def visualize_outputs_of(model, dataset, max_instances=100):
    """visualize_output.py:58-81: run the model over ``dataset`` and draw its outputs.  -> what ``model.generate`` returns,
    with the stacked 'pred_gazemaps', 'gt_gazemaps' and 'images' and the contact sheet under 'sheet'."""
    ret = model.generate(dataset, max_instances=max_instances)
    pred_gazemaps = ret['pred_gazemaps'] = np.asarray(ret['pred_gazemap_list'])
    gt_gazemaps = ret['gt_gazemaps'] = np.asarray(ret['gt_gazemap_list'])
    images = ret['images'] = np.asarray(ret['images_list'])
    ret['sheet'] = visualize_outputs(images, gt_gazemaps, pred_gazemaps)
    return ret


__all__ = ['tile_grid', 'frame_bytes', 'visualize_outputs', 'visualize_outputs_of']
