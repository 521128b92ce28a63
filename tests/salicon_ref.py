"""References of the SALICON pre-training tests (tests/test_salicon_cpu.py, tests/test_salicon_gpu.py): the batch of
rgp_salicon_batch in numpy, the ShallowNet with its dropout site in float64 torch, the total loss of
saliency_shallownet.py:246-250, and a small synthetic image set."""
import numpy as np
import scipy.sparse
import torch
import torch.nn.functional as F

from oracle import torch_ref

KEEP = 0.4                      # saliency_shallownet.py:330
BIASES = {'conv1_b': (-0.1, 0.1, 32), 'conv2_b': (0.05, -0.05, 64), 'conv3_b': (-0.02, 0.03, 32),
          'fc1_b': (-0.05, 0.05, 4802), 'fc2_b': (0.05, -0.05, 4802)}


def with_biases(p):
    """The synthetic initialisation has zero biases: give every one a value, so that a bias's gradient, its regulariser
    and its place in a checkpoint all show."""
    return dict(p, **{k: np.linspace(a, b, n).astype(np.float32) for k, (a, b, n) in BIASES.items()})


def image_set(seed, n, hw, fix_shape=(60, 80)):
    """uint8 images [n,hw,hw,3] and maps [n,49,49] of random bytes (no symmetry: a row reversed byte-wise instead of
    pixel-wise, or a mirrored height, gives other values) and raw-scale sparse fixation maps."""
    rs = np.random.RandomState(seed)
    images = rs.randint(0, 256, size=(n, hw, hw, 3)).astype(np.uint8)
    maps = rs.randint(0, 256, size=(n, 49, 49)).astype(np.uint8)
    fix = np.empty(n, dtype=object)
    for i in range(n):
        dense = np.zeros(fix_shape, np.float32)
        dense[rs.randint(0, fix_shape[0], 12), rs.randint(0, fix_shape[1], 12)] = 1.0
        fix[i] = scipy.sparse.csr_matrix(dense)
    return images, maps, fix


def scaled(u8):
    """The loader's float32 values (salicon_input_data.py:123-129)."""
    return np.multiply(u8.astype(np.float32), 1.0 / 255.0)


def batch(images_u8, maps_u8, index, flip):
    """What rgp_salicon_batch makes of in-range indices (saliency_shallownet.py:310-311 for the flipped samples)."""
    images, maps = scaled(images_u8[index]), scaled(maps_u8[index])
    sel = np.flatnonzero(np.asarray(flip))
    images[sel] = images[sel][:, :, ::-1, :]
    maps[sel] = maps[sel][:, :, ::-1]
    return images, maps


def shallownet_forward(images_nhwc, p, keep_prob=1.0, drop_mask=None):
    """oracle.torch_ref.shallownet_forward with tf.nn.dropout on relu(fc1) before the maxout (:152-158): drop_mask
    [n, 4802] keep bytes in the layer's unit order, kept values / keep_prob."""
    pool = torch_ref._max_pool_same
    x = images_nhwc.permute(0, 3, 1, 2)
    x = pool(torch.relu(F.conv2d(x, p['conv1_w'].permute(3, 2, 0, 1), p['conv1_b'])), 2, 2)
    x = pool(torch.relu(F.conv2d(x, p['conv2_w'].permute(3, 2, 0, 1), p['conv2_b'])), 3, 2)
    x = pool(torch.relu(F.conv2d(x, p['conv3_w'].permute(3, 2, 0, 1), p['conv3_b'])), 3, 2)
    x = x.permute(0, 2, 3, 1).reshape(x.shape[0], -1)
    x = torch.relu(x @ p['fc1_w'] + p['fc1_b'])
    if drop_mask is not None and keep_prob < 1.0:
        x = x * torch.as_tensor(np.asarray(drop_mask).reshape(x.shape[0], 4802), dtype=x.dtype) / keep_prob
    x = torch.maximum(x[:, :2401], x[:, 2401:])
    x = torch.relu(x @ p['fc2_w'] + p['fc2_b'])
    x = torch.maximum(x[:, :2401], x[:, 2401:])
    return x.reshape(-1, 49, 49)


def losses(sal, gt, p, batch_size, l2_reg):
    """(target_loss, reg_loss) of saliency_shallownet.py:247-249: 2 l2_loss(sal - gt) / 2401 / batch_size and
    l2_reg * sum of l2_loss over all ten variables, tf.nn.l2_loss(t) = sum t^2 / 2."""
    target = 2.0 * 0.5 * ((sal - gt) ** 2).sum() / (49 * 49) / batch_size
    reg = l2_reg * sum(0.5 * (v ** 2).sum() for v in p.values())
    return target, reg


def rel_err(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30)


def grad_errors(got, ref):
    """(rms error / rms of the reference, max error / max of the reference, cosine) as tests/test_shallownet_gpu.py."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    rms = float(np.sqrt(((got - ref) ** 2).mean()) / np.sqrt((ref ** 2).mean()))
    cos = float((got * ref).sum() / np.sqrt((got ** 2).sum() * (ref ** 2).sum()))
    return rms, float(rel_err(got, ref)), cos
