"""Mirror of /root/reference/salicon_input_data.py: SaliconDataset, read_salicon_data_set and SaliconData, the
loader of the ShallowNet pre-training (models/saliency_shallownet.py).

The host form is the reference's: float32 images and saliency maps in [0, 1], fixation maps at their raw scale as an
object array of scipy.sparse matrices, a permutation cursor (``next_batch``).  The device form keeps the decoded set as
uint8 on the GPU (``images_u8``, ``maps_u8``: a quarter of the float32 bytes) and makes a whole batch -- gather, flip
augmentation, scaling by 1 / 255 -- in one launch of rgp_salicon_batch (``next_batch_device``).  A file of another size
than the target is resized as the reference does (Pillow's antialiased resize, now called LANCZOS); with a ``device``
that resize runs on the GPU (frames.frame_images, the same bytes)."""
import os
from os import listdir
from os.path import isfile, join

import numpy as np
import scipy.sparse

SHUFFLE_SEED = 3024202          # salicon_input_data.py:34


def gather_filenames(folder_path):
    return [f for f in listdir(folder_path) if isfile(join(folder_path, f))]


class SaliconDataset(object):
    """salicon_input_data.py:21-72.  images [N,H,W,3] and saliencymaps [N,h,w] float32 in [0,1], fixationmaps an object
    array of N sparse matrices (or None)."""

    def __init__(self, images, saliencymaps, fixationmaps=None):
        self.images = images
        self.saliencymaps = saliencymaps
        self.fixationmaps = fixationmaps
        self.epochs_completed = 0
        self.index_in_epoch = 0
        assert self.image_count() > 0
        self.batch_perm = list(range(self.image_count()))
        np.random.RandomState(SHUFFLE_SEED).shuffle(self.batch_perm)
        self.images_u8 = self.maps_u8 = self._batcher = None

    def __len__(self):
        return self.image_count()

    def image_count(self):
        return len(self.images)

    def __repr__(self):
        return '<SaliconDataSet with %d images>' % self.image_count()

    def image_shape(self):
        return self.images[0].shape

    def saliencymaps_shape(self):
        return self.saliencymaps[0].shape

    def _next_indices(self, batch_size):
        """The cursor of next_batch (:52-69): past the end of the epoch the permutation is drawn again (numpy's global
        RNG, as in the reference), the batch restarts at 0 and the partial batch is dropped."""
        start = self.index_in_epoch
        self.index_in_epoch += batch_size
        if self.index_in_epoch > self.image_count():
            self.epochs_completed += 1
            self.batch_perm = list(range(self.image_count()))
            np.random.shuffle(self.batch_perm)
            start = 0
            self.index_in_epoch = batch_size
            assert batch_size <= self.image_count()
        return self.batch_perm[start:self.index_in_epoch]

    def _fixations(self, indices):
        return self.fixationmaps[indices] if self.fixationmaps is not None else None

    def next_batch(self, batch_size):
        idx = self._next_indices(batch_size)
        return self.images[idx], self.saliencymaps[idx], self._fixations(idx)

    # ---- device form ---------------------------------------------------------------------------------------------
    def to_device(self, device, images_u8=None, maps_u8=None):
        """Makes the set resident on ``device`` as uint8.  Without the decoded bytes they are recovered from the float32
        arrays, which must be bytes / 255 exactly (what the loader makes).  Returns self."""
        import torch
        from .engine import SaliconBatcher

        def as_bytes(given, scaled, what):
            if given is not None:
                b = np.ascontiguousarray(given)
                assert b.dtype == np.uint8 and b.shape == tuple(np.shape(scaled)), what
                return b
            x = np.asarray(scaled, np.float32)
            b = np.rint(x * np.float32(255.0)).astype(np.uint8)
            if not np.array_equal(np.multiply(b.astype(np.float32), 1.0 / 255.0).astype(np.float32), x):
                raise ValueError('%s are not uint8 values scaled by 1 / 255: the device form keeps bytes' % what)
            return b
        dev = torch.device(device)
        self.images_u8 = torch.from_numpy(as_bytes(images_u8, self.images, 'images')).to(dev)
        self.maps_u8 = torch.from_numpy(as_bytes(maps_u8, self.saliencymaps, 'saliencymaps')).to(dev)
        self._batcher = SaliconBatcher(self.images_u8, self.maps_u8)
        return self

    @property
    def on_device(self):
        return self._batcher is not None

    def next_batch_device(self, batch_size, flip=None):
        """next_batch on the device: advances the same cursor; -> (images [B,H,W,3], saliencymaps [B,h,w]) float32 device
        tensors and the fixation maps of the batch.  flip: [B] bytes / bools, a set one mirrors that sample (image and
        map) along the width; None: the values of next_batch exactly."""
        if self._batcher is None:
            raise RuntimeError('the set is not on a device: call to_device(device) first')
        idx = self._next_indices(batch_size)
        images, maps = self._batcher.batch(np.asarray(idx, np.int32), flip, check=False)     # the cursor's own indices
        return images, maps, self._fixations(idx)


def _resize_host(pil_images, size):
    from PIL import Image
    return [np.array(im.resize(size, Image.LANCZOS)) for im in pil_images]


def _resize_device(arrays, size, device):
    """uint8 arrays [h,w,3] or [h,w] of ONE shape -> resized to size = (width, height) by frames.frame_images.  A
    single-channel map goes through as three equal channels (the channels are independent) and channel 0 comes back."""
    from . import frames
    x = np.stack(arrays)
    grey = x.ndim == 3
    if grey:
        x = np.repeat(x[..., None], 3, axis=-1)
    out = frames.frame_images(np.ascontiguousarray(x), (size[1], size[0]), out='uint8', device=device).cpu().numpy()
    return list(out[..., 0] if grey else out)


def _decode(paths, mode, size, device):
    """Files -> list of uint8 arrays of the target size = (width, height); files of another size are resized, grouped by
    their own size when that runs on the device."""
    from PIL import Image
    out, odd = [None] * len(paths), {}
    for i, path in enumerate(paths):
        with Image.open(path) as f:
            im = f.convert(mode)
        if im.size == tuple(size):
            out[i] = np.array(im)
        else:
            print('WARN: resizing %s ...' % os.path.basename(path))
            odd.setdefault(im.size, []).append((i, im))
    for _, group in odd.items():
        ims = [im for _, im in group]
        res = _resize_host(ims, size) if device is None else _resize_device([np.array(im) for im in ims], size, device)
        for (i, _), r in zip(group, res):
            out[i] = r
    return out


def read_salicon_data_set(image_folder_path, saliencymap_folder_path, fixationmap_folder_path, image_height, image_width,
                          saliencymap_height, saliencymap_width, device=None):
    """salicon_input_data.py:75-131: every file of the image folder (sorted), its saliency map of the same name and its
    fixation map ``<name>.npy`` -> SaliconDataset (float32 in [0, 1]; fixation maps sparse, raw scale).  With a
    ``device`` the resizes run there and the returned set is also resident on it (to_device)."""
    filenames = sorted(gather_filenames(image_folder_path))
    images = _decode([join(image_folder_path, f) for f in filenames], 'RGB', (image_width, image_height), device)
    maps = _decode([join(saliencymap_folder_path, f) for f in filenames], 'L', (saliencymap_width, saliencymap_height), device)
    fixationmaps = np.empty(len(filenames), dtype=object)
    for i, f in enumerate(filenames):
        fixationmaps[i] = scipy.sparse.csr_matrix(np.load(join(fixationmap_folder_path, f + '.npy')), dtype=np.float32)
    images_u8, maps_u8 = np.stack(images, axis=0), np.stack(maps, axis=0)
    data = SaliconDataset(np.multiply(images_u8.astype(np.float32), 1.0 / 255.0),
                          np.multiply(maps_u8.astype(np.float32), 1.0 / 255.0), fixationmaps)
    if device is not None:
        data.to_device(device, images_u8, maps_u8)
    return data


class SaliconData(object):
    """salicon_input_data.py:134-212: the train / valid / test sets under ``root`` (the reference's folder layout).
    build() returns self (the reference returns None, which its own caller then dereferences)."""

    def __init__(self, image_height, image_width, saliencymap_height, saliencymap_width, dtype=np.float32,
                 use_example=False, use_val_split=False, root='salicon/', device=None):
        self.image_height, self.image_width = image_height, image_width
        self.saliencymap_height, self.saliencymap_width = saliencymap_height, saliencymap_width
        self.dtype = dtype
        self.use_example = use_example
        self.use_val_split = use_val_split
        self.root, self.device = root, device
        self.train = self.valid = self.test = None

    def _read(self, images, maps, fixations):
        return read_salicon_data_set(join(self.root, images), join(self.root, maps), join(self.root, fixations),
                                     self.image_height, self.image_width, self.saliencymap_height, self.saliencymap_width,
                                     device=self.device)

    def build(self):
        print('loading data set ...')
        if self.use_example:
            self.train = self._read('images/train2014examples/', 'saliencymaps/train2014examples/',
                                    'fixations/train2014examples/')
        else:
            self.train = self._read('images/train98x98/', 'saliencymaps/train49x49/', 'fixations/train/')
            # SALICON has no public test set: the validation set serves as one
            self.test = self._read('images/val98x98/', 'saliencymaps/val49x49/', 'fixations/val/')
        if self.use_val_split:
            import sklearn.model_selection
            parts = sklearn.model_selection.train_test_split(self.train.images, self.train.saliencymaps,
                                                             self.train.fixationmaps, test_size=0.2)
            self.train = SaliconDataset(parts[0], parts[2], parts[4])
            self.valid = SaliconDataset(parts[1], parts[3], parts[5])
            if self.device is not None:
                self.train.to_device(self.device)
                self.valid.to_device(self.device)
        else:
            self.valid = self.test
        print('Done.')
        return self


__all__ = ['SHUFFLE_SEED', 'gather_filenames', 'SaliconDataset', 'read_salicon_data_set', 'SaliconData']
