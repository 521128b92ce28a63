"""The cases of the frame-image tests (test_frames_cpu.py, test_frames_gpu.py): geometries, frame contents, and the
oracle's images of each, computed once per process (tests/frames_ref.py).

Geometries, (H, W) -> (out_h, out_w):
  odd       37 x 53 -> 11 x 7: rows of 159 bytes and frames of 5883 bytes, so frame 1 starts at an odd address
  up        20 x 24 -> 49 x 31: an upscale (ksize 7 / 3 / 5)
  rows      64 x 98 -> 16 x 98: the horizontal pass is skipped
  cols      98 x 64 -> 98 x 16: the vertical pass is skipped
  copy      98 x 98 -> 98 x 98: both skipped
  video     405 x 720 -> 98 x 98, 3 frames (the driver's geometry)
  video112  405 x 720 -> 112 x 112, 3 frames
  hd        1080 x 1920 -> 98 x 98, 1 frame (ksize 119 horizontally)
Contents: 'random' bytes, constant 255, constant 0, and 'blocks': random rectangles of 0 and 255, which drive the
negative lobes of Lanczos and the bicubic past both clamps.  The small cases hold the four in this order; the large
ones say what they hold below."""
import functools

import numpy as np

import frames_ref

FILTERS = ('lanczos', 'bilinear', 'bicubic')
CONTENTS = ('random', 'white', 'black', 'blocks')

# name -> (H, W, out_h, out_w, contents per frame, filters)
GEOMETRY = {
    'odd': (37, 53, 11, 7, CONTENTS, FILTERS),
    'up': (20, 24, 49, 31, CONTENTS, FILTERS),
    'rows': (64, 98, 16, 98, CONTENTS, FILTERS),
    'cols': (98, 64, 98, 16, CONTENTS, FILTERS),
    'copy': (98, 98, 98, 98, CONTENTS, FILTERS),
    'video': (405, 720, 98, 98, ('random', 'blocks', 'halves'), ('lanczos',)),
    'video112': (405, 720, 112, 112, ('random', 'blocks', 'halves'), ('lanczos',)),
    'hd': (1080, 1920, 98, 98, ('mixed',), ('lanczos',)),
}
SMALL = ('odd', 'up', 'rows', 'cols', 'copy')
CASES = [(name, f) for name, g in GEOMETRY.items() for f in g[5]]
IDS = ['%s-%s' % c for c in CASES]
BANDS = (1, 2, 3, 'out_h')


def _blocks(rs, H, W):
    """Rectangles of 0 and 255 a few filter supports wide, so that a lobe sees a full step on either side."""
    side_h, side_w = max(2, H // 9), max(2, W // 9)
    coarse = rs.randint(0, 2, size=((H + side_h - 1) // side_h, (W + side_w - 1) // side_w, 3)).astype(np.uint8) * 255
    return np.repeat(np.repeat(coarse, side_h, axis=0), side_w, axis=1)[:H, :W]


def _content(kind, rs, H, W):
    if kind == 'random':
        return rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    if kind == 'white':
        return np.full((H, W, 3), 255, np.uint8)
    if kind == 'black':
        return np.zeros((H, W, 3), np.uint8)
    if kind == 'blocks':
        return _blocks(rs, H, W)
    if kind == 'halves':                       # 255 above, 0 below: two constant regions and one edge
        img = np.zeros((H, W, 3), np.uint8)
        img[:H // 2] = 255
        return img
    if kind == 'mixed':                        # random bytes on the left, blocks on the right
        img = rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
        img[:, W // 2:] = _blocks(rs, H, W)[:, W // 2:]
        return img
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def frames(name):
    """uint8 [N, H, W, 3], read-only."""
    H, W, _, _, contents, _ = GEOMETRY[name]
    rs = np.random.RandomState(sorted(GEOMETRY).index(name) + 220)
    out = np.stack([_content(kind, rs, H, W) for kind in contents])
    out.setflags(write=False)
    return out


def out_hw(name):
    return GEOMETRY[name][2:4]


@functools.lru_cache(maxsize=None)
def oracle(name, filt):
    """-> (uint8 [N, oh, ow, 3], float32 [N, oh, ow, 3]) of frames_ref, read-only."""
    u8, f32 = frames_ref.loader_images(frames(name), out_hw(name), None, filt)
    u8.setflags(write=False)
    f32.setflags(write=False)
    return u8, f32


def band_requests(name):
    return [out_hw(name)[0] if b == 'out_h' else b for b in BANDS]
