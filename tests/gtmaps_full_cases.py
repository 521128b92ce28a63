"""Cases shared by tests/test_gtmaps_full_cpu.py and tests/test_gtmaps_full_gpu.py: the packed fixations, raw shapes and
sigmas the original-scale entry (gazemaps.gazemaps_original_scale, csrc/rgp_gtmaps_full.hip) is held to, and their
oracle (tests/gtmaps_ref.py with out_shape == raw_shape), computed once per case and never written to."""
import functools

import numpy as np

import gtmaps_ref as ref
from recurrent_gaze_prediction_amd import _lib
from recurrent_gaze_prediction_amd import gazemaps as gm

RAW = (97, 61)                  # radius 76 exceeds the 61 (the reflection repeats) and stays under the 97
N = 24
EMPTY, ONE, TWICE, SHARED, CORNERS, MANY = 0, 1, 2, 3, 4, 5            # the frames made by construction
# one more than a multiple of every tile extent of either filter pass, in both axes
TILE_RAW = (_lib.RGP_GTMAPS_FULL_TILE_COLS + 1, _lib.RGP_GTMAPS_FULL_TILE_ROWS + 1)
WORKLOAD_RAW = (720, 405)
SIGMA_ABOVE_LDS = 40            # radius 160 > RGP_GTMAPS_FULL_LDS_RADIUS: the taps are read through the caches


def pack(frames, n_obs, raw):
    frame_ptr = np.cumsum([0] + [len(f) for f in frames]).astype(np.int32)
    samples = np.array([s for f in frames for s in f], np.int32).reshape(-1, 3)
    return gm.PackedFixations(frame_ptr, samples, n_obs, raw)


def constructed(n_obs, raw, rs):
    """The frame kinds of tests/test_gtmaps_gpu.py on a raw frame of any size: empty, one sample, an observer twice in
    one cell, all observers in one cell, the four corners, 300 samples."""
    D1, D2 = raw
    last = n_obs - 1
    frames = [[] for _ in range(MANY + 1)]
    frames[ONE] = [(last, D1 // 3, D2 // 4)]
    frames[TWICE] = [(0, 8 % D1, D2 // 3), (0, 8 % D1, D2 // 3), (last, D1 // 2, 1)]
    frames[SHARED] = [(u, (2 * D1) // 5, D2 // 2) for u in range(n_obs)] + [(0, D1 - 1, 0)]
    corners = [(0, 0), (D1 - 1, 0), (0, D2 - 1), (D1 - 1, D2 - 1)]
    frames[CORNERS] = [(k % n_obs, a, b) for k, (a, b) in enumerate(corners)] + [(last, a, b) for a, b in corners[:2]]
    frames[MANY] = [(rs.randint(n_obs), rs.randint(D1), rs.randint(D2)) for _ in range(300)]
    return frames


def scattered(n_frames, n_obs, raw, rs):
    return [[(u, rs.randint(raw[0]), rs.randint(raw[1])) for u in range(n_obs) for _ in range(rs.randint(1, 4))]
            for _ in range(n_frames)]


@functools.lru_cache(maxsize=None)
def fixations(n_obs):
    """24 frames on raw 97 x 61: the six constructed ones, then 18 of one to three samples per observer."""
    rs = np.random.RandomState(200 + n_obs)
    frames = constructed(n_obs, RAW, rs) + scattered(N - MANY - 1, n_obs, RAW, rs)
    return pack(frames, n_obs, RAW)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (packed, sigma)"""
    rs = np.random.RandomState(sum(map(ord, name)))
    if name in ('obs1', 'obs5', 'obs32'):
        return fixations(int(name[3:])), 19
    if name == 'tiny53':            # extents far below the radius
        return pack(constructed(3, (5, 3), rs), 3, (5, 3)), 19
    if name == 'tiny22':            # 2 x 2: the 300 samples of one observer cover every cell, a constant frame: NaN
        return pack(constructed(1, (2, 2), rs), 1, (2, 2)), 19
    if name == 'odd':               # odd extents over several tiles
        return pack(scattered(3, 5, (257, 131), rs), 5, (257, 131)), 5
    if name == 'tile_plus_one':
        frames = scattered(2, 5, TILE_RAW, rs) + [[(0, TILE_RAW[0] - 1, TILE_RAW[1] - 1)]]
        return pack(frames, 5, TILE_RAW), 19
    if name == 'workload':          # 405 x 720 frames, sigma 19: empty, one corner sample, 16 observers at random
        D1, D2 = WORKLOAD_RAW
        frames = [[], [(3, D1 - 1, 0)], [(u, rs.randint(D1), rs.randint(D2)) for u in range(16)]]
        return pack(frames, 16, WORKLOAD_RAW), 19
    if name == 'above_lds':
        return pack(scattered(2, 5, (257, 131), rs), 5, (257, 131)), SIGMA_ABOVE_LDS
    if name == 'cross':             # where gazemaps_from_fixations applies too: 61 x 47 = 2867 cells, radius 8
        return pack(constructed(5, (61, 47), rs) + scattered(4, 5, (61, 47), rs), 5, (61, 47)), 2.0
    raise KeyError(name)


ORACLE_CASES = ('obs1', 'obs5', 'obs32', 'tiny53', 'tiny22', 'odd', 'tile_plus_one', 'workload', 'above_lds')


@functools.lru_cache(maxsize=None)
def counts(name):
    p, _ = case(name)
    c = ref.fixation_counts(p.frame_ptr, p.samples, p.n_observers, p.raw_shape, p.raw_shape)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(fixationmaps fp32, gazemaps fp32) [N, D2, D1]"""
    p, sigma = case(name)
    c = counts(name)
    fix, gaze = c.astype(np.float32), ref.gazemaps_from_counts(c, p.n_observers, sigma)
    fix.setflags(write=False)
    gaze.setflags(write=False)
    return fix, gaze
