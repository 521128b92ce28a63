"""CPU: the LDS layout and the tile order of conv2a's inference forward, by enumeration (scripts/check_conv2a_layout.py)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _checker():
    spec = importlib.util.spec_from_file_location('check_conv2a_layout', os.path.join(ROOT, 'scripts', 'check_conv2a_layout.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_row_fetch_feeds_every_fragment_read_without_bank_conflicts():
    """DMA destinations, fragment bases and the immediates of all 27 taps:
    every read finds the chunk its tap wants, and every ds_read_b128 lane group hits 16 different 16-byte slots."""
    _checker().check_layout()


@pytest.mark.parametrize('n', list(range(1, 41)) + [1024])
def test_tile_order_visits_every_tile_once_and_keeps_neighbours_and_short_tiles_even(n):
    """decode(): every (window, zp, yp) exactly once; (a) zp- and yp-neighbours inside a lockstep round; (b) every CU of an
    XCD gets each pooled plane once in any 8 consecutive rounds (two short tiles)."""
    assert _checker().check_order(n)


def test_decode_model_matches_the_kernel_source():
    """the model is only worth something while the kernel computes the same thing: pin the two lines it mirrors"""
    src = open(os.path.join(ROOT, 'recurrent_gaze_prediction_amd', 'csrc', 'conv_patch.hip.h')).read()
    assert 'yp = r >> 3;' in src and 'zp = ((r & 7) + (tile >> 5)) & 7;' in src
