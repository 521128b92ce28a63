"""GPU: the original-scale ground-truth maps (csrc/rgp_gtmaps_full.hip through gazemaps.gazemaps_original_scale) against
the numpy oracle of tests/gtmaps_ref.py, which tests/test_gtmaps_full_cpu.py pins to scipy at these shapes and sigmas.

Every operation behind `fixationmaps` and `gazemaps` is IEEE, element-wise, a sum in a prescribed order with host-made
weights, or a min / max: the claim is equality (torch.equal, a NaN equal to a NaN in the same place), not a tolerance.
The cases are tests/gtmaps_full_cases.py's."""
import numpy as np
import pytest
import torch

import gtmaps_full_cases as cases
from recurrent_gaze_prediction_amd import _lib
from recurrent_gaze_prediction_amd import gazemaps as gm

pytestmark = pytest.mark.gpu

OUTPUTS = ('gazemaps', 'fixationmaps')


def same(t, a):
    """torch.equal, a NaN equal to a NaN in the same place (a constant non-zero frame is NaN on both sides)."""
    t, a = t.cpu(), torch.from_numpy(np.array(a))
    return t.shape == a.shape and torch.equal(torch.isnan(t), torch.isnan(a)) and torch.equal(torch.nan_to_num(t, nan=0.0), torch.nan_to_num(a, nan=0.0))


def sub(packed, lo, hi):
    fp = packed.frame_ptr
    return packed._replace(frame_ptr=fp[lo:hi + 1] - fp[lo], samples=packed.samples[fp[lo]:fp[hi]])


@pytest.mark.parametrize('name', cases.ORACLE_CASES)
def test_maps_equal_the_oracle(gpu, name):
    packed, sigma = cases.case(name)
    fix, gaze = cases.oracle(name)
    N, (D1, D2) = len(packed.frame_ptr) - 1, packed.raw_shape
    out = gm.gazemaps_original_scale(packed, sigma=sigma, device=gpu)
    assert set(out) == set(OUTPUTS)
    for t in out.values():
        assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (N, D2, D1)
    assert same(out['fixationmaps'], fix), (out['fixationmaps'].cpu().numpy() != fix).sum()
    d_gaze = out['gazemaps'].cpu().numpy()
    diff = ~((d_gaze == gaze) | (np.isnan(d_gaze) & np.isnan(gaze)))
    with np.errstate(invalid='ignore'):
        worst = np.nanmax(np.abs(d_gaze - gaze)) if not np.isnan(d_gaze - gaze).all() else 0.0
    print('%s: raw %s sigma %g, %d observers: %d of %d gaze cells differ, max |d| %.3g'
          % (name, packed.raw_shape, sigma, packed.n_observers, diff.sum(), diff.size, worst))
    assert same(out['gazemaps'], gaze)
    # a call that wants one output gives the same bits for it
    for k in OUTPUTS:
        only = gm.gazemaps_original_scale(packed, sigma=sigma, want=k, device=gpu)
        assert set(only) == {k} and same(only[k], out[k].cpu().numpy()), k


def test_default_sigma_is_the_loaders(gpu):
    packed, sigma = cases.case('obs5')
    assert sigma == gm.SIGMA_ORIGINAL_SCALE
    assert same(gm.gazemaps_original_scale(packed, device=gpu)['gazemaps'], cases.oracle('obs5')[1])


def test_equals_the_one_launch_entry_where_both_apply(gpu):
    packed, sigma = cases.case('cross')
    ours = gm.gazemaps_original_scale(packed, sigma=sigma, device=gpu)
    theirs = gm.gazemaps_from_fixations(packed, out_shape=packed.raw_shape, sigma=sigma, device=gpu)
    assert float(theirs['gazemaps'].max()) == 1.0
    for k in OUTPUTS:
        assert torch.equal(ours[k], theirs[k]), k


def test_frames_are_independent(gpu):
    packed, sigma = cases.case('obs5')
    N = cases.N
    full = gm.gazemaps_original_scale(packed, sigma=sigma, device=gpu)
    again = gm.gazemaps_original_scale(packed, sigma=sigma, device=gpu)
    part = gm.gazemaps_original_scale(sub(packed, 5, 12), sigma=sigma, device=gpu)
    for k in OUTPUTS:
        assert torch.equal(again[k], full[k]), k               # the atomics are order-free
        assert tuple(part[k].shape)[0] == 7 and torch.equal(part[k], full[k][5:12]), k
    for per_call in (1, 5, N):
        split = gm.gazemaps_original_scale(packed, sigma=sigma, device=gpu, frames_per_call=per_call)
        for k in OUTPUTS:
            assert torch.equal(split[k], full[k]), (k, per_call)


def test_no_frames(gpu):
    empty = gm.PackedFixations(np.zeros(1, np.int32), np.zeros((0, 3), np.int32), 5, cases.RAW)
    out = gm.gazemaps_original_scale(empty, device=gpu)
    assert tuple(out['gazemaps'].shape) == (0, cases.RAW[1], cases.RAW[0])
    # frames, but not one sample
    blank = gm.PackedFixations(np.zeros(4, np.int32), np.zeros((0, 3), np.int32), 5, cases.RAW)
    out = gm.gazemaps_original_scale(blank, device=gpu)
    assert float(out['gazemaps'].abs().max()) == 0 and float(out['fixationmaps'].abs().max()) == 0


@pytest.mark.parametrize('column, value', [(1, 97), (1, -1), (2, 61), (2, -3), (0, 5), (0, -1)])
@pytest.mark.parametrize('per_call', [None, 5])
def test_a_bad_sample_refuses_its_frame_only(gpu, column, value, per_call):
    """Input validation on the device: the frame with an out-of-range a (b, observer id) is NaN in every output and
    counted in the status word, the other frames are computed, and the next clean call returns normally.  The value is
    checked before it is used; nothing here reaches an address."""
    bad_frame = 7
    packed, sigma = cases.case('obs5')
    fix, gaze = cases.oracle('obs5')
    samples = packed.samples.copy()
    samples[packed.frame_ptr[bad_frame] + 1, column] = value
    with pytest.raises(_lib.RgpError) as info:
        gm.gazemaps_original_scale(packed._replace(samples=samples), sigma=sigma, device=gpu, frames_per_call=per_call)
    assert info.value.code == -1 and '1 frame(s) refused' in str(info.value)               # RGP_EINVAL
    out = info.value.outputs
    rest = np.arange(cases.N) != bad_frame
    for k in OUTPUTS:
        assert bool(torch.isnan(out[k][bad_frame]).all()), k
    assert same(out['gazemaps'][rest], gaze[rest]) and same(out['fixationmaps'][rest], fix[rest])
    clean = gm.gazemaps_original_scale(packed, sigma=sigma, device=gpu, frames_per_call=per_call)   # does not raise
    assert same(clean['gazemaps'], gaze) and same(clean['fixationmaps'], fix)


def test_a_bad_frame_ptr_pair_refuses_its_frame_only(gpu):
    """Straight to the C entry (the Python wrapper refuses a decreasing frame_ptr itself): frame 1's pair decreases."""
    import ctypes
    packed, sigma = cases.case('obs5')
    fix, gaze = cases.oracle('obs5')
    D1, D2 = packed.raw_shape
    fp = packed.frame_ptr[:5].copy()                       # frames 0 .. 3
    fp[2] = fp[1] - 1 if fp[1] > 0 else -1                 # pair (fp[1], fp[2]) decreases or is negative: frame 1 refused;
    w, r = gm.gaussian_weights(sigma)                      # frame 2 then starts at fp[2] < its own start: also checked below
    lib = _lib.load()
    d_ptr, d_s = torch.from_numpy(fp).to(gpu), torch.from_numpy(packed.samples).to(gpu)
    d_w = torch.from_numpy(w).to(gpu)
    g = torch.empty((4, D2, D1), dtype=torch.float32, device=gpu)
    f = torch.empty_like(g)
    ws = torch.empty(lib.rgp_gtmaps_full_workspace_bytes(4, D1, D2), dtype=torch.uint8, device=gpu)
    args = _lib.GtmapsFullArgs(frame_ptr=d_ptr.data_ptr(), samples=d_s.data_ptr(), weights=d_w.data_ptr(), n_frames=4,
                               n_observers=5, raw_d1=D1, raw_d2=D2, radius=r, gazemaps=g.data_ptr(), fixationmaps=f.data_ptr(),
                               workspace=ws.data_ptr(), workspace_bytes=ws.numel())
    stream = torch.cuda.current_stream(gpu).cuda_stream
    assert lib.rgp_gazemaps_full_from_fixations(ctypes.byref(args), stream) == 0
    refused = ctypes.c_int(-7)
    assert fp[1] == 0 and fp[2] == -1                      # frame 0 is the empty one: frame 1 = (0, -1), frame 2 = (-1, ..)
    assert lib.rgp_gtmaps_full_status(ws.data_ptr(), ctypes.byref(refused), stream) == -1 and refused.value == 2
    assert b'2 frame(s) refused' in lib.rgp_last_error()
    assert bool(torch.isnan(g[1:3]).all()) and bool(torch.isnan(f[1:3]).all())
    assert same(g[[0, 3]], gaze[[0, 3]]) and same(f[[0, 3]], fix[[0, 3]])
