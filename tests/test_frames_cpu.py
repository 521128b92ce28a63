"""CPU: the host side of the loader's frame images (recurrent_gaze_prediction_amd/frames.py, rgp_frame_images in
include/rgp.h) and the oracle the GPU tests compare with (tests/frames_ref.py).

frames_ref is pinned to Pillow bit for bit where Pillow is installed; resample_coeffs is pinned to frames_ref's tables;
the cases are shown to be what they are for (both clamps are reached in both passes, a constant frame stays constant);
the band planner and every refusal the host can make are checked through the library's host code, without a device."""
import ctypes
import os
import re

import numpy as np
import pytest

import frames_cases as cases
import frames_ref as ref
from recurrent_gaze_prediction_amd import _lib
from recurrent_gaze_prediction_amd import frames as fr

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'rgp.h')
# the shapes the recipe was first compared with Pillow at, beyond those of the cases: (in, out) per axis
MORE_AXES = [(300, 98), (400, 98), (49, 7), (24, 31), (20, 49), (98, 98)]


def axes():
    out = set(MORE_AXES)
    for H, W, oh, ow, _, _ in cases.GEOMETRY.values():
        out |= {(H, oh), (W, ow)}
    return sorted(out)


@pytest.mark.parametrize('name, filt', cases.CASES, ids=cases.IDS)
def test_the_oracle_equals_pillow(name, filt):
    Image = pytest.importorskip('PIL.Image')
    pil_filter = {'lanczos': Image.LANCZOS, 'bilinear': Image.BILINEAR, 'bicubic': Image.BICUBIC}[filt]
    oh, ow = cases.out_hw(name)
    u8, _ = cases.oracle(name, filt)
    for i, frame in enumerate(cases.frames(name)):
        pil = np.array(Image.fromarray(frame).resize((ow, oh), pil_filter))
        assert pil.shape == u8[i].shape and pil.dtype == np.uint8
        assert np.array_equal(pil, u8[i]), (name, filt, i, int((pil != u8[i]).sum()))


@pytest.mark.parametrize('filt', cases.FILTERS)
def test_resample_coeffs_equal_the_oracles_tables(filt):
    for in_size, out_size in axes():
        k, b, ksize = fr.resample_coeffs(in_size, out_size, filt)
        rk, rb, rksize = ref.tables(in_size, out_size, filt)
        assert ksize == rksize and k.dtype == np.int32 and b.dtype == np.int32
        assert k.shape == (out_size, ksize) and b.shape == (out_size, 2)
        assert np.array_equal(k, rk) and np.array_equal(b, rb), (in_size, out_size, filt)
        assert not k[np.arange(ksize)[None, :] >= b[:, 1:2]].any()           # zero past n
        # the int32 accumulator is exact: 255 sum|k| + 2^21 < 2^31, i.e. sum|k| / 2^22 < 2.007
        assert 255 * int(np.abs(k.astype(np.int64)).sum(axis=1).max()) + (1 << 21) < 1 << 31
    assert fr.resample_coeffs(720, 98, filt)[2] == {'lanczos': 47, 'bilinear': 17, 'bicubic': 31}[filt]
    assert fr.resample_coeffs(405, 98, filt)[2] == {'lanczos': 27, 'bilinear': 11, 'bicubic': 19}[filt]
    assert fr.resample_coeffs(20, 49, filt)[2] == {'lanczos': 7, 'bilinear': 3, 'bicubic': 5}[filt]
    assert fr.resample_coeffs(1920, 98, 'lanczos')[2] == 119


def test_resample_coeffs_refuses_an_accumulator_that_could_overflow(monkeypatch):
    # a filter of alternating weights +-8 sums to a small number but has sum|k| far above 2.007 once normalised
    monkeypatch.setattr(fr, '_filter', lambda name, x: np.where(np.floor(x * 4) % 2 == 0, 8.0, -7.5))
    with pytest.raises(ValueError, match='overflow'):
        fr.resample_coeffs(64, 16, 'lanczos')
    monkeypatch.undo()
    fr.resample_coeffs(64, 16, 'lanczos')
    with pytest.raises(ValueError):
        fr.resample_coeffs(64, 16, 'nearest')
    with pytest.raises(ValueError):
        fr.resample_coeffs(0, 16)


def test_the_cases_are_what_they_are_for():
    assert cases.frames('odd').shape == (4, 37, 53, 3) and cases.frames('odd')[0].nbytes == 5883    # frame 1 at an odd address
    assert cases.frames('odd').shape[2] * 3 == 159
    for name in cases.SMALL:
        assert tuple(cases.GEOMETRY[name][4]) == cases.CONTENTS
    for name, filt in cases.CASES:
        H, W, oh, ow, contents, _ = cases.GEOMETRY[name]
        u8, f32 = cases.oracle(name, filt)
        assert u8.shape == (len(contents), oh, ow, 3) and f32.dtype == np.float32
        for i, kind in enumerate(contents):
            if kind == 'white':
                assert (u8[i] == 255).all() and (f32[i] == 1.0).all()            # a constant frame stays constant
            if kind == 'black':
                assert (u8[i] == 0).all() and (f32[i] == 0.0).all()
            if kind == 'blocks' and filt != 'bilinear' and H > oh and W > ow:
                # the negative lobes overshoot a 0 / 255 step in both directions, in both passes: both clamps act
                sums = {}
                again = ref.resize(cases.frames(name)[i:i + 1], (oh, ow), filt, sums)
                assert np.array_equal(again[0], u8[i])
                for which in ('h', 'v'):
                    assert sums[which].min() < 0 and sums[which].max() > 255, (name, filt, which)
    # the passes that are skipped
    for name, skipped in (('rows', 'h'), ('cols', 'v')):
        sums = {}
        ref.resize(cases.frames(name)[:1], cases.out_hw(name), 'lanczos', sums)
        assert set(sums) == {'h', 'v'} - {skipped}
    assert np.array_equal(cases.oracle('copy', 'lanczos')[0], cases.frames('copy'))
    assert fr.resample_coeffs(1920, 98)[2] == 119 <= _lib.RGP_FRAMES_MAX_KSIZE


def test_the_scale_is_the_loaders_on_all_256_levels():
    levels = np.arange(256, dtype=np.uint8)
    images = levels.astype(np.float32)                  # crc_input_data_seq.py:208-209
    images = np.multiply(images, 1.0 / 255.0)
    assert images.dtype == np.float32
    assert np.array_equal(ref.scaled(levels), images)
    # the kernel's form: one fp32 multiply by the literal 0.003921569f = float32(1 / 255)
    assert np.float32(0.003921569) == np.float32(1.0 / 255.0)
    assert np.array_equal(levels.astype(np.float32) * np.float32(0.003921569), images)
    assert images[255] == 1.0 and images[0] == 0.0


def test_loader_frame_index():
    assert fr.loader_frame_index(40).tolist() == [15, 20, 25, 30, 35]
    assert fr.loader_frame_index(41).tolist() == [15, 20, 25, 30, 35, 40]
    assert fr.loader_frame_index(16).tolist() == [15]
    for n in (0, 7, 15):
        assert fr.loader_frame_index(n).tolist() == []
    paths = list(range(1039))
    assert fr.loader_frame_index(len(paths)).tolist() == paths[15:len(paths):5] == ref.loader_frame_index(1039).tolist()


@pytest.mark.parametrize('name', list(cases.GEOMETRY))
def test_band_plan_covers_the_rows_once_within_the_lds_budget(name):
    H, W, oh, ow, contents, filters = cases.GEOMETRY[name]
    for filt in filters:
        ksh = ref.tables(W, ow, filt)[2] if W != ow else 0
        bv, ksv = (ref.tables(H, oh, filt)[1:] if H != oh else (None, 0))
        for n_out in (len(contents), 1024):
            for request in [None] + cases.band_requests(name):
                bands, lds, mid_rows = fr.band_plan((H, W), (oh, ow), (ksh, ksv), n_out, request)
                assert len(bands) >= (request or 1) and len(bands) <= oh
                assert lds <= _lib.RGP_FRAMES_LDS_BYTES <= 160 * 1024
                covered = np.zeros(oh, np.int64)
                for r0, r1 in bands:
                    assert 0 <= r0 < r1 <= oh
                    covered[r0:r1] += 1
                    assert (r1 - r0) * ow * 3 <= _lib.RGP_FRAMES_STAGE_BYTES               # the band's output image
                    if bv is None:
                        assert r1 - r0 <= mid_rows
                    else:                                                                   # the band's input rows
                        ya, yb = int(bv[r0:r1, 0].min()), int((bv[r0:r1, 0] + bv[r0:r1, 1]).max())
                        assert yb - ya <= mid_rows <= H, (name, filt, request, r0, r1)
                assert (covered == 1).all(), (name, filt, request)
    # the driver's call keeps two workgroups on a CU
    bands, lds, _ = fr.band_plan((405, 720), (98, 98), (47, 27), 1024)
    assert lds <= _lib.RGP_FRAMES_LDS_TARGET and 2 * _lib.RGP_FRAMES_LDS_TARGET <= 160 * 1024


def header_defines():
    text = open(HEADER).read()
    found = {}
    for name, value in re.findall(r'#define (RGP_FRAMES_\w+) (\([^)]*\)|\S+)', text):
        found[name] = eval(value.replace('ll', ''))
    return found


def test_symbols_and_limits():
    lib = _lib.load()
    for name in ('rgp_frames_workspace_bytes', 'rgp_frame_images', 'rgp_frames_status', 'rgp_frames_plan'):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    names = ('RGP_FRAMES_MAX_OUT', 'RGP_FRAMES_MAX_KSIZE', 'RGP_FRAMES_MAX_IN_W', 'RGP_FRAMES_MAX_BYTES', 'RGP_FRAMES_LDS_BYTES',
             'RGP_FRAMES_LDS_TARGET', 'RGP_FRAMES_STAGE_BYTES')
    assert header_defines() == {k: getattr(_lib, k) for k in names}
    assert (_lib.RGP_FRAMES_MAX_OUT, _lib.RGP_FRAMES_MAX_KSIZE, _lib.RGP_FRAMES_MAX_BYTES) == (256, 128, 2 ** 40)
    assert lib.rgp_frames_workspace_bytes() >= 4
    # the entry accepts the geometries the issue names, with all three filters
    for H, W in ((405, 720), (1080, 1920)):
        for side in (98, 112):
            for filt in cases.FILTERS:
                ksh, ksv = fr.resample_coeffs(W, side, filt)[2], fr.resample_coeffs(H, side, filt)[2]
                for n_out in (1, 1024):
                    assert fr.band_plan((H, W), (side, side), (ksh, ksv), n_out)[1] <= _lib.RGP_FRAMES_LDS_BYTES


def good_args(**kw):
    p = ctypes.c_void_p(1 << 20)            # never dereferenced: every case here is refused before any device call
    a = dict(frames=p, n_frames=8, fh=405, fw=720, frame_index=None, n_out=8, out_h=98, out_w=98, kh=p, bh=p, ksize_h=47, kv=p,
             bv=p, ksize_v=27, bands=0, images=p, images_u8=p, workspace=p, workspace_bytes=64)
    a.update(kw)
    return _lib.FramesArgs(**a)


@pytest.mark.parametrize('kw, word', [
    (dict(n_out=-1), b'n_out'),
    (dict(n_frames=-1), b'n_frames'),
    (dict(n_frames=0), b'n_frames'),
    (dict(fh=0), b'fh'),
    (dict(fw=0), b'fw'),
    (dict(fw=_lib.RGP_FRAMES_MAX_IN_W + 1), b'RGP_FRAMES_MAX_IN_W'),
    (dict(out_h=0), b'out_h'),
    (dict(out_h=257), b'out_h'),
    (dict(out_w=0), b'out_w'),
    (dict(out_w=257), b'out_w'),
    (dict(ksize_h=0), b'ksize_h'),
    (dict(ksize_h=129), b'ksize_h'),
    (dict(ksize_v=0), b'ksize_v'),
    (dict(ksize_v=129), b'ksize_v'),
    (dict(kh=None), b'kh'),
    (dict(bh=None), b'bh'),
    (dict(kv=None), b'kv'),
    (dict(bv=None), b'bv'),
    (dict(bands=-1), b'bands'),
    (dict(bands=99), b'bands'),
    (dict(images=None, images_u8=None), b'both NULL'),
    (dict(frames=None), b'frames'),
    (dict(images=ctypes.c_void_p((1 << 20) + 2)), b'images'),
    (dict(workspace=None), b'workspace'),
    (dict(workspace_bytes=3), b'workspace'),
    (dict(workspace=ctypes.c_void_p((1 << 20) + 4)), b'workspace'),
    (dict(n_frames=2 ** 31 - 1, fh=2000, fw=2000), b'RGP_FRAMES_MAX_BYTES'),
    (dict(n_out=2 ** 31 - 1, out_h=256, out_w=256), b'RGP_FRAMES_MAX_BYTES'),
    (dict(n_out=2 ** 24, out_h=256, out_w=1, bands=256), b'workgroups'),
    # 1700 x 256 -> 1 x 256 with 128 taps a side: one output row needs 128 rows of 768 bytes beside 128 x 256 weights
    (dict(fh=1700, fw=2040, out_h=80, out_w=256, ksize_h=128, ksize_v=128), b'RGP_FRAMES_LDS_BYTES'),
])
def test_bad_arguments_are_refused_on_the_host(kw, word):
    lib = _lib.load()
    assert lib.rgp_frame_images(ctypes.byref(good_args(**kw)), None) == -1          # RGP_EINVAL
    assert word in lib.rgp_last_error(), lib.rgp_last_error()


def test_null_args_no_frames_and_skipped_passes():
    lib = _lib.load()
    assert lib.rgp_frame_images(None, None) == -1 and b'args' in lib.rgp_last_error()
    assert lib.rgp_frames_status(None, None, None) == -1 and b'workspace' in lib.rgp_last_error()
    # n_out == 0: RGP_OK, nothing is launched (and nothing else is looked at)
    assert lib.rgp_frame_images(ctypes.byref(good_args(n_out=0)), None) == 0
    assert lib.rgp_frame_images(ctypes.byref(good_args(n_out=0, frames=None, images=None, images_u8=None, workspace=None)), None) == 0
    # the tables of a skipped pass are not asked for: what refuses these calls is the missing workspace, after the tables
    for kw in (dict(fw=98, kh=None, bh=None, ksize_h=0), dict(fh=98, kv=None, bv=None, ksize_v=0)):
        assert lib.rgp_frame_images(ctypes.byref(good_args(workspace=None, **kw)), None) == -1
        assert b'workspace' in lib.rgp_last_error()
    # the planner's own answer for what it refuses
    lds = ctypes.c_int(-1)
    assert lib.rgp_frames_plan(405, 720, 98, 98, 47, 27, 8, 99, ctypes.byref(lds), None) == 0 and lds.value == 0
    assert lib.rgp_frames_plan(405, 720, 98, 98, 47, 129, 8, 0, None, None) == 0


def test_python_refusals_need_no_device():
    frames = np.zeros((2, 37, 53, 3), np.uint8)
    bad = [
        (dict(frames=np.zeros((2, 37, 53, 4), np.uint8)), 'channels'),
        (dict(frames=np.zeros((2, 37, 53), np.uint8)), 'uint8'),
        (dict(frames=np.zeros((2, 37, 53, 3), np.float32)), 'uint8'),
        (dict(out_hw=(257, 98)), 'RGP_FRAMES_MAX_OUT'),
        (dict(out_hw=(98, 0)), 'RGP_FRAMES_MAX_OUT'),
        (dict(frames=np.zeros((1, 4, 2041, 3), np.uint8)), 'RGP_FRAMES_MAX_IN_W'),
        (dict(frames=np.zeros((1, 2, 2000, 3), np.uint8), out_hw=(2, 90)), 'RGP_FRAMES_MAX_KSIZE'),     # 22x down: 135 taps
        (dict(filter='nearest'), 'filter'),
        (dict(out='float16'), 'out'),
        (dict(bands=0), 'bands'),
        (dict(bands=99), 'bands'),
        (dict(frame_index=np.array([0.5])), 'integers'),
        (dict(frame_index=np.array([2 ** 31])), 'int32'),
    ]
    for kw, word in bad:
        args = dict(frames=frames, out_hw=(11, 7))
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            fr.frame_images(**args)
    import torch
    with pytest.raises(ValueError, match='uint8'):
        fr.frame_images(torch.zeros((2, 37, 53, 3)), (11, 7))
