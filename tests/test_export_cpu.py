"""CPU: the gaze-map export's oracle (tests/export_ref.py) against Pillow, its tables against the product's, the host-only
refusals of rgp_mapexport, and export_clips' files, padding, cutting and skipping with a stub model.  No kernel is
launched here."""
import ctypes
import os

import numpy as np
import pytest
import torch

import export_cases as cases
import export_ref as ref
import frames_ref
from recurrent_gaze_prediction_amd import _lib
from recurrent_gaze_prediction_amd import frames as fr
from recurrent_gaze_prediction_amd.models import extract_map as em


# ---------------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize('filt', cases.FILTERS)
@pytest.mark.parametrize('hw, out', cases.SHAPES, ids=['%dx%d-%dx%d' % (a + b) for a, b in cases.SHAPES])
def test_the_oracle_equals_pillow_on_every_shape_the_gpu_test_uses(hw, out, filt):
    Image = pytest.importorskip('PIL.Image')
    resample = {'bilinear': Image.BILINEAR, 'lanczos': Image.LANCZOS, 'bicubic': Image.BICUBIC}[filt]
    for n in cases.COUNTS:
        _, small, u8 = cases.oracle(hw, out, n, filt)
        for i in range(n):
            want = np.asarray(Image.fromarray(np.array(u8[i])).resize((out[1], out[0]), resample))
            assert np.array_equal(small[i], want), (hw, out, n, i, cases.kind_of(i))


def test_bytescale_is_the_same_for_fp32_and_fp64_inputs_and_raises_no_warning_on_ordinary_maps():
    for hw, _ in cases.SHAPES:
        a = cases.maps(hw, 67)
        for i in range(len(a)):
            kind = cases.kind_of(i)
            with np.errstate(all='raise' if kind in cases.RANDOM_KINDS + ('half_integers', 'negative') else 'ignore'):
                u = ref.bytescale(a[i])
                assert u.dtype == np.uint8 and u.shape == a[i].shape
                assert np.array_equal(u, ref.bytescale(a[i].astype(np.float64)))          # cast to fp32 inside: the same values
                assert np.array_equal(u, ref.bytescale(a[i].astype(np.float64).astype(np.float32)))
                assert np.array_equal(u, em.bytescale(a[i])), (hw, i, kind)                 # the product's host statement


def test_bytescale_by_hand():
    # scale exactly 1: every half-integer rounds up (trunc(x + 0.5)), 255 stays
    a = cases.one_map('half_integers', 49, 49, None)
    assert a.min() == 0.0 and a.max() == 255.0
    assert np.array_equal(ref.bytescale(a), np.floor(a.astype(np.float64) + 0.5).astype(np.uint8))
    # a constant map: cscale = 0 -> 1, every byte 0
    assert not ref.bytescale(np.full((7, 7), 0.3, np.float32)).any()
    # negative values: the least is 0, the greatest 255
    u = ref.bytescale(np.array([[-3.0, -1.0], [1.0, 0.0]], np.float32))
    assert u.tolist() == [[0, 128], [255, 191]]
    # cmax - cmin a subnormal: scale = +inf, the cells equal to cmin are 0 * inf -> byte 0, the others 255
    a = cases.one_map('subnormal_range', 14, 14, np.random.RandomState(1))
    u = ref.bytescale(a)
    assert 0 < float(a.max() - a.min()) < np.finfo(np.float32).tiny
    assert np.array_equal(u, np.where(a == a.min(), 0, 255).astype(np.uint8))


def test_the_products_tables_equal_the_oracles():
    for size, out in ((49, 7), (48, 7), (14, 7), (49, 1), (48, 3)):
        for filt in cases.FILTERS:
            k, b, ksize = fr.resample_coeffs(size, out, filt)
            rk, rb, rksize = frames_ref.tables(size, out, filt)
            assert ksize == rksize and np.array_equal(k, rk) and np.array_equal(b, rb), (size, out, filt)
    k, b, ksize = fr.resample_coeffs(49, 7, 'bilinear')
    assert ksize == 15
    assert [tuple(r) for r in b.tolist()] == [(0, 11), (4, 14), (11, 14), (18, 14), (25, 14), (32, 14), (39, 10)]
    assert (k.sum(axis=1) - (1 << 22)).max() <= 8 and (k >= 0).all()


def test_random_cases_have_a_non_zero_pooled_sum_and_the_cases_made_for_it_are_nan():
    """NaN in the GPU test can only come from the cases made for it."""
    for hw, out, n in cases.CASES:
        for filt in cases.FILTERS if (hw, out, n) == ((49, 49), (7, 7), 5) else ('bilinear',):
            pooled, small, _ = cases.oracle(hw, out, n, filt)
            for i in range(n):
                kind = cases.kind_of(i)
                total = int(small[i].astype(np.int64).sum())
                if kind in cases.RANDOM_KINDS:
                    assert total > 0 and np.isfinite(pooled[i]).all(), (hw, out, n, i, kind)
                    assert abs(pooled[i].sum() - 1.0) < 1e-12
                if kind == 'constant':
                    assert total == 0 and np.isnan(pooled[i]).all(), (hw, out, n, i, kind)
    # one hot pixel: 255 / 7 = 36 after the horizontal pass and 36 / 7 = 5 after the vertical one, in one to four cells of
    # 7 x 7 -- a finite map; to a single cell 255 / 49 = 5, then 5 / 49 = 0 -- NaN
    pooled, small, u8 = cases.oracle((49, 49), (7, 7), 67)
    hot = [i for i in range(67) if cases.kind_of(i) == 'one_hot']
    assert hot and all(int(u8[i].sum()) == 255 and 1 <= int((small[i] > 0).sum()) <= 4 and np.isfinite(pooled[i]).all() for i in hot)
    pooled, small, u8 = cases.oracle((49, 49), (1, 1), 67)
    assert all(int(u8[i].sum()) == 255 and np.isnan(pooled[i]).all() for i in hot)


# ---------------------------------------------------------------------------------------------------- the ABI, host only
def good_args():
    """Every pointer is a made-up address: each call below must be refused before anything reads it."""
    return dict(maps=0x1000, n=3, h=49, w=49, out_h=7, out_w=7, kh=0x2000, bh=0x3000, ksize_h=15, kv=0x4000, bv=0x5000, ksize_v=15,
                pooled=0x6000, pooled_u8=0x7000, bytes=0x8000, workspace=0x9000, workspace_bytes=64)


@pytest.mark.parametrize('change, word', [
    (dict(n=-1), 'n = -1'),
    (dict(h=0), 'h = 0'), (dict(h=65), 'h = 65'), (dict(w=0), 'w = 0'), (dict(w=65), 'w = 65'),
    (dict(pooled=None, pooled_u8=None, bytes=None), 'all NULL'),
    (dict(out_h=0), 'out_h = 0'), (dict(out_h=50), 'out_h = 50'), (dict(out_w=0), 'out_w = 0'), (dict(out_w=50), 'out_w = 50'),
    (dict(ksize_h=0), 'ksize_h = 0'), (dict(ksize_h=513), 'ksize_h = 513'), (dict(ksize_v=0), 'ksize_v = 0'),
    (dict(ksize_v=513), 'ksize_v = 513'),
    (dict(kh=None), 'kh or bh'), (dict(bh=None), 'kh or bh'), (dict(kv=None), 'kv or bv'), (dict(bv=None), 'kv or bv'),
    (dict(maps=None), 'maps is NULL'), (dict(maps=0x1002), 'maps must be 4-byte aligned'),
    (dict(pooled=0x6004), 'pooled must be 8-byte aligned'),
    (dict(workspace=None), 'workspace'), (dict(workspace_bytes=8), 'workspace'), (dict(workspace=0x9004), 'workspace'),
])
def test_the_abi_refuses_each_bad_argument_with_its_name(change, word):
    lib = _lib.load()
    args = _lib.MapExportArgs(**dict(good_args(), **change))
    assert lib.rgp_mapexport(ctypes.byref(args), None) == -1
    assert word.encode() in lib.rgp_last_error(), lib.rgp_last_error()


def test_the_abi_host_only_answers():
    lib = _lib.load()
    assert lib.rgp_mapexport(None, None) == -1 and b'args is NULL' in lib.rgp_last_error()
    assert lib.rgp_mapexport_workspace_bytes() == 64
    assert lib.rgp_mapexport(ctypes.byref(_lib.MapExportArgs(n=0)), None) == 0          # nothing to do, nothing launched
    assert lib.rgp_mapexport_status(None, None, None) == -1 and b'workspace is NULL' in lib.rgp_last_error()
    # a skipped pass needs no table; only the bytes: no output shape and no table at all -- refused for the next reason
    args = _lib.MapExportArgs(**dict(good_args(), w=7, kh=None, bh=None, ksize_h=0, workspace=None))
    assert lib.rgp_mapexport(ctypes.byref(args), None) == -1 and b'workspace' in lib.rgp_last_error()
    args = _lib.MapExportArgs(**dict(good_args(), pooled=None, pooled_u8=None, out_h=0, out_w=0, kh=None, bh=None, kv=None, bv=None,
                                     ksize_h=0, ksize_v=0, workspace=None))
    assert lib.rgp_mapexport(ctypes.byref(args), None) == -1 and b'workspace' in lib.rgp_last_error()
    assert (_lib.RGP_MAPEXPORT_MAX_SIDE, _lib.RGP_MAPEXPORT_MAX_KSIZE, _lib.RGP_MAPEXPORT_LDS_BYTES) == (64, 512, 152 * 1024)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'rgp.h')).read()
    for line in ('#define RGP_MAPEXPORT_MAX_SIDE 64', '#define RGP_MAPEXPORT_MAX_KSIZE 512', '#define RGP_MAPEXPORT_LDS_BYTES (152 * 1024)'):
        assert line in header


def test_python_refuses_what_the_kernel_does_not_cover_before_the_device_is_used():
    good = np.zeros((2, 49, 49), np.float32)
    for bad, match in ((np.zeros((2, 49, 49), np.float64), 'float32'), (np.zeros((49, 49), np.float32), 'float32'),
                       (np.zeros((2, 65, 49), np.float32), 'MAX_SIDE'), (torch.zeros(2, 49, 49, dtype=torch.float64), 'float32')):
        with pytest.raises(ValueError, match=match):
            em.avg_pool(bad)
        with pytest.raises(ValueError, match=match):
            em.bytescale_maps(bad)
    with pytest.raises(ValueError, match='interp'):
        em.avg_pool(good, interp='nearest')
    for shape in ((8, 50), (50, 7), (0, 7)):
        with pytest.raises(ValueError, match='out_shape'):
            em.avg_pool(good, out_shape=shape)


# ---------------------------------------------------------------------------------------------------- export_clips
class StubModel(object):
    """predict returns, for step t of lane b, a 49 x 49 ramp offset by the clip's feature [t, 0, 0, 0]; records its inputs."""
    gazemap_height = gazemap_width = 49

    def __init__(self, B, T):
        self.batch_size, self.n_lstm_steps, self.calls = B, T, []

    def predict(self, c3d, frames=None):
        c3d = np.array(c3d)
        assert c3d.shape == (self.batch_size, self.n_lstm_steps, 1024, 7, 7) and c3d.dtype == np.float32
        self.calls.append((c3d, None if frames is None else np.array(frames)))
        ramp = (np.arange(2401, dtype=np.float32) % 97).reshape(49, 49)
        return torch.from_numpy(c3d[:, :, 0, 0, 0][:, :, None, None] * ramp[None, None] + ramp.T[None, None])


def stub_clip(seed, n):
    c = np.random.RandomState(seed).rand(n, 1024, 7, 7).astype(np.float32)
    c[:, 0, 0, 0] = np.arange(1, n + 1)
    return c


def test_export_clips_files_padding_cutting_and_skipping(tmp_path, monkeypatch):
    pooled_calls = []

    def host_avg_pool(maps, out_shape=(7, 7), interp='bilinear'):
        maps = maps.numpy() if torch.is_tensor(maps) else np.asarray(maps)
        pooled_calls.append(maps.shape)
        return ref.avg_pool(maps, out_shape, interp)[0]
    monkeypatch.setattr(em, 'avg_pool', host_avg_pool)
    B, T = 2, 4
    model = StubModel(B, T)
    out_dir = str(tmp_path / 'gazemaps')
    os.makedirs(os.path.join(out_dir, 'done'))                                   # "already exists": skipped, never loaded
    frames_b = np.random.RandomState(3).rand(4, 98, 98, 3).astype(np.float32)
    clips = [('short', stub_clip(1, 3)), ('done', stub_clip(2, 4)), ('exact', stub_clip(3, 4), frames_b), ('long', stub_clip(4, 6))]
    written = em.export_clips(model, clips, out_dir)
    assert written == ['short', 'exact', 'long'] and os.listdir(os.path.join(out_dir, 'done')) == []
    assert len(model.calls) == 2 and pooled_calls == [(7, 49, 49), (4, 49, 49)]   # B clips per predict; only valid steps pooled
    first, second = model.calls
    assert np.array_equal(first[0][0, :3], clips[0][1]) and not first[0][0, 3:].any()               # padded with zeros
    assert np.array_equal(first[0][1], clips[2][1])
    assert first[1] is not None and not first[1][0].any() and np.array_equal(first[1][1], frames_b)
    assert np.array_equal(second[0][0], clips[3][1][:4]) and not second[0][1].any()                 # cut to T; the free lane is zero
    assert second[1] is None
    ramp = (np.arange(2401, dtype=np.float32) % 97).reshape(49, 49)
    for name, clip, length in (('short', clips[0][1], 3), ('exact', clips[2][1], 4), ('long', clips[3][1], 4)):
        assert sorted(os.listdir(os.path.join(out_dir, name))) == ['%s.gazemap.49.npy' % name, '%s.gazemap.npy' % name]
        m49 = np.load(os.path.join(out_dir, name, '%s.gazemap.49.npy' % name))
        m77 = np.load(os.path.join(out_dir, name, '%s.gazemap.npy' % name))
        want = clip[:length, 0, 0, 0][:, None, None] * ramp[None] + ramp.T[None]
        assert m49.dtype == np.float32 and m49.shape == (length, 49, 49) and np.array_equal(m49, want)
        assert m77.dtype == np.float64 and m77.shape == (length, 7, 7)
        assert ref.same_float64(m77, ref.avg_pool(want.astype(np.float32))[0])
    # a second run finds every folder and does nothing
    assert em.export_clips(model, clips, out_dir) == [] and len(model.calls) == 2
    with pytest.raises(ValueError, match='length differs'):
        em.export_clips(model, [('mismatch', stub_clip(5, 3), frames_b)], out_dir)


def test_write_frame_bytescale_rounds_where_minmax_truncates(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    from recurrent_gaze_prediction_amd.models import evaluate_gaze as eg
    a = cases.one_map('half_integers', 49, 49, None)          # lossless formats would show it; JPEG is lossy, so compare the arrays fed
    saved = []
    monkey = Image.fromarray
    try:
        Image.fromarray = lambda arr, *k, **kw: (saved.append(np.array(arr)), monkey(arr, *k, **kw))[1]
        for scale in eg.DUMP_SCALES:
            d = tmp_path / scale
            d.mkdir()
            eg._write_frame(0, 1, a, a, a, {'sim': 1.0}, str(d), True, dump_scale=scale)
            assert sorted(os.listdir(str(d))) == ['00000.frame.jpg', '00000.gaze_gt.jpg', '00000.gaze_pred.jpg', '00000.scores.txt']
        d = tmp_path / 'given'
        d.mkdir()
        eg._write_frame(0, 1, a, a, a, {}, str(d), True, dump_scale='bytescale', pred_bytes=np.full((49, 49), 9, np.uint8))
    finally:
        Image.fromarray = monkey
    assert len(saved) == 9
    today = (((a.astype(np.float64) - 0.0) / 255.0) * 255).astype(np.uint8)                 # a.min() = 0, a.max() = 255: truncation
    assert all(np.array_equal(s, today) for s in saved[:3]) and (today != ref.bytescale(a)).any()
    assert all(np.array_equal(s, ref.bytescale(a)) for s in saved[3:6])                     # scipy's: rounding
    assert (saved[7] == 9).all() and np.array_equal(saved[6], ref.bytescale(a))
    with pytest.raises(ValueError, match='dump_scale'):
        eg._write_frame(0, 1, a, a, a, {}, str(tmp_path), True, dump_scale='nearest')
