"""CPU: the overlay's oracle (tests/overlay_ref.py) against Pillow, matplotlib and scipy, the built-in colour tables, the
host-only refusals of rgp_overlay, tile_grid, overlay_clip's pairing and run_evaluation's files.  No kernel is launched."""
import ctypes
import os

import numpy as np
import pytest
import torch

import overlay_ref as ref
from recurrent_gaze_prediction_amd import _lib
from recurrent_gaze_prediction_amd import overlay as ov
from recurrent_gaze_prediction_amd.evaluation import visualize_output as vo

ALPHAS = (0.0, 0.25, 1.0 / 3.0, 0.4, 0.6, 0.999, 1.0)


def all_pairs():
    return np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing='ij')      # f along y, c along x


# ---------------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize('alpha', ALPHAS)
def test_the_blend_restatement_equals_pillow_at_all_byte_pairs(alpha):
    Image = pytest.importorskip('PIL.Image')
    f, c = all_pairs()
    want = np.asarray(Image.blend(Image.fromarray(f, 'L'), Image.fromarray(c, 'L'), alpha))
    assert np.array_equal(ref.blend(f, c, alpha), want)
    f3 = np.stack([f, c, f[::-1]], axis=-1)
    c3 = np.stack([c, f, c[:, ::-1]], axis=-1)
    want = np.asarray(Image.blend(Image.fromarray(np.ascontiguousarray(f3), 'RGB'), Image.fromarray(np.ascontiguousarray(c3), 'RGB'), alpha))
    assert np.array_equal(ref.blend(f3, c3, alpha), want)


def test_a_fused_multiply_add_differs_from_pillow_at_alpha_06_only():
    Image = pytest.importorskip('PIL.Image')
    f, c = all_pairs()
    differ = {}
    for alpha in ALPHAS:
        want = np.asarray(Image.blend(Image.fromarray(f, 'L'), Image.fromarray(c, 'L'), alpha))
        differ[alpha] = int((ref.blend_fused(f, c, alpha) != want).sum())
    assert differ[0.6] == 361                        # so 0.6 stays among the alphas of the GPU test
    assert all(v == 0 for a, v in differ.items() if a != 0.6)


@pytest.mark.parametrize('name', ['jet', 'gray'])
def test_the_builtin_tables_equal_matplotlibs(name):
    matplotlib = pytest.importorskip('matplotlib')
    want = matplotlib.colormaps[name](np.arange(256, dtype=np.uint8), bytes=True)[:, :3]
    got = ov.colormap_lut(name)
    assert got.dtype == np.uint8 and got.shape == (256, 3) and np.array_equal(got, want)


def test_colormap_lut_tables_names_and_refusals():
    table = np.random.RandomState(0).randint(0, 256, (256, 3)).astype(np.uint8)
    assert np.array_equal(ov.colormap_lut(table), table) and np.array_equal(ov.colormap_lut(torch.from_numpy(table)), table)
    for bad in (table.astype(np.int32), table[:255], table.T):
        with pytest.raises(ValueError, match='uint8 .256, 3.'):
            ov.colormap_lut(bad)
    with pytest.raises(ValueError, match="'jet' and 'gray'"):
        ov.colormap_lut('no_such_colormap')
    gray = ov.colormap_lut('gray')            # (i / 255) * 255 truncated: not the identity (33 -> 32), as matplotlib's
    assert gray[0].tolist() == [0, 0, 0] and gray[255].tolist() == [255, 255, 255] and gray[33].tolist() == [32, 32, 32]
    jet = ov.colormap_lut('jet')
    assert jet[0].tolist() == [0, 0, 127] and jet[255].tolist() == [127, 0, 0]


# seeds found by search: the property they were chosen for is asserted below
CLEAR_CASES = [((7, 7), (20, 24), (6, 9, 16)), ((5, 6), (15, 17), (4, 5, 6)), ((7, 7), (7, 7), (0, 1, 2))]


@pytest.mark.parametrize('hw, HW, seeds', CLEAR_CASES)
def test_the_restatement_equals_scipy_bytescale_matplotlib_and_pillow(hw, HW, seeds):
    Image = pytest.importorskip('PIL.Image')
    from recurrent_gaze_prediction_amd.evaluation_metrics import resize
    lut = ov.colormap_lut('jet')
    maps = np.stack([np.random.RandomState(s).rand(*hw).astype(np.float32) for s in seeds])
    frames = np.random.RandomState(99).randint(0, 256, (len(seeds),) + HW + (3,)).astype(np.uint8)
    for alpha in (0.4, 0.6):
        out, heat, refused = ref.overlay(frames, maps, lut, alpha)
        assert refused == []
        for i in range(len(maps)):
            # the property of the inputs: b + 0.5 stays 1e-3 clear of every integer, so the 1e-13 between scipy's resize
            # and the restatement (tests/test_metrics_scaled_cpu.py) cannot move a byte
            v = ref.resize32(maps[i], HW)
            scale = np.float32(255.0 / float(np.float32(v.max() - v.min())))
            t = np.clip((v - v.min()) * scale, 0, 255).astype(np.float64) + 0.5
            assert np.abs(t - np.rint(t)).min() >= 1e-3
            host_v = np.asarray(resize(maps[i].astype(np.float64), HW, order=3, mode='reflect')).astype(np.float32)
            assert np.abs(host_v.astype(np.float64) - v).max() <= 1e-6
            host_u = ref.export_ref.bytescale(host_v)
            assert np.array_equal(host_u, heat[i])
            want = np.asarray(Image.blend(Image.fromarray(frames[i]), Image.fromarray(np.ascontiguousarray(lut[host_u])), alpha))
            assert np.array_equal(out[i], want)


def test_the_oracle_by_hand():
    lut = np.stack([np.arange(256)] * 3, axis=1).astype(np.uint8)
    frames = np.full((3, 2, 2, 3), 10, np.uint8)
    frames[1] = 200
    maps = np.array([[[0, 1], [2, 4]], [[5, 5], [5, 5]], [[0, np.nan], [1, 2]]], np.float32)
    out, heat, refused = ref.overlay(frames, maps, lut, 0.5)
    assert refused == [2] and heat[0].tolist() == [[0, 64], [128, 255]] and not heat[1].any() and not heat[2].any()
    assert out[0, :, :, 0].tolist() == [[5, 37], [69, 132]] and (out[1] == 100).all() and np.array_equal(out[2], frames[2])
    # limits clip; 'clip' is the min and max over the maps that are not refused
    out, heat, refused = ref.overlay(frames, maps, lut, 1.0, limits=[1.0, 3.0])
    assert heat[0].tolist() == [[0, 0], [128, 255]] and (heat[1] == 255).all() and refused == [2]
    out, heat, refused = ref.overlay(frames, maps, lut, 1.0, limits='clip')
    assert heat[0].tolist() == [[0, 51], [102, 204]] and (heat[1] == 255).all()
    # a frame index out of range: refused, zeros; descending limits: refused, the frame
    out, heat, refused = ref.overlay(frames, maps[:2], lut, 0.5, frame_idx=[3, 1], limits=[[0, 1], [1, 0]])
    assert refused == [0, 1] and not out[0].any() and np.array_equal(out[1], frames[1])


# ---------------------------------------------------------------------------------------------------- the ABI, host only
def good_args():
    """Every pointer is a made-up address: each call below must be refused before anything reads it."""
    return dict(frames=0x100000, frame_idx=0x2000, maps=0x3000, limits=0x4000, lut=0x5000, alpha=0.4, flags=0, out=0x900000,
                heat_u8=0x7001, n=3, n_src=4, h=49, w=49, H=98, W=98)


def call(change, workspace=0x8000, workspace_bytes=1 << 20):
    lib = _lib.load()
    args = _lib.OverlayArgs(**dict(good_args(), **change))
    return lib.rgp_overlay(ctypes.byref(args), workspace, workspace_bytes, None), lib.rgp_last_error()


@pytest.mark.parametrize('change, word', [
    (dict(n=-1), 'n = -1'),
    (dict(n_src=0), 'n_src = 0'), (dict(n_src=2, frame_idx=None), 'frame_idx is NULL'),
    (dict(H=0), 'H*W'), (dict(H=2049, W=2049), 'RGP_METRICS_SCALED_MAX_PIX'),
    (dict(h=0), 'h x w'), (dict(h=1), 'h = 1'), (dict(w=1), 'w = 1'), (dict(h=65, w=64), 'RGP_METRICS_MAX_PIX'),
    (dict(alpha=-0.01), 'alpha'), (dict(alpha=1.5), 'alpha'), (dict(alpha=float('nan')), 'alpha'),
    (dict(flags=2), 'unknown flags'), (dict(flags=1), 'limits must be NULL'),
    (dict(out=None, heat_u8=None), 'out and heat_u8 are both NULL'),
    (dict(maps=None), 'maps is NULL'), (dict(maps=0x3002), 'maps must be 4-byte aligned'),
    (dict(lut=None), 'lut is NULL'), (dict(limits=0x4001), 'limits must be 4-byte aligned'),
    (dict(frame_idx=0x2002), 'frame_idx must be 4-byte aligned'),
    (dict(frames=None), 'frames is NULL'),
    (dict(out=0x100000), 'out must not alias frames'), (dict(out=0x100000 + 4 * 98 * 98 * 3 - 1), 'out must not alias frames'),
    (dict(out=0x100000 - 3 * 98 * 98 * 3 + 1), 'out must not alias frames'),
])
def test_the_abi_refuses_each_bad_argument_with_its_name(change, word):
    rc, err = call(change)
    assert rc == -1 and word.encode() in err, err


def test_the_abi_host_only_answers():
    lib = _lib.load()
    assert lib.rgp_overlay(None, None, 0, None) == -1 and b'args is NULL' in lib.rgp_last_error()
    assert lib.rgp_overlay(ctypes.byref(_lib.OverlayArgs(n=0)), None, 0, None) == 0          # nothing to do, nothing launched
    assert lib.rgp_overlay_status(None, None, None) == -1 and b'workspace is NULL' in lib.rgp_last_error()
    # the workspace: RGP_EWORKSPACE, after every argument has passed
    need = lib.rgp_overlay_workspace_bytes(3, 49, 49, 98, 98)
    assert need > 64 + (98 + 98) * 4 * 10
    for ws, size in ((None, need), (0x8000, need - 1), (0x8004, need)):
        rc, err = call({}, ws, size)
        assert rc not in (0, -1) and b'workspace' in err, (rc, err)
    # adjoining buffers do not alias; the identity needs no table, takes maps of any size and a heat-only call no frames
    rc, err = call(dict(out=0x100000 + 4 * 98 * 98 * 3), None, 0)
    assert b'workspace' in err
    rc, err = call(dict(h=405, w=720, H=405, W=720, frames=None, out=None), None, 0)
    assert b'workspace' in err
    assert lib.rgp_overlay_workspace_bytes(3, 98, 98, 98, 98) < lib.rgp_overlay_workspace_bytes(3, 49, 49, 98, 98)
    assert lib.rgp_overlay_workspace_bytes(0, 49, 49, 98, 98) == 64
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'rgp.h')).read()
    assert '#define RGP_OVERLAY_SHARED_LIMITS 1' in header and _lib.RGP_OVERLAY_SHARED_LIMITS == 1


def test_python_refuses_what_the_kernel_does_not_cover_before_the_device_is_used():
    frames, maps = np.zeros((3, 20, 24, 3), np.uint8), np.zeros((3, 7, 7), np.float32)
    for bad_frames, match in ((frames.astype(np.float32), 'frames must be uint8'), (frames[..., :2], 'the last of 3'), (frames[0], 'frames must be')):
        with pytest.raises(ValueError, match=match):
            ov.overlay_maps(bad_frames, maps)
    for bad_maps, match in ((maps.astype(np.float64), 'maps must be float32'), (maps[0], 'maps must be'), (np.zeros((3, 1, 7), np.float32), 'at least 2'),
                            (np.zeros((3, 65, 64), np.float32), 'MAX_PIX'), (np.zeros((4, 7, 7), np.float32), 'no frame_idx')):
        with pytest.raises(ValueError, match=match):
            ov.overlay_maps(frames, bad_maps)
    for alpha in (-0.1, 1.1, float('nan')):
        with pytest.raises(ValueError, match='alpha'):
            ov.overlay_maps(frames, maps, alpha=alpha)
    with pytest.raises(ValueError, match='one entry per map'):
        ov.overlay_maps(frames, maps, frame_idx=[0, 1])
    with pytest.raises(ValueError, match="'clip'"):
        ov.overlay_maps(frames, maps, limits='frame')
    with pytest.raises(ValueError, match='nothing to compute'):
        ov.overlay_maps(frames, maps, want_out=False)
    with pytest.raises(ValueError, match="'jet' and 'gray'"):
        ov.overlay_maps(frames, maps, colormap='no_such_colormap')
    with pytest.raises(ValueError, match='out must be'):
        ov.overlay_maps(frames, maps, out=np.zeros((3, 20, 24, 3), np.uint8))


# ---------------------------------------------------------------------------------------------------- tile_grid, overlay_clip
@pytest.mark.parametrize('N', [1, 5, 12])
def test_tile_grid_equals_the_references_arithmetic(N):
    rng = np.random.RandomState(N)
    for data in (rng.randint(1, 256, (N, 4, 6, 3)).astype(np.uint8), rng.rand(N, 5, 3).astype(np.float32)):
        for kw in ({}, dict(width=N), dict(width=4), dict(height=3, width=N), dict(width=5, padsize=2, padval=7), dict(padsize=0)):
            want = ref.tile_grid(data, **kw)
            got = vo.tile_grid(data, **kw)
            assert isinstance(got, np.ndarray) and got.dtype == data.dtype and np.array_equal(got, want), (N, kw)
            got_t = vo.tile_grid(torch.from_numpy(data), **kw)
            assert torch.is_tensor(got_t) and np.array_equal(got_t.numpy(), want)
    rows, cols = ref.grid_shape(N)
    assert ref.tile_grid(np.zeros((N, 4, 6)), padsize=1).shape == (rows * 5, cols * 7)
    assert {1: (1, 1), 5: (3, 2), 12: (4, 3)}[N] == (rows, cols)
    with pytest.raises(ValueError, match='fewer'):
        vo.tile_grid(np.zeros((N, 2, 2)), height=1, width=N - 1)


def test_overlay_clips_index_arithmetic(monkeypatch):
    assert ov.clip_frame_index(5).tolist() == [15, 20, 25, 30, 35] and ov.clip_frame_index(5).dtype == np.int32
    assert ov.clip_frame_index(5).tolist() == list(range(40))[15:40:5]               # the loader's slice of a 40-frame clip
    assert ov.clip_frame_index(3, first=2, step=7).tolist() == [2, 9, 16] and ov.clip_frame_index(0).tolist() == []
    seen = {}
    monkeypatch.setattr(ov, 'overlay_maps', lambda clip, maps, **kw: seen.update(kw) or 'drawn')
    clip, maps = np.zeros((40, 4, 4, 3), np.uint8), np.zeros((5, 2, 2), np.float32)
    assert ov.overlay_clip(clip, maps, alpha=0.6) == 'drawn'
    assert seen['frame_idx'].tolist() == [15, 20, 25, 30, 35] and seen['alpha'] == 0.6
    with pytest.raises(ValueError, match='need 41 frames'):
        ov.overlay_clip(clip, np.zeros((6, 2, 2), np.float32))
    with pytest.raises(ValueError, match='step'):
        ov.overlay_clip(clip, maps, step=0)


# ---------------------------------------------------------------------------------------------------- run_evaluation
class StubSession(object):
    device = 'cuda:0'


class StubModel(object):
    n_lstm_steps = 4
    session = StubSession()

    def generate(self, dataset, max_instances):
        rng = np.random.RandomState(5)
        n = 12
        fix = np.zeros((n, 8, 8), np.uint8)
        for i in range(n):
            fix[i].reshape(-1)[rng.choice(64, 4, replace=False)] = 1
        return dict(pred_gazemap_list=list(rng.rand(n, 8, 8).astype(np.float32)), gt_gazemap_list=list(rng.rand(n, 8, 8).astype(np.float32)),
                    images_list=list(rng.randint(0, 256, (n, 8, 8, 3)).astype(np.float32) / np.float32(255.0)), fixationmap_list=list(fix))


class StubData(object):
    valid = None


def test_run_evaluation_writes_exactly_todays_files_without_dump_overlays(tmp_path, monkeypatch):
    pytest.importorskip('PIL.Image')
    from recurrent_gaze_prediction_amd.models import evaluate_gaze as eg
    monkeypatch.setattr(ov, 'overlay_maps', lambda *a, **k: pytest.fail('overlay_maps called without dump_overlays'))
    per_frame = ['%05d.%s' % (i, s) for i in range(12) for s in ('frame.jpg', 'gaze_gt.jpg', 'gaze_pred.jpg', 'scores.txt')]
    plain = eg.run_evaluation(StubModel(), StubData(), str(tmp_path / 'plain'), num_frames=12, seed=3, dump_images=True)
    assert sorted(os.listdir(str(tmp_path / 'plain'))) == sorted(per_frame + ['overall.txt'])
    off = eg.run_evaluation(StubModel(), StubData(), str(tmp_path / 'off'), num_frames=12, seed=3, dump_images=True, dump_overlays=False)
    assert off == plain and sorted(os.listdir(str(tmp_path / 'off'))) == sorted(per_frame + ['overall.txt'])
    for name in per_frame + ['overall.txt']:
        assert open(str(tmp_path / 'off' / name), 'rb').read() == open(str(tmp_path / 'plain' / name), 'rb').read(), name
    eg.run_evaluation(StubModel(), StubData(), str(tmp_path / 'bare'), num_frames=12, seed=3)
    assert sorted(os.listdir(str(tmp_path / 'bare'))) == sorted(['%05d.scores.txt' % i for i in range(12)] + ['overall.txt'])

    # dump_overlays=True: the same numbers, two more files per frame, one overlay_maps call each for predictions and ground
    # truth, fed the frames as rint(img * 255) (the device call replaced by the oracle here)
    calls = []

    def host_overlay(frames, maps, alpha=0.4, colormap='jet', device=None, **kw):
        calls.append((np.array(frames), np.array(maps), alpha, colormap, device))
        return torch.from_numpy(ref.overlay(frames, maps, ov.colormap_lut(colormap), alpha)[0])
    monkeypatch.setattr(ov, 'overlay_maps', host_overlay)
    on = eg.run_evaluation(StubModel(), StubData(), str(tmp_path / 'on'), num_frames=12, seed=3, dump_images=True, dump_overlays=True)
    extra = ['%05d.%s' % (i, s) for i in range(12) for s in ('overlay_pred.jpg', 'overlay_gt.jpg')]
    assert on == plain and sorted(os.listdir(str(tmp_path / 'on'))) == sorted(per_frame + extra + ['overall.txt'])
    ret = StubModel().generate(None, 4)
    want_frames = np.rint(np.stack(ret['images_list']) * np.float32(255.0)).astype(np.uint8)
    assert len(calls) == 2 and all(c[2:] == (0.4, 'jet', 'cuda:0') and np.array_equal(c[0], want_frames) for c in calls)
    assert np.array_equal(calls[0][1], np.stack(ret['pred_gazemap_list'])) and np.array_equal(calls[1][1], np.stack(ret['gt_gazemap_list']))
