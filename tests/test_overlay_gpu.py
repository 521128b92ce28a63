"""GPU: rgp_overlay (csrc/rgp_overlay.hip) against the numpy oracle tests/overlay_ref.py, bit for bit: every comparison is
np.array_equal on bytes.  Shapes where the reflection repeats, odd widths (W * 3 no multiple of 4), several row bands per
frame, a band longer than one chunk, coordinates that skip source pixels and the identity; every stage alone; all 65 536
(frame byte, colour byte) pairs; the corner maps of scipy's bytescale; refused maps; frame_idx; limits; byte offsets."""
import functools

import numpy as np
import pytest
import torch

import export_cases
import overlay_ref as ref
from recurrent_gaze_prediction_amd import _lib
from recurrent_gaze_prediction_amd import overlay as ov

pytestmark = pytest.mark.gpu

KINDS = ('softmax1', 'constant', 'one_hot', 'subnormal_range', 'negative', 'softmax0')
# (h, w) -> (H, W), n
CASES = [((2, 3), (5, 4), 5), ((7, 7), (33, 47), 1), ((7, 7), (33, 47), 5), ((7, 7), (33, 47), 67), ((49, 49), (98, 98), 5),
         ((49, 49), (405, 720), 3), ((49, 49), (7, 9), 5), ((3, 40), (2, 5000), 2), ((14, 14), (14, 14), 5), ((33, 47), (33, 47), 5)]
IDS = ['%dx%d-%dx%d-n%d' % (hw + HW + (n,)) for hw, HW, n in CASES]


@functools.lru_cache(maxsize=None)
def lut():
    t = ov.colormap_lut('jet')
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def case_maps(hw, n):
    rs = np.random.RandomState(100 * hw[0] + hw[1] + 7 * n)
    m = np.stack([export_cases.one_map(KINDS[i % len(KINDS)], hw[0], hw[1], rs) for i in range(n)]).astype(np.float32)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def case_frames(HW, n):
    f = np.random.RandomState(HW[0] + 3 * HW[1] + n).randint(0, 256, (n,) + HW + (3,)).astype(np.uint8)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def oracle(hw, HW, n, alpha=0.4):
    out, heat, refused = ref.overlay(case_frames(HW, n), case_maps(hw, n), lut(), alpha)
    assert refused == []
    out.setflags(write=False)
    heat.setflags(write=False)
    return out, heat


def host(t):
    return t.cpu().numpy()


@pytest.mark.parametrize('hw, HW, n', CASES, ids=IDS)
def test_every_shape_and_every_stage_equals_the_oracle(gpu, hw, HW, n):
    from recurrent_gaze_prediction_amd.evaluation_metrics_gpu import resize_maps
    frames, maps = torch.from_numpy(np.array(case_frames(HW, n))).to(gpu), torch.from_numpy(np.array(case_maps(hw, n))).to(gpu)
    want_out, want_heat = oracle(hw, HW, n)
    out, heat = ov.overlay_maps(frames, maps, alpha=0.4, colormap=lut(), want_heat=True)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (n,) + HW + (3,) and tuple(heat.shape) == (n,) + HW
    assert np.array_equal(host(heat), want_heat)
    assert np.array_equal(host(out), want_out)
    if hw != HW:        # the stage alone: the existing resize entry point, then bytescale on the host
        v = host(resize_maps(maps, HW, out_dtype=torch.float32))
        assert np.array_equal(host(heat), np.stack([ref.export_ref.bytescale(x) for x in v]))
    # each output alone is the corresponding half of the joint call; numpy in gives the same
    assert torch.equal(ov.overlay_maps(frames, maps, alpha=0.4, colormap=lut()), out)
    assert torch.equal(ov.overlay_maps(frames, maps, alpha=0.4, colormap=lut(), want_heat=True, want_out=False), heat)
    if n == 5:
        assert torch.equal(ov.overlay_maps(np.array(case_frames(HW, n)), np.array(case_maps(hw, n)), alpha=0.4, colormap=lut(), device=gpu), out)


@pytest.mark.parametrize('alpha', [0.0, 0.4, 0.6, 1.0])
def test_all_65536_byte_pairs_blend_as_pillow_does(gpu, alpha):
    maps = np.tile(np.arange(256, dtype=np.float32)[None, None, :], (1, 256, 1))                 # identity path: u = x
    table = np.stack([np.arange(256, dtype=np.uint8)] * 3, axis=1)                               # lut[u] = (u, u, u)
    frames = np.tile(np.arange(256, dtype=np.uint8)[None, :, None, None], (1, 1, 256, 3))        # frame[y, x, :] = y
    out, heat = ov.overlay_maps(frames, maps, alpha=alpha, colormap=table, want_heat=True, device=gpu)
    assert np.array_equal(host(heat)[0], np.tile(np.arange(256, dtype=np.uint8)[None, :], (256, 1)))
    f, c = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing='ij')
    want = ref.blend(f, c, alpha)
    for ch in range(3):
        assert np.array_equal(host(out)[0, :, :, ch], want)
    if alpha == 0.6:
        assert (ref.blend_fused(f, c, alpha) != want).sum() == 361        # a fused multiply-add would have shown here


@pytest.mark.parametrize('hw, HW', [((7, 7), (33, 47)), ((14, 14), (14, 14))], ids=['resize', 'identity'])
def test_nan_and_inf_maps_are_refused_and_their_neighbours_are_not(gpu, hw, HW):
    n = 6
    maps = np.array(case_maps(hw, n))
    maps[1, 3, 2] = np.nan
    maps[4, hw[0] - 1, hw[1] - 1] = np.inf
    frames = np.array(case_frames(HW, n))
    for limits in (None, 'clip'):
        want_out, want_heat, refused = ref.overlay(frames, maps, lut(), 0.6, limits=limits)
        assert refused == [1, 4]
        with pytest.raises(_lib.RgpError, match='2 map.s. refused') as info:
            ov.overlay_maps(frames, maps, alpha=0.6, colormap=lut(), want_heat=True, limits=limits, device=gpu)
        got = info.value.outputs
        assert np.array_equal(host(got['heat']), want_heat) and np.array_equal(host(got['out']), want_out)
        for i in refused:
            assert np.array_equal(host(got['out'])[i], frames[i]) and not host(got['heat'])[i].any()
        keep = [0, 2, 3, 5]
        out, heat = ov.overlay_maps(frames[keep], maps[keep], alpha=0.6, colormap=lut(), want_heat=True, limits=limits, device=gpu)
        assert np.array_equal(host(out), want_out[keep]) and np.array_equal(host(heat), want_heat[keep])      # RGP_OK


def test_frame_idx(gpu):
    hw, HW, n = (7, 7), (33, 47), 5
    maps, clip = np.array(case_maps(hw, n)), np.array(case_frames(HW, 40))
    first = ov.overlay_maps(clip, maps, alpha=0.4, colormap=lut(), device=gpu)
    assert torch.equal(ov.overlay_maps(clip, maps, alpha=0.4, colormap=lut(), frame_idx=np.arange(n), device=gpu), first)
    assert np.array_equal(host(first), ref.overlay(clip, maps, lut(), 0.4)[0])
    every_fifth = ov.overlay_clip(clip, maps, alpha=0.4, colormap=lut(), device=gpu)
    assert np.array_equal(host(every_fifth), ref.overlay(clip, maps, lut(), 0.4, frame_idx=[15, 20, 25, 30, 35])[0])
    for idx in ([3, 3, 2, 0, 0], [39, 30, 20, 10, 0]):
        got = ov.overlay_maps(clip, maps, alpha=0.4, colormap=lut(), frame_idx=torch.tensor(idx, dtype=torch.int32, device=gpu), device=gpu)
        assert np.array_equal(host(got), ref.overlay(clip, maps, lut(), 0.4, frame_idx=idx)[0])
    for idx in ([0, 1, 40, 3, 4], [0, 1, 2, 3, -1], [2 ** 31 - 1, 1, 2, 3, 4]):
        want_out, want_heat, refused = ref.overlay(clip, maps, lut(), 0.4, frame_idx=idx)
        assert len(refused) == 1
        with pytest.raises(_lib.RgpError, match='1 map.s. refused') as info:
            ov.overlay_maps(clip, maps, alpha=0.4, colormap=lut(), frame_idx=idx, want_heat=True, device=gpu)
        assert np.array_equal(host(info.value.outputs['out']), want_out) and np.array_equal(host(info.value.outputs['heat']), want_heat)
        assert not want_out[refused[0]].any()


def test_limits(gpu):
    hw, HW, n = (7, 7), (33, 47), 7
    maps, frames = np.array(case_maps(hw, n)), np.array(case_frames(HW, n))
    rs = np.random.RandomState(4)
    limits = np.stack([maps.min(axis=(1, 2)) + rs.rand(n).astype(np.float32) * 0.01, maps.max(axis=(1, 2)) * 0.75], axis=1).astype(np.float32)
    limits[:, 1] = np.maximum(limits[:, 1], limits[:, 0])          # values below cmin and above cmax exist in most maps
    want_out, want_heat, refused = ref.overlay(frames, maps, lut(), 0.4, limits=limits)
    assert refused == [] and (want_heat == 0).sum() > n and (want_heat == 255).sum() > n
    out, heat = ov.overlay_maps(frames, maps, alpha=0.4, colormap=lut(), limits=limits, want_heat=True, device=gpu)
    assert np.array_equal(host(heat), want_heat) and np.array_equal(host(out), want_out)
    # maps [a, b) of the call equal maps [0, b - a) of a call on that slice
    a, b = 2, 6
    part = ov.overlay_maps(frames, maps[a:b], alpha=0.4, colormap=lut(), limits=limits[a:b], frame_idx=np.arange(a, b), device=gpu)
    assert torch.equal(part, out[a:b])
    # one pair for all maps, and 'clip': the min and max over the resized maps of the call
    want_out, want_heat, _ = ref.overlay(frames, maps, lut(), 0.4, limits=[0.0, 0.02])
    out, heat = ov.overlay_maps(frames, maps, alpha=0.4, colormap=lut(), limits=(0.0, 0.02), want_heat=True, device=gpu)
    assert np.array_equal(host(heat), want_heat) and np.array_equal(host(out), want_out)
    for hw2, HW2 in ((hw, HW), ((14, 14), (14, 14))):
        maps, frames = np.array(case_maps(hw2, n)), np.array(case_frames(HW2, n))
        want_out, want_heat, _ = ref.overlay(frames, maps, lut(), 0.4, limits='clip')
        out, heat = ov.overlay_maps(frames, maps, alpha=0.4, colormap=lut(), limits='clip', want_heat=True, device=gpu)
        assert np.array_equal(host(heat), want_heat) and np.array_equal(host(out), want_out)
    # limits that descend or are not finite refuse their map
    bad = np.array(limits)
    bad[3] = (1.0, 0.5)
    bad[5, 1] = np.nan
    want_out, want_heat, refused = ref.overlay(np.array(case_frames(HW, n)), np.array(case_maps(hw, n)), lut(), 0.4, limits=bad)
    assert refused == [3, 5]
    with pytest.raises(_lib.RgpError, match='2 map.s. refused') as info:
        ov.overlay_maps(np.array(case_frames(HW, n)), np.array(case_maps(hw, n)), alpha=0.4, colormap=lut(), limits=bad, device=gpu)
    assert np.array_equal(host(info.value.outputs['out']), want_out)


@pytest.mark.parametrize('frames_off', [0, 1, 2, 3])
def test_byte_offsets_of_frames_and_out_leave_the_guard_bytes_alone(gpu, frames_off):
    hw, HW, n = (7, 7), (33, 47), 5
    maps = torch.from_numpy(np.array(case_maps(hw, n))).to(gpu)
    frames = np.array(case_frames(HW, n))
    want_out, _ = oracle(hw, HW, n)
    size = frames.size
    src = torch.full((size + 64,), 0xAB, dtype=torch.uint8, device=gpu)
    src[16 + frames_off:16 + frames_off + size] = torch.from_numpy(frames.reshape(-1)).to(gpu)
    frames_view = src[16 + frames_off:16 + frames_off + size].view(n, HW[0], HW[1], 3)
    assert frames_view.data_ptr() % 4 == frames_off
    for out_off in (0, 1, 2, 3):
        dst = torch.full((size + 64,), 0xCD, dtype=torch.uint8, device=gpu)
        out_view = dst[32 + out_off:32 + out_off + size].view(n, HW[0], HW[1], 3)
        assert out_view.data_ptr() % 4 == out_off
        got = ov.overlay_maps(frames_view, maps, alpha=0.4, colormap=lut(), out=out_view)
        assert got.data_ptr() == out_view.data_ptr()
        d = host(dst)
        assert np.array_equal(d[32 + out_off:32 + out_off + size].reshape(want_out.shape), want_out), (frames_off, out_off)
        assert (d[:32 + out_off] == 0xCD).all() and (d[32 + out_off + size:] == 0xCD).all(), (frames_off, out_off)
    s = host(src)
    assert (s[:16 + frames_off] == 0xAB).all() and (s[16 + frames_off + size:] == 0xAB).all()
    assert np.array_equal(s[16 + frames_off:16 + frames_off + size], frames.reshape(-1))


def test_visualize_outputs_equals_the_sheet_of_the_oracles_overlays(gpu):
    from recurrent_gaze_prediction_amd.evaluation import visualize_output as vo
    hw, HW, n = (7, 7), (33, 47), 5
    frames = np.array(case_frames(HW, n))
    images = frames.astype(np.float32) / np.float32(255.0)              # the loader's float images: rint(img * 255) gives the bytes back
    assert np.array_equal(vo.frame_bytes(images), frames)
    pred, gt = np.array(case_maps(hw, n)), np.array(case_maps(hw, n + 1))[1:]
    sheet = vo.visualize_outputs(images, gt, pred, device=gpu)
    jet = ov.colormap_lut('jet')
    want = ref.tile_grid(np.concatenate([frames, ref.overlay(frames, pred, jet, 0.4)[0], ref.overlay(frames, gt, jet, 0.4)[0]]), height=3, width=n)
    assert sheet.is_cuda and sheet.dtype == torch.uint8 and tuple(sheet.shape) == (3 * 34, n * 48, 3)
    assert np.array_equal(host(sheet), want)
