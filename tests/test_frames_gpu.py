"""GPU: the loader's frame images (csrc/rgp_frames.hip through frames.frame_images) against the numpy oracle of
tests/frames_ref.py, which tests/test_frames_cpu.py pins to Pillow at these shapes (the GPU box may have no Pillow).

The arithmetic is integer up to one fp32 multiply: the claim is equality (torch.equal), for every case, filter and
banding.  The cases are tests/frames_cases.py's."""
import ctypes

import numpy as np
import pytest
import torch

import frames_cases as cases
import frames_ref as ref
from recurrent_gaze_prediction_amd import _lib
from recurrent_gaze_prediction_amd import frames as fr

pytestmark = pytest.mark.gpu


def differing(t, a):
    return int((t.cpu().numpy() != a).sum())


@pytest.mark.parametrize('name, filt', cases.CASES, ids=cases.IDS)
def test_images_equal_the_oracle_whatever_the_banding(gpu, name, filt):
    frames, (oh, ow) = cases.frames(name), cases.out_hw(name)
    u8, f32 = cases.oracle(name, filt)
    d_frames = torch.from_numpy(np.array(frames)).to(gpu)
    got_f32, got_u8 = fr.frame_images(d_frames, (oh, ow), filter=filt, out='both')
    assert got_f32.is_cuda and got_f32.dtype == torch.float32 and tuple(got_f32.shape) == (len(frames), oh, ow, 3)
    assert got_u8.is_cuda and got_u8.dtype == torch.uint8 and tuple(got_u8.shape) == (len(frames), oh, ow, 3)
    print('%s %s: %d of %d bytes differ, %d of %d floats' % (name, filt, differing(got_u8, u8), u8.size, differing(got_f32, f32), f32.size))
    assert torch.equal(got_u8.cpu(), torch.from_numpy(np.array(u8)))
    assert torch.equal(got_f32.cpu(), torch.from_numpy(np.array(f32)))
    assert torch.equal(got_f32, got_u8.float() * float(np.float32(1.0 / 255.0)))
    # one output at a time, and from host frames: the same bits
    assert torch.equal(fr.frame_images(d_frames, (oh, ow), filter=filt), got_f32)
    assert torch.equal(fr.frame_images(np.array(frames), (oh, ow), filter=filt, out='uint8', device=gpu), got_u8)
    # the banding changes nothing
    for request in cases.band_requests(name):
        b_f32, b_u8 = fr.frame_images(d_frames, (oh, ow), filter=filt, out='both', bands=request)
        assert torch.equal(b_u8, got_u8) and torch.equal(b_f32, got_f32), (name, filt, request)


def test_frame_index_selects_repeats_and_reverses(gpu):
    frames, (oh, ow) = cases.frames('odd'), cases.out_hw('odd')
    u8, f32 = cases.oracle('odd', 'lanczos')
    d_frames = torch.from_numpy(np.array(frames)).to(gpu)
    for index in ([2], [3, 1], [0, 0, 3, 3, 0], [3, 2, 1, 0], list(range(4)) * 3):
        got_f32, got_u8 = fr.frame_images(d_frames, (oh, ow), frame_index=index, out='both')
        assert tuple(got_u8.shape) == (len(index), oh, ow, 3)
        assert torch.equal(got_u8.cpu(), torch.from_numpy(u8[index])) and torch.equal(got_f32.cpu(), torch.from_numpy(f32[index])), index
    # a device tensor of indices, any integer type
    for dtype in (torch.int32, torch.int64):
        got = fr.frame_images(d_frames, (oh, ow), frame_index=torch.tensor([1, 3], dtype=dtype, device=gpu), out='uint8')
        assert torch.equal(got.cpu(), torch.from_numpy(u8[[1, 3]]))
    # no index: all frames in order; the loader's own selection on a longer clip
    assert torch.equal(fr.frame_images(d_frames, (oh, ow), out='uint8').cpu(), torch.from_numpy(np.array(u8)))
    clip = np.random.RandomState(5).randint(0, 256, size=(31, 37, 53, 3)).astype(np.uint8)
    got = fr.frame_images(clip, (oh, ow), frame_index=fr.loader_frame_index(len(clip)), out='uint8', device=gpu)
    assert torch.equal(got.cpu(), torch.from_numpy(ref.resize(clip[15::5], (oh, ow))))


@pytest.mark.parametrize('value', [4, -1, 2 ** 31 - 1, -2 ** 31])
def test_a_bad_index_refuses_its_frame_only(gpu, value):
    """The index is checked on the device before it is used: that image is NaN / 0 and counted, the others are computed,
    and the next clean call returns normally.  Nothing here reaches an address."""
    frames, (oh, ow) = cases.frames('odd'), cases.out_hw('odd')
    u8, f32 = cases.oracle('odd', 'lanczos')
    d_frames = torch.from_numpy(np.array(frames)).to(gpu)
    index = [1, value, 3, 0]
    for bands in (None, 3):
        with pytest.raises(_lib.RgpError) as info:
            fr.frame_images(d_frames, (oh, ow), frame_index=index, out='both', bands=bands)
        assert info.value.code == -1 and '1 output frame(s) refused' in str(info.value)
        got_f32, got_u8 = info.value.outputs
        assert bool(torch.isnan(got_f32[1]).all()) and int(got_u8[1].max()) == 0
        rest = [0, 2, 3]
        assert torch.equal(got_u8[rest].cpu(), torch.from_numpy(u8[[1, 3, 0]]))
        assert torch.equal(got_f32[rest].cpu(), torch.from_numpy(f32[[1, 3, 0]]))
    clean = fr.frame_images(d_frames, (oh, ow), frame_index=[1, 3, 0], out='uint8')
    assert torch.equal(clean.cpu(), torch.from_numpy(u8[[1, 3, 0]]))


def test_the_status_word_counts_refused_frames(gpu):
    """Straight to the C entry: two bad entries of five; and a bounds table with an entry past the frame refuses every
    output frame before anything is read through it."""
    frames, (oh, ow) = cases.frames('odd'), cases.out_hw('odd')
    N, H, W, _ = frames.shape
    u8, _ = cases.oracle('odd', 'lanczos')
    lib = _lib.load()
    d_frames = torch.from_numpy(np.array(frames)).to(gpu)
    kh, bh, ksh = fr.resample_coeffs(W, ow)
    kv, bv, ksv = fr.resample_coeffs(H, oh)
    stream = torch.cuda.current_stream(gpu).cuda_stream

    def run(index, bv_host):
        t = [torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in (kh, bh, kv, bv_host, np.asarray(index, np.int32))]
        out = torch.full((len(index), oh, ow, 3), 7, dtype=torch.uint8, device=gpu)
        ws = torch.empty(lib.rgp_frames_workspace_bytes(), dtype=torch.uint8, device=gpu)
        args = _lib.FramesArgs(frames=d_frames.data_ptr(), n_frames=N, fh=H, fw=W, frame_index=t[4].data_ptr(), n_out=len(index),
                               out_h=oh, out_w=ow, kh=t[0].data_ptr(), bh=t[1].data_ptr(), ksize_h=ksh, kv=t[2].data_ptr(),
                               bv=t[3].data_ptr(), ksize_v=ksv, bands=2, images=None, images_u8=out.data_ptr(),
                               workspace=ws.data_ptr(), workspace_bytes=ws.numel())
        assert lib.rgp_frame_images(ctypes.byref(args), stream) == 0
        refused = ctypes.c_int(-7)
        rc = lib.rgp_frames_status(ws.data_ptr(), ctypes.byref(refused), stream)
        return rc, refused.value, out.cpu().numpy()

    rc, refused, out = run([0, 9, 2, -5, 3], bv)
    assert rc == -1 and refused == 2 and b'2 output frame(s) refused' in lib.rgp_last_error()
    assert (out[[1, 3]] == 0).all() and np.array_equal(out[[0, 2, 4]], u8[[0, 2, 3]])
    rc, refused, out = run([0, 1], bv)
    assert rc == 0 and refused == 0 and np.array_equal(out, u8[:2])
    bad_bv = bv.copy()
    bad_bv[oh - 1, 1] += 1                                   # the last row's taps end one row past the frame
    rc, refused, out = run([0, 1, 2], bad_bv)
    assert rc == -1 and refused == 3 and (out == 0).all()
    bad_bv = bv.copy()
    bad_bv[3, 0] = -1
    rc, refused, out = run([0, 1, 2], bad_bv)
    assert rc == -1 and refused == 3 and (out == 0).all()


def test_no_output_frames(gpu):
    d_frames = torch.from_numpy(np.array(cases.frames('odd'))).to(gpu)
    f32, u8 = fr.frame_images(d_frames, (11, 7), frame_index=[], out='both')
    assert tuple(f32.shape) == (0, 11, 7, 3) and tuple(u8.shape) == (0, 11, 7, 3) and f32.is_cuda
    empty = fr.frame_images(np.zeros((0, 37, 53, 3), np.uint8), (11, 7), device=gpu)
    assert tuple(empty.shape) == (0, 11, 7, 3)
    lib = _lib.load()
    args = _lib.FramesArgs(n_out=0)
    assert lib.rgp_frame_images(ctypes.byref(args), torch.cuda.current_stream(gpu).cuda_stream) == 0


def test_a_non_contiguous_tensor_raises(gpu):
    d_frames = torch.from_numpy(np.array(cases.frames('odd'))).to(gpu)
    with pytest.raises(ValueError, match='contiguous'):
        fr.frame_images(d_frames[:, :, ::2], (11, 7))
    with pytest.raises(ValueError, match='contiguous'):
        fr.frame_images(d_frames.permute(0, 2, 1, 3), (11, 7))
    # a contiguous slice of frames is fine, and starts at an odd address
    u8, _ = cases.oracle('odd', 'lanczos')
    assert d_frames[1:].data_ptr() % 2 == 1
    assert torch.equal(fr.frame_images(d_frames[1:], (11, 7), out='uint8').cpu(), torch.from_numpy(u8[1:]))


def test_shallownet_on_device_images_equals_shallownet_on_the_oracles(gpu):
    from recurrent_gaze_prediction_amd import synthetic as syn
    from recurrent_gaze_prediction_amd.engine import ShallowNetEngine
    _, f32 = cases.oracle('video', 'lanczos')
    images = fr.frame_images(np.array(cases.frames('video')), (98, 98), device=gpu)
    net = ShallowNetEngine(len(f32), image_hw=98, dtype='f32', device=gpu)
    net.set_weights(syn.shallownet_params(31, 98))
    ours, ours7 = net.forward(images, want_7x7=True)
    ours, ours7 = ours.clone(), ours7.clone()
    theirs, theirs7 = net.forward(torch.from_numpy(np.array(f32)).to(gpu), want_7x7=True)
    assert torch.equal(ours, theirs) and torch.equal(ours7, theirs7)
    assert bool(torch.isfinite(ours).all()) and float(ours.abs().max()) > 0


def test_video_inputs_pairs_windows_and_frames(gpu):
    from recurrent_gaze_prediction_amd import c3d_frontend as fe
    from recurrent_gaze_prediction_amd import synthetic as syn
    from recurrent_gaze_prediction_amd.engine import C3DEngine
    clip = np.random.RandomState(40).randint(0, 256, size=(40, 37, 53, 3)).astype(np.uint8)
    engine = C3DEngine(5, dtype='bf16', device=gpu)
    engine.set_weights(syn.c3d_params(3))
    extractor = fe.C3DFeatureExtractor(engine)
    starts, feats, images = fr.video_inputs(clip, extractor, image_hw=98)
    assert list(starts) == [0, 5, 10, 15, 20]
    assert feats.shape == (5, 1, 512, 2, 7, 7) and feats.dtype == np.float32
    want = ref.scaled(ref.resize(clip[[15, 20, 25, 30, 35]], (98, 98)))
    assert images.is_cuda and tuple(images.shape) == (5, 98, 98, 3)
    assert torch.equal(images.cpu(), torch.from_numpy(want))
    # the features are the extractor's own for these windows
    again = extractor.extract(clip, starts)[1]
    assert np.array_equal(feats, again)
