"""GPU: the aligned byte-run store of csrc/image_shared.hip.h ("aligned dwords, single bytes at the two ends") under the
two launches that hand it LDS bytes: the loader's frame images and the gaze-map export.

Both go straight through the C entries with their byte outputs moved by 0, 1, 2 and 3 bytes inside a larger buffer of a
fill value.  The claim is equality with the oracles (tests/frames_cases.py, tests/export_ref.py) and that everything
around the output, eight guard bytes on each side among it, still holds the fill value.  A refused item (a frame_index
entry outside the clip, a map that holds a NaN) comes back as zeros and counted; a refused index never reaches an address.
The shapes are the smallest with a head, words and a tail in every run: bands of 105 and 126 bytes of images of 231,
maps of 35 and pooled maps of 9 bytes."""
import ctypes

import numpy as np
import pytest
import torch

import export_ref
import frames_cases
from recurrent_gaze_prediction_amd import _lib
from recurrent_gaze_prediction_amd import frames as fr

pytestmark = pytest.mark.gpu

FILL, GUARD = 0xA5, 8


class Shifted:
    """n_bytes of output that start `shift` bytes past a 4-byte aligned address, GUARD bytes of FILL and more around them."""

    def __init__(self, n_bytes, shift, gpu):
        self.buf = torch.full((GUARD + 3 + n_bytes + GUARD,), FILL, dtype=torch.uint8, device=gpu)
        assert self.buf.data_ptr() % 4 == 0
        self.lo, self.hi = GUARD + shift, GUARD + shift + n_bytes
        self.ptr = self.buf.data_ptr() + self.lo

    def read(self):
        """-> the output bytes, after the check that nothing around them was written."""
        b = self.buf.cpu().numpy()
        assert (b[:self.lo] == FILL).all() and (b[self.hi:] == FILL).all(), 'bytes outside the output were written'
        return b[self.lo:self.hi]


def test_byte_outputs_at_every_alignment_leave_their_guards_alone(gpu):
    lib = _lib.load()
    stream = torch.cuda.current_stream(gpu).cuda_stream

    def dev(a):
        return torch.from_numpy(np.array(a)).to(gpu)                # a copy: the cases are read-only

    # ---- the frames: 37 x 53 -> 11 x 7, four frames in two bands each
    frames, (oh, ow) = frames_cases.frames('odd'), frames_cases.out_hw('odd')
    N, H, W, _ = frames.shape
    u8, _ = frames_cases.oracle('odd', 'lanczos')
    kh, bh, ksh = fr.resample_coeffs(W, ow)
    kv, bv, ksv = fr.resample_coeffs(H, oh)
    d_frames, t = dev(frames), [dev(a) for a in (kh, bh, kv, bv)]
    for shift in range(4):
        for index, refused in (([0, 1, 2, 3], []), ([3, 9, 0, 2], [1])):
            d_index = dev(np.asarray(index, np.int32))
            out = Shifted(len(index) * oh * ow * 3, shift, gpu)
            ws = torch.empty(lib.rgp_frames_workspace_bytes(), dtype=torch.uint8, device=gpu)
            args = _lib.FramesArgs(frames=d_frames.data_ptr(), n_frames=N, fh=H, fw=W, frame_index=d_index.data_ptr(), n_out=len(index),
                                   out_h=oh, out_w=ow, kh=t[0].data_ptr(), bh=t[1].data_ptr(), ksize_h=ksh, kv=t[2].data_ptr(),
                                   bv=t[3].data_ptr(), ksize_v=ksv, bands=2, images=None, images_u8=out.ptr,
                                   workspace=ws.data_ptr(), workspace_bytes=ws.numel())
            assert lib.rgp_frame_images(ctypes.byref(args), stream) == 0
            count = ctypes.c_int(-7)
            rc = lib.rgp_frames_status(ws.data_ptr(), ctypes.byref(count), stream)
            assert (rc, count.value) == ((-1, len(refused)) if refused else (0, 0)), (shift, index)
            want = np.stack([np.zeros_like(u8[0]) if i in refused else u8[src] for i, src in enumerate(index)])
            assert np.array_equal(out.read(), want.reshape(-1)), (shift, index)

    # ---- the export: three 5 x 7 maps pooled to 3 x 3, the second one refused for its NaN
    rs = np.random.RandomState(57)
    clean = rs.rand(3, 5, 7).astype(np.float32)
    _, small, u8 = (np.array(a) for a in export_ref.avg_pool(clean, (3, 3), 'bilinear'))
    small[1], u8[1] = 0, 0
    maps = clean.copy()
    maps[1, 2, 3] = np.nan
    kh, bh, ksh = fr.resample_coeffs(7, 3, 'bilinear')
    kv, bv, ksv = fr.resample_coeffs(5, 3, 'bilinear')
    d_maps, t = dev(maps), [dev(a) for a in (kh, bh, kv, bv)]
    for shift in range(4):
        o_bytes, o_small = Shifted(3 * 5 * 7, shift, gpu), Shifted(3 * 3 * 3, shift, gpu)
        ws = torch.empty(lib.rgp_mapexport_workspace_bytes(), dtype=torch.uint8, device=gpu)
        args = _lib.MapExportArgs(maps=d_maps.data_ptr(), n=3, h=5, w=7, out_h=3, out_w=3, kh=t[0].data_ptr(), bh=t[1].data_ptr(),
                                  ksize_h=ksh, kv=t[2].data_ptr(), bv=t[3].data_ptr(), ksize_v=ksv, pooled=None,
                                  pooled_u8=o_small.ptr, bytes=o_bytes.ptr, workspace=ws.data_ptr(), workspace_bytes=ws.numel())
        assert lib.rgp_mapexport(ctypes.byref(args), stream) == 0
        count = ctypes.c_int(-7)
        rc = lib.rgp_mapexport_status(ws.data_ptr(), ctypes.byref(count), stream)
        assert (rc, count.value) == (-1, 1), shift
        assert np.array_equal(o_bytes.read(), u8.reshape(-1)), shift
        assert np.array_equal(o_small.read(), small.reshape(-1)), shift
