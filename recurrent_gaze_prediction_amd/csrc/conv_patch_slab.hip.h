// Plane-slab variant of the patch kernel (conv_patch.hip.h), kept for conv2a + pool2 (64 -> 128 channels on 56 x 56 x 16),
// inference plans.  Spec: /root/reference/C3D/.../c3d_prototxt/feature_extration.prototxt:67-107.
//
// Up to round 5 this file held round 2's kernel: a plane slab = 348 consecutive pixels of the halo-padded input in one
// contiguous LDS buffer, fragments of 2 pooling windows x (dz, dy, dx) on a row pitch of 58 * 64 = 128 (mod 256) bytes.
// That fragment order mixes the two output planes of a pooled plane in every MFMA, so it cannot leave out the tap groups
// that multiply the zero halo planes z = -1 / z = DEPTH (1/24 of conv2a's MFMAs), and a dz-pure order on that pitch is
// 2-way bank-conflicted (8 rows of a ds_read_b128 lane group fall on 4 of the 16 sixteen-byte slots).
//
// Now it is the body of conv_patch.hip.h -- dz-pure fragments on the row pitch of 32 (mod 256), fetched row by row, skipped
// halo-plane tap groups, the rotated tile order of its decode() -- under the kernel name the inference plans report
// (rgp_c3d_layer_kernel_name, the profiles): the skipped MFMAs are worth more than the slab's smaller byte count was
// (same-box A/B, profiles/conv2a_halo_skip_ab.txt).  A variant that masked the fourth LDS-DMA instruction of a slab row to
// the 10 pixels the row has -- the slab's 348 pixels per plane with the slab's 24 instructions -- was measured and dropped:
// 0.05 - 0.1 ms SLOWER per 1024 windows than the plain row fetch (the exec-mask branch in the LOAD phase costs more than the
// 36 pixels save, all of them L2 hits).  The layout is enumerated by scripts/check_conv2a_layout.py (DMA destinations,
// fragment bases, immediates of all 27 taps).  The two kernels are interchangeable per launch: inference plans take this
// one unless created with RGP_C3D_CONV2A_ROWWISE, and the results are bit-identical (tests/test_c3d_gpu.py and
// tests/test_conv2a_halo_skip_gpu.py compare the plans with torch.equal).
#pragma once
#include "conv_patch.hip.h"

namespace rgp {

template <int CIN, int NOUT, int HW, int DEPTH>
static __global__ __launch_bounds__(512) void conv_patch_slab_bf16_kernel(const ConvPatchParams p) {
  conv_patch_body<CIN, NOUT, HW, DEPTH, true, false, false, false>(p);
}

}  // namespace rgp
