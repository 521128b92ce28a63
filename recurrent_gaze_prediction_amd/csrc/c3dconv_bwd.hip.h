// Backward of gaze_c3d_conv (training plans; rgp_c3dconv.hip): the chain rule head_fold.hip.h documents with y := E,
//
//   dz = d loss / d logits (dlogits_kernel), d out_b = sum dz, Pm = the 19x19 patches of dz (head_fold_patches_kernel)
//   dK[(r,t),s] = sum_m Pm[m,(r,t)] E[m,s]     dE[m,s] = sum_(r,t) Pm[m,(r,t)] K[(r,t),s]
//   head_unfold_* : dK -> d weight1 / dH -> d weight2 / dG -> d weight3, d out_W
//   d proj_c3d_W[k,s] = sum_m X[m,k] dE[m,s]    d proj_c3d_b = colsum(dE)     d rows = dE proj_c3d_W^T
//
// with NO float atomics: the two filter gradients (reductions over the M = frames x 49 rows) run as plain GEMMs on
// transposed copies of their operands -- XT [1024][Mp], PmT [384][Mp], ET / dET [P][Mp], Mp = M rounded up to 64, zero
// padded -- with the existing igemm kernel, K = Mp split over blockIdx.y: every split STORES its partial sum into a slice
// of its own (EpiStoreSplitF32) and head_fold_sum_kernel adds the slices in a fixed order.  Two backward calls on the
// same inputs give the same bits.
#pragma once
#include "igemm.hip.h"

namespace rgp {

// out[blockIdx.y][row][n0 .. n0+7] = acc: the partial sum of K-split blockIdx.y (e.xpre_img_stride: elements per slice)
struct EpiStoreSplitF32 {
  static __device__ __forceinline__ void apply(const EpiParams& e, int N, int img, int ml, int n0, float* v) {
    apply_at(e, N, img, ml, epi_out_base(e, img, ml), n0, v);
  }
  static __device__ __forceinline__ void apply_at(const EpiParams& e, int N, int, int, long long base, int n0, float* v) {
    const int nvalid = N - n0;
    if (nvalid <= 0) return;
    store8<float>((float*)e.out + (long long)blockIdx.y * e.xpre_img_stride + base + n0, v, nvalid);
  }
};

// dst[c][m] = src[m][c] for m < M, 0 for M <= m < Mp   (src [M][C], dst [C][Mp]; C and Mp multiples of 64)
// grid (Mp / 64, C / 64), 256 threads
template <typename T>
static __global__ __launch_bounds__(256) void c3dconv_transpose_kernel(const T* __restrict__ src, T* __restrict__ dst, long long M, int C,
                                                                       long long Mp) {
  __shared__ T tile[64][65];
  const long long m0 = (long long)blockIdx.x * 64;
  const int c0 = blockIdx.y * 64;
  for (int i = threadIdx.x; i < 4096; i += 256) {
    const int r = i >> 6, c = i & 63;
    tile[r][c] = (m0 + r < M) ? src[(m0 + r) * C + c0 + c] : (T)0;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 4096; i += 256) {
    const int c = i >> 6, r = i & 63;
    dst[(long long)(c0 + c) * Mp + m0 + r] = tile[r][c];
  }
}

}  // namespace rgp
