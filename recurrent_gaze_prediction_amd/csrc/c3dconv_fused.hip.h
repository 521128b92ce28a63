// gaze_c3d_conv (the no-recurrence baseline) as ONE launch, bf16 inference plans.
// Spec: /root/reference/models/gaze_c3d_conv.py:105-218.
//
// The graph has no non-linearity: the 1024 -> P projection, the three bias-free transposed convolutions and out_W are one
// linear map per frame.  With K[(r,t)][s] the 19 x 19 stride-6 filter of head_fold.hip.h (S = P),
//
//   M2[(r,t)][k] = sum_s proj_c3d_W[k,s] K[(r,t),s]                    [384][1024]   (rows 361 .. 383 zero)
//   beta[(r,t)]  = sum_s proj_c3d_b[s]   K[(r,t),s]
//   Pl[y,x]      = out_b + sum_{m,n} beta[(y-6m, x-6n)]                 the bias PLANE: border pixels gather fewer terms
//   Z[(f,m,n)][(r,t)] = sum_k X[(f,m,n)][k] M2[(r,t)][k]
//   logit[f,y,x] = Pl[y,x] + sum_{m,n} Z[(f,m,n)][(y-6m, x-6n)]          same term order as head_col2im_kernel
//
// exactly (checked in float64 against the staged graph: 3e-16 of max|logit|).  The fold kernels below build M2 / beta /
// Pl at set_weights in fp32 with sums in a fixed order and no atomics: equal weights give equal bits.
//
// c3dconv_fused_kernel: one 512-thread workgroup per PAIR of frames (98 rows = 7 row tiles of 16, 112 with padding; an
// odd frame count leaves the last workgroup one frame, its other rows re-read the last valid row and are dropped).
//   * K = 1024 in 16 steps of 64: per step the 112 x 128 B slab of X and the 384 x 128 B slab of M2 (786 KB in all:
//     L2-resident) arrive by LDS-DMA into a double buffer (2 x 62 KB), lane-linear with the XOR swizzle of igemm.hip.h.
//   * wave w owns columns 48w .. 48w+47 of all 7 row tiles: 21 accumulators, v_mfma_f32_16x16x32_bf16, fp32 accumulation.
//   * after the K loop the 98 x 384 fp32 tile of Z goes into the LDS the ring occupied (row stride 388 floats, 152 KB)
//     and never to HBM; threads 0 .. 255 gather the 2401 logit pixels of the first frame, 256 .. 511 those of the second
//     (<= 4 x 4 terms each), add the bias plane, write the logits and -- on request -- the per-frame softmax (block-half
//     max / sum reductions in a fixed tree).
// No atomics anywhere: the output is bit-reproducible, and a frame's bits do not depend on which slot of which
// workgroup it lands in (every element of Z is the same chain of MFMAs over k, every pixel the same chain of adds).
// The kernel issues 38.5 MFLOP per frame: it is bound by ingest and latency, not by the matrix pipe.
#pragma once
#include "head_fold.hip.h"

namespace rgp {

constexpr int CF_NT = 512;                                  // threads
constexpr int CF_ROWS = 98, CF_ROWS_PAD = 112;              // rows of a frame pair / padded to 7 tiles of 16
constexpr int CF_A_BYTES = CF_ROWS_PAD * 128;               // one K step of X
constexpr int CF_STAGE_BYTES = CF_A_BYTES + HF_PK * 128;    // + one K step of M2: 63 488
constexpr int CF_ZLD = 388;                                 // floats per row of Z in LDS
constexpr int CF_Z_BYTES = CF_ROWS * CF_ZLD * 4;            // 152 096
constexpr int CF_RED_OFF = CF_Z_BYTES;                      // 16 floats of reduction scratch behind Z
constexpr int CF_SMEM = CF_RED_OFF + 64;
static_assert(2 * CF_STAGE_BYTES <= CF_Z_BYTES, "the ring lies inside the area Z takes over");
static_assert(CF_SMEM <= 160 * 1024, "LDS of one CU");

// M2[(r,t)][k] (see above): block = one row (r,t) of K (staged in LDS), thread = k, fixed order over s.
// w: proj_c3d_W [1024][P]; kf: [361][P]; m2n: [384][1024] with column k = the placeholder's channel c*2+d; m2r: the same
// with column d*512+c (the rows C3D produces).  Rows 361 .. 383 are written as zeros.
template <typename T>
static __global__ __launch_bounds__(256) void c3dconv_fold_m2_kernel(const float* __restrict__ w, const float* __restrict__ kf,
                                                                     T* __restrict__ m2n, T* __restrict__ m2r, int P) {
  extern __shared__ __attribute__((aligned(16))) float krow[];
  const int rt = blockIdx.x;
  const bool live = rt < HF_KP * HF_KP;
  for (int s = threadIdx.x; s < P; s += 256) krow[s] = live ? kf[(long long)rt * P + s] : 0.f;
  __syncthreads();
  for (int k = threadIdx.x; k < 1024; k += 256) {
    float acc = 0.f;
    if (live) {
      const f32x4* wr = (const f32x4*)(w + (long long)k * P);
      for (int s = 0; s < P / 4; ++s) {
        const f32x4 x = wr[s];
        const f32x4 y = *(const f32x4*)(krow + 4 * s);
        acc += x[0] * y[0];
        acc += x[1] * y[1];
        acc += x[2] * y[2];
        acc += x[3] * y[3];
      }
    }
    const T v = Elem<T>::to(acc);
    m2n[(long long)rt * 1024 + k] = v;
    m2r[(long long)rt * 1024 + (k & 1) * 512 + (k >> 1)] = v;
  }
}

// beta[(r,t)] = sum_s b[s] K[(r,t),s]   (fixed order; 361 threads)
static __global__ void c3dconv_fold_beta_kernel(const float* __restrict__ b, const float* __restrict__ kf, float* __restrict__ beta, int P) {
  const int rt = blockIdx.x * blockDim.x + threadIdx.x;
  if (rt >= HF_PK) return;
  float acc = 0.f;
  if (rt < HF_KP * HF_KP)
    for (int s = 0; s < P; ++s) acc += b[s] * kf[(long long)rt * P + s];
  beta[rt] = acc;
}

// Pl[y,x] = out_b + sum_{m,n} beta[(y-6m, x-6n)]   (the loop of head_col2im_kernel on a one-row Z)
static __global__ void c3dconv_bias_plane_kernel(const float* __restrict__ beta, const float* __restrict__ out_b, float* __restrict__ plane) {
  const int pix = blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= 2401) return;
  const int y = pix / 49, x = pix - y * 49;
  const int m0 = y > 15 ? (y - 10) / 6 : 0, m1 = min(6, (y + 3) / 6);
  const int n0 = x > 15 ? (x - 10) / 6 : 0, n1 = min(6, (x + 3) / 6);
  float acc = out_b[0];
  for (int m = m0; m <= m1; ++m)
    for (int n = n0; n <= n1; ++n) acc += beta[(y - 6 * m + 3) * HF_KP + (x - 6 * n + 3)];
  plane[pix] = acc;
}

// max / sum over the 256 threads of one half of the block (4 waves), fixed tree; red: 4 floats of this half
template <bool MAX>
__device__ __forceinline__ float cf_half_reduce(float v, float* red, int tid) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float u = __shfl_xor(v, o, 64);
    v = MAX ? fmaxf(v, u) : v + u;
  }
  if ((tid & 63) == 0) red[(tid >> 6) & 3] = v;
  __syncthreads();
  const float a = red[0], b = red[1], c = red[2], d = red[3];
  const float r = MAX ? fmaxf(fmaxf(a, b), fmaxf(c, d)) : (a + b) + (c + d);
  __syncthreads();
  return r;
}

// x: rows [F*49][1024] bf16; m2: [384][1024] bf16 in the K order of x; plane: [2401]; logits / probs: [F][2401] (probs may be null)
static __global__ __launch_bounds__(CF_NT) void c3dconv_fused_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ m2,
                                                                     const float* __restrict__ plane, float* __restrict__ logits,
                                                                     float* __restrict__ probs, int F) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int f0 = blockIdx.x * 2;
  const int nfr = min(2, F - f0);                            // frames of this workgroup (1 at an odd tail)
  const int nrows = nfr * 49;

  // LDS-DMA: a wave instruction fills 8 rows x 128 B; lane l -> row l>>3, physical 16-B slot l&7 = logical chunk (l&7)^(l>>3).
  // 14 row groups of X + 48 of M2 per K step = 62 instructions over 8 waves: wave w takes groups w, w+8, ...
  const int lrow = lane >> 3, lchunk = (lane & 7) ^ lrow;
  const char* src[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int g = j * 8 + wave;
    if (g < CF_ROWS_PAD / 8) {
      const int r = min(g * 8 + lrow, nrows - 1);            // padding rows: a valid row again, result dropped
      src[j] = (const char*)x + ((long long)f0 * 49 + r) * 2048 + lchunk * 16;
    } else {
      const int r = min((g - CF_ROWS_PAD / 8) * 8 + lrow, HF_PK - 1);
      src[j] = (const char*)m2 + (long long)r * 2048 + lchunk * 16;
    }
  }
  auto stage = [&](int buf, int kt) {
    char* base = smem + buf * CF_STAGE_BYTES;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int g = j * 8 + wave;
      if (g < CF_ROWS_PAD / 8 + HF_PK / 8)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src[j] + kt * 128),
                                         (__attribute__((address_space(3))) void*)(base + g * 1024), 16, 0, 0);
    }
  };

  f32x4 acc[7][3];
#pragma unroll
  for (int i = 0; i < 7; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int frow = lane & 15, fk = lane >> 4;
  auto compute = [&](int buf) {
    const char* abuf = smem + buf * CF_STAGE_BYTES + frow * 128;
    const char* bbuf = smem + buf * CF_STAGE_BYTES + CF_A_BYTES + (wave * 48 + frow) * 128;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int pc = ((s * 4 + fk) ^ (frow & 7)) * 16;
      f32x4 a[7], b[3];
#pragma unroll
      for (int i = 0; i < 7; ++i) a[i] = *(const f32x4*)(abuf + i * 16 * 128 + pc);
#pragma unroll
      for (int j = 0; j < 3; ++j) b[j] = *(const f32x4*)(bbuf + j * 16 * 128 + pc);
#pragma unroll
      for (int i = 0; i < 7; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Mma<bf16_t>::step(acc[i][j], a[i], b[j]);
    }
  };

  stage(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  int cur = 0;
#pragma clang loop unroll(disable)
  for (int kt = 0; kt < 16; ++kt) {
    if (kt + 1 < 16) stage(cur ^ 1, kt + 1);
    compute(cur);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    cur ^= 1;
  }

  // Z into the LDS the ring occupied (every wave is past its last read: the barrier above)
  float* z = (float*)smem;
#pragma unroll
  for (int i = 0; i < 7; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = i * 16 + fk * 4 + r;
        if (row < CF_ROWS) z[row * CF_ZLD + wave * 48 + j * 16 + frow] = acc[i][j][r];
      }
  __syncthreads();

  // col2im: threads 0 .. 255 the first frame, 256 .. 511 the second; pixel = ht + 256 q
  const int slot = tid >> 8, ht = tid & 255;
  const bool live = slot < nfr;
  const float* zf = z + slot * 49 * CF_ZLD;
  float* lo = logits + (long long)(f0 + slot) * 2401;
  float v[10];
  float mx = -INFINITY;
#pragma unroll
  for (int q = 0; q < 10; ++q) {
    const int pix = ht + 256 * q;
    v[q] = -INFINITY;
    if (live && pix < 2401) {
      const int y = pix / 49, xx = pix - y * 49;
      const int m0 = y > 15 ? (y - 10) / 6 : 0, m1 = min(6, (y + 3) / 6);
      const int n0 = xx > 15 ? (xx - 10) / 6 : 0, n1 = min(6, (xx + 3) / 6);
      float a = plane[pix];
      for (int m = m0; m <= m1; ++m)
        for (int n = n0; n <= n1; ++n) a += zf[(m * 7 + n) * CF_ZLD + (y - 6 * m + 3) * HF_KP + (xx - 6 * n + 3)];
      lo[pix] = a;
      v[q] = a;
      mx = fmaxf(mx, a);
    }
  }
  if (!probs) return;                                        // (uniform: no barrier follows)
  float* red = (float*)(smem + CF_RED_OFF) + slot * 4;
  mx = cf_half_reduce<true>(mx, red, tid);
  float sum = 0.f;
#pragma unroll
  for (int q = 0; q < 10; ++q) {
    v[q] = (live && ht + 256 * q < 2401) ? __expf(v[q] - mx) : 0.f;
    sum += v[q];
  }
  sum = cf_half_reduce<false>(sum, red, tid);
  if (live) {
    const float inv = 1.0f / sum;
    float* po = probs + (long long)(f0 + slot) * 2401;
#pragma unroll
    for (int q = 0; q < 10; ++q)
      if (ht + 256 * q < 2401) po[ht + 256 * q] = v[q] * inv;
  }
}

}  // namespace rgp
