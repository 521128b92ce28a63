// Kernels of the action classifier on gaze-attended C3D features (rgp_action.hip; reference graph
// models/action_classification.py:210-292).  The first layer is a K = 49*C -> N fully connected layer at a batch of at most
// 64 rows: a weight-streaming problem.  Three kernels carry it:
//
//   action_fc1_fwd_kernel     split-K skinny GEMM.  A block owns one slab of ACT_KS rows of W1 (and 64 of its columns); the
//                             attention multiply x[b,k] = c3d[b,k] * a[b,k%49] is applied to the A operand as it is loaded,
//                             x is never written.  W1 is read from the plan's operand copy [Kp][Npad] (bf16 or f32).  Every
//                             slab STORES its partial sums into a slice of its own (no float atomics) ...
//   action_tail_kernel        ... which one workgroup adds in slab order, then runs the rest of the network, the loss and
//   action_svm_tail_kernel    (training plans) every small gradient in fp32.
//   action_fc1_update_kernel  one pass over W1, m and v: a wave owns 16 rows of W1 and all 256 columns.  Per 16-byte chunk
//                             of a row it forms dx (an MFMA over the chunk's columns, from the values BEFORE the update),
//                             the gradient g[k,n] = sum_b x[b,k] dh1[b,n] in registers (x recomputed from c3d and a), the
//                             Adam update in place and the refreshed operand copy.  dW1 never exists in memory.
//
// Lane maps (igemm.hip.h, Mma<T>): a 16-byte fragment holds CH = 8 (bf16) / 4 (f32) consecutive values of the contraction
// index; lane l = (r = l & 15, g = l >> 4) holds row/column r and chunk g of a 4*CH wide step.  The forward contracts over
// k, the update's dx over n: the update kernel therefore reads W1 in its own [K][N] layout (n contiguous, 16-byte loads)
// and the forward gathers its k-strided fragment element by element from the same layout (25.7 MB per forward at C = 1024).
#pragma once
#include "igemm.hip.h"
#include "kernels_misc.hip.h"

namespace rgp {

constexpr int ACT_KS = 512;          // rows of W1 per forward slab
constexpr int ACT_NH = 256;          // hidden width (action_classification.py:269-270)
constexpr int ACT_NC = 13;           // classes
constexpr int ACT_GM = 2401;         // gaze map pixels
constexpr int ACT_P = 49;            // feature map pixels
constexpr int ACT_UPD_ROWS = 64;     // rows of W1 per update block (16 per wave)
constexpr int ACT_LDD = ACT_NH + 4;  // LDS row stride of dh1 in the update kernel (16-byte reads of 16 rows: no bank conflict)
constexpr float ACT_SVM_C = 50.f;    // svmC (action_classification.py:250)

template <typename T> __device__ __forceinline__ f32x4 act_frag(const float* v);
template <> __device__ __forceinline__ f32x4 act_frag<float>(const float* v) { return (f32x4){v[0], v[1], v[2], v[3]}; }
template <> __device__ __forceinline__ f32x4 act_frag<bf16_t>(const float* v) {
  u32x4 pk;
#pragma unroll
  for (int i = 0; i < 4; ++i) pk[i] = (unsigned)f2bf(v[2 * i]) | ((unsigned)f2bf(v[2 * i + 1]) << 16);
  return __builtin_bit_cast(f32x4, pk);
}

__device__ __forceinline__ float act_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// a[b][p] = sum_q gazemap[b][q] Wg[q][p] (fp32).  One block per sample: 16 q-parts x 64 lanes (p), the parts added in order.
static __global__ __launch_bounds__(1024) void action_gaze_proj_kernel(const float* __restrict__ gm, const float* __restrict__ Wg,
                                                                       float* __restrict__ a) {
  __shared__ float sh[16][64];
  const int b = blockIdx.x, p = threadIdx.x & 63, part = threadIdx.x >> 6;
  float s = 0.f;
  if (p < ACT_P)
    for (int q = part; q < ACT_GM; q += 16) s += gm[(long long)b * ACT_GM + q] * Wg[q * ACT_P + p];
  sh[part][p] = s;
  __syncthreads();
  if (part == 0 && p < ACT_P) {
    float r = sh[0][p];
    for (int i = 1; i < 16; ++i) r += sh[i][p];
    a[b * ACT_P + p] = r;
  }
}

// conv5b rows [B*49][1024] (operand dtype, column d*512+c', reference channel c = 2c'+d) -> c3d [B][1024][49] fp32
template <typename T>
static __global__ __launch_bounds__(256) void action_rows_to_c3d_kernel(const T* __restrict__ rows, float* __restrict__ c3d, long long n) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int p = (int)(i % ACT_P), c = (int)((i / ACT_P) % 1024);
    const long long b = i / (ACT_P * 1024);
    c3d[i] = Elem<T>::from(rows[(b * ACT_P + p) * 1024 + (c & 1) * 512 + (c >> 1)]);
  }
}

// operand copy of W1: dst [Kp][Npad] (padding stays zero) = src [K][N]
template <typename T>
static __global__ __launch_bounds__(256) void action_pack_kernel(const float* __restrict__ src, T* __restrict__ dst, long long total, int N,
                                                                  int Npad) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long k = i / N;
    dst[k * Npad + (int)(i - k * N)] = Elem<T>::to(src[i]);
  }
}

// Partial sums of one slab: part[slab][b][n] (b < B, n < N) = sum over the slab's rows k of x[b,k] W1[k,n].
// grid (slabs, ceil(Npad / 64)), one 16-column tile per wave.  a == null: x = c3d (no attention, or x materialised).
// wsq (SVM): wsq[slab] = sum of squares of the slab's rows of the fp32 master `wmaster` [K][N], for the regulariser.
template <typename T, int MT>
static __global__ __launch_bounds__(256) void action_fc1_fwd_kernel(const float* __restrict__ c3d, const float* __restrict__ a,
                                                                    const T* __restrict__ w1op, float* __restrict__ part,
                                                                    const float* __restrict__ wmaster, float* __restrict__ wsq, int B,
                                                                    int K, int N, int Npad) {
  constexpr int CH = 16 / (int)sizeof(T), KSTEP = 4 * CH;
  __shared__ float a_s[64 * ACT_P];
  const int slab = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
  if (a) {
    for (int i = threadIdx.x; i < B * ACT_P; i += blockDim.x) a_s[i] = a[i];
    __syncthreads();
  }
  if (wsq && blockIdx.y == 0 && wave == 0) {
    const long long lo = (long long)slab * ACT_KS * N, hi = (long long)min(K, (slab + 1) * ACT_KS) * N;
    float s = 0.f;
    for (long long i = lo + lane; i < hi; i += 64) s += wmaster[i] * wmaster[i];
    s = act_wave_sum(s);
    if (lane == 0) wsq[slab] = s;
  }
  const int n0 = (blockIdx.y * 4 + wave) * 16;
  if (n0 >= Npad) return;
  f32x4 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
  for (int ks = 0; ks < ACT_KS; ks += KSTEP) {
    const int kb = slab * ACT_KS + ks + g * CH;
    const T* wp = w1op + (long long)kb * Npad + n0 + r;          // (rows up to Kp exist and are zero beyond K)
    f32x4 wf;
    if constexpr (sizeof(T) == 2) {
      u32x4 pk;
#pragma unroll
      for (int i = 0; i < 4; ++i) pk[i] = (unsigned)wp[(2 * i) * Npad] | ((unsigned)wp[(2 * i + 1) * Npad] << 16);
      wf = __builtin_bit_cast(f32x4, pk);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) wf[i] = wp[i * Npad];
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int b = mt * 16 + r;
      float xv[CH];
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const int k = kb + j;
        float x = 0.f;
        if (b < B && k < K) {
          x = c3d[(long long)b * K + k];
          if (a) x *= a_s[b * ACT_P + k % ACT_P];
        }
        xv[j] = x;
      }
      Mma<T>::step(acc[mt], act_frag<T>(xv), wf);
    }
  }
  const int n = n0 + r;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int b = mt * 16 + g * 4 + i;
      if (b < B && n < N) part[((long long)slab * B + b) * N + n] = acc[mt][i];
    }
}

struct ActionTailArgs {
  const float *part, *wsq;                       // per-slab partial sums [nslab][B][N]; SVM: per-slab sums of squares of W
  int nslab, B, train;
  const float *b1, *W2, *b2, *W3, *b3, *labels;  // fp32 masters; labels null = no loss
  float *h1, *h2, *logits, *ypred, *dlog, *dh2, *dh1, *loss;
  float *logits_out, *ypred_out, *loss_out;      // the caller's (may be null)
  float *g_b1, *g_W2, *g_b2, *g_W3, *g_b3;       // gradients (training)
};

// NN mode, one workgroup, fp32: h1 = sum of the slabs (in slab order) + b1, h2 = h1 W2 + b2, logits = h2 W3 + b3, sigmoid,
// mean sigmoid cross entropy; training: d logits, d h2, d h1 and the gradients of W2, W3, b1, b2, b3.  Every sum runs in a
// fixed order.  (The intermediates live in global memory; a workgroup's waves share the CU's L1 and __syncthreads orders them.)
static __global__ __launch_bounds__(1024) void action_tail_kernel(ActionTailArgs p) {
  __shared__ float sh[16];
  const int t = threadIdx.x, col = t & 255, bq = t >> 8, B = p.B;
  constexpr int H = ACT_NH, NC = ACT_NC;
  for (int b = bq; b < B; b += 4) {
    float s = 0.f;
    for (int sl = 0; sl < p.nslab; ++sl) s += p.part[((long long)sl * B + b) * H + col];
    p.h1[b * H + col] = s + p.b1[col];
  }
  __syncthreads();
  {
    float acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int n = 0; n < H; ++n) {
      const float w = p.W2[n * H + col];
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (bq + 4 * i < B) acc[i] += p.h1[(bq + 4 * i) * H + n] * w;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (bq + 4 * i < B) p.h2[(bq + 4 * i) * H + col] = acc[i] + p.b2[col];
  }
  __syncthreads();
  float l = 0.f;
  if (t < B * NC) {
    const int b = t / NC, c = t % NC;
    float z = 0.f;
    for (int j = 0; j < H; ++j) z += p.h2[b * H + j] * p.W3[j * NC + c];
    z += p.b3[c];
    const float yp = 1.f / (1.f + expf(-z));
    p.logits[t] = z;
    p.ypred[t] = yp;
    if (p.logits_out) p.logits_out[t] = z;
    if (p.ypred_out) p.ypred_out[t] = yp;
    if (p.labels) {
      const float y = p.labels[t];
      l = fmaxf(z, 0.f) - z * y + log1pf(expf(-fabsf(z)));
      p.dlog[t] = (yp - y) / (float)(B * NC);
    }
  }
  if (!p.labels) return;
  l = block_reduce(l, sh, false);
  if (t == 0) {
    const float loss = l / (float)(B * NC);
    *p.loss = loss;
    if (p.loss_out) *p.loss_out = loss;
  }
  if (!p.train) return;
  __syncthreads();
  for (int b = bq; b < B; b += 4) {
    float s = 0.f;
    for (int c = 0; c < NC; ++c) s += p.dlog[b * NC + c] * p.W3[col * NC + c];
    p.dh2[b * H + col] = s;
  }
  for (int i = t; i < H * NC; i += 1024) {
    const int j = i / NC, c = i % NC;
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += p.h2[b * H + j] * p.dlog[b * NC + c];
    p.g_W3[i] = s;
  }
  if (t < NC) {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += p.dlog[b * NC + t];
    p.g_b3[t] = s;
  }
  __syncthreads();
  {  // d h1[b][n] = sum_j d h2[b][j] W2[n][j]: a wave per row n of W2, lanes over j
    const int wave = t >> 6, lane = t & 63;
    for (int n = wave; n < H; n += 16) {
      float w[4];                                    // (W2 sits behind Wg in the caller's flat buffer: 4-byte aligned only)
#pragma unroll
      for (int i = 0; i < 4; ++i) w[i] = p.W2[n * H + lane + 64 * i];
      for (int b = 0; b < B; ++b) {
        float d[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) d[i] = p.dh2[b * H + lane + 64 * i];
        const float s = act_wave_sum((d[0] * w[0] + d[1] * w[1]) + (d[2] * w[2] + d[3] * w[3]));
        if (lane == 0) p.dh1[b * H + n] = s;
      }
    }
  }
  for (int n = bq; n < H; n += 4) {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += p.h1[b * H + n] * p.dh2[b * H + col];
    p.g_W2[n * H + col] = s;
  }
  if (bq == 0) {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += p.dh2[b * H + col];
    p.g_b2[col] = s;
  }
  __syncthreads();
  if (bq == 0) {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += p.dh1[b * H + col];
    p.g_b1[col] = s;
  }
}

// SVM mode (action_classification.py:242-263): y = sum of the slabs + b; loss = 0.5 sum W^2 + 50 sum max(0, 1 - labels y).
// d h1 = d (hinge sum) / d y = -labels where 1 - labels y > 0 (strictly), else 0: the factor 50 is applied by the update.
// Labels stay {0, 1} as the reference writes them: a zero label adds the constant 1 to the hinge sum and no gradient.
static __global__ __launch_bounds__(1024) void action_svm_tail_kernel(ActionTailArgs p) {
  __shared__ float sh[16];
  const int t = threadIdx.x, B = p.B;
  constexpr int NC = ACT_NC;
  float hl = 0.f;
  if (t < B * NC) {
    const int b = t / NC, c = t % NC;
    float y = 0.f;
    for (int sl = 0; sl < p.nslab; ++sl) y += p.part[((long long)sl * B + b) * NC + c];
    y += p.b1[c];
    p.h1[t] = y;
    if (p.logits_out) p.logits_out[t] = y;
    if (p.ypred_out) p.ypred_out[t] = y;
    if (p.labels) {
      const float lab = p.labels[t], mrg = 1.f - lab * y;
      hl = fmaxf(mrg, 0.f);
      p.dh1[t] = mrg > 0.f ? -lab : 0.f;
    }
  }
  if (!p.labels) return;
  hl = block_reduce(hl, sh, false);
  if (t == 0) {
    float reg = 0.f;
    for (int sl = 0; sl < p.nslab; ++sl) reg += p.wsq[sl];
    const float loss = 0.5f * reg + ACT_SVM_C * hl;
    *p.loss = loss;
    if (p.loss_out) *p.loss_out = loss;
  }
  if (!p.train) return;
  __syncthreads();
  if (t < NC) {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += p.dh1[b * NC + t];
    p.g_b1[t] = ACT_SVM_C * s;
  }
}

// The fused update pass of the NN plans (N = 256).  Block = 4 waves = 64 rows of W1; dynamic LDS: dh1 [16*MT][ACT_LDD]
// (rows >= B zero) + x [16*MT][64] (rows < B used).  dx (null: not wanted) [B][K] is computed from W1 as read, before the update.
// Adam in the TF form of adam_clip_kernel (no clipping): m = b1 m + c1 g; v = b2 v + c2 g^2; w -= lr_t m / (sqrt(v) + eps), with
// c1 = 1 - beta1 and c2 = 1 - beta2 rounded from double by the host (1.f - 0.999f is 1.3e-5 away from 0.001: v would carry that).
template <typename T, int MT>
static __global__ __launch_bounds__(256) void action_fc1_update_kernel(const float* __restrict__ c3d, const float* __restrict__ a,
                                                                       const float* __restrict__ dh1, float* __restrict__ W,
                                                                       float* __restrict__ m, float* __restrict__ v, T* __restrict__ w1op,
                                                                       float* __restrict__ dx, int B, int K, float lr_t, float b1, float b2,
                                                                       float c1, float c2, float eps) {
  constexpr int CH = 16 / (int)sizeof(T), S = ACT_NH / (4 * CH), F4 = CH / 4;
  extern __shared__ __attribute__((aligned(16))) float act_sm[];
  float* dh_s = act_sm;
  float* x_s = act_sm + 16 * MT * ACT_LDD;
  const int k0 = blockIdx.x * ACT_UPD_ROWS;
  for (int i = threadIdx.x; i < 16 * MT * ACT_NH; i += 256) {
    const int b = i >> 8, n = i & 255;
    dh_s[b * ACT_LDD + n] = b < B ? dh1[b * ACT_NH + n] : 0.f;
  }
  for (int i = threadIdx.x; i < B * ACT_UPD_ROWS; i += 256) {
    const int b = i >> 6, k = k0 + (i & 63);
    float x = 0.f;
    if (k < K) {
      x = c3d[(long long)b * K + k];
      if (a) x *= a[b * ACT_P + k % ACT_P];
    }
    x_s[i] = x;
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
  const int kr = wave * 16 + r, k = k0 + kr;
  const bool valid = k < K;
  f32x4 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < S; ++s) {
    const int n0 = s * 4 * CH + g * CH;
    const long long o = (long long)k * ACT_NH + n0;
    float wv[CH], mv[CH], vv[CH], gv[CH];
#pragma unroll
    for (int q = 0; q < F4; ++q) {
      const f32x4 z = (f32x4){0.f, 0.f, 0.f, 0.f};
      const f32x4 w4 = valid ? *(const f32x4*)(W + o + 4 * q) : z, m4 = valid ? *(const f32x4*)(m + o + 4 * q) : z,
                  v4 = valid ? *(const f32x4*)(v + o + 4 * q) : z;
#pragma unroll
      for (int j = 0; j < 4; ++j) { wv[4 * q + j] = w4[j]; mv[4 * q + j] = m4[j]; vv[4 * q + j] = v4[j]; gv[4 * q + j] = 0.f; }
    }
    if (dx) {
      const f32x4 wf = act_frag<T>(wv);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) Mma<T>::step(acc[mt], act_frag<T>(dh_s + (mt * 16 + r) * ACT_LDD + n0), wf);
    }
    for (int b = 0; b < B; ++b) {
      const float xv = x_s[b * ACT_UPD_ROWS + kr];
      const float* d = dh_s + b * ACT_LDD + n0;
#pragma unroll
      for (int j = 0; j < CH; ++j) gv[j] += xv * d[j];
    }
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      mv[j] = b1 * mv[j] + c1 * gv[j];
      vv[j] = b2 * vv[j] + c2 * gv[j] * gv[j];
      wv[j] -= lr_t * mv[j] / (sqrtf(vv[j]) + eps);
    }
    if (valid) {
#pragma unroll
      for (int q = 0; q < F4; ++q) {
        *(f32x4*)(W + o + 4 * q) = (f32x4){wv[4 * q], wv[4 * q + 1], wv[4 * q + 2], wv[4 * q + 3]};
        *(f32x4*)(m + o + 4 * q) = (f32x4){mv[4 * q], mv[4 * q + 1], mv[4 * q + 2], mv[4 * q + 3]};
        *(f32x4*)(v + o + 4 * q) = (f32x4){vv[4 * q], vv[4 * q + 1], vv[4 * q + 2], vv[4 * q + 3]};
      }
      *(f32x4*)(w1op + o) = act_frag<T>(wv);
    }
  }
  if (dx) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int b = mt * 16 + g * 4 + i;
        if (b < B && valid) dx[(long long)b * K + k] = acc[mt][i];
      }
  }
}

// The fused update pass of the SVM plans: W [K][13] is 2.6 MB at C = 1024, a thread owns a row.  SGD on
// 0.5 sum W^2 + 50 hinge: W -= lr (W + 50 g), g[k,n] = sum_b x[b,k] dh[b,n]; dx[b,k] = 50 sum_n dh[b,n] W[k,n] (before the update).
template <typename T>
static __global__ __launch_bounds__(256) void action_svm_update_kernel(const float* __restrict__ c3d, const float* __restrict__ a,
                                                                       const float* __restrict__ dh, float* __restrict__ W,
                                                                       T* __restrict__ wop, float* __restrict__ dx, int B, int K, float lr) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  float w[ACT_NC], gv[ACT_NC];
#pragma unroll
  for (int n = 0; n < ACT_NC; ++n) { w[n] = W[(long long)k * ACT_NC + n]; gv[n] = 0.f; }
  for (int b = 0; b < B; ++b) {
    float x = c3d[(long long)b * K + k];
    if (a) x *= a[b * ACT_P + k % ACT_P];
    float s = 0.f;
#pragma unroll
    for (int n = 0; n < ACT_NC; ++n) {
      const float d = dh[b * ACT_NC + n];
      gv[n] += x * d;
      s += d * w[n];
    }
    if (dx) dx[(long long)b * K + k] = ACT_SVM_C * s;
  }
#pragma unroll
  for (int n = 0; n < ACT_NC; ++n) {
    w[n] -= lr * (w[n] + ACT_SVM_C * gv[n]);
    W[(long long)k * ACT_NC + n] = w[n];
    wop[(long long)k * 16 + n] = Elem<T>::to(w[n]);
  }
}

// d a[b][p] = sum_c c3d[b][c][p] dx[b][c*49+p]: one block per sample, 16 c-parts x 64 lanes (p), the parts added in order
static __global__ __launch_bounds__(1024) void action_da_kernel(const float* __restrict__ c3d, const float* __restrict__ dx,
                                                                float* __restrict__ da, int C) {
  __shared__ float sh[16][64];
  const int b = blockIdx.x, p = threadIdx.x & 63, part = threadIdx.x >> 6;
  float s = 0.f;
  if (p < ACT_P)
    for (int c = part; c < C; c += 16) {
      const long long i = ((long long)b * C + c) * ACT_P + p;
      s += c3d[i] * dx[i];
    }
  sh[part][p] = s;
  __syncthreads();
  if (part == 0 && p < ACT_P) {
    float r = sh[0][p];
    for (int i = 1; i < 16; ++i) r += sh[i][p];
    da[b * ACT_P + p] = r;
  }
}

// d Wg[q][p] = sum_b gazemap[b][q] d a[b][p]
static __global__ __launch_bounds__(256) void action_dwg_kernel(const float* __restrict__ gm, const float* __restrict__ da,
                                                                float* __restrict__ dWg, int B) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= ACT_GM * ACT_P) return;
  const int q = i / ACT_P, p = i % ACT_P;
  float s = 0.f;
  for (int b = 0; b < B; ++b) s += gm[(long long)b * ACT_GM + q] * da[b * ACT_P + p];
  dWg[i] = s;
}

// plain SGD on a small variable: p -= lr g
static __global__ __launch_bounds__(256) void action_sgd_kernel(float* __restrict__ p, const float* __restrict__ g, long long n, float lr) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) p[i] -= lr * g[i];
}

// ---- the second implementation (RGP_ACTION_UNFUSED): x, dW1 and dx exist in memory

static __global__ __launch_bounds__(256) void action_x_kernel(const float* __restrict__ c3d, const float* __restrict__ a,
                                                              float* __restrict__ x, int K, long long total) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long b = i / K;
    const int k = (int)(i - b * K);
    x[i] = c3d[i] * a[b * ACT_P + k % ACT_P];
  }
}

// dW[k][n] = sum_b x[b][k] dh[b][n]
static __global__ __launch_bounds__(256) void action_dw1_plain_kernel(const float* __restrict__ x, const float* __restrict__ dh,
                                                                      float* __restrict__ dW, int B, int K, int N) {
  const long long total = (long long)K * N;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long k = i / N;
    const int n = (int)(i - k * N);
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += x[(long long)b * K + k] * dh[b * N + n];
    dW[i] = s;
  }
}

// dx[b][k] = scale sum_n dh[b][n] W[k][n]: a wave per row k, lanes over n (N <= 256)
static __global__ __launch_bounds__(256) void action_dx_plain_kernel(const float* __restrict__ W, const float* __restrict__ dh,
                                                                     float* __restrict__ dx, int B, int K, int N, float scale) {
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (k >= K) return;
  float w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = lane + 64 * i < N ? W[(long long)k * N + lane + 64 * i] : 0.f;
  for (int b = 0; b < B; ++b) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (lane + 64 * i < N) s += dh[b * N + lane + 64 * i] * w[i];
    s = act_wave_sum(s);
    if (lane == 0) dx[(long long)b * K + k] = scale * s;
  }
}

// SVM: W -= lr (W + 50 dW)
static __global__ __launch_bounds__(256) void action_sgd_l2_kernel(float* __restrict__ W, const float* __restrict__ dW, long long n, float lr) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    W[i] -= lr * (W[i] + ACT_SVM_C * dW[i]);
}

}  // namespace rgp
