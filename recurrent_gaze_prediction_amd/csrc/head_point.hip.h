// The read-out of gaze_grcn77 (gfx950): a per-pixel 128 -> 1 product on the fp32 ConvGRU state and a 49-way softmax per
// frame -- the whole model behind the recurrence in ONE launch forward, and one launch plus a fixed-order sum backward.
// Reference graph: /root/reference/models/gaze_grcn77.py:183-212 (out_W [128,1], out_b [1]; the dropout of :209 is inert).
//
// Geometry of both kernels: one wavefront per frame, four frames per 256-thread block, no LDS.  A lane owns four
// consecutive channels (lane & 31) of one pixel of a pair (lane >> 5): a wave load instruction reads two whole 512-byte
// pixel rows as 16-byte lane loads, 25 trips cover the 49 pixels (the odd 50th is masked, not read).  The four out_W values
// a lane needs stay in registers.  A pixel's 128-term sum is the lane's four products in channel order, then a fixed xor
// butterfly over the 32 lanes of its half-wave; pixel 2i + half is kept by lane 32 half + i, so the 49 logits end up one
// per lane for the softmax (lanes 0..24: even pixels, 32..55: odd pixels).
//
// No float atomics; the order of every sum depends neither on the number of frames nor on the grid, and a frame's
// results depend on that frame's states only: equal inputs give equal bits, a NaN state poisons its own frame alone.
// Frame (b, t) reads its state [49][128] at states + b*stride_b + t*stride_t (elements), which serves the plan's
// time-major state buffer (slot t + 1 of [T+1][B]) and a caller's frame-major [B,T,49,128]; outputs are in the
// reference's frame order b*T + t.
#pragma once
#include <hip/hip_runtime.h>

namespace rgp {

constexpr int HP_PIX = 49, HP_S = 128, HP_TRIPS = 25, HP_FRAMES_PER_BLOCK = 4;

// sum over the 32 lanes of a half-wave, the same bits in each of them
__device__ __forceinline__ float hp_half_sum(float v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float hp_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
// NaN-propagating maximum over the wave (fmaxf alone drops a NaN operand)
__device__ __forceinline__ float hp_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float w = __shfl_xor(v, o);
    v = (v != v || w != w) ? __builtin_nanf("") : fmaxf(v, w);
  }
  return v;
}

// logits [F][49] (and, probs != null, their per-frame softmax with the maximum subtracted)
static __global__ __launch_bounds__(256) void head_point_fwd_kernel(const float* __restrict__ states, long long stride_b,
                                                                    long long stride_t, const float* __restrict__ out_W,
                                                                    const float* __restrict__ out_b, float* __restrict__ logits,
                                                                    float* __restrict__ probs, int F, int T) {
  const int lane = threadIdx.x & 63, half = lane >> 5, j = lane & 31;
  const int f = blockIdx.x * HP_FRAMES_PER_BLOCK + (threadIdx.x >> 6);
  if (f >= F) return;                                       // (whole waves leave: no barrier below)
  const float4 w = *(const float4*)(out_W + 4 * j);
  const float bias = out_b[0];
  const float* h = states + (long long)(f / T) * stride_b + (long long)(f % T) * stride_t + 4 * j;
  // the frame's 25 KB are asked for at once (25 loads in flight per wave: one memory latency per frame, not 25), then reduced
  float4 x[HP_TRIPS];
#pragma unroll
  for (int i = 0; i < HP_TRIPS; ++i) {
    x[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (2 * i + half < HP_PIX) x[i] = *(const float4*)(h + (2 * i + half) * HP_S);
  }
  float z = 0.f;
#pragma unroll
  for (int i = 0; i < HP_TRIPS; ++i) {
    const float s = hp_half_sum(((x[i].x * w.x + x[i].y * w.y) + x[i].z * w.z) + x[i].w * w.w);
    if (j == i) z = s + bias;
  }
  const int p = 2 * j + half;                               // this lane's pixel
  const bool valid = j < HP_TRIPS && p < HP_PIX;
  if (valid) logits[(long long)f * HP_PIX + p] = z;
  if (!probs) return;
  const float m = hp_wave_max(valid ? z : -__builtin_inff());
  const float e = valid ? expf(z - m) : 0.f;
  const float inv = 1.0f / hp_wave_sum(e);
  if (valid) probs[(long long)f * HP_PIX + p] = e * inv;
}

// d loss / d logits of the loss of gaze_rnn.py:363-408 as dlogits_kernel forms it (xentropy: (probs sum(labels) - labels)
// / F, labels are per-frame normalised; l2: (logits - labels) / F), then in the same launch
//   d_h[f][p][c]     = dlogit[f][p] out_W[c]                 the state gradient rgp_grcn_backward_from_states takes
//   part_W[f][c]     = sum_p dlogit[f][p] h[f][p][c]         pixels in order within a half-wave, then even + odd
//   part_b[f]        = sum_p dlogit[f][p]
// head_point_sum_kernel adds the per-frame partials in a fixed order.
static __global__ __launch_bounds__(256) void head_point_bwd_kernel(const float* __restrict__ states, long long stride_b,
                                                                    long long stride_t, const float* __restrict__ out_W,
                                                                    const float* __restrict__ probs_or_logits,
                                                                    const float* __restrict__ labels, int l2, float scale,
                                                                    float* __restrict__ d_h, float* __restrict__ part_W,
                                                                    float* __restrict__ part_b, int F, int T) {
  const int lane = threadIdx.x & 63, half = lane >> 5, j = lane & 31;
  const int f = blockIdx.x * HP_FRAMES_PER_BLOCK + (threadIdx.x >> 6);
  if (f >= F) return;
  const float4 w = *(const float4*)(out_W + 4 * j);
  const int pl = 2 * j + half;
  const bool valid = j < HP_TRIPS && pl < HP_PIX;
  const float a = valid ? probs_or_logits[(long long)f * HP_PIX + pl] : 0.f;
  const float g = valid ? labels[(long long)f * HP_PIX + pl] : 0.f;
  const float gs = l2 ? 0.f : hp_wave_sum(g);
  const float d = valid ? (l2 ? (a - g) : (a * gs - g)) * scale : 0.f;
  const float db = hp_wave_sum(d);
  if (lane == 0) part_b[f] = db;
  const float* h = states + (long long)(f / T) * stride_b + (long long)(f % T) * stride_t + 4 * j;
  float* dh = d_h + (long long)f * HP_PIX * HP_S + 4 * j;
  float4 x[HP_TRIPS];                                       // (all loads of the frame in flight at once, as in the forward)
#pragma unroll
  for (int i = 0; i < HP_TRIPS; ++i) {
    x[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (2 * i + half < HP_PIX) x[i] = *(const float4*)(h + (2 * i + half) * HP_S);
  }
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int i = 0; i < HP_TRIPS; ++i) {
    const int p = 2 * i + half;
    const float dp = __shfl(d, 32 * half + i);              // the lane that holds pixel p (0 for the masked 50th)
    acc.x += dp * x[i].x; acc.y += dp * x[i].y; acc.z += dp * x[i].z; acc.w += dp * x[i].w;
    if (p < HP_PIX) *(float4*)(dh + p * HP_S) = make_float4(dp * w.x, dp * w.y, dp * w.z, dp * w.w);
  }
  acc.x += __shfl_xor(acc.x, 32); acc.y += __shfl_xor(acc.y, 32);
  acc.z += __shfl_xor(acc.z, 32); acc.w += __shfl_xor(acc.w, 32);
  if (half == 0) *(float4*)(part_W + (long long)f * HP_S + 4 * j) = acc;
}

// d out_W[c] = sum_f part_W[f][c] (blocks 0..7: 16 channels each), d out_b = sum_f part_b[f] (block 8).  A thread adds every
// 16th frame in order, then one thread per column adds the 16 lanes in order: no atomics, one order for a given F.
static __global__ __launch_bounds__(256) void head_point_sum_kernel(const float* __restrict__ part_W, const float* __restrict__ part_b,
                                                                    float* __restrict__ d_W, float* __restrict__ d_b, int F) {
  __shared__ float sh[16][17];
  const int c = threadIdx.x & 15, r = threadIdx.x >> 4;
  const bool is_b = blockIdx.x == HP_S / 16;
  float a = 0.f;
  if (!is_b) {
#pragma unroll 16
    for (int f = r; f < F; f += 16) a += part_W[(long long)f * HP_S + blockIdx.x * 16 + c];
  } else if (c == 0) {
#pragma unroll 16
    for (int f = r; f < F; f += 16) a += part_b[f];
  }
  sh[r][c] = a;
  __syncthreads();
  if (r == 0 && (!is_b || c == 0)) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) s += sh[k][c];
    if (is_b) d_b[0] = s; else d_W[blockIdx.x * 16 + c] = s;
  }
}

}  // namespace rgp
