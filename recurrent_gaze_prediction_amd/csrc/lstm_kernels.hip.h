// gaze_lstm, per-step path and backward (rgp_lstm.hip): the epilogue of the per-timestep recurrent GEMM and the
// element-wise kernels of the BPTT.  Cell: /root/reference/models/gaze_lstm.py:103-133 (see convlstm_seq.hip.h).
#pragma once
#include "igemm.hip.h"

namespace rgp {

// Epilogue of the recurrent GEMM of one step: GEMM columns are INTERLEAVED by channel, column 4 c + q with q = 0 W_hi*h,
// 1 W_hf*h, 2 unused (zero filter rows: g reuses column 0, gaze_lstm.py:125), 3 W_ho*h -- an epilogue item is 8 consecutive
// columns of one row, so it holds everything of two channels; the hoisted x parts (xpre) use the same column order
// (q = i, f, g, o).  Adds xpre, applies the peepholes on the OLD c (:117, :121, :130), updates c and h, writes the fp32
// states, the gates (training) and the halo-padded operand image of h_t (the next step's input and the head's).
// EpiParams fields as used here (the struct is shared and stays as it is): xpre / xpre_img_stride / xpre_ld; S, state_rows;
// h_prev = c_{t-1}, h_next = c_t, u_gate = h_t (all [img][49][S] fp32); r_save = gates of this step (i; f, g, o follow at
// multiples of out2_img_mul elements) or null; bn_gamma = the peephole planes [3][49][S]; out (+ out_extra) = operand image.
template <typename T> struct EpiLstm {
  static __device__ __forceinline__ void apply(const EpiParams& e, int N, int img, int ml, int n0, float* v) {
    apply_at(e, N, img, ml, epi_out_base(e, img, ml), n0, v);
  }
  static __device__ __forceinline__ void apply_at(const EpiParams& e, int N, int img, int ml, long long base, int n0, float* v) {
    if (n0 >= N) return;
    const float* xp = e.xpre + (long long)img * e.xpre_img_stride + (long long)ml * e.xpre_ld + n0;
    const f32x4 x0 = *(const f32x4*)xp, x1 = *(const f32x4*)(xp + 4);
    const int c0 = n0 >> 2;
    const long long srow = ((long long)img * e.state_rows + ml) * e.S + c0;
    const float* pp = e.bn_gamma + (long long)ml * e.S + c0;
    const long long ps = (long long)e.state_rows * e.S;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const f32x4 x = k ? x1 : x0;
      const float cp = e.h_prev[srow + k];
      const float si = v[4 * k], sf = v[4 * k + 1], so = v[4 * k + 3];
      const float ig = sigmoidf_(si + x[0] + pp[k] * cp);
      const float fg = sigmoidf_(sf + x[1] + pp[ps + k] * cp);
      const float gg = tanhf_(si + x[2]);
      const float og = sigmoidf_(so + x[3] + pp[2 * ps + k] * cp);
      const float cn = fg * cp + ig * gg;
      const float hn = tanhf_(cn) * og;
      e.h_next[srow + k] = cn;
      e.u_gate[srow + k] = hn;
      if (e.r_save) {
        float* gs = e.r_save + srow + k;
        gs[0] = ig; gs[e.out2_img_mul] = fg; gs[2 * e.out2_img_mul] = gg; gs[3 * e.out2_img_mul] = og;
      }
      ((T*)e.out)[base + c0 + k] = Elem<T>::to(hn);
    }
  }
};

// Column blocks of the padded gradient image dpre [frame][81][5 S] (operand dtype): g | i | i+g | f | o.  The input
// filters' gradients read blocks 0, 1, 3, 4; the recurrent filters' read 2, 3, 4 -- one contiguous 3 S run, which is
// also the operand of the per-step input-gradient GEMM (d(W_hi*h) = d i_pre + d g_pre, gaze_lstm.py:116,125).
constexpr int LSTM_DG = 0, LSTM_DI = 1, LSTM_DIG = 2, LSTM_DF = 3, LSTM_DO = 4;

// One BPTT step, element-wise: dh = dh_head(b, t) + dh_carry; through h' = tanh(c').o, c' = f.c + i.g and the three
// peepholes on the old c.  Writes the five column blocks of frame (b, t) of dpre and the new dc carry.
template <typename T>
__global__ __launch_bounds__(256) void lstm_bwd_step_kernel(const float* __restrict__ dh_head, const float* __restrict__ dh_carry,
                                                            float* __restrict__ dc_carry, const float* __restrict__ gates,
                                                            const float* __restrict__ call, const float* __restrict__ peep,
                                                            T* __restrict__ dpre, int B, int T_, int t, int S, int first) {
  const long long st = (long long)B * 49 * S, gs = (long long)T_ * st;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < st; i += (long long)gridDim.x * 256) {
    const int ch = (int)(i % S), pos = (int)((i / S) % 49), b = (int)(i / (49LL * S));
    const long long go = (long long)t * st + i;
    const float ig = gates[go], fg = gates[gs + go], gg = gates[2 * gs + go], og = gates[3 * gs + go];
    const float cp = call[(long long)t * st + i], cn = call[(long long)(t + 1) * st + i];
    const float dh = dh_head[(((long long)b * T_ + t) * 49 + pos) * S + ch] + (first ? 0.f : dh_carry[i]);
    const float tc = tanhf_(cn);
    const float d_o = dh * tc * og * (1.f - og);
    const float dc = (first ? 0.f : dc_carry[i]) + dh * og * (1.f - tc * tc);
    const float d_i = dc * gg * ig * (1.f - ig);
    const float d_f = dc * cp * fg * (1.f - fg);
    const float d_g = dc * ig * (1.f - gg * gg);
    const float* pp = peep + (long long)pos * S + ch;
    dc_carry[i] = dc * fg + d_i * pp[0] + d_f * pp[49LL * S] + d_o * pp[98LL * S];
    T* d = dpre + ((((long long)b * T_ + t) * 81 + (pos / 7 + 1) * 9 + pos % 7 + 1) * 5) * S + ch;
    d[LSTM_DG * S] = Elem<T>::to(d_g); d[LSTM_DI * S] = Elem<T>::to(d_i); d[LSTM_DIG * S] = Elem<T>::to(d_i + d_g);
    d[LSTM_DF * S] = Elem<T>::to(d_f); d[LSTM_DO * S] = Elem<T>::to(d_o);
  }
}

// Peephole gradients d W_c{i,f,o}[pos, ch] = sum over frames of d{i,f,o}_pre . c_{t-1}: one thread per element, a chain
// over the steps of a clip inside a chain over the clips -- a fixed order, no atomics.  B * T dependent strided loads
// per thread (1024 at 64 x 16) on 18 816 threads: 313 us at 64 x 16, 76 us at 8 x 35 ("gaze_lstm").
template <typename T>
__global__ __launch_bounds__(256) void lstm_peephole_grad_kernel(const T* __restrict__ dpre, const float* __restrict__ call,
                                                                 float* __restrict__ d_ci, float* __restrict__ d_cf,
                                                                 float* __restrict__ d_co, int B, int T_, int S) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 3 * 49 * S) return;
  const int ch = i % S, pos = (i / S) % 49, plane = i / (49 * S);
  const int blk = plane == 0 ? LSTM_DI : plane == 1 ? LSTM_DF : LSTM_DO;
  const long long st = (long long)B * 49 * S;
  float acc = 0.f;
  for (int b = 0; b < B; ++b) {
    float a = 0.f;
    for (int t = 0; t < T_; ++t) {
      const float d = Elem<T>::from(dpre[((((long long)b * T_ + t) * 81 + (pos / 7 + 1) * 9 + pos % 7 + 1) * 5 + blk) * S + ch]);
      a += d * call[(long long)t * st + ((long long)b * 49 + pos) * S + ch];
    }
    acc += a;
  }
  (plane == 0 ? d_ci : plane == 1 ? d_cf : d_co)[pos * S + ch] = acc;
}

// Column block `blk` of dpre [frame][81][5 S], un-padded, as fp32 [frame][49][S] (read_buffer)
template <typename T>
__global__ __launch_bounds__(256) void lstm_dpre_block_kernel(const T* __restrict__ dpre, float* __restrict__ dst, int blk, int S,
                                                              long long total) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int ch = (int)(i % S), pos = (int)((i / S) % 49);
    const long long frame = i / (49LL * S);
    dst[i] = Elem<T>::from(dpre[((frame * 81 + (pos / 7 + 1) * 9 + pos % 7 + 1) * 5 + blk) * S + ch]);
  }
}

// [T,B,49,S] -> [B,T,49,S] (read_buffer)
static __global__ void lstm_tb_to_bt_kernel(const float* __restrict__ src, float* __restrict__ dst, int T_, int B_, long long inner) {
  const long long total = (long long)T_ * B_ * inner;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long in = i % inner;
    const int t = (int)((i / inner) % T_);
    const int b = (int)(i / (inner * T_));
    dst[i] = src[((long long)t * B_ + b) * inner + in];
  }
}

}  // namespace rgp
