// Persistent ConvLSTM sequence kernel (gfx950, bf16 operands): ALL T steps of LSTM_RCN_Cell.__call__
// (/root/reference/models/gaze_lstm.py:103-133, unrolled at :270-286) in ONE launch, on the group scheme of
// seq_group.hip.h (decomposition, exchange protocol, time-out), with the cell's own shape:
//
//   i = sigmoid(W_xi*x + W_hi*h + W_ci.c)     f = sigmoid(W_xf*x + W_hf*h + W_cf.c)
//   g = tanh(W_xc*x + W_hi*h)                  (:125 reuses W_hi; W_hc is never read)
//   c' = f.c + i.g       o = sigmoid(W_xo*x + W_ho*h + W_co.c)   (:130 the OLD c)      h' = tanh(c').o
//
// All four gates read h_{t-1} only, so a step has ONE group hand-off (h'), where the ConvGRU has two (r.h, h').  There are
// three distinct recurrent filters (W_hi, W_hf, W_ho): member j of a group of 8 workgroups keeps their columns of state
// channels [16j, 16j+16) in registers -- 3 x 16 columns x K = 1152, 108 VGPRs per lane, the ConvGRU's z / r / c budget --
// split over its 4 waves as K quarters, plus its slice of the three peephole planes [7,7,128] (24 VGPRs: a lane's 8 rows
// x 3 planes).  c of a tile lives in fp32 in the registers of the wave that finalises it for the whole sequence; h is
// needed only as the bf16 operand image (LDS), which is what the exchange delivers.
// LDS: one 9x9 operand image pair (50 592 B) + 4 waves x 7 fragments x 3 gates partial tiles (84 KiB) + staging = 138 672 B.
//
// The h' exchange image is double-buffered by step parity: with one hand-off per step nothing else separates a fast
// member's stores of step t+1 from a slow member's loads of step t.  (A member can be at most one step ahead: its
// wait for step t+1 needs everybody's arrival, which follows everybody's loads of step t.)
// No float atomics; a clip's bits depend on neither its group slot nor the batch size (NF only pads with zero rows).
#pragma once
#include "seq_group.hip.h"

namespace rgp {

struct LstmSeqParams {
  const bf16_t* w_rec;       // packed [512][K]: row 4 c + q, q = 0 W_hi, 1 W_hf, 3 W_ho (2 stays zero); K = tap*128 + channel
  const float* xpre;         // [B][T][49][512] hoisted x parts, column 4 c + q, q = i, f, g, o
  const float* peep;         // [3][49][128] W_ci, W_cf, W_co
  float* hall;               // [T+1][B][49][128] fp32 h (slot 0 = the zero state, or seeded by a streaming call)
  float* call;               // [T+1][B][49][128] fp32 c
  float* gates;              // optional (training): [4][T][B][49][128] i, f, g, o
  bf16_t* hseq;              // [B][T+1][81][128] halo-padded h_t at slot t+1 (slot 0 zero): the head's input
  bf16_t* xch;               // [2][ngroups][98][128] exchange images of h' (step parity)
  SeqGroupArgs g;            // T phase counters per group
  int T, K;
  int carry;                 // streaming call with a state: c_0 = slot 0 of call, the image of h_0 seeded in parity 1 of xch
};

constexpr int LSQ_RED_OFF = SEQ_IMG;                   // 4 waves x 7 fragments x 3 gates partial tiles of 1 KiB
constexpr int LSQ_STAGE_OFF = LSQ_RED_OFF + 84 * 1024;
constexpr int LSQ_FLAG_OFF = LSQ_STAGE_OFF + 4 * 512;
constexpr int LSQ_SMEM = LSQ_FLAG_OFF + 16;
static_assert(LSQ_SMEM <= 160 * 1024, "LDS budget");

// STREAM: the instantiation of the streaming calls with a carried state; the zero-state forward runs <NF, false>, whose
// source is the one it had before streaming existed (convgru_seq.hip.h says why).
template <int NF, bool STREAM>
static __global__ __launch_bounds__(SEQ_NT) void convlstm_seq_kernel(const LstmSeqParams p) {
  extern __shared__ __attribute__((aligned(16))) char lq_smem[];
  char* img_h = lq_smem;
  char* red = lq_smem + LSQ_RED_OFF;
  SeqGroup<NF> g;
  if (!g.init(lq_smem, SEQ_IMG, LSQ_STAGE_OFF, LSQ_FLAG_OFF, p.g, p.T)) return;
  const int kq = g.kq, ch = g.ch, clip0 = g.clip0;
  const int S = 128, T_ = p.T;
  const long long st = (long long)p.g.B * 49 * S;
  const unsigned xbytes = 2u * (unsigned)p.g.ngroups * 98u * 256u;

  // ---- resident filter fragments: k-steps [9 kq, 9 kq + 9) of the W_hi, W_hf, W_ho columns of channels 16 j .. 16 j + 15
  f32x4 bi[9], bf[9], bo[9];
  {
    const bf16_t* wi = p.w_rec + (long long)(4 * ch + 0) * p.K;
    const bf16_t* wf = p.w_rec + (long long)(4 * ch + 1) * p.K;
    const bf16_t* wo = p.w_rec + (long long)(4 * ch + 3) * p.K;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      const int k = (kq * 9 + i) * 32 + g.fk * 8;
      bi[i] = *(const f32x4*)(wi + k);
      bf[i] = *(const f32x4*)(wf + k);
      bo[i] = *(const f32x4*)(wo + k);
    }
  }
  // per owned row, resolved once: xo = element of (clip, step 0, position, channel) in xpre, so = in a state snapshot,
  // po = in slot 0 of the clip's padded h images; xo = -1: a padding row.  (Per-lane integers: the row -> (clip, position)
  // arithmetic is not redone per step, and the loop keeps no scalar state per row.)
  int xo[2][4], so_[2][4], po[2][4];
  float wci[2][4], wcf[2][4], wco[2][4];
#pragma unroll
  for (int o = 0; o < 2; ++o)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = g.own_row(o, r);
      const int c = row / 49, r49 = row - c * 49;
      const bool ok = g.own_valid(o, r);
      xo[o][r] = ok ? (((clip0 + c) * T_) * 49 + r49) * (4 * S) + 4 * ch : -1;
      so_[o][r] = (clip0 * 49 + row) * S + ch;
      po[o][r] = (((clip0 + c) * (T_ + 1)) * 81 + seq_pad_pix(r49)) * S + ch;
      wci[o][r] = p.peep[(0 * 49 + r49) * S + ch];
      wcf[o][r] = p.peep[(1 * 49 + r49) * S + ch];
      wco[o][r] = p.peep[(2 * 49 + r49) * S + ch];
    }
  float c_prev[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  __syncthreads();                                       // image zeroed, flag cleared (init)
  // A carried state (wave-uniform, outside the loop): c from slot 0, the operand image of h_0 from the exchange image
  // of parity 1, where a step -1 would have published it (seq_seed_kernel).  The parity argument above holds for it: a
  // member stores into parity 1 again at step 1, behind wait(0), which follows everybody's loads here.
  const bool carry = STREAM && p.carry != 0;
  if (carry) {
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (xo[o][r] >= 0) c_prev[o][r] = p.call[so_[o][r]];
    g.load_image(p.xch, xbytes, p.g.ngroups + g.group, img_h);
    __syncthreads();
  }

  for (int t = 0; t < T_; ++t) {
    // hoisted input parts of this lane's rows: one 16-byte load per row (i, f, g, o of its channel), in flight during the MFMAs
    f32x4 xv[2][4];
    const float* xpre_t = p.xpre + (long long)t * (49 * 4 * S);
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        xv[o][r] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (xo[o][r] >= 0) xv[o][r] = *(const f32x4*)(xpre_t + xo[o][r]);
      }
    // ---- the three recurrent convolutions on h_{t-1}: partial sums of this wave's K quarter, reduced through LDS
    if (t > 0 || carry) {
      f32x4 ai[NF], af[NF], ao[NF];
#pragma unroll
      for (int f = 0; f < NF; ++f) { ai[f] = (f32x4){0.f, 0.f, 0.f, 0.f}; af[f] = ai[f]; ao[f] = ai[f]; }
      f32x4 a0[NF], a1[NF];                              // two k-steps of A fragments in flight (software pipeline)
      g.a_frags(img_h, 0, a0);
#pragma unroll
      for (int i = 0; i < 9; i += 2) {
        if (i + 1 < 9) g.a_frags(img_h, i + 1, a1);
        __builtin_amdgcn_sched_barrier(0);
        g.mma(a0, bi[i], ai); g.mma(a0, bf[i], af); g.mma(a0, bo[i], ao);
        if (i + 2 < 9) g.a_frags(img_h, i + 2, a0);
        __builtin_amdgcn_sched_barrier(0);
        if (i + 1 < 9) { g.mma(a1, bi[i + 1], ai); g.mma(a1, bf[i + 1], af); g.mma(a1, bo[i + 1], ao); }
      }
      g.template store_partials<3>(red, 0, ai);
      g.template store_partials<3>(red, 1, af);
      g.template store_partials<3>(red, 2, ao);
    }
    __syncthreads();
    float ig[2][4], fg[2][4], gg[2][4], og[2][4], cn[2][4], hn[2][4];
#pragma unroll
    for (int o = 0; o < 2; ++o) {
      const int f = kq + 4 * o;
      f32x4 si = (f32x4){0.f, 0.f, 0.f, 0.f}, sf = si, so = si;
      if (f < NF && (t > 0 || carry)) {                   // (step 0 from the zero state: the sums are exact zeros)
        si = g.template reduce_tile<3>(red, 0, f);
        sf = g.template reduce_tile<3>(red, 1, f);
        so = g.template reduce_tile<3>(red, 2, f);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float cp = c_prev[o][r];
        ig[o][r] = sigmoidf_(si[r] + xv[o][r][0] + wci[o][r] * cp);
        fg[o][r] = sigmoidf_(sf[r] + xv[o][r][1] + wcf[o][r] * cp);
        gg[o][r] = tanhf_(si[r] + xv[o][r][2]);
        og[o][r] = sigmoidf_(so[r] + xv[o][r][3] + wco[o][r] * cp);
        cn[o][r] = fg[o][r] * cp + ig[o][r] * gg[o][r];
        hn[o][r] = tanhf_(cn[o][r]) * og[o][r];
        c_prev[o][r] = cn[o][r];
      }
    }
    if (t + 1 < T_) {
      const int par = (t & 1) * p.g.ngroups + g.group;   // exchange image of this step's parity
#pragma unroll
      for (int o = 0; o < 2; ++o)
        if (kq + 4 * o < NF) g.publish_tile(p.xch, xbytes, par, kq + 4 * o, hn[o]);
      g.arrive(t);
      g.wait(t);
      __syncthreads();
      g.load_image(p.xch, xbytes, par, img_h);
      __syncthreads();
    }
    // the step's plain outputs go out BEHIND the hand-off (convgru_seq.hip.h: in front of it they sit in the queue that
    // arrive() drains); they drain under the next step's MFMAs
    {
      float* hall_t = p.hall + (long long)(t + 1) * st;
      float* call_t = p.call + (long long)(t + 1) * st;
      float* gates_t = p.gates ? p.gates + (long long)t * st : nullptr;
      bf16_t* hseq_t = p.hseq + (long long)(t + 1) * (81 * S);
      const long long gs = (long long)T_ * st;
#pragma unroll
      for (int o = 0; o < 2; ++o)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (xo[o][r] >= 0) {
            hall_t[so_[o][r]] = hn[o][r];
            call_t[so_[o][r]] = cn[o][r];
            if (gates_t) {
              float* gp = gates_t + so_[o][r];
              gp[0] = ig[o][r]; gp[gs] = fg[o][r]; gp[2 * gs] = gg[o][r]; gp[3 * gs] = og[o][r];
            }
            hseq_t[po[o][r]] = f2bf(hn[o][r]);
          }
    }
  }
  // a group that timed out must not look like a result: the head reads hseq, the tests and the backward hall / call
  if (g.timed_out()) {
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (xo[o][r] >= 0) {
          for (int t = 0; t < T_; ++t) {
            p.hseq[(long long)(t + 1) * (81 * S) + po[o][r]] = (bf16_t)0x7FC0;     // bf16 NaN
            p.hall[(long long)(t + 1) * st + so_[o][r]] = __builtin_nanf("");
            p.call[(long long)(t + 1) * st + so_[o][r]] = __builtin_nanf("");
          }
        }
  }
}

}  // namespace rgp
