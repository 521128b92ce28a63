// Persistent BPTT of the ConvLSTM (gfx950, bf16 operands): all T backward steps of the recurrence of LSTM_RCN_Cell
// (models/gaze_lstm.py:114-131 of the reference, with its quirks: see convlstm_seq.hip.h) in ONE launch -- the mirror of
// convlstm_seq.hip.h on the group scheme of seq_group.hip.h.  The per-step path (rgp_lstm.hip) runs 2 T - 1 dependent
// launches: lstm_bwd_step_kernel, then the input-gradient GEMM of the step.  The arithmetic here is theirs.
//
// Per step t (descending), for the owner of a (row, channel), with the saved gates i, f, g, o of step t, c_{t-1}, c_t:
//   dh  = dh_head[b,t] + carry_h            tc = tanh(c_t)
//   d_o = dh.tc.o(1-o)                      dc = carry_c + dh.o.(1-tc^2)
//   d_i = dc.g.i(1-i)    d_f = dc.c_{t-1}.f(1-f)    d_g = dc.i.(1-g^2)
//   carry_c = dc.f + d_i.W_ci + d_f.W_cf + d_o.W_co            (all three peepholes read the OLD c)
//   carry_h = conv3x3([d_i+d_g | d_f | d_o]; rot180 [W_hi | W_hf | W_ho]^T)          (g reuses W_hi)
// and frame (b, t) of dpre = [d_g | d_i | d_i+d_g | d_f | d_o] (bf16, halo-padded) is what the hoisted filter gradients,
// the peephole gradients and the input-gradient GEMM consume afterwards.
//
// Member j owns state channels [16j, 16j+16): both carries and its slice of the peephole planes live in the registers of
// the wave that finalises a tile, for the whole sequence; its 16 columns of the packed input-gradient filter
// (b_rec: [128][K = tap*384 + block*128 + channel], 108 k-steps) stay resident across its 4 waves as K quarters, 27 k-steps
// = 108 VGPRs per lane, arranged as 9 per gradient block: block q's k-steps [9 kq, 9 kq + 9) of its own 9 x 128 image, so
// SeqGroup::a_frags addresses every block's image unchanged.
// ONE hand-off per step: the three bf16 tiles go into three exchange images, double-buffered by step parity (the reason is
// convlstm_seq.hip.h's: one hand-off per step separates nothing else).  Step 0 publishes nothing and runs no MFMAs.
// LDS: three image pairs do not fit next to the partial tiles, so two buffers take the three blocks in turn -- blocks 0
// and 1 are loaded, the K pass over a runs, block 2 is fetched into registers and lands in a behind the K pass over b.
// No float atomics; a clip's bits depend on neither its group slot nor the batch size.
#pragma once
#include "lstm_kernels.hip.h"
#include "seq_group.hip.h"

namespace rgp {

struct LstmBpttParams {
  const bf16_t* w_rec;       // packed dgrad filter of W_hi | W_hf | W_ho: [128][K = tap*384 + block*128 + o]
  const float* dh_head;      // [B][T][49][128] gradient reaching h_t from the head
  const float* gates;        // [4][T][B][49][128] i, f, g, o
  const float* call;         // [T+1][B][49][128] c (slot 0 = the zero state)
  const float* peep;         // [3][49][128] W_ci, W_cf, W_co
  bf16_t* dpre;              // [B][T][81][5 x 128] column blocks g | i | i+g | f | o (halos stay zero)
  bf16_t* xch;               // [2][3][ngroups][98][128] exchange images (step parity, gradient block)
  SeqGroupArgs g;            // T phase counters per group
  int T, K;
};

// LDS: two operand images, 4 x NF partial tiles of 1 KiB (in 28 KiB), staging, flag
constexpr int LBP_RED_OFF = 2 * SEQ_IMG;
constexpr int LBP_STAGE_OFF = LBP_RED_OFF + 28 * 1024;
constexpr int LBP_FLAG_OFF = LBP_STAGE_OFF + 4 * 512;
constexpr int LBP_SMEM = LBP_FLAG_OFF + 32;
static_assert(LBP_SMEM <= 160 * 1024, "LDS budget");

template <int NF>
static __global__ __launch_bounds__(SEQ_NT) void convlstm_bptt_kernel(const LstmBpttParams p) {
  extern __shared__ __attribute__((aligned(16))) char lb_smem[];
  char* img_a = lb_smem;                 // d_i + d_g, later d_o
  char* img_b = lb_smem + SEQ_IMG;       // d_f
  char* red = lb_smem + LBP_RED_OFF;
  SeqGroup<NF> g;
  if (!g.init(lb_smem, 2 * SEQ_IMG, LBP_STAGE_OFF, LBP_FLAG_OFF, p.g, p.T)) return;
  const int kq = g.kq, ch = g.ch, clip0 = g.clip0;
  const int S = 128, T_ = p.T;
  const long long st = (long long)p.g.B * 49 * S, gs = (long long)T_ * st;
  const unsigned xbytes = 6u * (unsigned)p.g.ngroups * 98u * 256u;

  // ---- resident filter fragments: for each gradient block, k-steps [9 kq, 9 kq + 9) of its 9 x 128 image
  f32x4 bw[3][9];
  {
    const bf16_t* w = p.w_rec + (long long)ch * p.K;
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        const int ks = kq * 9 + i;
        bw[q][i] = *(const f32x4*)(w + (ks >> 2) * (3 * S) + q * S + (ks & 3) * 32 + g.fk * 8);
      }
  }
  // per owned row, resolved once: so = element in a state snapshot, yo = of (clip, step 0) in dh_head, po = in dpre;
  // so = -1: a padding row
  int so_[2][4], yo[2][4], po[2][4];
  float wci[2][4], wcf[2][4], wco[2][4];
#pragma unroll
  for (int o = 0; o < 2; ++o)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = g.own_row(o, r);
      const int c = row / 49, r49 = row - c * 49;
      so_[o][r] = g.own_valid(o, r) ? (clip0 * 49 + row) * S + ch : -1;
      yo[o][r] = (((clip0 + c) * T_) * 49 + r49) * S + ch;
      po[o][r] = (((clip0 + c) * T_) * 81 + seq_pad_pix(r49)) * (5 * S) + ch;
      wci[o][r] = p.peep[(0 * 49 + r49) * S + ch];
      wcf[o][r] = p.peep[(1 * 49 + r49) * S + ch];
      wco[o][r] = p.peep[(2 * 49 + r49) * S + ch];
    }
  // saved forward quantities of this lane's rows at step t (none of them depends on the carries)
  struct Saved { float ig[2][4], fg[2][4], gg[2][4], og[2][4], cp[2][4], dh[2][4]; };
  auto load_saved = [&](int t, Saved& v) {
    const float* gt = p.gates + (long long)t * st;
    const float* ct = p.call + (long long)t * st;
    const float* yt = p.dh_head + (long long)t * (49 * S);
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        v.ig[o][r] = v.fg[o][r] = v.gg[o][r] = v.og[o][r] = v.cp[o][r] = v.dh[o][r] = 0.f;
        if (so_[o][r] >= 0) {
          const float* gp = gt + so_[o][r];
          v.ig[o][r] = gp[0]; v.fg[o][r] = gp[gs]; v.gg[o][r] = gp[2 * gs]; v.og[o][r] = gp[3 * gs];
          v.cp[o][r] = ct[so_[o][r]];
          v.dh[o][r] = yt[yo[o][r]];
        }
      }
  };
  float carry_h[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  float carry_c[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  float cn[2][4];                                          // c_t of the step at hand: the cp of the step before it
#pragma unroll
  for (int o = 0; o < 2; ++o)
#pragma unroll
    for (int r = 0; r < 4; ++r) cn[o][r] = so_[o][r] >= 0 ? p.call[(long long)T_ * st + so_[o][r]] : 0.f;
  Saved sv;
  load_saved(T_ - 1, sv);
  __syncthreads();                                         // images zeroed, flag cleared (init)

  for (int t = T_ - 1; t >= 0; --t) {
    // ---- the element-wise step (lstm_bwd_step_kernel), on the owned rows
    float d_g[2][4], d_i[2][4], d_ig[2][4], d_f[2][4], d_o[2][4];
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float ig = sv.ig[o][r], fg = sv.fg[o][r], gg = sv.gg[o][r], og = sv.og[o][r], cp = sv.cp[o][r];
        const float dh = sv.dh[o][r] + carry_h[o][r];
        const float tc = tanhf_(cn[o][r]);
        d_o[o][r] = dh * tc * og * (1.f - og);
        const float dc = carry_c[o][r] + dh * og * (1.f - tc * tc);
        d_i[o][r] = dc * gg * ig * (1.f - ig);
        d_f[o][r] = dc * cp * fg * (1.f - fg);
        d_g[o][r] = dc * ig * (1.f - gg * gg);
        d_ig[o][r] = d_i[o][r] + d_g[o][r];
        carry_c[o][r] = dc * fg + d_i[o][r] * wci[o][r] + d_f[o][r] * wcf[o][r] + d_o[o][r] * wco[o][r];
        cn[o][r] = cp;
      }
    auto store_dpre = [&]() {                              // interiors only, rounded as lstm_bwd_step_kernel rounds them
      bf16_t* dt = p.dpre + (long long)t * (81 * 5 * S);
#pragma unroll
      for (int o = 0; o < 2; ++o)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (so_[o][r] >= 0) {
            bf16_t* d = dt + po[o][r];
            d[LSTM_DG * S] = Elem<bf16_t>::to(d_g[o][r]); d[LSTM_DI * S] = Elem<bf16_t>::to(d_i[o][r]);
            d[LSTM_DIG * S] = Elem<bf16_t>::to(d_ig[o][r]);
            d[LSTM_DF * S] = Elem<bf16_t>::to(d_f[o][r]); d[LSTM_DO * S] = Elem<bf16_t>::to(d_o[o][r]);
          }
    };
    // (nothing reads d h_0, the zero state: the last step publishes nothing and runs no MFMAs)
    if (t == 0) { store_dpre(); break; }
    const int ph = T_ - 1 - t;
    const int x0 = ((ph & 1) * 3) * p.g.ngroups + g.group;  // exchange image of block 0 at this step's parity
#pragma unroll
    for (int o = 0; o < 2; ++o)
      if (kq + 4 * o < NF) {
        g.publish_tile(p.xch, xbytes, x0, kq + 4 * o, d_ig[o]);
        g.publish_tile(p.xch, xbytes, x0 + p.g.ngroups, kq + 4 * o, d_f[o]);
        g.publish_tile(p.xch, xbytes, x0 + 2 * p.g.ngroups, kq + 4 * o, d_o[o]);
      }
    g.arrive(ph);
    g.wait(ph);
    __syncthreads();
    g.load_image(p.xch, xbytes, x0, img_a);
    g.load_image(p.xch, xbytes, x0 + p.g.ngroups, img_b);
    __syncthreads();
    // the step's plain stores go out BEHIND the hand-off (convgru_seq.hip.h: in front of it they sit in the queue that
    // arrive() drains): they pass under the MFMAs below
    __builtin_amdgcn_sched_barrier(0);
    store_dpre();
    __builtin_amdgcn_sched_barrier(0);

    // ---- carry_h = conv3x3 of the three blocks: this wave's K quarter of each, ONE sum, reduced through LDS
    f32x4 acc[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) acc[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
    auto k_pass = [&](const char* img, const f32x4 (&b)[9]) {
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        f32x4 a[NF];
        g.a_frags(img, i, a);
        g.mma(a, b[i], acc);
        if (i % 3 == 2) __builtin_amdgcn_sched_barrier(0);
      }
    };
    k_pass(img_a, bw[0]);
    __syncthreads();                                       // every wave has read block 0: a is free
    {
      u32x4 q2[SeqGroup<NF>::IMG_IT];
      g.fetch_image(p.xch, xbytes, x0 + 2 * p.g.ngroups, q2);
      __builtin_amdgcn_sched_barrier(0);
      k_pass(img_b, bw[1]);
      g.put_image(img_a, q2);
      __builtin_amdgcn_sched_barrier(0);
    }
    // the next step's saved quantities depend on no carry: asked for here, they arrive under the last K pass and the
    // reduction.  (Asked for in front of the first K pass they are live next to q2: convlstm_bptt_kernel<7> then spills.)
    load_saved(t - 1, sv);
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
    k_pass(img_a, bw[2]);
    g.template store_partials<1>(red, 0, acc);
    __syncthreads();
#pragma unroll
    for (int o = 0; o < 2; ++o) {
      f32x4 d = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (kq + 4 * o < NF) d = g.template reduce_tile<1>(red, 0, kq + 4 * o);
#pragma unroll
      for (int r = 0; r < 4; ++r) carry_h[o][r] = d[r];
    }
    // (the next step's barriers -- arrive() at the latest, or none where it is the last -- order these reads of the
    // partial tiles and of image a against whatever overwrites them)
  }
  // a group that timed out must not look like a result: all five blocks of frame (clip, 0), own channels
  if (g.timed_out()) {
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (so_[o][r] >= 0) {
#pragma unroll
          for (int q = 0; q < 5; ++q) p.dpre[po[o][r] + q * S] = (bf16_t)0x7FC0;     // bf16 NaN
        }
  }
}

}  // namespace rgp
