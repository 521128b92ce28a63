// Persistent ConvGRU sequence kernel (gfx950, bf16 operands): ALL T steps of GRU_RCN_Cell.__call__
// (/root/reference/models/gaze_grcn.py:95-129, unrolled at :259-288) plus the per-timestep inference batch-norm
// (:325) in ONE launch.  The per-step path (rgp_grcn.hip seq_impl) runs 2 T dependent launches of ~13 us whose
// M = B*49 rows fill a fraction of the chip; here the recurrent filters never move and only the state does
// (seq_group.hip.h: decomposition, exchange protocol, time-out).
//
// The serial critical path is  h_{t-1} -> [U_z|U_r] conv -> r.h -> U conv -> h_t , 43 MFLOP per clip and step against
// 884 KB of bf16 filters.  Member j of a group keeps the z, r and c filter columns of its 16 state channels in registers
// (3 x 16 columns x K = 1152: 110 KB per workgroup = 108 VGPRs per lane, 9 MFMA k-steps of 32 per wave and filter).  Per
// step it computes its 16 channels of
//   u = sigmoid(W_z*x + U_z*h), r = sigmoid(W_r*x + U_r*h)        (x-parts hoisted: xpre)
//   c = tanh(W*x + U*(r.h)),  h' = u.h + (1-u).c
// for the group's clips; r.h and h' are exchanged between the 8 members twice per step.
#pragma once
#include "seq_group.hip.h"

namespace rgp {

struct SeqParams {
  const bf16_t* w_zr;        // packed [256][K] (rows 0..127 U_z columns, 128..255 U_r), K = tap*128 + c
  const bf16_t* w_c;         // packed [128][K]
  const float* xpre;         // [B][T][49][384] hoisted W_z|W_r|W * x
  float* hall;               // [T+1][B][49][128] fp32 states (slot 0 = h_0: zeroed, or seeded by a streaming call)
  float* uall;               // [T][B][49][128]
  float* rall;               // optional (training)
  float* call;               // optional (training)
  bf16_t* hbn;               // [B*T][81][128] halo-padded BN(h_t): the head's input image of frame b*T+t
  const float* bn_gamma;     // [T][128]
  const float* bn_beta;
  float bn_inv_std;
  bf16_t* xch_h;             // [ngroups][98][128] exchange image of h'
  bf16_t* xch_rh;            // [ngroups][98][128] exchange image of r.h
  SeqGroupArgs g;            // 2 T phase counters per group
  int T, K;
  int carry;                 // streaming call with a state: h_0 = slot 0 of hall, its operand image seeded in xch_h (seq_seed_kernel)
  int bn_phase;              // step t uses batch-norm slot (bn_phase + t) % T
};

constexpr int SEQ_RED_OFF = 2 * SEQ_IMG;             // 4 waves x 7 fragments x 2 gates partial tiles of 1 KiB (56 KiB)
constexpr int SEQ_STAGE_OFF = SEQ_RED_OFF + 56 * 1024;
constexpr int SEQ_FLAG_OFF = SEQ_STAGE_OFF + 4 * 512;
constexpr int SEQ_SMEM = SEQ_FLAG_OFF + 16;          // 160 592 B (no static __shared__: the dynamic base stays 16-B aligned)
static_assert(SEQ_SMEM <= 160 * 1024, "LDS budget");

// STREAM: the instantiation of the streaming calls (a carried state and / or a batch-norm phase).  The zero-state forward runs
// <NF, false>, whose source -- and so whose loop -- is the one it had before streaming existed: convgru_seq_kernel<7> sits at
// the edge of its register file, and a run-time branch in front of the loop moved its register allocation enough to show in
// the plain forward.
template <int NF, bool STREAM>
static __global__ __launch_bounds__(SEQ_NT) void convgru_seq_kernel(const SeqParams p) {
  extern __shared__ __attribute__((aligned(16))) char sq_smem[];
  char* img_h = sq_smem;
  char* img_rh = sq_smem + SEQ_IMG;
  char* red_zr = sq_smem + SEQ_RED_OFF;  // 4 x 7 x 2 partial tiles of 1 KiB, z|r phase.  NOT overlaid on the images: their
  char* red_c = red_zr;                  // halo pixels and zero region must stay zero for the whole sequence.
  SeqGroup<NF> g;
  if (!g.init(sq_smem, 2 * SEQ_IMG, SEQ_STAGE_OFF, SEQ_FLAG_OFF, p.g, 2 * p.T)) return;
  const int kq = g.kq, ch = g.ch, clip0 = g.clip0;
  const int S = 128, T_ = p.T;
  const long long st = (long long)p.g.B * 49 * S;
  const unsigned xbytes = (unsigned)p.g.ngroups * 98u * 256u;

  // ---- resident filter fragments: k-steps [9 kq, 9 kq + 9) of the z, r, c columns of channels 16 j .. 16 j + 15
  f32x4 bz[9], br[9], bc[9];
  {
    const bf16_t* wz = p.w_zr + (long long)ch * p.K;
    const bf16_t* wr = p.w_zr + (long long)(128 + ch) * p.K;
    const bf16_t* wc = p.w_c + (long long)ch * p.K;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      const int k = (kq * 9 + i) * 32 + g.fk * 8;
      bz[i] = *(const f32x4*)(wz + k);
      br[i] = *(const f32x4*)(wr + k);
      bc[i] = *(const f32x4*)(wc + k);
    }
  }
  // the rows this wave finalises: a lane keeps their fp32 state for the whole sequence
  int orow[2][4];
  bool ovalid[2][4];
#pragma unroll
  for (int o = 0; o < 2; ++o)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      orow[o][r] = g.own_row(o, r);
      ovalid[o][r] = g.own_valid(o, r);
    }
  float h_prev[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  __syncthreads();                                       // images zeroed, flag cleared (init)
  // A carried state (wave-uniform, outside the loop): the fp32 state from slot 0, the operand image from the seeded
  // exchange image -- what the hand-off of a step -1 would have left.  Without one nothing here runs.
  if (STREAM && p.carry) {
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (ovalid[o][r]) h_prev[o][r] = p.hall[((long long)(clip0 * 49 + orow[o][r])) * S + ch];
    g.load_image(p.xch_h, xbytes, g.group, img_h);
    __syncthreads();
  }
  int bn_slot = STREAM ? p.bn_phase : 0;                 // (scalar; no division in the loop)
  // hand-off of phase `ph`: publish this wave's tiles v, rendezvous, load the group's exchange image into an LDS image.
  // (The step's plain output stores are issued after it, see the loop.)
  auto hand_off = [&](int ph, bf16_t* xch, char* img, const float (&v)[2][4]) {
#pragma unroll
    for (int o = 0; o < 2; ++o)
      if (kq + 4 * o < NF) g.publish_tile(xch, xbytes, g.group, kq + 4 * o, v[o]);
    g.arrive(ph);
    g.wait(ph);
    __syncthreads();
    g.load_image(xch, xbytes, g.group, img);
    __syncthreads();
  };

  for (int t = 0; t < T_; ++t) {
    // hoisted input parts of this lane's rows x {z, r, c} (in flight during the MFMAs)
    float xz[2][4], xr[2][4], xc[2][4], gam, bet;
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        xz[o][r] = xr[o][r] = xc[o][r] = 0.f;
        if (ovalid[o][r]) {
          const int c = orow[o][r] / 49, r49 = orow[o][r] - c * 49;
          const float* xp = p.xpre + (((long long)(clip0 + c) * T_ + t) * 49 + r49) * (3 * S) + ch;
          xz[o][r] = xp[0]; xr[o][r] = xp[S]; xc[o][r] = xp[2 * S];
        }
      }
    if constexpr (STREAM) {
      gam = p.bn_gamma[bn_slot * S + ch];
      bet = p.bn_beta[bn_slot * S + ch];
      bn_slot = bn_slot + 1 == T_ ? 0 : bn_slot + 1;
    } else {
      gam = p.bn_gamma[t * S + ch];
      bet = p.bn_beta[t * S + ch];
    }

    // ---- z | r phase: partial sums of this wave's K quarter, reduced over the 4 quarters through LDS
    {
      f32x4 az[NF], ar[NF];
#pragma unroll
      for (int f = 0; f < NF; ++f) { az[f] = (f32x4){0.f, 0.f, 0.f, 0.f}; ar[f] = az[f]; }
      f32x4 a0[NF], a1[NF];                              // two k-steps of A fragments in flight (software pipeline)
      g.a_frags(img_h, 0, a0);
#pragma unroll
      for (int i = 0; i < 9; i += 2) {
        if (i + 1 < 9) g.a_frags(img_h, i + 1, a1);
        __builtin_amdgcn_sched_barrier(0);
        g.mma(a0, bz[i], az); g.mma(a0, br[i], ar);
        if (i + 2 < 9) g.a_frags(img_h, i + 2, a0);
        __builtin_amdgcn_sched_barrier(0);
        if (i + 1 < 9) { g.mma(a1, bz[i + 1], az); g.mma(a1, br[i + 1], ar); }
      }
      g.template store_partials<2>(red_zr, 0, az);
      g.template store_partials<2>(red_zr, 1, ar);
    }
    __syncthreads();
    float u[2][4], rh[2][4], rgs[2][4];
#pragma unroll
    for (int o = 0; o < 2; ++o) {
      const int f = kq + 4 * o;
      f32x4 sz = (f32x4){0.f, 0.f, 0.f, 0.f}, sr = sz;
      if (f < NF) { sz = g.template reduce_tile<2>(red_zr, 0, f); sr = g.template reduce_tile<2>(red_zr, 1, f); }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        u[o][r] = sigmoidf_(sz[r] + xz[o][r]);
        rgs[o][r] = sigmoidf_(sr[r] + xr[o][r]);
        rh[o][r] = rgs[o][r] * h_prev[o][r];
      }
    }
    hand_off(2 * t, p.xch_rh, img_rh, rh);
    // this phase's plain outputs go out BEHIND the hand-off, under the candidate phase's MFMAs: in front of it they sit
    // in the queue that its arrive() drains (the hand-off then waits for their HBM acknowledgements), between its two parts
    // they delay the poll and the image loads (+25 % per step, measured)
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (ovalid[o][r]) {
          const long long off = (long long)t * st + ((long long)(clip0 * 49 + orow[o][r])) * S + ch;
          p.uall[off] = u[o][r];
          if (p.rall) p.rall[off] = rgs[o][r];
        }

    // ---- candidate phase on r.h, blend, batch-norm
    {
      f32x4 ac[NF];
#pragma unroll
      for (int f = 0; f < NF; ++f) ac[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
      f32x4 a0[NF], a1[NF];
      g.a_frags(img_rh, 0, a0);
#pragma unroll
      for (int i = 0; i < 9; i += 2) {
        if (i + 1 < 9) g.a_frags(img_rh, i + 1, a1);
        __builtin_amdgcn_sched_barrier(0);
        g.mma(a0, bc[i], ac);
        if (i + 2 < 9) g.a_frags(img_rh, i + 2, a0);
        __builtin_amdgcn_sched_barrier(0);
        if (i + 1 < 9) g.mma(a1, bc[i + 1], ac);
      }
      g.template store_partials<1>(red_c, 0, ac);
    }
    __syncthreads();
    float hn[2][4], cgs[2][4];
#pragma unroll
    for (int o = 0; o < 2; ++o) {
      const int f = kq + 4 * o;
      f32x4 sc = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (f < NF) sc = g.template reduce_tile<1>(red_c, 0, f);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        cgs[o][r] = tanhf_(sc[r] + xc[o][r]);
        hn[o][r] = u[o][r] * h_prev[o][r] + (1.f - u[o][r]) * cgs[o][r];
        h_prev[o][r] = hn[o][r];
      }
    }
    if (t + 1 < T_) hand_off(2 * t + 1, p.xch_h, img_h, hn);
    // (outputs behind the hand-off, as above: they drain under the next step's z | r MFMAs)
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (ovalid[o][r]) {
          const int c = orow[o][r] / 49, r49 = orow[o][r] - c * 49;
          const long long off = ((long long)(clip0 * 49 + orow[o][r])) * S + ch;
          if (p.call) p.call[(long long)t * st + off] = cgs[o][r];
          p.hall[(long long)(t + 1) * st + off] = hn[o][r];
          const long long fr = (long long)(clip0 + c) * T_ + t;
          p.hbn[(fr * 81 + seq_pad_pix(r49)) * S + ch] = f2bf(gam * (hn[o][r] * p.bn_inv_std) + bet);
        }
  }
  // a group that timed out must not look like a result: the head reads hbn (every frame of the group's clips: the
  // exchange images were stale from the first missed phase on), the training path hall
  if (g.timed_out()) {
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (ovalid[o][r]) {
          const int c = orow[o][r] / 49, r49 = orow[o][r] - c * 49;
          const long long off = ((long long)(clip0 * 49 + orow[o][r])) * S + ch;
          for (int t = 0; t < T_; ++t) {
            const long long fr = (long long)(clip0 + c) * T_ + t;
            p.hbn[(fr * 81 + seq_pad_pix(r49)) * S + ch] = (bf16_t)0x7FC0;     // bf16 NaN
            p.hall[(long long)(t + 1) * st + off] = __builtin_nanf("");
          }
        }
  }
}

}  // namespace rgp
