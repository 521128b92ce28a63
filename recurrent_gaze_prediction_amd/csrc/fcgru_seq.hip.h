// Persistent fc-GRU sequence kernel (gfx950, bf16 operands): ALL T steps of the TF-1.x GRUCell(1617) of gaze_rnn /
// gaze_rnn77 in ONE launch.  The per-step path (rgp_fcgru.hip forward_impl) runs 2 T dependent launches, each of which
// re-streams the h-side kernels ([1664 x 3328] + [1664 x 1664] bf16 = 16.6 MB) from L2 / Infinity Cache for at most 64 rows;
// here the kernels never move and only the state does.
//
// Decomposition, exchange, rendezvous, padding and time-out are described in fcgru_member.hip.h.  This kernel's own:
// Residency.  The member's 8 u, 8 r and 8 c rows of the packed kernels (g->zr rows [u | r], g->c; set_weights_impl) in
// REGISTERS for the whole sequence: wave kq keeps K steps [13 kq, 13 kq + 13) of the 52, i.e. 2 x 13 B fragments = 104 VGPRs
// per lane.  Per step:
//   phase A  [u(8) | r(8)] = one 16x16x32 column block per K step on the bf16 rows of h_{t-1};
//            u = sigmoid(. + xpre_u), r = sigmoid(. + xpre_r); publish bf16(r * h_{t-1}) (fp32 product, rounded once:
//            EpiGruZR); rendezvous
//   phase B  c block (columns 8..15 of the tile multiply zeros) on the r.h rows; c = tanh(. + xpre_c),
//            h_t = u h_{t-1} + (1 - u) c (EpiGruC, identity batch-norm); publish bf16(h_t); rendezvous
// (none behind the last phase: the kernel boundary orders it.)
//
// Exchange buffers: the plan's own row-major operand rows, so the per-step consumers read what they always read.
//   h:   hrows, row b T + t -- the rows the output projection reads.  Every step has its own row: nothing is overwritten
//        while it is still read.  (Training plans also get hp_all, plain stores: the backward reads it, not this kernel.)
//   r.h: training plans rh_all, a row per (clip, step), as above.  Inference plans the single rh buffer [B][np], and that
//        is safe (write-after-read): a member publishes r.h of step t + 1 only behind the phase-B rendezvous of step t, and
//        every member arrives at that rendezvous only after its phase-B MFMAs, i.e. after it has read r.h of step t.
// A wave's A-fragment load of one K step is 16 rows x 64 bytes; all 13 x NF loads of a phase are issued before the first
// MFMA (>= 13 sixteen-byte loads per lane in flight).  That order is pinned by a scheduling barrier in fcs_gemm and checked
// in the assembly by scripts/check_isa_waits.py: without it the compiler keeps 2 - 3 loads in flight.
//
// Streaming (rgp_fcgru_forward_stream), template argument STREAM.  STREAM = false is what zero-state calls over all T steps
// launch.  STREAM = true starts from a caller's state: gru_seed_kernel has put fp32 h_{-1} into slot 0 of hall and its bf16
// rows into the plan's operand row of step 0 -- hp (row b, stride np) on inference plans, slot (b, 0) of hp_all (stride
// (T + 1) np) on training plans -- so thread b loads its 8 fp32 h from slot 0 ahead of the step loop (it alone writes those 8
// floats later: no race), and phase A of step 0 runs the same fcs_gemm on the seeded rows instead of skipping; base and strides
// are selected per step, so the phase still is ONE run of loads in front of ONE run of MFMAs.  No new exchange buffer.
// Write-after-read: the seeded rows are only READ, in phase A of step 0, and never written by this kernel (h_t goes to hrows,
// and to slots >= 1 of hp_all): nothing to order.
// State out: inference hall is a two-slot ping-pong, so h behind step n_valid < T does not survive the launch; on inference
// plans thread b stores its 8 fp32 h behind step n_valid - 1 into hsnap [B][np] (training plans: the host reads slot n_valid
// of hall_t).
#pragma once
#include "fcgru_member.hip.h"

namespace rgp {

constexpr int FCS_KW = FCS_NP / 32 / 4;              // K steps per wave: 13
static_assert(FCS_KW * 4 * 32 == FCS_NP, "K split");

// E: the element type of the plan's operand rows (bf16_t here, float in fcgru_seq_f32.hip.h)
template <typename E>
struct FcSeqParamsT {
  const E* w_zr;             // packed [2 np][np]: rows [0, np) u, [np, 2 np) r
  const E* w_c;              // packed [np][np]
  const float* xpre;         // [B T][3 np] hoisted x parts + biases, columns [u | r | c]
  E* hrows;                  // [B T][np] h_t, row b T + t: exchange rows of h and the output projection's input
  E* rh;                     // training: rh_all [B T][np]; inference: rh [B][np]
  float* hall;               // training: hall_t [T+1][B][np] (slot 0 = h_0 = 0); inference: [2][B][np], h_t in slot (t+1) & 1
  float* uall;               // training [T][B][np] (else null) ...
  float* rall;
  float* call;
  E* hp_all;                 // training [B][T+1][np], slot (b, 0) untouched
  unsigned* cnt;             // [2 T][FCS_SHARDS][FCS_CNT_STRIDE] phase counters, zeroed ahead of the launch
  unsigned* err;             // the plan's pinned error word
  int B, T;
};
// STREAM = true takes these on top (the STREAM = false instantiations keep the parameter block they were measured with)
template <typename E>
struct FcSeqStreamParamsT : FcSeqParamsT<E> {
  const E* seed;             // rows of h_{-1}: inference hp [B][np]; training hp_all, slot (b, 0)
  unsigned seed_bytes;       // extent of that buffer (rows >= B lie behind it and read zeros)
  unsigned seed_stride;      // bytes from clip b to clip b + 1: one row, or T + 1 rows
  float* hsnap;              // inference: [B][np] fp32 h behind step n_valid - 1; training: null
  int n_valid;
};
template <typename E, bool STREAM> struct FcSeqParamsOf { typedef FcSeqParamsT<E> type; };
template <typename E> struct FcSeqParamsOf<E, true> { typedef FcSeqStreamParamsT<E> type; };

// A fragments of this wave's K quarter from exchange rows (sc1), then the MFMAs of one resident column block on them.
// off0: the lane's byte offset at fragment 0, K step 0; fragments are fstride bytes apart, K steps 64.
template <int NF>
__device__ __forceinline__ void fcs_gemm(const void* base, unsigned bytes, unsigned off0, unsigned fstride, const f32x4 (&b)[FCS_KW],
                                         f32x4 (&acc)[NF]) {
  u32x4 a[NF][FCS_KW];
#pragma unroll
  for (int f = 0; f < NF; ++f)
#pragma unroll
    for (int i = 0; i < FCS_KW; ++i) a[f][i] = seq_ld_sc1(base, bytes, off0 + (unsigned)f * fstride + (unsigned)i * 64u);
  // The scheduler must not sink the loads between the MFMAs: left alone it re-uses 2 - 4 A registers under vmcnt(1..2), a
  // chain of dependent round trips per phase (scripts/check_isa_waits.py counts the loads in front of the first MFMA).
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int i = 0; i < FCS_KW; ++i)
#pragma unroll
    for (int f = 0; f < NF; ++f)
      acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(s16x8, a[f][i]), __builtin_bit_cast(s16x8, b[i]), acc[f], 0, 0, 0);
}

template <int NF, bool SAVE, bool STREAM>
static __global__ __launch_bounds__(SEQ_NT) void fcgru_seq_kernel(const typename FcSeqParamsOf<bf16_t, STREAM>::type p) {
  __shared__ __attribute__((aligned(16))) char red[4 * NF * 16 * FCS_PITCH];   // [K quarter][row][16 columns]
  __shared__ int s_timeout;
  const int tid = threadIdx.x, lane = tid & 63;
  const int kq = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int frow = lane & 15, fk = lane >> 4;
  const int j = blockIdx.x, u0 = FCS_UNITS * j;          // member, its first unit
  const int np = FCS_NP, T_ = p.T, B = p.B;
  const unsigned members = gridDim.x;
  if (tid == 0) s_timeout = 0;

  // ---- resident B fragments: K steps [13 kq, 13 kq + 13) of columns [u(8) | r(8)] and [c(8) | 0]
  f32x4 bzr[FCS_KW], bc[FCS_KW];
  {
    const bf16_t* wz = p.w_zr + (long long)((frow < 8 ? 0 : np) + u0 + (frow & 7)) * np;
    const bf16_t* wc = p.w_c + (long long)(u0 + (frow & 7)) * np;
#pragma unroll
    for (int i = 0; i < FCS_KW; ++i) {
      const int k = (kq * FCS_KW + i) * 32 + fk * 8;
      bzr[i] = *(const f32x4*)(wz + k);
      const f32x4 c = *(const f32x4*)(wc + k);
      bc[i] = frow < 8 ? c : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
  }
  // thread b of wave 0 finalises clip b: its fp32 state and update gate live here for the whole sequence
  const int b = tid;
  const bool red_row = tid < NF * 16;                      // (rows >= B are summed and dropped)
  const bool own = red_row && b < B;
  float h[8], u[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) { h[i] = 0.f; u[i] = 0.f; }
  const unsigned hbytes = (unsigned)B * (unsigned)T_ * (unsigned)np * 2u;
  const unsigned rbytes = SAVE ? hbytes : (unsigned)B * (unsigned)np * 2u;
  const unsigned koff = (unsigned)((kq * FCS_KW * 32 + fk * 8) * 2);     // the lane's K offset in a row, bytes
  const long long st = (long long)B * np;
  if constexpr (STREAM) {                                  // the caller's state: slot 0 of hall (fcgru_seed_kernel)
    if (own) {
      const float* h0 = p.hall + (long long)b * np + u0;
      const f32x4 lo = *(const f32x4*)h0, hi = *(const f32x4*)(h0 + 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) { h[i] = lo[i]; h[4 + i] = hi[i]; }
    }
  }
  __syncthreads();                                         // flag cleared

  // this wave's partial tiles -> LDS; the sum over the 4 quarters of row `tid` (16 columns).  This kernel's own text: on
  // fcm_store_partials and a 16-column fcm_reduce_row its STREAM instantiations compile to other code than the one measured
  auto store_partials = [&](const f32x4 (&acc)[NF]) {
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int r = 0; r < 4; ++r) *(float*)(red + ((kq * NF + f) * 16 + fk * 4 + r) * FCS_PITCH + frow * 4) = acc[f][r];
  };
  auto reduce_row = [&](float (&s)[16]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int q = 0; q < 4; ++q) v += *(const f32x4*)(red + (q * NF * 16 + tid) * FCS_PITCH + c * 16);
#pragma unroll
      for (int e = 0; e < 4; ++e) s[4 * c + e] = v[e];
    }
  };
  const FcRendezvous rendezvous{p.cnt, tid, j, kq, s_timeout, members, lane};

  for (int t = 0; t < T_; ++t) {
    // the step's xpre slice of this clip, ahead of the waits: 3 x 8 fp32
    f32x4 x[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) x[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (own) {
      const float* xp = p.xpre + ((long long)b * T_ + t) * (3 * np) + u0;
#pragma unroll
      for (int g3 = 0; g3 < 3; ++g3) { x[2 * g3] = *(const f32x4*)(xp + g3 * np); x[2 * g3 + 1] = *(const f32x4*)(xp + g3 * np + 4); }
    }

    // ---- phase A: [u | r] on the rows of h_{t-1} (h_0 = 0: nothing to multiply at t = 0)
    {
      f32x4 acc[NF];
#pragma unroll
      for (int f = 0; f < NF; ++f) acc[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if constexpr (STREAM) {                              // step 0: the seeded rows of h_{-1}
        const bool first = t == 0;
        const unsigned rstride = first ? p.seed_stride : (unsigned)T_ * (unsigned)(np * 2);
        fcs_gemm<NF>(first ? (const void*)p.seed : (const void*)p.hrows, first ? p.seed_bytes : hbytes,
                     (unsigned)frow * rstride + (first ? 0u : (unsigned)(t - 1) * (unsigned)(np * 2)) + koff, 16u * rstride, bzr, acc);
      } else if (t > 0)
        fcs_gemm<NF>(p.hrows, hbytes, ((unsigned)frow * (unsigned)T_ + (unsigned)(t - 1)) * (unsigned)(np * 2) + koff,
                     16u * (unsigned)T_ * (unsigned)(np * 2), bzr, acc);
      store_partials(acc);
    }
    __syncthreads();
    float rg[8];
    if (red_row) {
      float s[16], rh[8];
      reduce_row(s);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        u[i] = sigmoidf_(s[i] + x[i >> 2][i & 3]);
        rg[i] = sigmoidf_(s[8 + i] + x[2 + (i >> 2)][i & 3]);
        rh[i] = rg[i] * h[i];
      }
      if (own) {
        const unsigned row = SAVE ? (unsigned)b * (unsigned)T_ + (unsigned)t : (unsigned)b;
        FcExch<bf16_t>::publish8(p.rh, rbytes, (row * (unsigned)np + (unsigned)u0) * 2u, rh);
      }
    }
    rendezvous(2 * t);
    // (plain outputs behind the hand-off, under the next phase's loads: in front of it they sit in the queue its drain waits for)
    if (SAVE && own) {
      const long long off = (long long)t * st + (long long)b * np + u0;
      store8f(p.uall + off, u);
      store8f(p.rall + off, rg);
    }

    // ---- phase B: c on the rows of r.h, blend
    {
      f32x4 acc[NF];
#pragma unroll
      for (int f = 0; f < NF; ++f) acc[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (SAVE)
        fcs_gemm<NF>(p.rh, rbytes, ((unsigned)frow * (unsigned)T_ + (unsigned)t) * (unsigned)(np * 2) + koff,
                     16u * (unsigned)T_ * (unsigned)(np * 2), bc, acc);
      else
        fcs_gemm<NF>(p.rh, rbytes, (unsigned)frow * (unsigned)(np * 2) + koff, 16u * (unsigned)(np * 2), bc, acc);
      store_partials(acc);
    }
    __syncthreads();
    float cg[8];
    if (red_row) {
      float s[16];
      reduce_row(s);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        cg[i] = tanhf_(s[i] + x[4 + (i >> 2)][i & 3]);
        // The blend with its roundings spelled out: ONE product rounded, then one fused multiply-add.  Written as
        // u h + (1 - u) c the compiler is free to fuse either product into the add, and it chose differently from unit to unit
        // and from instantiation to instantiation (STREAM = false / true differed in rare last bits, measured at B = 64): a
        // stream cut between a zero-state launch and a seeded one must give the bits of the uncut recurrence.
        h[i] = __builtin_fmaf(u[i], h[i], (1.f - u[i]) * cg[i]);
      }
      if (own) FcExch<bf16_t>::publish8(p.hrows, hbytes, (((unsigned)b * (unsigned)T_ + (unsigned)t) * (unsigned)np + (unsigned)u0) * 2u, h);
    }
    if (t + 1 < T_) rendezvous(2 * t + 1);
    if (own) {
      const long long off = (long long)b * np + u0;
      store8f(p.hall + (long long)(SAVE ? t + 1 : ((t + 1) & 1)) * st + off, h);
      if (SAVE) {
        store8f(p.call + (long long)t * st + off, cg);
        *(u32x4*)(p.hp_all + ((long long)b * (T_ + 1) + t + 1) * np + u0) = fcs_pack8(h);
      }
      if constexpr (STREAM && !SAVE) {
        if (t + 1 == p.n_valid) store8f(p.hsnap + off, h);
      }
    }
  }
  // a launch that lost a member must not look like a result
  __syncthreads();
  if (s_timeout) {
    if (tid == 0 && p.err) { *(volatile unsigned*)p.err = 1u; __threadfence_system(); }
    if (own) {
      float fnan[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) fnan[i] = __builtin_nanf("");
      const long long off = (long long)b * np + u0;
      for (int t = 0; t < T_; ++t) {
        FcExch<bf16_t>::poison8(p.hrows, hbytes, (((unsigned)b * (unsigned)T_ + (unsigned)t) * (unsigned)np + (unsigned)u0) * 2u);
        if (SAVE) store8f(p.hall + (long long)(t + 1) * st + off, fnan);
      }
      if (!SAVE) { store8f(p.hall + off, fnan); store8f(p.hall + st + off, fnan); }
      if constexpr (STREAM && !SAVE) store8f(p.hsnap + off, fnan);
    }
  }
}

}  // namespace rgp
