// Persistent fc-GRU BPTT kernel (gfx950, bf16 operands): step 2 of backward_impl (rgp_fcgru.hip) for ALL T steps in ONE
// launch -- the mirror of fcgru_seq.hip.h.  The per-step path runs 4 T dependent launches (fc_bwd1_kernel, the b_c
// input-gradient GEMM, fc_bwd2_kernel, the b_zr GEMM), and both GEMMs re-stream the transposed h-side kernels (16.6 MB in
// bf16) for at most 64 rows; here the transposed kernels never move and only the gradient rows do.
//
// Decomposition, exchange, rendezvous, padding and time-out are described in fcgru_member.hip.h (the member owns h units
// k in [8j, 8j + 8); thread b of wave 0 keeps the clip's 8 fp32 `carry` values, d loss / d h_{t-1} as far as it is known).
// This kernel's own:
// Resident B fragments, from the packed images set_weights_impl makes for training plans: rows k of g->b_c (Wc_h
// transposed, K = 1664) and rows k of g->b_zr ([Wu_h | Wr_h] transposed, K = 2 x 1664, u half first) = 3 x 13 fragments
// = 156 VGPRs per lane (the forward holds 104).  The tiles are 16x16x32 with columns 8..15 multiplying zeros, as the
// forward's c block: the phases are bound by latency and ingest, not by the matrix pipe.
//
// The exchange goes through dxpre itself: rows [F + 1][3 np], row b T + t + 1 = [du_pre | dr_pre | dc_pre].  Every step has
// its own row, so nothing is overwritten while it is still read (no write-after-read hazard to order), no second copy is
// stored, and the hoisted filter gradients and the b_x GEMM read what they always read.  The du_pre | dr_pre columns of a
// row are contiguous, in the K order b_zr was packed with.  (dcp and dzr of the workspace are not used by this path.)
//
// Per step t = T - 1 .. 0 (the clip's 8-unit slices of dh_head, hall_t[t], uall[t], call[t], rall[t] are loaded one step
// ahead, under the previous step's phases, into a second set of registers):
//   1. local (fc_bwd1_kernel):  dh = dh_head + carry (no carry at t = T - 1); du = dh (h_prev - c), dc = dh (1 - u),
//      carry = dh u; du_pre = bf16(du u (1 - u)), dc_pre = bf16(dc (1 - c^2)); publish both (16-byte sc1); rendezvous
//   2. GEMM C:   drh = dc_pre rows . Wc_h^T on the member's units, K quarters summed through LDS; then fc_bwd2_kernel:
//      carry += drh r, dr_pre = bf16(drh h_prev r (1 - r)); publish; rendezvous
//   3. GEMM ZR:  carry += [du_pre | dr_pre] rows . [Wu_h | Wr_h]^T, as two fcs_gemm passes (u half, r half), each 13 NF
//      loads in front of 13 NF MFMAs.  Step t - 1's local math follows without a rendezvous: the carry is member-local.
// 2 T counters of its own; none behind the last phase.  Step 0 still runs GEMM ZR and stores the final carry (d loss / d h_{-1},
// fp32 [B][np]) into g->carry, where the per-step path leaves the same quantity.
//
// Streaming (rgp_fcgru_backward_stream), template argument STREAM.  STREAM = false is what a call without a state gradient over
// all T steps launches: the source and the parameter block it was measured with.  STREAM = true differentiates the first n_valid
// steps of a streaming forward: the loop runs t = n_valid - 1 .. 0 on 2 n_valid counters (phase 2 (n_valid - 1 - t)), so a film's
// one-step tail pays two rendezvous, not 2 T; thread b's carry starts from g->carry, where the host has seeded d loss / d state_out
// (padded [B][np], zeros for a null gradient), instead of zero.  The rows keep the plan's T as their stride: no row is addressed
// that STREAM = false does not address, and the host's 32-bit limits hold as they are.  Rows t >= n_valid of dxpre are neither
// read nor written (the host has zeroed them); a launch that lost a member poisons the rows t < n_valid and the carry.
//
// Registers: 156 resident + 13 NF x 4 in flight; at NF = 4 that is 364 of the 512 a wave of a 4-wave workgroup may use, and
// all four instantiations compile without scratch (profiles/fcgru_bptt_kernel_resources.txt): every phase issues its
// 13 NF loads in ONE run at every NF.
#pragma once
#include "fcgru_seq.hip.h"

namespace rgp {

// E: the element type of the plan's operand rows (bf16_t here, float in fcgru_bptt_f32.hip.h)
template <typename E>
struct FcBpttParamsT {
  const E* b_c;              // packed [np][np]: row k = Wc_h[k][:]
  const E* b_zr;             // packed [np][2 np]: row k = [Wu_h[k][:] | Wr_h[k][:]]
  const float* dh_head;      // [B T][np] d loss / d h_t through the read-out
  const float* hall;         // hall_t [T+1][B][np]: slot t = h_{t-1} of step t
  const float* uall;         // [T][B][np]
  const float* rall;
  const float* call;
  E* dxpre;                  // [B T + 1][3 np], row 0 zero and untouched
  float* carry;              // [B][np]: the final carry
  unsigned* cnt;             // [2 T][FCS_SHARDS][FCS_CNT_STRIDE] phase counters, zeroed ahead of the launch
  unsigned* err;             // the plan's pinned error word
  int B, T;
};
// STREAM = true takes this on top (the STREAM = false instantiations keep the parameter block they were measured with)
template <typename E>
struct FcBpttStreamParamsT : FcBpttParamsT<E> {
  int n_valid;               // steps of the streaming forward to differentiate, 1 .. T; carry holds the seed on entry
};
template <typename E, bool STREAM> struct FcBpttParamsOf { typedef FcBpttParamsT<E> type; };
template <typename E> struct FcBpttParamsOf<E, true> { typedef FcBpttStreamParamsT<E> type; };

template <int NF, bool STREAM>
static __global__ __launch_bounds__(SEQ_NT) void fcgru_bptt_kernel(const typename FcBpttParamsOf<bf16_t, STREAM>::type p) {
  __shared__ __attribute__((aligned(16))) char red[4 * NF * 16 * FCS_PITCH];   // [K quarter][row][16 columns]
  __shared__ int s_timeout;
  const int tid = threadIdx.x, lane = tid & 63;
  const int kq = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int frow = lane & 15, fk = lane >> 4;
  const int j = blockIdx.x, u0 = FCS_UNITS * j;          // member, its first unit
  const int np = FCS_NP, T_ = p.T, B = p.B;
  // steps of this launch.  A reference: with STREAM = false every use below IS T_, and the kernel compiles to the code that was
  // measured; as a variable of its own (equal to T_) the same kernel took another register allocation
  int nv = 0;
  if constexpr (STREAM) nv = p.n_valid;
  const int& Tv = STREAM ? (const int&)nv : T_;
  const unsigned members = gridDim.x;
  if (tid == 0) s_timeout = 0;

  // ---- resident B fragments: K steps [13 kq, 13 kq + 13) of the member's 8 rows of b_c and of both halves of b_zr,
  // columns 8..15 of every tile zero
  f32x4 bcw[FCS_KW], bzu[FCS_KW], bzr[FCS_KW];
  {
    const bf16_t* wc = p.b_c + (long long)(u0 + (frow & 7)) * np;
    const bf16_t* wz = p.b_zr + (long long)(u0 + (frow & 7)) * (2 * np);
    const f32x4 zero = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < FCS_KW; ++i) {
      const int k = (kq * FCS_KW + i) * 32 + fk * 8;
      const f32x4 c = *(const f32x4*)(wc + k), zu = *(const f32x4*)(wz + k), zr = *(const f32x4*)(wz + np + k);
      bcw[i] = frow < 8 ? c : zero;
      bzu[i] = frow < 8 ? zu : zero;
      bzr[i] = frow < 8 ? zr : zero;
    }
  }
  // thread b of wave 0 finalises clip b: its carry lives here for the whole sequence
  const int b = tid;
  const bool red_row = tid < NF * 16;                      // (rows >= B are summed and dropped)
  const bool own = red_row && b < B;
  const unsigned dxbytes = ((unsigned)B * (unsigned)T_ + 1u) * FCB_ROW;     // (below 2^32: rgp_fcgru_create_flags)
  const unsigned koff = (unsigned)((kq * FCS_KW * 32 + fk * 8) * 2);        // the lane's K offset in a row part, bytes
  const unsigned fstride = 16u * (unsigned)T_ * FCB_ROW;                   // fragment f + 1 = clips 16 further on
  const long long st = (long long)B * np;
  const long long coff = (long long)b * np + u0;                            // the clip's slice in a [B][np] slab
  __syncthreads();                                         // flag cleared

  const FcRendezvous rendezvous{p.cnt, tid, j, kq, s_timeout, members, lane};
  // (lambdas that capture the coordinates by reference, as this kernel always had: with the shared functions called directly,
  // or own_off made one of them, the kernel compiles to other code than the one that was measured)
  auto load_step = [&](int t, FcbSlices& s) { fcb_load_step(p, b, u0, coff, st, t, s); };
  auto own_off = [&](int t, int part) { return ((unsigned)b * (unsigned)T_ + (unsigned)t + 1u) * FCB_ROW + (unsigned)((part * np + u0) * 2); };
  auto frag_off = [&](int t, int part) { return fcb_frag_off<bf16_t>(frow, koff, T_, t, part); };

  float carry[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) carry[i] = 0.f;
  FcbSlices cur, nxt;
#pragma unroll
  for (int i = 0; i < 8; ++i) cur.dh[i] = cur.h[i] = cur.u[i] = cur.c[i] = cur.r[i] = nxt.dh[i] = nxt.h[i] = nxt.u[i] = nxt.c[i] = nxt.r[i] = 0.f;
  if constexpr (STREAM) {                                  // d loss / d state_out, seeded by the host (this thread alone stores there later)
    if (own) load8(p.carry + coff, carry);
  }
  if (own) load_step(Tv - 1, cur);

  for (int t = Tv - 1; t >= 0; --t) {
    const int ph = 2 * (Tv - 1 - t);
    // ---- 1. local math (carry = 0 at t = T - 1: dh = dh_head; STREAM: the seed)
    if (own) {
      float dup[8], dcp[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float dh = cur.dh[i] + carry[i];
        const float uu = cur.u[i], cc = cur.c[i];
        const float du = dh * (cur.h[i] - cc), dc = dh * (1.f - uu);
        carry[i] = dh * uu;
        dup[i] = du * uu * (1.f - uu);
        dcp[i] = dc * (1.f - cc * cc);
      }
      FcExch<bf16_t>::publish8(p.dxpre, dxbytes, own_off(t, 0), dup);
      FcExch<bf16_t>::publish8(p.dxpre, dxbytes, own_off(t, 2), dcp);
    }
    rendezvous(ph);
    // the next step's slices, under this step's phases (the next rendezvous drains them)
    if (own && t > 0) load_step(t - 1, nxt);

    // ---- 2. GEMM C on the dc_pre rows, then the r gate
    {
      f32x4 acc[NF];
#pragma unroll
      for (int f = 0; f < NF; ++f) acc[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
      fcs_gemm<NF>(p.dxpre, dxbytes, frag_off(t, 2), fstride, bcw, acc);
      fcm_store_partials<NF>(red, kq, fk, frow, acc);
    }
    __syncthreads();
    if (red_row) {
      float drh[8], drp[8];
      fcm_reduce_row8<NF>(red, tid, drh);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float rr = cur.r[i];
        carry[i] += drh[i] * rr;
        drp[i] = drh[i] * cur.h[i] * rr * (1.f - rr);
      }
      if (own) FcExch<bf16_t>::publish8(p.dxpre, dxbytes, own_off(t, 1), drp);
    }
    rendezvous(ph + 1);

    // ---- 3. GEMM ZR on the [du_pre | dr_pre] rows: the u half, then the r half, into one accumulator
    {
      f32x4 acc[NF];
#pragma unroll
      for (int f = 0; f < NF; ++f) acc[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
      fcs_gemm<NF>(p.dxpre, dxbytes, frag_off(t, 0), fstride, bzu, acc);
      // (fcs_gemm pins its loads in front of ITS MFMAs; without this the scheduler hoists the r half's loads in between the
      // u half's MFMAs a few at a time, and at NF = 4 re-uses their registers under short counted waits)
      __builtin_amdgcn_sched_barrier(0);
      fcs_gemm<NF>(p.dxpre, dxbytes, frag_off(t, 1), fstride, bzr, acc);
      fcm_store_partials<NF>(red, kq, fk, frow, acc);
    }
    __syncthreads();
    if (red_row) {
      float s[8];
      fcm_reduce_row8<NF>(red, tid, s);
#pragma unroll
      for (int i = 0; i < 8; ++i) carry[i] += s[i];
    }
    cur = nxt;
    // (the next store_partials stands behind the next step's first rendezvous: its barriers order it behind these reads)
  }
  if (own) store8f(p.carry + coff, carry);                 // d loss / d h_{-1}
  // a launch that lost a member must not look like a result
  __syncthreads();
  if (s_timeout) {
    if (tid == 0 && p.err) { *(volatile unsigned*)p.err = 1u; __threadfence_system(); }
    if (own) {
      const u32x4 qnan = (u32x4){FcExch<bf16_t>::QNAN, FcExch<bf16_t>::QNAN, FcExch<bf16_t>::QNAN, FcExch<bf16_t>::QNAN};
      float fnan[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) fnan[i] = __builtin_nanf("");
      for (int t = 0; t < Tv; ++t)
        for (int part = 0; part < 3; ++part) seq_st_sc1(p.dxpre, dxbytes, own_off(t, part), qnan);
      store8f(p.carry + coff, fnan);
    }
  }
}

}  // namespace rgp
