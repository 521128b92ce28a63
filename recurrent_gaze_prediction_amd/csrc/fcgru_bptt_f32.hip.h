// Persistent fc-GRU BPTT kernel for f32 plans (gfx950, fp32 operands): step 2 of backward_impl (rgp_fcgru.hip) for ALL T steps
// in ONE launch, the fp32 form of fcgru_bptt.hip.h (DESIGN 31 -> 33).  The per-step f32 path runs 4 T dependent launches and
// both of its GEMMs re-stream the transposed fp32 h-side kernels (33.2 MB per step) for at most 64 rows; here they are read
// from memory once per launch.
//
// Decomposition, exchange, rendezvous, padding and time-out are described in fcgru_member.hip.h.  The step, its exchange through the
// plan's own dxpre and the final carry: fcgru_bptt.hip.h (the same algebra; the published values are NOT
// rounded here: this is fc_bwd1_kernel<float> / fc_bwd2_kernel<float>).  MFMA, operand loads and the K permutation:
// fcgru_seq_f32.hip.h, so every product is that of the per-step path and only the fp32 summation order differs (chunk,
// component, fk per quarter; quarters ascending).  The host refuses sequences whose (B16 T + 1) dxpre rows pass 2^32 bytes.
//
// Residency.  Three 8-row blocks of fp32 (b_c and the u and r halves of b_zr), 52 KB each.  A block in registers is 104
// dwords per lane (columns 8..15 of every tile multiply zeros), the ring of two A-fragment buffers of fcs32_gemm is 208:
//   b_c           REGISTERS (bcw, 104 dwords): GEMM C stands between the two rendezvous of a step, the short leg
//   b_zr, u half  LDS, 8 rows at the 1668-word pitch of fcgru_seq_f32.hip.h (53 376 bytes)
//   b_zr, r half  LDS, the same
// and GEMM ZR is two fcs32_gemm<NF, true> passes (u half on the du_pre part, r half on the dr_pre part) into one accumulator.
// LDS: 2 x 53 376 + the K-quarter partial tiles (5 120 NF) + the flag = at most 127 236 of 163 840 bytes.
// Registers: wave 0 also carries the clip's slices.  Those of step t - 1 are loaded behind step t's second rendezvous, under
// GEMM ZR (the longer GEMM phase), straight into the registers step t's slices have just left: at that point u, c and dh_head
// are dead since the local math and h_prev and r since the r gate, so ONE set of 40 dwords is enough where fcgru_bptt.hip.h
// holds two.  profiles/fcgru_f32_bptt_kernel_resources.txt: no scratch, no spill at NF = 1 .. 4.
// Streaming: template argument STREAM, as fcgru_bptt.hip.h has it (the loop over n_valid steps, the seeded carry, the poisoning).
#pragma once
#include "fcgru_seq_f32.hip.h"
#include "fcgru_bptt.hip.h"

namespace rgp {

template <int NF, bool STREAM>
static __global__ __launch_bounds__(SEQ_NT) void fcgru_bptt_f32_kernel(const typename FcBpttParamsOf<float, STREAM>::type p) {
  __shared__ __attribute__((aligned(16))) char red[4 * NF * 16 * FCS_PITCH];   // [K quarter][row][16 columns]
  __shared__ __attribute__((aligned(16))) char zw[2 * FCS_UNITS * FCS32_CPITCH];   // [u half | r half][unit][K]
  __shared__ int s_timeout;
  const int tid = threadIdx.x, lane = tid & 63;
  const int kq = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int frow = lane & 15, fk = lane >> 4;
  const int j = blockIdx.x, u0 = FCS_UNITS * j;          // member, its first unit
  const int np = FCS_NP, T_ = p.T, B = p.B;
  // steps of this launch: a reference, so that STREAM = false reads T_ itself (fcgru_bptt.hip.h)
  int nv = 0;
  if constexpr (STREAM) nv = p.n_valid;
  const int& Tv = STREAM ? (const int&)nv : T_;
  const unsigned members = gridDim.x;
  if (tid == 0) s_timeout = 0;

  // ---- resident B operands: chunks [26 kq, 26 kq + 26) of the member's 8 rows of b_c in registers (columns 8..15 zero), its
  // rows of both halves of b_zr in LDS
  f32x4 bcw[FCS32_KC];
  {
    const float* wc = p.b_c + (long long)(u0 + (frow & 7)) * np;
    const f32x4 zero = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < FCS32_KC; ++i) {
      const f32x4 c = *(const f32x4*)(wc + (kq * FCS32_KC + i) * 16 + fk * 4);
      bcw[i] = frow < 8 ? c : zero;
    }
    const float* wz = p.b_zr + (long long)u0 * (2 * np);   // 2 halves x 8 rows x 416 sixteen-byte pieces
    for (int i = tid; i < 2 * FCS_UNITS * (FCS_NP / 4); i += SEQ_NT) {
      const int hr = i / (FCS_NP / 4), k4 = i - hr * (FCS_NP / 4);   // hr = half * 8 + row
      const int half = hr >> 3, row = hr & 7;
      *(f32x4*)(zw + hr * FCS32_CPITCH + k4 * 16) = *(const f32x4*)(wz + (long long)row * (2 * np) + half * np + k4 * 4);
    }
  }
  const unsigned koff = (unsigned)((kq * FCS32_KC * 16 + fk * 4) * 4);      // the lane's K offset in a row part, bytes
  const char* blu = zw + (frow & 7) * FCS32_CPITCH + koff;
  const char* blr = blu + FCS_UNITS * FCS32_CPITCH;
  const bool bzero = frow >= 8;
  // thread b of wave 0 finalises clip b: its carry lives here for the whole sequence
  const int b = tid;
  const bool red_row = tid < NF * 16;                      // (rows >= B are summed and dropped)
  const bool own = red_row && b < B;
  const unsigned dxbytes = ((unsigned)B * (unsigned)T_ + 1u) * FCB32_ROW;    // (below 2^32: rgp_fcgru_create_flags)
  const unsigned fstride = 16u * (unsigned)T_ * FCB32_ROW;                  // fragment f + 1 = clips 16 further on
  const long long st = (long long)B * np;
  const long long coff = (long long)b * np + u0;                            // the clip's slice in a [B][np] slab
  __syncthreads();                                         // flag cleared, both halves of b_zr in LDS

  const FcRendezvous rendezvous{p.cnt, tid, j, kq, s_timeout, members, lane};
  // (lambdas that capture the coordinates by reference, as this kernel always had: DESIGN 34)
  auto load_step = [&](int t, FcbSlices& s) { fcb_load_step(p, b, u0, coff, st, t, s); };
  // the member's 8 units of part `part` (0 du_pre, 1 dr_pre, 2 dc_pre) of this thread's clip row
  auto own_off = [&](int t, int part) { return ((unsigned)b * (unsigned)T_ + (unsigned)t + 1u) * FCB32_ROW + (unsigned)((part * np + u0) * 4); };
  auto publish8f = [&](int t, int part, const float (&v)[8]) { FcExch<float>::publish8(p.dxpre, dxbytes, own_off(t, part), v); };
  // the byte offset of part `part` of this lane's fragment row, chunk 0
  auto frag_off = [&](int t, int part) { return fcb_frag_off<float>(frow, koff, T_, t, part); };

  float carry[8];
  FcbSlices cur;
#pragma unroll
  for (int i = 0; i < 8; ++i) carry[i] = cur.dh[i] = cur.h[i] = cur.u[i] = cur.c[i] = cur.r[i] = 0.f;
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
      publish8f(t, 0, dup);
      publish8f(t, 2, dcp);
    }
    rendezvous(ph);

    // ---- 2. GEMM C on the dc_pre rows (b_c from registers), then the r gate
    {
      f32x4 acc[NF];
#pragma unroll
      for (int f = 0; f < NF; ++f) acc[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
      fcs32_gemm<NF, false>(p.dxpre, dxbytes, frag_off(t, 2), fstride, bcw, nullptr, false, acc);
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
      if (own) publish8f(t, 1, drp);
    }
    rendezvous(ph + 1);
    // the next step's slices, under GEMM ZR, into the registers this step's slices have left (the loads are drained by the
    // vmcnt(0) of the next rendezvous at the latest; the local math of step t - 1 waits for them on its own)
    if (own && t > 0) load_step(t - 1, cur);

    // ---- 3. GEMM ZR on the [du_pre | dr_pre] rows (both halves of b_zr from LDS): the u half, then the r half, one accumulator
    {
      f32x4 acc[NF];
#pragma unroll
      for (int f = 0; f < NF; ++f) acc[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
      fcs32_gemm<NF, true>(p.dxpre, dxbytes, frag_off(t, 0), fstride, bcw, blu, bzero, acc);
      // (fcs32_gemm pins its loads in front of ITS MFMAs; this keeps the r half's loads behind the u half's MFMAs)
      __builtin_amdgcn_sched_barrier(0);
      fcs32_gemm<NF, true>(p.dxpre, dxbytes, frag_off(t, 1), fstride, bcw, blr, bzero, acc);
      fcm_store_partials<NF>(red, kq, fk, frow, acc);
    }
    __syncthreads();
    if (red_row) {
      float s[8];
      fcm_reduce_row8<NF>(red, tid, s);
#pragma unroll
      for (int i = 0; i < 8; ++i) carry[i] += s[i];
    }
    // (the next store_partials stands behind the next step's first rendezvous: its barriers order it behind these reads)
  }
  if (own) store8f(p.carry + coff, carry);                 // d loss / d h_{-1}
  // a launch that lost a member must not look like a result
  __syncthreads();
  if (s_timeout) {
    if (tid == 0 && p.err) { *(volatile unsigned*)p.err = 1u; __threadfence_system(); }
    if (own) {
      float fnan[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) fnan[i] = __builtin_nanf("");
      for (int t = 0; t < Tv; ++t)
        for (int part = 0; part < 3; ++part) FcExch<float>::poison8(p.dxpre, dxbytes, own_off(t, part));
      store8f(p.carry + coff, fnan);
    }
  }
}

}  // namespace rgp
