// Persistent fc-GRU BPTT kernel for f32 plans (gfx950, fp32 operands): step 2 of backward_impl (rgp_fcgru.hip) for ALL T steps
// in ONE launch, the fp32 form of fcgru_bptt.hip.h (DESIGN 31 -> 33).  The per-step f32 path runs 4 T dependent launches and
// both of its GEMMs re-stream the transposed fp32 h-side kernels (33.2 MB per step) for at most 64 rows; here they are read
// from memory once per launch.
//
// Decomposition, barriers, rendezvous and time-out are those of fcgru_bptt.hip.h: member j (one 256-thread workgroup, 203
// members) owns units [8j, 8j + 8), wave kq owns K quarter [416 kq, 416 kq + 416), thread b of wave 0 owns clip b and keeps its
// 8 fp32 `carry` values in registers across the sequence; two rendezvous per step on 2 T sharded counters zeroed every call.
// MFMA, operand loads and the K permutation are those of fcgru_seq_f32.hip.h: v_mfma_f32_16x16x4_f32, lane (frow, fk) loads
// 16 bytes at k = 416 kq + 16 i + 4 fk and component e of chunk i feeds MFMA (i, e), A and B alike, so every product is that
// of the per-step path and only the fp32 summation order differs (chunk, component, fk per quarter; quarters ascending).
// The published values are NOT rounded: this is fc_bwd1_kernel<float> / fc_bwd2_kernel<float>.
//
// Exchange: the plan's own fp32 dxpre, rows [F + 1][3 np] = [du_pre | dr_pre | dc_pre], row b T + t + 1.  A member publishes
// 8 units x 4 bytes = TWO 16-byte sc1 stores per clip and part.  Every step has its own row: nothing is overwritten while it
// is read, and the hoisted filter gradients and the b_x GEMM read what they always read.
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
//
// Per step t = T - 1 .. 0:
//   1. local:   dh = dh_head + carry (no carry at T - 1); du_pre = dh (h_prev - c) u (1 - u); dc_pre = dh (1 - u)(1 - c^2);
//               carry = dh u; publish du_pre, dc_pre; rendezvous
//   2. GEMM C:  drh = dc_pre rows . Wc_h^T, quarters summed through LDS ascending; carry += drh r;
//               dr_pre = drh h_prev r (1 - r); publish; rendezvous
//   3. GEMM ZR: carry += [du_pre | dr_pre] rows . [Wu_h | Wr_h]^T.  No rendezvous behind it: the carry is member-local.
// Step 0 stores the final carry into g->carry, where the per-step path leaves dh0.
// Padding: rows >= B of the last fragment lie behind the end of dxpre and read zeros (buffer bounds; the host refuses sequences
// whose (B16 T + 1) rows pass 2^32 bytes); nothing is stored for them.
// Time-out: as fcgru_bptt.hip.h.  A member past its deadline stops waiting and sets the plan's error word; at the end of the
// launch it NaN-poisons its 8 units of all three parts of every dxpre row and of g->carry.
#pragma once
#include "fcgru_seq_f32.hip.h"
#include "fcgru_bptt.hip.h"

namespace rgp {

constexpr unsigned FCB32_ROW = 3u * FCS_NP * 4u;     // bytes per fp32 dxpre row

struct FcBptt32Params {
  const float* b_c;          // packed [np][np]: row k = Wc_h[k][:]
  const float* b_zr;         // packed [np][2 np]: row k = [Wu_h[k][:] | Wr_h[k][:]]
  const float* dh_head;      // [B T][np] d loss / d h_t through the read-out
  const float* hall;         // hall_t [T+1][B][np]: slot t = h_{t-1} of step t
  const float* uall;         // [T][B][np]
  const float* rall;
  const float* call;
  float* dxpre;              // [B T + 1][3 np], row 0 zero and untouched
  float* carry;              // [B][np]: the final carry
  unsigned* cnt;             // [2 T][FCS_SHARDS][FCS_CNT_STRIDE] phase counters, zeroed ahead of the launch
  unsigned* err;             // the plan's pinned error word
  int B, T;
};

template <int NF>
static __global__ __launch_bounds__(SEQ_NT) void fcgru_bptt_f32_kernel(const FcBptt32Params p) {
  __shared__ __attribute__((aligned(16))) char red[4 * NF * 16 * FCS_PITCH];   // [K quarter][row][16 columns]
  __shared__ __attribute__((aligned(16))) char zw[2 * FCS_UNITS * FCS32_CPITCH];   // [u half | r half][unit][K]
  __shared__ int s_timeout;
  const int tid = threadIdx.x, lane = tid & 63;
  const int kq = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int frow = lane & 15, fk = lane >> 4;
  const int j = blockIdx.x, u0 = FCS_UNITS * j;          // member, its first unit
  const int np = FCS_NP, T_ = p.T, B = p.B;
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

  auto rendezvous = [&](int ph) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // every storing wave drains its write-through stores
    __syncthreads();
    unsigned* c = p.cnt + (long long)ph * (FCS_SHARDS * FCS_CNT_STRIDE);
    if (tid == 0) __hip_atomic_fetch_add(c + (j & (FCS_SHARDS - 1)) * FCS_CNT_STRIDE, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (kq == 0 && !s_timeout) {                           // (a member that timed out once stops waiting)
      if (!fcs_wait_phase(c, members, lane) && lane == 0) s_timeout = 1;
    }
    __syncthreads();
  };
  auto load8 = [&](const float* src, float (&v)[8]) {
    const f32x4 lo = *(const f32x4*)src, hi = *(const f32x4*)(src + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[i] = lo[i]; v[4 + i] = hi[i]; }
  };
  auto store8f = [&](float* dst, const float (&v)[8]) {
    *(f32x4*)dst = (f32x4){v[0], v[1], v[2], v[3]};
    *(f32x4*)(dst + 4) = (f32x4){v[4], v[5], v[6], v[7]};
  };
  // the clip's slices of step t: dh_head, h_{t-1}, u, c, r
  struct Slices { float dh[8], h[8], u[8], c[8], r[8]; };
  auto load_step = [&](int t, Slices& s) {
    const long long off = (long long)t * st + coff;
    load8(p.dh_head + ((long long)b * T_ + t) * np + u0, s.dh);
    load8(p.hall + off, s.h);
    load8(p.uall + off, s.u);
    load8(p.call + off, s.c);
    load8(p.rall + off, s.r);
  };
  // the member's 8 units of part `part` (0 du_pre, 1 dr_pre, 2 dc_pre) of this thread's clip row: two 16-byte write-through stores
  auto publish8 = [&](int t, int part, u32x4 lo, u32x4 hi) {
    const unsigned off = ((unsigned)b * (unsigned)T_ + (unsigned)t + 1u) * FCB32_ROW + (unsigned)((part * np + u0) * 4);
    seq_st_sc1(p.dxpre, dxbytes, off, lo);
    seq_st_sc1(p.dxpre, dxbytes, off + 16u, hi);
  };
  auto publish8f = [&](int t, int part, const float (&v)[8]) {
    publish8(t, part, __builtin_bit_cast(u32x4, (f32x4){v[0], v[1], v[2], v[3]}), __builtin_bit_cast(u32x4, (f32x4){v[4], v[5], v[6], v[7]}));
  };
  // the byte offset of part `part` of this lane's fragment row, chunk 0
  auto frag_off = [&](int t, int part) { return ((unsigned)frow * (unsigned)T_ + (unsigned)t + 1u) * FCB32_ROW + (unsigned)(part * np * 4) + koff; };

  float carry[8];
  Slices cur;
#pragma unroll
  for (int i = 0; i < 8; ++i) carry[i] = cur.dh[i] = cur.h[i] = cur.u[i] = cur.c[i] = cur.r[i] = 0.f;
  if (own) load_step(T_ - 1, cur);

  for (int t = T_ - 1; t >= 0; --t) {
    const int ph = 2 * (T_ - 1 - t);
    // ---- 1. local math (carry = 0 at t = T - 1: dh = dh_head)
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
      fcb_store_partials<NF>(red, kq, fk, frow, acc);
    }
    __syncthreads();
    if (red_row) {
      float drh[8], drp[8];
      fcb_reduce_row8<NF>(red, tid, drh);
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
      fcb_store_partials<NF>(red, kq, fk, frow, acc);
    }
    __syncthreads();
    if (red_row) {
      float s[8];
      fcb_reduce_row8<NF>(red, tid, s);
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
      const u32x4 qnan = (u32x4){0x7FC00000u, 0x7FC00000u, 0x7FC00000u, 0x7FC00000u};
      float fnan[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) fnan[i] = __builtin_nanf("");
      for (int t = 0; t < T_; ++t)
        for (int part = 0; part < 3; ++part) publish8(t, part, qnan, qnan);
      store8f(p.carry + coff, fnan);
    }
  }
}

}  // namespace rgp
