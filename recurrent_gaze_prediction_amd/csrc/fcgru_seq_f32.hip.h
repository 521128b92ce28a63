// Persistent fc-GRU sequence kernel for f32 plans (gfx950, fp32 operands): ALL T steps of the GRUCell(1617) of gaze_rnn /
// gaze_rnn77 in ONE launch, the fp32 form of fcgru_seq.hip.h (DESIGN 28 -> 32).  The per-step f32 path re-streams the h-side
// kernels ([1664 x 3328] + [1664 x 1664] fp32 = 33.2 MB) every timestep; here they are read from memory once per launch.
//
// Decomposition, exchange, rendezvous, padding and time-out are described in fcgru_member.hip.h.  Phases, exchange buffers, their
// write-after-read argument and streaming: fcgru_seq.hip.h (the gate math is the same text, so STREAM = true and
// STREAM = false round alike here too).  What differs for fp32:
// MFMA: v_mfma_f32_16x16x4_f32, an exact fp32 FMA chain (the instruction of the per-step f32 path, Mma<float>).  Its A and B
//   operands are ONE dword per lane: A[row = l & 15][k = l >> 4], B[k = l >> 4][col = l & 15].
// Operand loads: no dword exchange loads.  Lane (frow, fk) loads 16 bytes at k = 416 kq + 16 i + 4 fk, i in [0, 26), and
//   component e of chunk i feeds MFMA (i, e); the resident B dword of MFMA (i, e) is W[col][416 kq + 16 i + 4 fk + e].  A and B see
//   the same permutation of K, so the product is that of the per-step path and only the fp32 summation order differs: per
//   quarter, chunks i ascending, components e ascending, each MFMA adding its 4 products (fk) to the running sum; then the four
//   quarters kq ascending (reduce_row).
// Residency: the [u | r] block in REGISTERS (one wave's share is 26 x 4 = 104 dwords per lane), the c block in LDS: 8 rows of
//   1664 fp32 (pitch 1668: rows 4 banks apart), 52 KB, copied once ahead of the step loop and read as B operands by
//   ds_read_b128 in phase B (lanes frow and frow + 8 read one address; frow >= 8 then selects zeros).  One fragment's A
//   operands of a K quarter are 104 dwords per lane, so at most TWO fragments' loads fit ahead of their MFMAs: fcs32_gemm
//   keeps a ring of two fragment buffers -- the loads of fragments 0 and 1 in front of the MFMAs of fragment 0, the loads of
//   fragment f + 2 into the buffer fragment f has just freed, in front of the MFMAs of fragment f + 1 (so they fly under 104
//   MFMAs).  Every such order is pinned by a scheduling barrier, and scripts/check_isa_waits.py reads it back from the
//   assembly.  (Tried first: both blocks in registers, 208 + 208 for the ring, which spilled up to 196 VGPRs at
//   NF >= 2.  Resident [u | r] 104 + ring 208 + a transient pair of c chunks leaves the gate math of wave 0 its registers:
//   256 VGPRs + at most 244 AGPRs, no scratch; profiles/fcgru_f32_kernel_resources.txt.)
// Exchange rows: the plan's own fp32 operand rows; hp_all rows are the fp32 h itself, bit for bit, and rh is exactly the fp32
//   product r * h_{t-1}.  64 rows x T x 6656 bytes stay below 2^32: the host refuses T > 8192.
#pragma once
#include "fcgru_seq.hip.h"

namespace rgp {

constexpr int FCS32_KC = FCS_NP / 16 / 4;            // 16-float chunks per wave: 26
constexpr int FCS32_CPITCH = (FCS_NP + 4) * 4;       // bytes per row of the c block in LDS
static_assert(FCS32_KC * 4 * 16 == FCS_NP, "K split");

// A operands of this wave's K quarter from exchange rows (sc1), then the MFMAs of one resident column block on them.
// off0: the lane's byte offset at fragment 0, chunk 0; fragments are fstride bytes apart, chunks 64.
// BLDS = false: the block is b (registers).  true: it is read from LDS at bl (the lane's row and K offset; chunks 64 bytes
// apart), zeros where bzero.
template <int NF, bool BLDS>
__device__ __forceinline__ void fcs32_gemm(const void* base, unsigned bytes, unsigned off0, unsigned fstride, const f32x4 (&b)[FCS32_KC],
                                           const char* bl, bool bzero, f32x4 (&acc)[NF]) {
  constexpr int R = NF < 2 ? NF : 2;                       // fragment buffers: 104 dwords per lane each
  f32x4 a[R][FCS32_KC];
  auto issue = [&](int f) {
    // ONE address register per fragment, the chunk in the instruction's immediate offset: left to reassociate the sum the
    // compiler keeps an address register per load (26 per group; with them NF >= 3 spilled)
    unsigned vf = off0 + (unsigned)f * fstride;
    asm volatile("" : "+v"(vf));
#pragma unroll
    for (int i = 0; i < FCS32_KC; ++i) a[f % R][i] = __builtin_bit_cast(f32x4, seq_ld_sc1(base, bytes, vf + (unsigned)i * 64u));
  };
#pragma unroll
  for (int f = 0; f < R; ++f) issue(f);
  // as in fcs_gemm: left alone the scheduler sinks the loads between the MFMAs and keeps 2 - 3 in flight
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    if constexpr (BLDS) {
      // The LDS block is read again for every fragment, two chunks ahead of their MFMAs and no further: left to the scheduler
      // all 26 reads of a fragment stand in front of its MFMAs, 104 more live registers (spills at NF >= 3).
      f32x4 bq[2][2];
      auto fetch = [&](int g) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          bq[g & 1][c] = *(const f32x4*)(bl + (2 * g + c) * 64);
          if (bzero) bq[g & 1][c] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
      };
      asm volatile("" ::: "memory");
      fetch(0);
#pragma unroll
      for (int g = 0; g < FCS32_KC / 2; ++g) {
        if (g + 1 < FCS32_KC / 2) fetch(g + 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            acc[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[f % R][2 * g + c][e], bq[g & 1][c][e], acc[f], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
#pragma unroll
      for (int i = 0; i < FCS32_KC; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[f % R][i][e], b[i][e], acc[f], 0, 0, 0);
    }
    if (f + R < NF) {                                      // the buffer is free: the next group of loads, under fragment f + 1's MFMAs
      __builtin_amdgcn_sched_barrier(0);
      issue(f + R);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

template <int NF, bool SAVE, bool STREAM>
static __global__ __launch_bounds__(SEQ_NT) void fcgru_seq_f32_kernel(const typename FcSeqParamsOf<float, STREAM>::type p) {
  __shared__ __attribute__((aligned(16))) char red[4 * NF * 16 * FCS_PITCH];   // [K quarter][row][16 columns]
  __shared__ __attribute__((aligned(16))) char cw[FCS_UNITS * FCS32_CPITCH];   // the member's c block [unit][K]
  __shared__ int s_timeout;
  const int tid = threadIdx.x, lane = tid & 63;
  const int kq = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int frow = lane & 15, fk = lane >> 4;
  const int j = blockIdx.x, u0 = FCS_UNITS * j;          // member, its first unit
  const int np = FCS_NP, T_ = p.T, B = p.B;
  const unsigned members = gridDim.x;
  if (tid == 0) s_timeout = 0;

  // ---- resident B operands: chunks [26 kq, 26 kq + 26) of columns [u(8) | r(8)] in registers, the c rows in LDS
  f32x4 bzr[FCS32_KC];
  {
    const float* wz = p.w_zr + (long long)((frow < 8 ? 0 : np) + u0 + (frow & 7)) * np;
#pragma unroll
    for (int i = 0; i < FCS32_KC; ++i) bzr[i] = *(const f32x4*)(wz + (kq * FCS32_KC + i) * 16 + fk * 4);
    const float* wc = p.w_c + (long long)u0 * np;          // 8 rows x 416 sixteen-byte pieces
    for (int i = tid; i < FCS_UNITS * (FCS_NP / 4); i += SEQ_NT) {
      const int row = i / (FCS_NP / 4), k4 = i - row * (FCS_NP / 4);
      *(f32x4*)(cw + row * FCS32_CPITCH + k4 * 16) = *(const f32x4*)(wc + (long long)row * np + k4 * 4);
    }
  }
  const char* bl = cw + (frow & 7) * FCS32_CPITCH + (kq * FCS32_KC * 16 + fk * 4) * 4;
  const bool bzero = frow >= 8;
  // thread b of wave 0 finalises clip b: its fp32 state and update gate live here for the whole sequence
  const int b = tid;
  const bool red_row = tid < NF * 16;                      // (rows >= B are summed and dropped)
  const bool own = red_row && b < B;
  float h[8], u[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) { h[i] = 0.f; u[i] = 0.f; }
  const unsigned hbytes = (unsigned)B * (unsigned)T_ * (unsigned)FCS32_ROW;
  const unsigned rbytes = SAVE ? hbytes : (unsigned)B * (unsigned)FCS32_ROW;
  const unsigned koff = (unsigned)((kq * FCS32_KC * 16 + fk * 4) * 4);   // the lane's K offset in a row, bytes
  const long long st = (long long)B * np;
  if constexpr (STREAM) {                                  // the caller's state: slot 0 of hall (gru_seed_kernel)
    if (own) load8(p.hall + (long long)b * np + u0, h);
  }
  __syncthreads();                                         // flag cleared, c block in LDS

  // (this kernel's own text, as in fcgru_seq.hip.h and for its reason: DESIGN 34)
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
  // the member's 8 units of an exchange row: two 16-byte write-through stores
  auto publish8 = [&](float* base, unsigned bytes, unsigned row, const float (&v)[8]) {
    const unsigned off = (row * (unsigned)np + (unsigned)u0) * 4u;
    seq_st_sc1(base, bytes, off, __builtin_bit_cast(u32x4, (f32x4){v[0], v[1], v[2], v[3]}));
    seq_st_sc1(base, bytes, off + 16u, __builtin_bit_cast(u32x4, (f32x4){v[4], v[5], v[6], v[7]}));
  };

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
        const unsigned rstride = first ? p.seed_stride : (unsigned)T_ * (unsigned)FCS32_ROW;
        fcs32_gemm<NF, false>(first ? (const void*)p.seed : (const void*)p.hrows, first ? p.seed_bytes : hbytes,
                       (unsigned)frow * rstride + (first ? 0u : (unsigned)(t - 1) * (unsigned)FCS32_ROW) + koff, 16u * rstride, bzr, nullptr, false, acc);
      } else if (t > 0)
        fcs32_gemm<NF, false>(p.hrows, hbytes, ((unsigned)frow * (unsigned)T_ + (unsigned)(t - 1)) * (unsigned)FCS32_ROW + koff,
                              16u * (unsigned)T_ * (unsigned)FCS32_ROW, bzr, nullptr, false, acc);
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
      if (own) publish8(p.rh, rbytes, SAVE ? (unsigned)b * (unsigned)T_ + (unsigned)t : (unsigned)b, rh);
    }
    rendezvous(2 * t);
    // (plain outputs behind the hand-off, under the next phase's loads)
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
        fcs32_gemm<NF, true>(p.rh, rbytes, ((unsigned)frow * (unsigned)T_ + (unsigned)t) * (unsigned)FCS32_ROW + koff,
                             16u * (unsigned)T_ * (unsigned)FCS32_ROW, bzr, bl, bzero, acc);
      else
        fcs32_gemm<NF, true>(p.rh, rbytes, (unsigned)frow * (unsigned)FCS32_ROW + koff, 16u * (unsigned)FCS32_ROW, bzr, bl, bzero, acc);
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
        // ONE product rounded, then one fused multiply-add: the blend of fcgru_seq.hip.h (both instantiations round alike)
        h[i] = __builtin_fmaf(u[i], h[i], (1.f - u[i]) * cg[i]);
      }
      if (own) publish8(p.hrows, hbytes, (unsigned)b * (unsigned)T_ + (unsigned)t, h);
    }
    if (t + 1 < T_) rendezvous(2 * t + 1);
    if (own) {
      const long long off = (long long)b * np + u0;
      store8f(p.hall + (long long)(SAVE ? t + 1 : ((t + 1) & 1)) * st + off, h);
      if (SAVE) {
        store8f(p.call + (long long)t * st + off, cg);
        store8f(p.hp_all + ((long long)b * (T_ + 1) + t + 1) * np + u0, h);
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
        publish8(p.hrows, hbytes, (unsigned)b * (unsigned)T_ + (unsigned)t, fnan);   // (on FcExch<float>::poison8 <4, true, *> compile anew)
        if (SAVE) store8f(p.hall + (long long)(t + 1) * st + off, fnan);
      }
      if (!SAVE) { store8f(p.hall + off, fnan); store8f(p.hall + st + off, fnan); }
      if constexpr (STREAM && !SAVE) store8f(p.hsnap + off, fnan);
    }
  }
}

}  // namespace rgp
