// The member layer under the four persistent fc-GRU kernels (gfx950): fcgru_seq.hip.h / fcgru_seq_f32.hip.h (the recurrence, bf16
// and f32 plans) and fcgru_bptt.hip.h / fcgru_bptt_f32.hip.h (the backward-through-time pass).  What is said here holds for all
// four and is described once.  The rendezvous is one piece of code now (FcRendezvous): a change to the protocol or to the
// time-out wait is made here.  Each kernel's file keeps what is its own (which blocks are resident where, its GEMM, its load
// schedule) and, as its own text, what does not survive being moved: the member coordinates, the gate math and the time-out
// epilogue -- as functions they make the compiler schedule and allocate whole kernels anew (DESIGN 34 has the list and the
// figures).  A change to the poisoning is still made in all four files.
//
// Decomposition.  Work is split by hidden unit, so a unit's gate math is local to one workgroup.  Member j (one 256-thread
// workgroup, 4 waves) owns units [8j, 8j + 8) of the padded 1664; members that would own padding only (units >= 1624) are not
// launched: 203 members.  Wave kq owns K quarter [416 kq, 416 kq + 416) of every contraction.  The rows of a GEMM are the clips:
// NF = (B + 15) / 16 fragments of 16, a template parameter, no run-time guards in the MFMA loops.  Rows >= B of the last
// fragment lie behind the end of the exchange buffer and read zeros (buffer bounds; the host refuses sequences whose offsets
// pass 2^32); MFMA rows are independent, and nothing is stored for them.  The 4 K-quarter partial tiles are summed through LDS,
// quarters ascending, by thread b of wave 0, which owns clip b: what it carries from step to step (the forward's 8 fp32 h and
// u, the BPTT's 8 fp32 carry) stays in its registers for the whole sequence, and it publishes the member's 8 units of a row.
// Units 1617 .. 1623 of member 202 have zero kernel rows and zero inputs and stay 0.
//
// Exchange: the plan's own row-major operand rows (FcExch<E>: bf16 rows of 2-byte units, one 16-byte store per member and row;
// fp32 rows, two).  Stores and loads are sc1 (seq_st_sc1 / seq_ld_sc1).
//
// Rendezvous: the protocol of seq_group.hip.h with every member of the launch as the group -- payload as 16-byte sc1
// stores, vmcnt(0), workgroup barrier, one lane adds to the phase's monotonic counter, wave 0 polls it (relaxed,
// agent scope, s_sleep) against the s_memrealtime deadline, barrier, payload read with sc1 loads only.  Two per step: 2 T
// counters, each sharded 8 ways (fcs_wait_phase; measured against one counter, before the loads were pinned: 0.494 vs 0.539 ms
// per forward at 64x16, 0.506 vs 0.610 at 8x35), zeroed ahead of EVERY launch.  No fence per phase.
//
// Time-out: a member whose wait passes the deadline stops waiting (its flag in LDS stays set) and, at the end of the launch,
// sets the plan's error word and NaN-poisons its units of everything the launch hands on -- forward: every h row (all steps,
// all clips), the fp32 states and hsnap, so the logits are NaN; BPTT: all three parts of every dxpre row (streaming
// instantiations: of the n_valid rows they wrote) and g->carry, so every filter gradient, dE and d_state_in is NaN.  A launch that lost a member gives NaN, never finite and wrong.  No test runs this
// path, and none may.
#pragma once
#include "seq_group.hip.h"

namespace rgp {

constexpr int FCS_NP = 1664;                         // padded state (a multiple of 64)
constexpr int FCS_UNITS = 8;                         // units per member
constexpr int FCS_MEMBERS = (1617 + FCS_UNITS - 1) / FCS_UNITS;      // 203
constexpr int FCS_SHARDS = 8;                        // counters per phase (a power of two), 64 bytes apart; member j adds to shard j % 8
constexpr int FCS_CNT_STRIDE = 16;                   // unsigned per shard
constexpr int FCS_PITCH = 80;                        // bytes per row of a partial tile in LDS: 16 fp32 + 4 (bank rotation)

// Wait of a whole wave for a phase whose arrivals are spread over FCS_SHARDS counters (a phase counter that all 203
// members add to is 203 atomics on one address, served one after the other: the fan-in the price list puts at 3 - 4.5 us).
// Lane l < FCS_SHARDS polls shard l; the counters only grow, so their sum, read at different times, never overstates the
// arrivals.  The deadline is seq_wait_phase's.  One shard: the single-lane wait of seq_group.hip.h.
__device__ __forceinline__ bool fcs_wait_phase(const unsigned* cnt, unsigned n, int lane) {
  if (FCS_SHARDS == 1) {
    int ok = 1;
    if (lane == 0) ok = seq_wait_phase_n(cnt, n) ? 1 : 0;
    return __builtin_amdgcn_readfirstlane(ok) != 0;
  }
  const unsigned* mine = cnt + (lane & (FCS_SHARDS - 1)) * FCS_CNT_STRIDE;
  auto arrived = [&]() {
    unsigned v = lane < FCS_SHARDS ? __hip_atomic_load(mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
#pragma unroll
    for (int m = 1; m < FCS_SHARDS; m <<= 1) v += (unsigned)__shfl_xor((int)v, m);
    return (unsigned)__builtin_amdgcn_readfirstlane((int)v) >= n;
  };
  if (arrived()) return true;
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  for (unsigned spins = 1;; ++spins) {
    __builtin_amdgcn_s_sleep(2);
    if (arrived()) return true;
    if ((spins & 63u) == 0 && __builtin_amdgcn_s_memrealtime() - t0 > SEQ_DEADLINE_TICKS) return false;
  }
}

// Rendezvous of phase ph on the counters at cnt: this member's rows are published; on return all members' are.  timed_out: the
// member's flag in LDS (cleared by the kernel ahead of its first barrier).  A function object on references to the kernel's own
// coordinates, made once per kernel: the form of the lambda each kernel had.  In this form the four kernels keep every line of
// their resource reports and their counts of MFMAs, exchange loads and stores, barriers and drains, though not their instruction
// order; as a function on values, or on a struct of coordinates, they do not.
struct FcRendezvous {
  unsigned* const& cnt; const int& tid; const int& j; const int& kq; int& timed_out; const unsigned& members; const int& lane;
  __device__ void operator()(int ph) const {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // every storing wave drains its write-through stores
    __syncthreads();
    unsigned* c = cnt + (long long)ph * (FCS_SHARDS * FCS_CNT_STRIDE);
    if (tid == 0) __hip_atomic_fetch_add(c + (j & (FCS_SHARDS - 1)) * FCS_CNT_STRIDE, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (kq == 0 && !timed_out) {                           // (a member that timed out once stops waiting)
      if (!fcs_wait_phase(c, members, lane) && lane == 0) timed_out = 1;
    }
    __syncthreads();
  }
};

// this wave's partial tiles -> LDS red [K quarter][row][16 columns]; the sum over the 4 quarters of columns 0..7 of row `row`
// (the BPTT pair; the forward kernels keep their 16-column lambdas, see there)
template <int NF>
__device__ __forceinline__ void fcm_store_partials(char* red, int kq, int fk, int frow, const f32x4 (&acc)[NF]) {
#pragma unroll
  for (int f = 0; f < NF; ++f)
#pragma unroll
    for (int r = 0; r < 4; ++r) *(float*)(red + ((kq * NF + f) * 16 + fk * 4 + r) * FCS_PITCH + frow * 4) = acc[f][r];
}
template <int NF>
__device__ __forceinline__ void fcm_reduce_row8(const char* red, int row, float (&s)[8]) {
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; ++q) v += *(const f32x4*)(red + (q * NF * 16 + row) * FCS_PITCH + c * 16);
#pragma unroll
    for (int e = 0; e < 4; ++e) s[4 * c + e] = v[e];
  }
}

__device__ __forceinline__ void load8(const float* src, float (&v)[8]) {
  const f32x4 lo = *(const f32x4*)src, hi = *(const f32x4*)(src + 4);
#pragma unroll
  for (int i = 0; i < 4; ++i) { v[i] = lo[i]; v[4 + i] = hi[i]; }
}
__device__ __forceinline__ void store8f(float* dst, const float (&v)[8]) {
  *(f32x4*)dst = (f32x4){v[0], v[1], v[2], v[3]};
  *(f32x4*)(dst + 4) = (f32x4){v[4], v[5], v[6], v[7]};
}

__device__ __forceinline__ u32x4 fcs_pack8(const float (&v)[8]) {
  u32x4 q;
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = (unsigned)f2bf(v[2 * i]) | ((unsigned)f2bf(v[2 * i + 1]) << 16);
  return q;
}

// The exchange rows per element type: a member's 8 units of a row at byte offset off (16-byte write-through stores)
template <typename E> struct FcExch;
template <> struct FcExch<bf16_t> {
  static constexpr int UNIT = 2;                         // bytes per unit
  static constexpr int ROW = FCS_NP * UNIT;              // bytes per row of h / r.h
  static constexpr unsigned ROW3 = 3u * FCS_NP * 2u;     // bytes per dxpre row [du_pre | dr_pre | dc_pre]
  static constexpr unsigned QNAN = 0x7FC07FC0u;          // two quiet NaNs
  static __device__ __forceinline__ void publish8(void* base, unsigned bytes, unsigned off, const float (&v)[8]) {
    seq_st_sc1(base, bytes, off, fcs_pack8(v));          // rounded once
  }
  static __device__ __forceinline__ void poison8(void* base, unsigned bytes, unsigned off) {
    seq_st_sc1(base, bytes, off, (u32x4){QNAN, QNAN, QNAN, QNAN});
  }
};
template <> struct FcExch<float> {
  static constexpr int UNIT = 4;
  static constexpr int ROW = FCS_NP * UNIT;
  static constexpr unsigned ROW3 = 3u * FCS_NP * 4u;
  static constexpr unsigned QNAN = 0x7FC00000u;
  static __device__ __forceinline__ void store2(void* base, unsigned bytes, unsigned off, u32x4 lo, u32x4 hi) {
    seq_st_sc1(base, bytes, off, lo);
    seq_st_sc1(base, bytes, off + 16u, hi);
  }
  static __device__ __forceinline__ void publish8(void* base, unsigned bytes, unsigned off, const float (&v)[8]) {
    store2(base, bytes, off, __builtin_bit_cast(u32x4, (f32x4){v[0], v[1], v[2], v[3]}), __builtin_bit_cast(u32x4, (f32x4){v[4], v[5], v[6], v[7]}));
  }
  static __device__ __forceinline__ void poison8(void* base, unsigned bytes, unsigned off) {
    const u32x4 qnan = (u32x4){QNAN, QNAN, QNAN, QNAN};
    store2(base, bytes, off, qnan, qnan);
  }
};
constexpr int FCS32_ROW = FcExch<float>::ROW;
constexpr unsigned FCB_ROW = FcExch<bf16_t>::ROW3, FCB32_ROW = FcExch<float>::ROW3;

// ---------------------------------------------------------------- the BPTT pair
// the clip's slices of step t: dh_head, h_{t-1}, u, c, r
struct FcbSlices { float dh[8], h[8], u[8], c[8], r[8]; };
// (b: the clip, u0: the member's first unit, coff = b np + u0, st = B np)
template <typename P>
__device__ __forceinline__ void fcb_load_step(const P& p, int b, int u0, long long coff, long long st, int t, FcbSlices& s) {
  const long long off = (long long)t * st + coff;
  load8(p.dh_head + ((long long)b * p.T + t) * FCS_NP + u0, s.dh);
  load8(p.hall + off, s.h);
  load8(p.uall + off, s.u);
  load8(p.call + off, s.c);
  load8(p.rall + off, s.r);
}
// the byte offset of part `part` (0 du_pre, 1 dr_pre, 2 dc_pre) of dxpre row frow T + t + 1 at the lane's K offset koff: a lane's
// fragment row of fragment 0
template <typename E>
__device__ __forceinline__ unsigned fcb_frag_off(int frow, unsigned koff, int T_, int t, int part) {
  return ((unsigned)frow * (unsigned)T_ + (unsigned)t + 1u) * FcExch<E>::ROW3 + (unsigned)(part * FCS_NP * FcExch<E>::UNIT) + koff;
}

}  // namespace rgp
