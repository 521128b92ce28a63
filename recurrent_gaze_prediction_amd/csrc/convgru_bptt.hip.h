// Persistent BPTT of the ConvGRU (gfx950, bf16 operands): all T backward steps of the recurrence of
// /root/reference/models/gaze_grcn.py:95-129 (what tf.gradients builds for the unrolled cell, base.py:278-281) in ONE
// launch -- the mirror of convgru_seq.hip.h on the same group scheme (seq_group.hip.h).  The per-step path
// (rgp_grcn_bwd.hip) runs 4 T dependent launches.
//
// Per step t (descending), for the gradient dh arriving at h_t (head part dh_head[t] + carry from step t+1):
//   du = dh (h_{t-1} - c), dc = dh (1 - u), carry = dh u;   dz_pre = du u (1-u),  dc_pre = dc (1 - c^2)
//   d(r.h) = conv3x3(dc_pre ; rot180 U^T)                    dr_pre = d(r.h) h_{t-1} r (1-r),  carry += d(r.h) r
//   carry += conv3x3([dz_pre | dr_pre] ; rot180 [U_z ; U_r]^T)
// and dXpre[:, t] = [dz_pre | dr_pre | dc_pre] is what the hoisted filter gradients consume afterwards.
//
// Member j owns the 16 state channels [16j, 16j+16) of every quantity above; its columns of the two transposed filters
// (K = 1152 and 2304: 27 k-steps per wave and K-quarter = 108 VGPRs) stay in registers for the whole sequence, the carry
// of a tile in the registers of the wave that finalises it.  dc_pre, then dz_pre | dr_pre (bf16 operand images) are
// exchanged between the members twice per step.
//
// Streaming (rgp_grcn_backward_stream), template argument STREAM.  STREAM = false is what a backward over all T steps from the
// zero state launches: the source and the parameter block it was measured with.  STREAM = true differentiates the first n_valid
// steps of a streaming forward: the loop runs t = n_valid - 1 .. 0 on phase counters 2 (n_valid - 1 - t), so a film's one-step
// tail pays two rendezvous, not 2 T; the carry registers start from d loss / d state_out (null: zeros); step 0 runs its second
// half as well when d loss / d state_in is wanted, and the wave that owns a tile stores the finished carry there.  Rows keep the
// plan's T as their stride: rows t >= n_valid of dxpre are neither read nor written (the host has zeroed them), and no row is
// addressed that STREAM = false does not address.  A launch that lost a member poisons the dxpre rows t < n_valid -- the bound
// of the poison loop is the bound of the step loop -- and d_state_in.
#pragma once
#include "seq_group.hip.h"

namespace rgp {

struct BpttParams {
  const bf16_t* w_c;         // packed dgrad filter of U:        [128][K = tap*128 + o]
  const bf16_t* w_zr;        // packed dgrad filter of U_z|U_r:  [128][K = tap*256 + gate*128 + o]
  const float* dh_head;      // [T][B][49][128] gradient reaching h_t from the head (after the batch-norm backward)
  const float* hall;         // [T+1][B][49][128]
  const float* uall;         // [T][B][49][128]
  const float* rall;
  const float* call;
  float* dxpre;              // [B][T][49][384]
  bf16_t* xch_c;             // [ngroups][98][128] exchange images
  bf16_t* xch_z;
  bf16_t* xch_r;
  SeqGroupArgs g;            // 2 T phase counters per group
  int T;
};
// STREAM = true takes this on top (the STREAM = false instantiations keep the parameter block they were measured with)
struct BpttStreamParams : BpttParams {
  int n_valid;               // steps of the streaming forward to differentiate, 1 .. T
  const float* d_state_out;  // [B][49][128] fp32 gradient reaching the state behind step n_valid, or null = zeros
  float* d_state_in;         // [B][49][128] fp32 d loss / d state_in, or null = not wanted
};
// The streaming arguments that only the prologue and the epilogue need (the two state pointers, the poison loop's bound) are read
// from the kernel's argument block again where they are used, behind an opaque barrier the compiler cannot hoist the load over:
// held in SGPRs across the step loop they were spilled to VGPR lanes (the <7> kernel has no scalar register to spare).  The block
// is the kernel's only argument: it starts at the kernarg segment.
__device__ __forceinline__ const BpttStreamParams* bptt_stream_args() {
  auto k = __builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(k));
  return (const BpttStreamParams*)k;
}
template <bool STREAM> struct BpttParamsOf { typedef BpttParams type; };
template <> struct BpttParamsOf<true> { typedef BpttStreamParams type; };

// LDS, the forward kernel's layout and size: two operand images, 4 x NF partial tiles of 1 KiB (in 56 KiB), staging, flag
constexpr int BPTT_RED_OFF = 2 * SEQ_IMG;
constexpr int BPTT_STAGE_OFF = BPTT_RED_OFF + 56 * 1024;
constexpr int BPTT_FLAG_OFF = BPTT_STAGE_OFF + 4 * 512;
constexpr int BPTT_SMEM = BPTT_FLAG_OFF + 16;
static_assert(BPTT_SMEM <= 160 * 1024, "LDS budget");

template <int NF, bool STREAM>
static __global__ __launch_bounds__(SEQ_NT) void convgru_bptt_kernel(const typename BpttParamsOf<STREAM>::type p) {
  extern __shared__ __attribute__((aligned(16))) char sq_smem[];
  char* img_a = sq_smem;                 // dc_pre, later dz_pre
  char* img_b = sq_smem + SEQ_IMG;       // dr_pre
  char* red = sq_smem + BPTT_RED_OFF;
  SeqGroup<NF> g;
  if (!g.init(sq_smem, 2 * SEQ_IMG, BPTT_STAGE_OFF, BPTT_FLAG_OFF, p.g, 2 * p.T)) return;
  const int kq = g.kq, ch = g.ch, clip0 = g.clip0;
  const int S = 128, T_ = p.T;
  // steps of this launch.  A reference: with STREAM = false every use below IS T_, and the kernel compiles to the code that was
  // measured (as a variable of its own, equal to T_, such a kernel took another register allocation)
  int nv = 0;
  if constexpr (STREAM) nv = p.n_valid;
  const int& Tv = STREAM ? (const int&)nv : T_;
  const long long st = (long long)p.g.B * 49 * S;
  const unsigned xbytes = (unsigned)p.g.ngroups * 98u * 256u;

  f32x4 bc[9], bzr[18];
  {
    const bf16_t* wc = p.w_c + (long long)ch * (9 * S);
    const bf16_t* wz = p.w_zr + (long long)ch * (18 * S);
#pragma unroll
    for (int i = 0; i < 9; ++i) bc[i] = *(const f32x4*)(wc + (kq * 9 + i) * 32 + g.fk * 8);
#pragma unroll
    for (int i = 0; i < 18; ++i) bzr[i] = *(const f32x4*)(wz + (kq * 18 + i) * 32 + g.fk * 8);
  }
  int orow[2][4];
  bool ovalid[2][4];
#pragma unroll
  for (int o = 0; o < 2; ++o)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      orow[o][r] = g.own_row(o, r);
      ovalid[o][r] = g.own_valid(o, r);
    }
  float carry[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  if constexpr (STREAM) {                                // d loss / d state_out: this lane's rows, its own channel
    const float* seed = bptt_stream_args()->d_state_out;
    if (seed) {
#pragma unroll
      for (int o = 0; o < 2; ++o)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (ovalid[o][r]) carry[o][r] = seed[((long long)(clip0 * 49 + orow[o][r])) * S + ch];
    }
  }
  __syncthreads();                                       // images zeroed, flag cleared (init)

  for (int t = Tv - 1; t >= 0; --t) {
    // saved forward quantities of this lane's rows (own channels)
    float hp[2][4], uu[2][4], rr[2][4], cc[2][4], dh[2][4];
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        hp[o][r] = uu[o][r] = rr[o][r] = cc[o][r] = dh[o][r] = 0.f;
        if (ovalid[o][r]) {
          const long long off = (long long)t * st + ((long long)(clip0 * 49 + orow[o][r])) * S + ch;
          hp[o][r] = p.hall[off]; uu[o][r] = p.uall[off]; rr[o][r] = p.rall[off]; cc[o][r] = p.call[off];
          dh[o][r] = p.dh_head[off] + carry[o][r];
        }
      }
    float dzp[2][4], dcp[2][4];
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float du = dh[o][r] * (hp[o][r] - cc[o][r]), dc = dh[o][r] * (1.f - uu[o][r]);
        carry[o][r] = dh[o][r] * uu[o][r];
        dcp[o][r] = dc * (1.f - cc[o][r] * cc[o][r]);
        dzp[o][r] = du * uu[o][r] * (1.f - uu[o][r]);
      }
#pragma unroll
    for (int o = 0; o < 2; ++o)
      if (kq + 4 * o < NF) g.publish_tile(p.xch_c, xbytes, g.group, kq + 4 * o, dcp[o]);
    g.arrive(2 * (Tv - 1 - t));
    g.wait(2 * (Tv - 1 - t));
    __syncthreads();
    g.load_image(p.xch_c, xbytes, g.group, img_a);
    __syncthreads();
    // the plain outputs go out BEHIND the hand-off, under the MFMAs that follow (convgru_seq.hip.h): in front of it the
    // hand-off's drain waits for their HBM acknowledgements
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (ovalid[o][r]) {
          const int c = orow[o][r] / 49, r49 = orow[o][r] - c * 49;
          float* row = p.dxpre + (((long long)(clip0 + c) * T_ + t) * 49 + r49) * (3 * S) + ch;
          row[0] = dzp[o][r];
          row[2 * S] = dcp[o][r];
        }

    // ---- d(r.h) = conv3x3(dc_pre; U^T): this wave's K quarter, reduced through LDS
    {
      f32x4 acc[NF];
#pragma unroll
      for (int f = 0; f < NF; ++f) acc[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        f32x4 a[NF];
        g.a_frags(img_a, i, a);
        g.mma(a, bc[i], acc);
        if (i % 3 == 2) __builtin_amdgcn_sched_barrier(0);
      }
      g.template store_partials<1>(red, 0, acc);
    }
    __syncthreads();
    float drp[2][4];
#pragma unroll
    for (int o = 0; o < 2; ++o) {
      f32x4 d = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (kq + 4 * o < NF) d = g.template reduce_tile<1>(red, 0, kq + 4 * o);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        drp[o][r] = d[r] * hp[o][r] * rr[o][r] * (1.f - rr[o][r]);
        carry[o][r] += d[r] * rr[o][r];
      }
    }
    auto store_drp = [&]() {
#pragma unroll
      for (int o = 0; o < 2; ++o)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (ovalid[o][r]) {
            const int c = orow[o][r] / 49, r49 = orow[o][r] - c * 49;
            p.dxpre[(((long long)(clip0 + c) * T_ + t) * 49 + r49) * (3 * S) + S + ch] = drp[o][r];
          }
    };
    // (the last step's carry is not needed by anybody: the recurrence starts from h_0 = 0, gaze_grcn.py:262 -- unless a
    // streaming call asks for it: d loss / d state_in)
    bool last = t == 0;
    if constexpr (STREAM) {
      if (last) last = !bptt_stream_args()->d_state_in;
    }
    if (last) { store_drp(); break; }
#pragma unroll
    for (int o = 0; o < 2; ++o)
      if (kq + 4 * o < NF) {
        g.publish_tile(p.xch_z, xbytes, g.group, kq + 4 * o, dzp[o]);
        g.publish_tile(p.xch_r, xbytes, g.group, kq + 4 * o, drp[o]);
      }
    g.arrive(2 * (Tv - 1 - t) + 1);                       // (the hand-off's barriers also order the partial-tile reads above)
    g.wait(2 * (Tv - 1 - t) + 1);
    __syncthreads();
    g.load_image(p.xch_z, xbytes, g.group, img_a);
    g.load_image(p.xch_r, xbytes, g.group, img_b);
    __syncthreads();
    store_drp();                                           // behind the hand-off, as above

    // ---- carry += conv3x3([dz_pre | dr_pre]; [U_z ; U_r]^T)
    {
      f32x4 acc[NF];
#pragma unroll
      for (int f = 0; f < NF; ++f) acc[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < 18; ++i) {
        const int ks = kq * 18 + i, tap = ks >> 3, gate = (ks >> 2) & 1, cb = ks & 3;
        f32x4 a[NF];
        g.a_frags_at(gate ? img_b : img_a, tap, cb, a);
        g.mma(a, bzr[i], acc);
        if (i % 3 == 2) __builtin_amdgcn_sched_barrier(0);
      }
      g.template store_partials<1>(red, 0, acc);
    }
    __syncthreads();
#pragma unroll
    for (int o = 0; o < 2; ++o) {
      if (kq + 4 * o < NF) {
        const f32x4 d = g.template reduce_tile<1>(red, 0, kq + 4 * o);
#pragma unroll
        for (int r = 0; r < 4; ++r) carry[o][r] += d[r];
      }
    }
    __syncthreads();                                      // partial tiles read before the next step overwrites them
  }
  if constexpr (STREAM) {                                // the finished carry = d loss / d state_in
    float* out = bptt_stream_args()->d_state_in;
    if (out) {
#pragma unroll
      for (int o = 0; o < 2; ++o)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (ovalid[o][r]) out[((long long)(clip0 * 49 + orow[o][r])) * S + ch] = carry[o][r];
    }
  }
  // a group that timed out must not look like a result
  if (g.timed_out()) {
    if constexpr (STREAM) {
      float* out = bptt_stream_args()->d_state_in;
      for (int t = 0; t < Tv; ++t)
#pragma unroll
        for (int o = 0; o < 2; ++o)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (ovalid[o][r]) {
              const int c = orow[o][r] / 49, r49 = orow[o][r] - c * 49;
              p.dxpre[(((long long)(clip0 + c) * T_ + t) * 49 + r49) * (3 * S) + ch] = __builtin_nanf("");
              if (t == 0 && out) out[((long long)(clip0 * 49 + orow[o][r])) * S + ch] = __builtin_nanf("");
            }
    } else {
#pragma unroll
      for (int o = 0; o < 2; ++o)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (ovalid[o][r]) {
            const int c = orow[o][r] / 49, r49 = orow[o][r] - c * 49;
            p.dxpre[(((long long)(clip0 + c) * T_) * 49 + r49) * (3 * S) + ch] = __builtin_nanf("");
          }
    }
  }
}

}  // namespace rgp
