// The group-exchange layer of the persistent recurrence kernels (convgru_seq.hip.h, convgru_bptt.hip.h,
// convlstm_seq.hip.h, convlstm_bptt.hip.h; gfx950, bf16 operands): what a kernel that runs a whole recurrence in ONE
// launch shares with the others.  Each kernel keeps its resident filters, its K-loop schedule, its gate math and its
// output stores.
//
// Decomposition.  A recurrent 3x3 convolution on a 7x7 state of 128 channels is K = 1152 deep against a few hundred KB of
// bf16 filters: re-streaming the filters per step costs 12.6 us per CU at the measured 66-73 GB/s L2 -> LDS ingest,
// however the clips are dealt.  So the filters are made RESIDENT: a group of 8 workgroups (one per CU) owns up to 2 clips;
// member j keeps the filter columns of state channels [16j, 16j+16) in REGISTERS, split over its 4 waves (one per SIMD,
// 512 registers each) as 4 K-quarters.  Per phase a wave multiplies the group's 16-row fragments (NF = 4: one clip, 49
// rows; 7: two clips, 98 rows) by its K quarter, the 4 partial tiles are summed through LDS by the wave that OWNS the
// tile (fragments kq and kq + 4 of wave kq: it keeps their fp32 state in registers for the whole sequence), and the new
// bf16 operand image (12.5 KB per clip) is exchanged between the 8 members through an L2-resident buffer.
//
// Exchange protocol (counter form; placement-independent): every payload byte is stored write-through (sc1) as 16-byte
// rows, every storing wave drains (`s_waitcnt vmcnt(0)`), the workgroup barriers, ONE lane adds to the group's monotonic
// phase counter; consumers poll that counter with sc1 loads from one lane (bounded, with s_sleep), barrier, and read the
// payload with sc1 loads only.  Counters are zeroed ahead of the launch.  All 8 x ngroups <= 256 workgroups (256
// threads, 129 - 157 KB of LDS: one per CU) must be resident together; the host checks the CU count and falls back to
// per-step launches otherwise.  A member that never arrives (e.g. two such launches interleaved on one device from
// different processes: keep ONE in flight per device) makes its group time out after ~1 s, NaN-poison its results and
// leave -- a loud failure, never a hang.
// (Measured and not kept: 8-byte {tag, 2 x bf16} granules polled by every member instead of image + counter: 0.61 ms
// instead of 0.23 at B = 64, T = 16; 25 atomic loads per thread and sweep over a 50 KB image are far beyond the <= 4 KB
// that form is meant for.)
#pragma once
#include "igemm.hip.h"

namespace rgp {

constexpr int SEQ_PIXB = 272;                        // bytes per padded pixel: 128 ch bf16 + 16 pad (bank rotation)
constexpr int SEQ_NPIX = 2 * 81 + 24;                // two 9x9 images + a zero region for padding rows (all 9 taps)
constexpr int SEQ_IMG = SEQ_NPIX * SEQ_PIXB;         // 50 592 B
constexpr int SEQ_NT = 256;                          // 4 waves = one per SIMD, each with the whole 512-register file

// What the host hands every such kernel (rgp_host.h, SeqGroupPlan::args)
struct SeqGroupArgs {
  unsigned* cnt;             // [ngroups][phases] phase counters, zeroed before the launch
  unsigned* err;             // host-visible error word of the plan (pinned, mapped): set to 1 by a group that timed out
  int B, NC, ngroups;        // clips, clips per group, groups
  int skip_member;           // fault injection: this member of group 0 leaves at once; -1 = none
};

__device__ __forceinline__ u32x4 seq_ld_sc1(const void* base, unsigned bytes, unsigned off) {
  return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(
      __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000), off, 0, 16));
}
__device__ __forceinline__ void seq_st_sc1(void* base, unsigned bytes, unsigned off, u32x4 v) {
  __builtin_amdgcn_raw_buffer_store_b128(v, __builtin_amdgcn_make_buffer_rsrc(base, 0, bytes, 0x00020000), off, 0, 16);
}

// Bounded wait for a group's phase counter (one lane).  The bound is a DEADLINE on the constant-rate real-time counter
// (s_memrealtime: 100 MHz on gfx950, independent of the shader clock), not an iteration count: how long an iteration takes
// depends on the clock the chip holds and on what else loads the same L2 channel (e.g. a concurrent RCCL kernel), so a
// count bounds nothing in particular.  ~1 s of wall clock; the clock is read every 64th poll.
constexpr unsigned long long SEQ_DEADLINE_TICKS = 100ull * 1000 * 1000;
__device__ __forceinline__ bool seq_wait_phase(const unsigned* cnt) {      // true = all 8 members arrived, false = deadline passed
  if (__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= 8u) return true;
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  for (unsigned spins = 1;; ++spins) {
    __builtin_amdgcn_s_sleep(2);
    if (__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= 8u) return true;
    if ((spins & 63u) == 0 && __builtin_amdgcn_s_memrealtime() - t0 > SEQ_DEADLINE_TICKS) return false;
  }
}
// The same wait for a rendezvous of `n` members (fcgru_seq.hip.h: every workgroup of the launch).  A sibling, not a
// parameter of the function above: the conv-recurrent kernels keep the code they were measured with.
__device__ __forceinline__ bool seq_wait_phase_n(const unsigned* cnt, unsigned n) {
  if (__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= n) return true;
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  for (unsigned spins = 1;; ++spins) {
    __builtin_amdgcn_s_sleep(2);
    if (__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= n) return true;
    if ((spins & 63u) == 0 && __builtin_amdgcn_s_memrealtime() - t0 > SEQ_DEADLINE_TICKS) return false;
  }
}

// pixel of position r49 = 7 y + x in a halo-padded 9x9 image
__device__ __forceinline__ int seq_pad_pix(int r49) { return (r49 / 7 + 1) * 9 + (r49 % 7 + 1); }

// Streaming calls (rgp_*_forward_stream): a recurrence that starts from a caller's state instead of zeros.  One launch
// ahead of the recurrence puts the state where each path reads its step -1 from: the fp32 slot 0 of the state
// snapshots (and of the cell state), the halo-padded operand image of the per-step launches, and the groups' exchange
// image of the persistent kernels, which then `load_image` it as they do behind every hand-off.  The conversion of the
// operand copies is Elem<T>::to = f2bf, the one of publish_tile and of the per-step epilogues: a stream cut anywhere
// sees the bits an uncut recurrence has at that step.  A null source seeds zeros.
struct SeqSeedArgs {
  const float* h_in;         // [B][49][S] fp32, or null
  const float* c_in;         // the same for a cell state (h_in null <=> c_in null)
  float* h0;                 // slot 0 of hall
  float* c0;                 // slot 0 of call, or null: no cell state
  void* pad;                 // operand images (T) of h_0, interior of clip b at pad + b * pad_img_stride; or null
  long long pad_img_stride;  // elements
  bf16_t* xch;               // exchange images [..][98][128], clip b = rows 49 (b % NC) .. of image xch_image0 + b / NC; or null
  int xch_image0, NC;
  int B, S;
};
template <typename T>
static __global__ __launch_bounds__(256) void seq_seed_kernel(const SeqSeedArgs a) {
  const int S4 = a.S >> 2;
  const int total = a.B * 49 * S4;                       // (B <= 2^31 / 2401: far below 2^31)
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int c4 = i % S4, row = i / S4;                 // row = 49 b + r49
    const int b = row / 49, r49 = row - b * 49;
    const long long e = (long long)row * a.S + 4 * c4;
    f32x4 h = (f32x4){0.f, 0.f, 0.f, 0.f}, c = h;
    if (a.h_in) h = *(const f32x4*)(a.h_in + e);
    if (a.c_in) c = *(const f32x4*)(a.c_in + e);
    *(f32x4*)(a.h0 + e) = h;
    if (a.c0) *(f32x4*)(a.c0 + e) = c;
    if (a.pad) {
      T* d = (T*)a.pad + (long long)b * a.pad_img_stride + (long long)seq_pad_pix(r49) * a.S + 4 * c4;
#pragma unroll
      for (int k = 0; k < 4; ++k) d[k] = Elem<T>::to(h[k]);
    }
    if (a.xch) {
      bf16_t* d = a.xch + ((long long)(a.xch_image0 + b / a.NC) * 98 + (b % a.NC) * 49 + r49) * 128 + 4 * c4;
#pragma unroll
      for (int k = 0; k < 4; ++k) d[k] = f2bf(h[k]);
    }
  }
}

// NF is a template parameter so that the MFMA loops carry no run-time guards (measured: wave-uniform `if (f < MF)`
// around the reads / MFMAs cost 25 %).  Every member function is inlined into the kernel: the object is a set of registers.
template <int NF>
struct SeqGroup {
  int tid, lane, kq;         // kq: wave = K quarter (wave-uniform)
  int frow, fk;              // fragment row / k-group of this lane: lane & 15, lane >> 4
  int group, j, ch;          // group, member of it, this lane's state channel 16 j + frow
  int clip0, rows;           // first clip of the group, its rows (49 per clip)
  int abase[NF];             // per-lane A-fragment bases: row frow of fragment f -> pixel of tap (0,0); padding rows -> the zero region
  char* stage;               // this wave's 512-byte staging tile
  unsigned* cnt;             // the group's phase counters
  unsigned* err;
  int* s_timeout;            // LDS flag of the workgroup

  // LDS of the kernel: `img_bytes` of operand images at smem (zeroed here: halo pixels and the zero region stay zero for the
  // whole sequence), 4 staging tiles at stage_off, the flag at flag_off.  false = this workgroup leaves at once.  The
  // kernel barriers once before its first step -- behind its filter loads, which are then in flight across the barrier
  // (in front of them it costs convgru_seq<7> 14 spilled VGPRs).
  __device__ __forceinline__ bool init(char* smem, int img_bytes, int stage_off, int flag_off, const SeqGroupArgs& g, int phases) {
    tid = threadIdx.x; lane = tid & 63;
    kq = __builtin_amdgcn_readfirstlane(tid >> 6);
    frow = lane & 15; fk = lane >> 4;
    stage = smem + stage_off + kq * 512;
    // group / member of this workgroup; with a multiple of 8 groups a group's members sit on one XCD (speed only)
    const int b = blockIdx.x;
    if ((g.ngroups & 7) == 0) { const int slot = b >> 3; group = (slot >> 3) * 8 + (b & 7); j = slot & 7; }
    else { group = b >> 3; j = b & 7; }
    if (group == 0 && j == g.skip_member) return false;     // fault injection: a member that never arrives
    ch = 16 * j + frow;
    clip0 = group * g.NC;
    rows = min(g.NC, g.B - clip0) * 49;
    for (int i = tid; i < img_bytes / 16; i += SEQ_NT) ((u32x4*)smem)[i] = (u32x4){0u, 0u, 0u, 0u};
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const int m = f * 16 + frow;
      int pix = 2 * 81;
      if (m < rows) { const int c = m / 49, q = m - c * 49; pix = c * 81 + (q / 7) * 9 + (q % 7); }
      abase[f] = pix * SEQ_PIXB + fk * 16;
    }
    cnt = g.cnt + (long long)group * phases;
    err = g.err;
    s_timeout = (int*)(smem + flag_off);
    if (tid == 0) *s_timeout = 0;
    return true;
  }

  // Row of the group that element r of this lane's accumulator of owned tile o (fragment kq + 4 o) holds (accumulator
  // layout: row 4 (lane >> 4) + r, column lane & 15); a padding row if it is not below `rows`.
  __device__ __forceinline__ int own_row(int o, int r) const { return (kq + 4 * o) * 16 + fk * 4 + r; }
  // (the first term is what tells the compiler that the NF = 4 kernels own one tile per wave, not two)
  __device__ __forceinline__ bool own_valid(int o, int r) const { return kq + 4 * o < NF && own_row(o, r) < rows; }

  // A fragments of channel block cb of tap `tap`; of k-step i of this wave's quarter of a K = 9 x 128 convolution
  __device__ __forceinline__ void a_frags_at(const char* img, int tap, int cb, f32x4 (&a)[NF]) const {
    const int toff = ((tap / 3) * 9 + tap % 3) * SEQ_PIXB + cb * 64;
#pragma unroll
    for (int f = 0; f < NF; ++f) a[f] = *(const f32x4*)(img + abase[f] + toff);
  }
  __device__ __forceinline__ void a_frags(const char* img, int i, f32x4 (&a)[NF]) const {
    const int ks = kq * 9 + i;
    a_frags_at(img, ks >> 2, ks & 3, a);
  }
  // the MFMAs of one filter column block on them
  __device__ __forceinline__ void mma(const f32x4 (&a)[NF], const f32x4& b, f32x4 (&acc)[NF]) const {
#pragma unroll
    for (int f = 0; f < NF; ++f)
      acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(s16x8, a[f]), __builtin_bit_cast(s16x8, b), acc[f], 0, 0, 0);
  }

  // K-quarter partial tiles of 1 KiB at `red`, G gates per tile: this wave's store, and the sum over the 4 quarters
  template <int G>
  __device__ __forceinline__ void store_partials(char* red, int gate, const f32x4 (&acc)[NF]) const {
#pragma unroll
    for (int f = 0; f < NF; ++f) *(f32x4*)(red + (((kq * NF + f) * G + gate) << 10) + lane * 16) = acc[f];
  }
  template <int G>
  __device__ __forceinline__ f32x4 reduce_tile(const char* red, int gate, int f) const {
    f32x4 s = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; ++q) s += *(const f32x4*)(red + (((q * NF + f) * G + gate) << 10) + lane * 16);
    return s;
  }

  // publish owned 16 x 16 tile f (bf16) as 16-byte rows into exchange image `image` of xch, write-through
  __device__ __forceinline__ void publish_tile(bf16_t* xch, unsigned xbytes, int image, int f, const float (&v)[4]) const {
    bf16_t* sg = (bf16_t*)stage;
#pragma unroll
    for (int r = 0; r < 4; ++r) sg[(fk * 4 + r) * 16 + frow] = f2bf(v[r]);
    // DS operations of one wave execute in order; the COMPILER must not move the 16-byte reads above the 2-byte
    // stores (different access types: type-based alias analysis would let it)
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
    if (lane < 32) {
      const int row = f * 16 + (lane >> 1);
      if (row < rows) {
        const u32x4 q = *(const u32x4*)(stage + lane * 16);
        seq_st_sc1(xch, xbytes, (unsigned)(((image * 98 + row) * 128 + 16 * j + (lane & 1) * 8) * 2), q);
      }
    }
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
  }
  // group rendezvous, part 1: this member's tiles of phase `ph` are published (drain, barrier, one counter add)
  __device__ __forceinline__ void arrive(int ph) const {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // every storing wave drains its write-through stores
    __syncthreads();
    if (tid == 0) __hip_atomic_fetch_add(cnt + ph, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // part 2: all 8 members have published.  Bounded: ~1 s; a workgroup that timed out once stops waiting altogether (its
  // results are poisoned by the kernel's epilogue), so a group with a missing member costs a second, not a second per phase
  __device__ __forceinline__ void wait(int ph) const {
    if (tid == 0) {
      if (!*s_timeout && !seq_wait_phase(cnt + ph)) *s_timeout = 1;
    }
  }
  // part 3, behind a barrier: exchange image `image` into the interior of the 9x9 LDS images at img (the caller barriers
  // again before it reads them)
  __device__ __forceinline__ void load_image(const bf16_t* xch, unsigned xbytes, int image, char* img) const {
    for (int i = tid; i < rows * 16; i += SEQ_NT) {
      const int row = i >> 4, c16 = i & 15;
      const u32x4 q = seq_ld_sc1(xch, xbytes, (unsigned)(((image * 98 + row) * 128 + c16 * 8) * 2));
      const int c = row / 49;
      *(u32x4*)(img + (c * 81 + seq_pad_pix(row - c * 49)) * SEQ_PIXB + c16 * 16) = q;
    }
  }
  // load_image in two halves, for a kernel that has MFMAs to run between the loads and the LDS stores (convlstm_bptt.hip.h):
  // the rows of the image in this thread's registers, then into the 9x9 images
  static constexpr int IMG_IT = ((NF == 4 ? 49 : 98) * 16 + SEQ_NT - 1) / SEQ_NT;
  __device__ __forceinline__ void fetch_image(const bf16_t* xch, unsigned xbytes, int image, u32x4 (&q)[IMG_IT]) const {
#pragma unroll
    for (int k = 0; k < IMG_IT; ++k) {
      const int i = tid + k * SEQ_NT;
      q[k] = (u32x4){0u, 0u, 0u, 0u};
      if (i < rows * 16) q[k] = seq_ld_sc1(xch, xbytes, (unsigned)(((image * 98 + (i >> 4)) * 128 + (i & 15) * 8) * 2));
    }
  }
  __device__ __forceinline__ void put_image(char* img, const u32x4 (&q)[IMG_IT]) const {
#pragma unroll
    for (int k = 0; k < IMG_IT; ++k) {
      const int i = tid + k * SEQ_NT;
      if (i < rows * 16) {
        const int row = i >> 4, c = row / 49;
        *(u32x4*)(img + (c * 81 + seq_pad_pix(row - c * 49)) * SEQ_PIXB + (i & 15) * 16) = q[k];
      }
    }
  }
  // Epilogue: a group that timed out must not look like a result.  true = it did: the plan's error word is set, and the
  // caller NaN-poisons what its consumers read.
  __device__ __forceinline__ bool timed_out() const {
    if (!*s_timeout) return false;
    if (tid == 0 && err) { *(volatile unsigned*)err = 1u; __threadfence_system(); }
    return true;
  }
};

}  // namespace rgp
