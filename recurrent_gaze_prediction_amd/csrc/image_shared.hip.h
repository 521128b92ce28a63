// The layer under librgp_hip.so's image-side launches (rgp_frames.hip, rgp_mapexport.hip, rgp_overlay.hip, rgp_gtmaps.hip,
// rgp_gtmaps_full.hip; rgp_salicon.hip for quiet_nanf and the status read-back).  Each of them is pinned bit for bit to
// a host library, and every rule of arithmetic or safety that more than one of them rests on is written down here once:
// the aligned byte-run store, scipy's bytescale, Pillow's checked bounds pairs, transposed weight tables and clip8,
// scipy's `reflect`, the fixation-sample check, the min/max reductions, and the refusal status word of the workspace.
// The kernels hold only how they fetch and lay out their data.  DESIGN.md section 26.
#pragma once
#include <cstdint>

#include "rgp_host.h"

namespace rgp {
namespace img {

// ---------------------------------------------------------------------------------------------------- device: values
__device__ __forceinline__ float quiet_nanf() { return __int_as_float(0x7fc00000); }
__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ __forceinline__ float pos_inf() { return __int_as_float(0x7f800000); }
__device__ __forceinline__ float neg_inf() { return __int_as_float(0xff800000); }
// neither NaN nor Inf: the exponent bits, so that no compiler flag can fold the test away
__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// ------------------------------------------------------------------------------------------- device: the byte store
// n_bytes at dst, which starts at any address, by kT threads of which this one is t: aligned dwords from word_at(e)
// (bytes e .. e + 3 of the run, lowest first), single bytes from byte_at(e) at the two ends (at most 3 each).
template <int kT, class F1, class F4>
__device__ __forceinline__ void store_run(unsigned char* dst, int n_bytes, int t, F1&& byte_at, F4&& word_at) {
  static_assert(kT >= 4, "one thread per byte of an end");
  const int head = min((int)((0 - (uintptr_t)dst) & 3), n_bytes), words = (n_bytes - head) >> 2;
  if (t < head) dst[t] = byte_at(t);
  unsigned* dst32 = (unsigned*)(dst + head);
  for (int i = t; i < words; i += kT) dst32[i] = word_at(head + 4 * i);
  const int tail = head + 4 * words;
  if (t < n_bytes - tail) dst[tail + t] = byte_at(tail + t);
}

// The run from LDS bytes `src`; a null src is a refused item, and what a refused run of bytes holds is said here: 0.
// (rgp_mapexport.hip keeps a form of its own for one wave, with loops at the two ends: this one cost its launch 0.3 us.)
template <int kT>
__device__ __forceinline__ void store_lds_bytes(unsigned char* dst, const unsigned char* src, int n_bytes, int t) {
  store_run<kT>(dst, n_bytes, t,
                [&](int e) -> unsigned char { return src ? src[e] : 0; },
                [&](int e) -> unsigned {
                  if (!src) return 0u;
                  const unsigned char* s = src + e;
                  return (unsigned)s[0] | (unsigned)s[1] << 8 | (unsigned)s[2] << 16 | (unsigned)s[3] << 24;
                });
}

// ----------------------------------------------------------------------------------------------- device: bytescale
// scipy.misc.bytescale (scipy <= 1.2, a NumPy before NEP 50) of fp32 data between cmin and cmax: cscale = cmax - cmin in
// fp32, 1 if that is 0; scale = float32(255.0 / float64(cscale)); b = (v - cmin) * scale, an fp32 subtract and an fp32
// multiply that never fuse; u = uint8(trunc(clip(b, 0, 255) + 0.5f)).  !(b >= 0) takes in the NaN of 0 * inf (255 /
// cscale overflows fp32 for a subnormal range): byte 0, as the x86 conversion gives.
__device__ __forceinline__ float bytescale_scale(float cmin, float cmax) {
#pragma clang fp contract(off)
  float cscale = cmax - cmin;
  if (cscale == 0.f) cscale = 1.f;
  return (float)(255.0 / (double)cscale);
}

__device__ __forceinline__ unsigned char bytescale_byte(float v, float cmin, float scale) {
#pragma clang fp contract(off)
  float b = (v - cmin) * scale;
  if (!(b >= 0.f)) b = 0.f;
  if (b > 255.f) b = 255.f;
  return (unsigned char)(int)(b + 0.5f);
}

// -------------------------------------------------------------------------- device: Pillow's 8-bit resample tables
// a 22-bit fixed-point sum to its byte: round at bit 21, shift, clamp
__device__ __forceinline__ int clip8(int acc) { return min(max((acc + (1 << 21)) >> 22, 0), 255); }

// Entry i of a bounds table as (first, count), checked before anything addresses memory through it: first >= 0,
// 0 <= count <= ksize, first + count <= in.  An entry that fails comes back as (0, 0) and sets `bad`.
__device__ __forceinline__ int2 checked_bounds(const int* bounds, int i, int ksize, int in, bool& bad) {
  int first = bounds[2 * i], n = bounds[2 * i + 1];
  if (first < 0 || n < 0 || n > ksize || first > in - n) { bad = true; first = 0; n = 0; }
  return make_int2(first, n);
}

// The weights k[n_out][ksize] of one pass into LDS transposed, sK[tap][out] for tap < rows: lanes run along the output
// index, so a tap's weights are one conflict-free row.  Zeros past an entry's count sB[out].y (checked: count <= ksize).
// rows: what the reader steps over, at least every count (the frames kernel pads it to a multiple of 4).
template <int kT>
__device__ __forceinline__ void stage_weights_transposed(int* sK, const int* k, const int2* sB, int n_out, int ksize, int rows, int t) {
  for (int i = t; i < n_out * rows; i += kT) {
    const int o = i / rows, tap = i - o * rows;
    sK[tap * n_out + o] = tap < sB[o].y ? k[o * ksize + tap] : 0;
  }
}

// ---------------------------------------------------------------------------------- device: scipy and the fixations
// scipy's `reflect` (d c b a | a b c d | d c b a) at any distance from the line of n entries
__device__ __forceinline__ int reflect(int j, int n) {
  if ((unsigned)j < (unsigned)n) return j;
  const int period = 2 * n;
  int m = j % period;
  if (m < 0) m += period;
  return m < n ? m : period - 1 - m;
}

// a frame's rows [beg, end) of `samples`, and one sample (observer u, raw coordinates a, b): checked before they address.
// Stated as what is refused: the scatter loops branch on it, and the negated form compiled to a slower loop.
__device__ __forceinline__ bool frame_ptr_bad(int beg, int end) { return beg < 0 || end < beg; }
__device__ __forceinline__ bool sample_bad(int u, int a, int b, int n_obs, int d1, int d2) {
  return u < 0 || u >= n_obs || a < 0 || a >= d1 || b < 0 || b >= d2;
}

// ---------------------------------------------------------------------------------------------- device: reductions
// min and max over the wave, to every lane; they do not depend on the order
__device__ __forceinline__ void wave_minmax(float& mn, float& mx) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o));
    mx = fmaxf(mx, __shfl_xor(mx, o));
  }
}

// min and max over the workgroup of kWaves waves, to every thread.  sRed: kWaves * 2 floats, free again at the next call.
template <int kWaves>
__device__ __forceinline__ void block_minmax(float& mn, float& mx, float* sRed) {
  wave_minmax(mn, mx);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) { sRed[wave * 2] = mn; sRed[wave * 2 + 1] = mx; }
  __syncthreads();
  mn = sRed[0]; mx = sRed[1];
#pragma unroll
  for (int wv = 1; wv < kWaves; ++wv) { mn = fminf(mn, sRed[wv * 2]); mx = fmaxf(mx, sRed[wv * 2 + 1]); }
}

// ------------------------------------------------------------------------------------- host: the status protocol
// The workspace of an image-side entry starts with a status area whose first word counts the refused items (frames,
// maps): cleared on the stream ahead of the launch, raised once per refused item with one atomicAdd, read by the
// entry's rgp_*_status.
constexpr int kStatusBytes = 64;

inline int align_i(int v, int a) { return (v + a - 1) / a * a; }

inline int require_workspace(const char* fn, const void* ws, size_t have, size_t need, int code = RGP_EINVAL) {
  if (ws && have >= need && ((size_t)ws & 7) == 0) return RGP_OK;
  return set_err(code, "%s: workspace missing, misaligned or too small (%zu < %zu bytes)", fn, ws ? have : (size_t)0, need);
}

inline int clear_status(void* ws, hipStream_t s) {
  RGP_HIP(hipMemsetAsync(ws, 0, kStatusBytes, s));
  return RGP_OK;
}

// The count, once everything queued on the stream is done, into *refused and (if given) *refused_out; the caller says
// in its own words what a count above 0 means.
inline int read_status(const char* fn, const void* ws, int* refused_out, rgp_stream_t stream, int* refused) {
  RGP_REQUIRE(ws != nullptr, "%s: workspace is NULL", fn);
  hipStream_t s = (hipStream_t)stream;
  *refused = 0;
  RGP_HIP(hipMemcpyAsync(refused, ws, sizeof(int), hipMemcpyDeviceToHost, s));
  RGP_HIP(hipStreamSynchronize(s));
  if (refused_out) *refused_out = *refused;
  return RGP_OK;
}

// A resample pass that runs (in != out) needs its tables.  axis: 'h' or 'v'; in_name: what the entry calls the input's
// extent along it; max_name: the entry's cap on the taps of an output.
inline int require_pass(const char* fn, char axis, int ksize, const void* k, const void* b, const char* in_name, int in, int out,
                        const char* max_name, int max_ksize) {
  RGP_REQUIRE(ksize >= 1 && ksize <= max_ksize, "%s: ksize_%c = %d must be in [1, %s = %d]", fn, axis, ksize, max_name, max_ksize);
  RGP_REQUIRE(k && b, "%s: k%c or b%c is NULL and %s = %d differs from out_%c = %d", fn, axis, axis, in_name, in,
              axis == 'h' ? 'w' : 'h', out);
  return RGP_OK;
}

}  // namespace img
}  // namespace rgp
