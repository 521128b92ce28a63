// librgp_hip.so: the gaze-map export (include/rgp.h, "gaze-map export"): extract_map.py:35-41 -- avg_pool(), which is
// scipy.misc.imresize(a[i], (7, 7)) and p /= p.sum() -- and the bytescale inside scipy.misc.imsave
// (evaluate_gaze.py:148-152), for n fp32 maps [n, H, W] in ONE launch.
//
// Per map (scipy <= 1.2, a NumPy before NEP 50):
//   bytescale   between the map's own fp32 min and max: image_shared.hip.h states the rule (bytescale_scale / _byte).
//   imresize   Pillow's 8-bit resample of one channel with host-made 22-bit tables (frames.resample_coeffs):
//               horizontal, then vertical on the 8-bit intermediate; a pass with in == out is skipped.
//   normalise   p = float64(resized) / float64(sum of the resized bytes): an exact integer sum and one IEEE division;
//               a zero sum gives NaN in every cell, as NumPy's 0 / 0 does.
//
// A wave owns a map, a workgroup kWaves maps.  The workgroup first checks both bounds tables (nothing unchecked
// addresses memory) and stages the weights in LDS transposed ([tap][out]: lanes run along the output index); that ends
// with the only workgroup-wide barriers.  Then every wave works alone: it loads its map once (dword loads, coalesced;
// a map of H * W * 4 bytes starts at no better alignment), keeps it in LDS while the lanes reduce min, max and the
// finite test across the wave, writes the bytes to LDS, resamples from LDS to LDS and divides.  DS operations of one
// wave execute in order, so a wave barrier that only stops the compiler from reordering separates the phases.  Byte
// outputs leave as aligned dwords with single bytes at the two ends (store_bytes).  No scratch, no float atomics.
#include <climits>
#include <cstdint>

#include "image_shared.hip.h"

using namespace rgp;
using namespace rgp::img;

namespace {

constexpr int kWaves = 4;
constexpr int kThreads = 64 * kWaves;
constexpr int kHeadBytes = 16;                         // the flag of the bounds check
constexpr int kMaxSide = RGP_MAPEXPORT_MAX_SIDE;

struct MapExportParams {
  const float* maps;
  const int *kh, *bh, *kv, *bv;
  double* pooled;
  unsigned char *pooled_u8, *bytes;
  int* status;
  int n, h, w, out_h, out_w, ksize_h, ksize_v;
  int taps_h, taps_v;                                   // rows of the transposed weight tables in LDS (0: pass skipped)
  int off_kv, off_bh, off_bv, off_wave;                 // byte offsets into the dynamic LDS
  int wave_bytes, off_bytes, off_mid, off_out;          // a wave's area, and the offsets of its parts behind the map
};

struct Layout {
  int taps_h, taps_v, off_kv, off_bh, off_bv, off_wave, wave_bytes, off_bytes, off_mid, off_out, total;
};

// resize: pooled or pooled_u8 is wanted.  A table row holds ksize entries of which the first n <= min(ksize, in) count.
Layout layout_for(int h, int w, int out_h, int out_w, int ksize_h, int ksize_v, bool resize) {
  Layout L{};
  const bool hpass = resize && w != out_w, vpass = resize && h != out_h;
  L.taps_h = hpass ? std::min(ksize_h, w) : 0;
  L.taps_v = vpass ? std::min(ksize_v, h) : 0;
  int off = kHeadBytes;
  off += L.taps_h * out_w * 4;
  L.off_kv = off;
  off += L.taps_v * out_h * 4;
  L.off_bh = off = align_i(off, 8);
  if (hpass) off += out_w * 8;
  L.off_bv = off;
  if (vpass) off += out_h * 8;
  L.off_wave = off = align_i(off, 16);
  int wo = align_i(h * w * 4, 16);
  L.off_bytes = wo;
  wo += align_i(h * w, 16);
  L.off_mid = wo;
  if (hpass) wo += align_i(h * out_w, 16);
  L.off_out = wo;
  if (vpass) wo += align_i(out_h * out_w, 16);
  L.wave_bytes = wo;
  L.total = L.off_wave + kWaves * L.wave_bytes;
  return L;
}

// the largest layout: 64 x 64 -> 64 x 63 ... every table row as long as a side
static_assert(kHeadBytes + 2 * kMaxSide * kMaxSide * 4 + 2 * kMaxSide * 8 + 16 +
              kWaves * (kMaxSide * kMaxSide * 4 + 3 * kMaxSide * kMaxSide) <= RGP_MAPEXPORT_LDS_BYTES, "the worst case fits");
static_assert(RGP_MAPEXPORT_LDS_BYTES <= 160 * 1024, "LDS of a CU");

// DS operations of one wave execute in order; the compiler must not move LDS reads above the other lanes' writes
__device__ __forceinline__ void wave_sync() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
}

// store_lds_bytes (image_shared.hip.h) for one wave, the ends as loops: with `if (lane < head)` there the launch of 1024
// maps measured 0.3 us (1.5 %) above the parent's, with loops it is equal (profiles/image_shared_ab.txt)
__device__ __forceinline__ void store_bytes(unsigned char* dst, const unsigned char* src, int n_bytes, int lane) {
  const int head = min((int)((0 - (uintptr_t)dst) & 3), n_bytes), words = (n_bytes - head) >> 2;
  for (int e = lane; e < head; e += 64) dst[e] = src ? src[e] : 0;
  unsigned* dst32 = (unsigned*)(dst + head);
  for (int i = lane; i < words; i += 64) {
    const unsigned char* s = src + head + 4 * i;
    dst32[i] = src ? (unsigned)s[0] | (unsigned)s[1] << 8 | (unsigned)s[2] << 16 | (unsigned)s[3] << 24 : 0u;
  }
  for (int e = head + 4 * words + lane; e < n_bytes; e += 64) dst[e] = src ? src[e] : 0;
}

__global__ __launch_bounds__(kThreads) void mapexport_kernel(const MapExportParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  int* sBad = (int*)lds;
  int* sKh = (int*)(lds + kHeadBytes);
  int* sKv = (int*)(lds + p.off_kv);
  int2* sBh = (int2*)(lds + p.off_bh);
  int2* sBv = (int2*)(lds + p.off_bv);

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int h = p.h, w = p.w, out_h = p.out_h, out_w = p.out_w, HW = h * w, OUT = out_h * out_w;
  const bool resize = p.pooled || p.pooled_u8;
  const bool hpass = resize && w != out_w, vpass = resize && h != out_h;

  // ---- 1. the workgroup: every table value that will address memory is checked first, then the weights are staged
  if (hpass || vpass) {
    if (tid == 0) *sBad = 0;
    __syncthreads();
    bool bad = false;
    if (hpass)
      for (int xx = tid; xx < out_w; xx += kThreads) sBh[xx] = checked_bounds(p.bh, xx, p.ksize_h, w, bad);
    if (vpass)
      for (int yy = tid; yy < out_h; yy += kThreads) sBv[yy] = checked_bounds(p.bv, yy, p.ksize_v, h, bad);
    if (bad) atomicOr(sBad, 1);
    __syncthreads();
    // n <= ksize and xmin + n <= in: n <= taps = min(ksize, in), the rows the LDS table has
    stage_weights_transposed<kThreads>(sKh, p.kh, sBh, out_w, p.ksize_h, p.taps_h, tid);
    stage_weights_transposed<kThreads>(sKv, p.kv, sBv, out_h, p.ksize_v, p.taps_v, tid);
    __syncthreads();
  }

  // ---- 2. the wave and its map
  const long long m = (long long)blockIdx.x * kWaves + wave;
  if (m >= p.n) return;
  unsigned char* area = lds + p.off_wave + wave * p.wave_bytes;
  float* sMap = (float*)area;
  unsigned char* sBytes = area + p.off_bytes;
  unsigned char* sMid = area + p.off_mid;
  unsigned char* sOut = area + p.off_out;

  const float* g = p.maps + m * HW;
  float mn = pos_inf(), mx = neg_inf();
  bool finite = true;
#pragma unroll 8
  for (int i = lane; i < HW; i += 64) {
    const float v = g[i];
    sMap[i] = v;
    finite = finite && finite_f(v);
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
  wave_minmax(mn, mx);
  const bool refused = __ballot(!finite) != 0ull || ((hpass || vpass) && *sBad != 0);
  if (refused) {   // a NaN or an Inf in the map, or a bounds table entry out of range: NaN and 0, counted
    if (p.pooled)
      for (int i = lane; i < OUT; i += 64) p.pooled[m * OUT + i] = quiet_nan();
    if (p.pooled_u8) store_bytes(p.pooled_u8 + m * OUT, nullptr, OUT, lane);
    if (p.bytes) store_bytes(p.bytes + m * HW, nullptr, HW, lane);
    if (lane == 0) atomicAdd(p.status, 1);
    return;
  }

  // ---- 3. bytescale: every lane reads back the cells it wrote
  const float scale = bytescale_scale(mn, mx);
  for (int i = lane; i < HW; i += 64) sBytes[i] = bytescale_byte(sMap[i], mn, scale);
  wave_sync();
  if (p.bytes) store_bytes(p.bytes + m * HW, sBytes, HW, lane);
  if (!resize) return;

  // ---- 4. horizontal, then vertical on the 8-bit intermediate; rows of `src` are out_w long from here on
  const unsigned char* src = sBytes;
  if (hpass) {
    for (int item = lane; item < h * out_w; item += 64) {
      const int y = item / out_w, xx = item - y * out_w;
      const int2 bx = sBh[xx];
      const unsigned char* s = sBytes + y * w + bx.x;
      unsigned acc = 0;
      for (int t = 0; t < bx.y; ++t) acc += (unsigned)s[t] * (unsigned)sKh[t * out_w + xx];
      sMid[item] = (unsigned char)clip8((int)acc);
    }
    wave_sync();
    src = sMid;
  }
  if (vpass) {
    for (int item = lane; item < OUT; item += 64) {
      const int yy = item / out_w, xx = item - yy * out_w;
      const int2 by = sBv[yy];
      const unsigned char* s = src + by.x * out_w + xx;
      unsigned acc = 0;
      for (int t = 0; t < by.y; ++t) acc += (unsigned)s[t * out_w] * (unsigned)sKv[t * out_h + yy];
      sOut[item] = (unsigned char)clip8((int)acc);
    }
    wave_sync();
    src = sOut;
  }

  // ---- 5. the sum is an integer, so its order is free; one IEEE float64 division per cell (0 / 0 = NaN)
  int sum = 0;
  for (int i = lane; i < OUT; i += 64) sum += src[i];
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  if (p.pooled) {
    const double s = (double)sum;
    for (int i = lane; i < OUT; i += 64) p.pooled[m * OUT + i] = (double)src[i] / s;
  }
  if (p.pooled_u8) store_bytes(p.pooled_u8 + m * OUT, src, OUT, lane);
}

}  // namespace

extern "C" {

size_t rgp_mapexport_workspace_bytes(void) { return kStatusBytes; }

int rgp_mapexport(const rgp_mapexport_args* a, rgp_stream_t stream) {
  RGP_REQUIRE(a != nullptr, "rgp_mapexport: args is NULL");
  RGP_REQUIRE(a->n >= 0, "rgp_mapexport: n = %d must not be negative", a->n);
  if (a->n == 0) return RGP_OK;
  RGP_REQUIRE(a->h >= 1 && a->h <= kMaxSide, "rgp_mapexport: h = %d must be in [1, RGP_MAPEXPORT_MAX_SIDE = %d]", a->h, kMaxSide);
  RGP_REQUIRE(a->w >= 1 && a->w <= kMaxSide, "rgp_mapexport: w = %d must be in [1, RGP_MAPEXPORT_MAX_SIDE = %d]", a->w, kMaxSide);
  RGP_REQUIRE(a->pooled || a->pooled_u8 || a->bytes, "rgp_mapexport: pooled, pooled_u8 and bytes are all NULL: nothing to compute");
  const bool resize = a->pooled || a->pooled_u8;
  const bool hpass = resize && a->w != a->out_w, vpass = resize && a->h != a->out_h;
  if (resize) {
    RGP_REQUIRE(a->out_h >= 1 && a->out_h <= a->h, "rgp_mapexport: out_h = %d must be in [1, h = %d]", a->out_h, a->h);
    RGP_REQUIRE(a->out_w >= 1 && a->out_w <= a->w, "rgp_mapexport: out_w = %d must be in [1, w = %d]", a->out_w, a->w);
  }
  const char* cap = "RGP_MAPEXPORT_MAX_KSIZE";
  if (hpass) RGP_TRY(require_pass("rgp_mapexport", 'h', a->ksize_h, a->kh, a->bh, "w", a->w, a->out_w, cap, RGP_MAPEXPORT_MAX_KSIZE));
  if (vpass) RGP_TRY(require_pass("rgp_mapexport", 'v', a->ksize_v, a->kv, a->bv, "h", a->h, a->out_h, cap, RGP_MAPEXPORT_MAX_KSIZE));
  RGP_REQUIRE(a->maps != nullptr, "rgp_mapexport: maps is NULL");
  RGP_REQUIRE(((size_t)a->maps & 3) == 0, "rgp_mapexport: maps must be 4-byte aligned");
  RGP_REQUIRE(((size_t)a->pooled & 7) == 0, "rgp_mapexport: pooled must be 8-byte aligned");
  RGP_TRY(require_workspace("rgp_mapexport", a->workspace, a->workspace_bytes, kStatusBytes));
  const Layout L = layout_for(a->h, a->w, resize ? a->out_h : a->h, resize ? a->out_w : a->w, hpass ? a->ksize_h : 0,
                              vpass ? a->ksize_v : 0, resize);
  RGP_REQUIRE(L.total <= RGP_MAPEXPORT_LDS_BYTES, "rgp_mapexport: %d bytes of LDS, above RGP_MAPEXPORT_LDS_BYTES = %d", L.total,
              RGP_MAPEXPORT_LDS_BYTES);

  MapExportParams p{};
  p.maps = a->maps;
  p.kh = hpass ? a->kh : nullptr; p.bh = hpass ? a->bh : nullptr; p.kv = vpass ? a->kv : nullptr; p.bv = vpass ? a->bv : nullptr;
  p.pooled = a->pooled; p.pooled_u8 = a->pooled_u8; p.bytes = a->bytes;
  p.status = (int*)a->workspace;
  p.n = a->n; p.h = a->h; p.w = a->w;
  p.out_h = resize ? a->out_h : a->h; p.out_w = resize ? a->out_w : a->w;
  p.ksize_h = hpass ? a->ksize_h : 0; p.ksize_v = vpass ? a->ksize_v : 0;
  p.taps_h = L.taps_h; p.taps_v = L.taps_v;
  p.off_kv = L.off_kv; p.off_bh = L.off_bh; p.off_bv = L.off_bv; p.off_wave = L.off_wave;
  p.wave_bytes = L.wave_bytes; p.off_bytes = L.off_bytes; p.off_mid = L.off_mid; p.off_out = L.off_out;
  hipStream_t s = (hipStream_t)stream;
  RGP_TRY(ensure_dyn_smem((const void*)mapexport_kernel, RGP_MAPEXPORT_LDS_BYTES));
  RGP_TRY(clear_status(a->workspace, s));
  hipLaunchKernelGGL(mapexport_kernel, dim3((a->n - 1) / kWaves + 1), dim3(kThreads), L.total, s, p);
  RGP_HIP(hipGetLastError());
  return RGP_OK;
}

int rgp_mapexport_status(const void* workspace, int* refused_out, rgp_stream_t stream) {
  int refused;
  RGP_TRY(read_status("rgp_mapexport_status", workspace, refused_out, stream, &refused));
  RGP_REQUIRE(refused == 0,
              "rgp_mapexport: %d map(s) refused (a NaN or an Inf in the map, or a bounds table entry out of range): NaN in "
              "pooled, 0 in pooled_u8 and bytes", refused);
  return RGP_OK;
}

}  // extern "C"
