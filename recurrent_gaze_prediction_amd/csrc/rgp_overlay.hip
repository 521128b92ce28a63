// librgp_hip.so: frame overlays (include/rgp.h, "frame overlays"): n fp32 gaze maps [n, h, w] drawn over uint8 RGB frames
// [n_src, H, W, 3] that are already in device memory, in the arithmetic the host libraries use, bit for bit:
//   resize     the order-3 spline of rgp_spline_resize (spline.hip.h; fp64 prefilter and taps, rounded once to fp32);
//              (h, w) == (H, W) takes the map as it is, as the host's resize does
//   bytescale  scipy's, as image_shared.hip.h states it, between the fp32 min and max of the RESIZED map or the caller's
//              limits
//   colour     c = lut[u], the caller's [256, 3] table (matplotlib's cmap(u8, bytes=True)[..., :3])
//   blend      PIL.Image.blend per byte: alpha 0 the frame's byte, alpha 1 the colour's, otherwise
//              uint8(trunc(float(f) + alpha * float(c - f))), one fp32 multiply and one fp32 add, NOT fused
//
// Work is dealt as (map, band of target rows), 256 threads per workgroup, so that a call of a few frames fills the chip.
// Every workgroup turns its map into spline coefficients in LDS again (h * w fp64, dynamic; a few microseconds).  cmin
// and cmax need the whole resized map, and the resized floats are never stored (1.2 GB for 1024 frames of 405 x 720), so
// there are two launches: overlay_minmax_kernel leaves (min, max, finite) of every band in the workspace,
// overlay_render_kernel combines the bands of its map -- min and max do not depend on the order -- evaluates the spline
// again and renders.  With the caller's limits and a resize the first launch is skipped (every workgroup of the second
// sees the whole source map and can refuse it alone).
//
// The spline.  In rgp_spline_resize's grouping v = wy0 s0 + wy1 s1 + wy2 s2 + wy3 s3 the row sums s_a = wx0 c + wx1 c +
// wx2 c + wx3 c depend on (source row, X) alone.  A wave owns a strip of 192 columns (three per lane) and walks down the
// band's rows; it keeps the sums of the four source rows in use in LDS cells that only the lane that wrote them reads
// (slot = source row mod 4: the rows a target row needs lie in a window of four, so they never collide), and forms a
// row's sums only when a target row first needs it: 4 LDS reads and 7 operations per pixel instead of 16 and 36, no
// table read and no division per pixel, the same bits.  Frames wider than 4 x 192 = 768 columns give a wave several
// strips, whose sums are formed again per chunk (more work per pixel, the same bytes); where a row is longer than a
// chunk only the strips that hold the chunk's columns are walked.
//
// The render works in chunks of whole rows, up to 4096 pixels: the heat bytes of a chunk go to LDS, then `heat_u8` and
// `out` leave as aligned dwords with single bytes at the two ends of the chunk; the frame is read as aligned dwords too
// (read once, non-temporal), shifted into place where frame and output differ in alignment.  Every dword read holds at
// least one byte of the frame.  LDS: 18.8 KiB of coefficients at 49 x 49 (32 KiB at most) + 24 KiB of row sums + 4 KiB
// of heat bytes + the colour table: 48 KiB, three workgroups per CU.
//
// Nothing addresses memory before it is checked: frame_idx[m] is compared with n_src on the device first.  A refused map
// (a NaN or an Inf in it, limits that are not finite or descend, a frame index out of range) passes its frame through
// (zeros where there is no frame), gives heat 0 and is counted once in the status word: the only atomic.  No scratch.
#include <climits>
#include <cstdint>

#include "image_shared.hip.h"
#include "spline.hip.h"

using namespace rgp;
using namespace rgp::img;

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kChunk = 4096;          // pixels whose heat bytes wait in LDS between evaluation and the stores
constexpr int kCols = 3, kStrip = 64 * kCols;   // columns per lane / per wave: 4 strips cover 768 columns
constexpr int kMaxBands = 128;
constexpr int kBlocksWanted = 3072;   // workgroups aimed at: four rounds of 256 CUs x 3; every one prefilters its map again, so no more (measured: 1024 and 8192 are slower)

struct OverlayParams {
  const unsigned char* frames;
  const int* frame_idx;
  const float *maps, *limits;
  const unsigned char* lut;
  unsigned char *out, *heat;
  float* partial;                     // [n][bands][4]: min, max, 1 = nothing refuses the map here, unused
  int* status;
  const double* tab_w;
  const unsigned short* tab_i;
  float alpha, inv_w;                 // 1 / w: the source row of a table entry row * w without a division
  int n, n_src, h, w, H, W, bands, rows_per_band, identity, shared;
  SplineConsts sc;
};

// map m as fp64 in sC, turned into B-spline coefficients in place; false (for the whole workgroup, and sC is then
// undefined) if the map holds a NaN or an Inf
__device__ __forceinline__ bool stage_coefficients(const OverlayParams& p, long long m, double* sC) {
  const int tid = threadIdx.x, n_src = p.h * p.w;
  const float* g = p.maps + m * n_src;
  bool ok = true;
  for (int i = tid; i < n_src; i += kThreads) {
    const float v = g[i];
    ok = ok && finite_f(v);
    sC[i] = (double)v;
  }
  if (__syncthreads_or(!ok)) return false;
  for (int l = tid; l < p.w; l += kThreads) filter_line(sC + l, p.h, p.w, p.sc.z, p.sc.zn[0], p.sc.gain, p.sc.k0[0], p.sc.last);
  __syncthreads();
  for (int l = tid; l < p.h; l += kThreads) filter_line(sC + l * p.w, p.w, 1, p.sc.z, p.sc.zn[1], p.sc.gain, p.sc.k0[1], p.sc.last);
  __syncthreads();
  return true;
}

// the row sums of one source row (sC + row_off) at the strip's columns x0 + lane + 64 j, into the lane's own cells of `slot`
__device__ __forceinline__ void fill_row(const OverlayParams& p, const double* sC, double* slot, int row_off, int x0, int lane) {
#pragma unroll
  for (int j = 0; j < kCols; ++j) {
    const int X = x0 + lane + 64 * j;
    if (X < p.W) slot[lane + 64 * j] = spline_row_sum(sC + row_off, p.tab_w + (p.H + X) * 4, p.tab_i + (p.H + X) * 4);
  }
}

// f(Y, X, v) for the wave's strip [x0, x0 + kStrip) of the target rows [Ya, Yb): v is the fp32 value rgp_spline_resize
// writes at (Y, X).  sS: the wave's 4 slots of kStrip row sums; tags: the source row each slot holds, 16 bits each
// (kNoRows: none).  Everything but the pixel loop is the same for the whole wave.
constexpr unsigned long long kNoRows = ~0ull;

template <class F>
__device__ __forceinline__ void strip_rows(const OverlayParams& p, const double* sC, double* sS, int x0, int Ya, int Yb,
                                           unsigned long long& tags, F&& f) {
  const int lane = threadIdx.x & 63;
  for (int Y = Ya; Y < Yb; ++Y) {
    double wy[4];
    const double* s[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      wy[a] = p.tab_w[Y * 4 + a];
      const int off = p.tab_i[Y * 4 + a];                        // the source row times w, at most 4095
      const unsigned r = (unsigned)(int)((float)off * p.inv_w + 0.5f);   // off is a multiple of w: exact
      const unsigned sh = (r & 3u) * 16u;
      double* slot = sS + (r & 3u) * kStrip;
      if ((unsigned)(tags >> sh & 0xffffull) != r) {
        fill_row(p, sC, slot, off, x0, lane);
        tags = (tags & ~(0xffffull << sh)) | (unsigned long long)r << sh;
      }
      s[a] = slot + lane;
    }
#pragma unroll
    for (int j = 0; j < kCols; ++j) {
      const int X = x0 + lane + 64 * j;
      if (X < p.W) {
        double v = wy[0] * s[0][64 * j];
        v = v + wy[1] * s[1][64 * j];
        v = v + wy[2] * s[2][64 * j];
        v = v + wy[3] * s[3][64 * j];
        f(Y, X, (float)v);
      }
    }
  }
}

// the wave's strips among [s_lo, s_hi) of the rows [Ya, Yb), one after the other; strip s is always wave s % kWaves's
template <class F>
__device__ __forceinline__ void wave_strips(const OverlayParams& p, const double* sC, double* sS, int Ya, int Yb, int s_lo, int s_hi,
                                            unsigned long long& tags, F&& f) {
  const int wave = threadIdx.x >> 6, n_strips = (p.W + kStrip - 1) / kStrip;
  for (int s = wave + (s_lo - wave + kWaves - 1) / kWaves * kWaves; s < s_hi; s += kWaves) {
    if (n_strips > kWaves) tags = kNoRows;                            // the slots held another strip's sums
    strip_rows(p, sC, sS, s * kStrip, Ya, Yb, tags, f);
  }
}

__device__ __forceinline__ bool frame_index_ok(const OverlayParams& p, long long m, int* fi) {
  *fi = p.frame_idx ? p.frame_idx[m] : (int)m;
  return *fi >= 0 && *fi < p.n_src;
}

// ---- first launch: (min, max, finite) of one band of one resized map
__global__ __launch_bounds__(kThreads) void overlay_minmax_kernel(const OverlayParams p) {
  extern __shared__ __attribute__((aligned(16))) double sC[];
  __shared__ double sS[kWaves][4 * kStrip];
  __shared__ float sRed[kWaves * 2];
  const int tid = threadIdx.x;
  const long long m = blockIdx.x / p.bands;
  const int band = blockIdx.x - (int)m * p.bands;
  int fi;
  bool good = frame_index_ok(p, m, &fi);
  if (!p.identity) good = stage_coefficients(p, m, sC) && good;
  const int y0 = band * p.rows_per_band, y1 = min(p.H, y0 + p.rows_per_band);
  float mn = pos_inf(), mx = neg_inf();
  if (good && p.identity) {
    const float* g = p.maps + m * p.H * p.W;
    bool ok = true;
    for (int pix = y0 * p.W + tid; pix < y1 * p.W; pix += kThreads) {
      const float v = g[pix];
      ok = ok && finite_f(v);
      mn = fminf(mn, v);
      mx = fmaxf(mx, v);
    }
    good = !__syncthreads_or(!ok);
  } else if (good) {                             // a resized value is finite, or an overflow of finite data: kept
    unsigned long long tags = kNoRows;
    wave_strips(p, sC, sS[tid >> 6], y0, y1, 0, (p.W + kStrip - 1) / kStrip, tags, [&](int, int, float v) {
      mn = fminf(mn, v);
      mx = fmaxf(mx, v);
    });
  }
  block_minmax<kWaves>(mn, mx, sRed);
  if (tid == 0) {
    float* q = p.partial + 4ll * blockIdx.x;
    q[0] = good ? mn : pos_inf();
    q[1] = good ? mx : neg_inf();
    q[2] = good ? 1.f : 0.f;
    q[3] = 0.f;
  }
}

// PIL.Image.blend on one byte; mode 0: alpha == 0, 1: alpha == 1
__device__ __forceinline__ unsigned blend_byte(unsigned f, unsigned c, float alpha, int mode) {
  if (mode == 0) return f;
  if (mode == 1) return c;
  const float d = alpha * (float)((int)c - (int)f);
  return (unsigned)(int)((float)f + d);
}

// ---- second launch: one band of one map, rendered
__global__ __launch_bounds__(kThreads) void overlay_render_kernel(const OverlayParams p) {
  extern __shared__ __attribute__((aligned(16))) double sC[];
  __shared__ double sS[kWaves][4 * kStrip];
  __shared__ float sRed[kWaves * 2];
  __shared__ __attribute__((aligned(4))) unsigned char sLut[768];
  __shared__ __attribute__((aligned(4))) unsigned char sU[kChunk];
  const int tid = threadIdx.x;
  const long long m = blockIdx.x / p.bands;
  const int band = blockIdx.x - (int)m * p.bands;
  const int HW = p.H * p.W;

  int fi;
  const bool idx_ok = frame_index_ok(p, m, &fi);
  bool good = idx_ok;
  if (!p.identity) good = stage_coefficients(p, m, sC) && good;
  for (int i = tid; i < 768; i += kThreads) sLut[i] = p.lut[i];

  // cmin and cmax: the bands of this map (or, shared, of every map that is not refused), or the caller's
  float mn = pos_inf(), mx = neg_inf();
  if (p.partial) {
    const float* q = p.partial + 4 * m * p.bands;
    for (int b = 0; b < p.bands; ++b) {
      good = good && q[4 * b + 2] != 0.f;
      mn = fminf(mn, q[4 * b]);
      mx = fmaxf(mx, q[4 * b + 1]);
    }
    if (p.shared) {
      mn = pos_inf(); mx = neg_inf();
      for (int mm = tid; mm < p.n; mm += kThreads) {
        const float* r = p.partial + 4ll * mm * p.bands;
        bool all = true;
        float lo = pos_inf(), hi = neg_inf();
        for (int b = 0; b < p.bands; ++b) {
          all = all && r[4 * b + 2] != 0.f;
          lo = fminf(lo, r[4 * b]);
          hi = fmaxf(hi, r[4 * b + 1]);
        }
        if (all) { mn = fminf(mn, lo); mx = fmaxf(mx, hi); }
      }
      block_minmax<kWaves>(mn, mx, sRed);
    }
  }
  if (p.limits) {
    mn = p.limits[2 * m];
    mx = p.limits[2 * m + 1];
    good = good && finite_f(mn) && finite_f(mx) && mx >= mn;
  }
  const bool refused = !good;
  const float scale = bytescale_scale(mn, mx);
  const float alpha = p.alpha;
  const int mode = alpha == 0.f ? 0 : (alpha == 1.f ? 1 : 2);

  const int y0 = band * p.rows_per_band, y1 = min(p.H, y0 + p.rows_per_band);
  const int p1 = y1 * p.W;
  const float* g = p.maps + m * HW;                                  // read by the identity path only
  const unsigned char* fr = idx_ok && p.out ? p.frames + (long long)fi * HW * 3 : nullptr;
  const int step = p.W <= kChunk ? kChunk / p.W * p.W : kChunk;       // whole rows where a row fits
  unsigned long long tags = kNoRows;
  __syncthreads();                                                    // sLut
  for (int c0 = y0 * p.W; c0 < p1; c0 += step) {
    const int cn = min(step, p1 - c0);
    if (!refused && p.identity) {
      for (int i = tid; i < cn; i += kThreads) sU[i] = bytescale_byte(g[c0 + i], mn, scale);
    } else if (!refused) {
      auto put = [&](int Y, int X, float v) {
        const int i = Y * p.W + X - c0;
        if ((unsigned)i < (unsigned)cn) sU[i] = bytescale_byte(v, mn, scale);
      };
      const int Ya = c0 / p.W, Yb = (c0 + cn - 1) / p.W + 1;
      if (p.W <= kChunk) {                                            // whole rows, every strip
        wave_strips(p, sC, sS[tid >> 6], Ya, Yb, 0, (p.W + kStrip - 1) / kStrip, tags, put);
      } else {                                                        // parts of one or two rows: the strips that hold them
        for (int Y = Ya; Y < Yb; ++Y) {
          const int xa = max(c0 - Y * p.W, 0), xb = min(c0 + cn - Y * p.W, p.W);
          wave_strips(p, sC, sS[tid >> 6], Y, Y + 1, xa / kStrip, (xb - 1) / kStrip + 1, tags, put);
        }
      }
    }
    __syncthreads();
    if (p.heat) store_lds_bytes<kThreads>(p.heat + m * HW + c0, refused ? nullptr : sU, cn, tid);
    if (p.out) {
      const unsigned char* frb = fr ? fr + 3ll * c0 : nullptr;        // byte e of the chunk's output is byte e from here
      store_run<kThreads>(p.out + (m * HW + c0) * 3, cn * 3, tid,
                [&](int e) -> unsigned char {
                  const unsigned f = frb ? frb[e] : 0u;
                  if (refused) return (unsigned char)f;
                  const int pix = e / 3;
                  return (unsigned char)blend_byte(f, sLut[sU[pix] * 3 + (e - 3 * pix)], alpha, mode);
                },
                [&](int e) -> unsigned {
                  unsigned fw = 0u;
                  if (frb) {                                          // the aligned dword(s) that hold frame bytes e .. e + 3
                    const uintptr_t a = (uintptr_t)(frb + e);
                    const unsigned sh = (unsigned)(a & 3);            // the same for every dword of the chunk
                    const unsigned* q = (const unsigned*)(a - sh);
                    fw = __builtin_nontemporal_load(q);
                    if (sh) fw = fw >> (8 * sh) | __builtin_nontemporal_load(q + 1) << (32 - 8 * sh);
                  }
                  if (refused) return fw;
                  int pix = e / 3, ch = e - 3 * pix;
                  unsigned r = 0u;
#pragma unroll
                  for (int k = 0; k < 4; ++k) {
                    r |= blend_byte(fw >> (8 * k) & 255u, sLut[sU[pix] * 3 + ch], alpha, mode) << (8 * k);
                    if (++ch == 3) { ch = 0; ++pix; }
                  }
                  return r;
                });
    }
    __syncthreads();
  }
  if (refused && band == 0 && tid == 0) atomicAdd(p.status, 1);
}

struct Bands { int bands, rows; };

// enough workgroups to fill the chip at few maps; a function of (n, H) alone, so both launches agree
Bands bands_for(int n, int H) {
  const int want = std::max(1, std::min(std::min(H, kMaxBands), kBlocksWanted / std::min(n, kBlocksWanted)));
  Bands b;
  b.rows = (H + want - 1) / want;
  b.bands = (H + b.rows - 1) / b.rows;
  return b;
}

size_t partial_bytes(int n, int H) { return align_up((size_t)n * (size_t)bands_for(n, H).bands * 4 * sizeof(float), 64); }

}  // namespace

extern "C" {

size_t rgp_overlay_workspace_bytes(int n, int h, int w, int H, int W) {
  if (n <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return kStatusBytes;
  return kStatusBytes + ((h == H && w == W) ? 0 : spline_tables_bytes(H, W)) + partial_bytes(n, H);
}

int rgp_overlay(const rgp_overlay_args* a, void* workspace, size_t workspace_bytes, rgp_stream_t stream) {
  const char* fn = "rgp_overlay";
  RGP_REQUIRE(a != nullptr, "%s: args is NULL", fn);
  RGP_REQUIRE(a->n >= 0, "%s: n = %d must not be negative", fn, a->n);
  if (a->n == 0) return RGP_OK;
  const int n = a->n, h = a->h, w = a->w, H = a->H, W = a->W;
  RGP_REQUIRE(a->n_src >= 1, "%s: n_src = %d must be positive", fn, a->n_src);
  RGP_REQUIRE(a->frame_idx || a->n_src >= n, "%s: n_src = %d is below n = %d and frame_idx is NULL", fn, a->n_src, n);
  RGP_REQUIRE(H >= 1 && W >= 1 && (long long)H * W <= RGP_METRICS_SCALED_MAX_PIX,
              "%s: frames of H x W = %d x %d: H*W must be in [1, RGP_METRICS_SCALED_MAX_PIX = %d]", fn, H, W, RGP_METRICS_SCALED_MAX_PIX);
  RGP_REQUIRE(h >= 1 && w >= 1, "%s: maps of h x w = %d x %d: both must be positive", fn, h, w);
  const bool identity = h == H && w == W;
  if (!identity) {
    RGP_REQUIRE(h >= 2, "%s: h = %d must be at least 2 when the maps are resized", fn, h);
    RGP_REQUIRE(w >= 2, "%s: w = %d must be at least 2 when the maps are resized", fn, w);
    RGP_REQUIRE((long long)h * w <= RGP_METRICS_MAX_PIX, "%s: maps of %d x %d: h*w must be at most RGP_METRICS_MAX_PIX = %d when they are resized",
                fn, h, w, RGP_METRICS_MAX_PIX);
  }
  RGP_REQUIRE(a->alpha >= 0.f && a->alpha <= 1.f, "%s: alpha = %g must be in [0, 1]", fn, (double)a->alpha);
  RGP_REQUIRE((a->flags & ~(unsigned)RGP_OVERLAY_SHARED_LIMITS) == 0, "%s: unknown flags 0x%x", fn, a->flags);
  const bool shared = (a->flags & RGP_OVERLAY_SHARED_LIMITS) != 0;
  RGP_REQUIRE(!(shared && a->limits), "%s: RGP_OVERLAY_SHARED_LIMITS takes the limits from the data: limits must be NULL", fn);
  RGP_REQUIRE(a->out || a->heat_u8, "%s: out and heat_u8 are both NULL: nothing to compute", fn);
  RGP_REQUIRE(a->maps != nullptr, "%s: maps is NULL", fn);
  RGP_REQUIRE(((size_t)a->maps & 3) == 0, "%s: maps must be 4-byte aligned", fn);
  RGP_REQUIRE(a->lut != nullptr, "%s: lut is NULL", fn);
  RGP_REQUIRE(((size_t)a->limits & 3) == 0, "%s: limits must be 4-byte aligned", fn);
  RGP_REQUIRE(((size_t)a->frame_idx & 3) == 0, "%s: frame_idx must be 4-byte aligned", fn);
  const Bands B = bands_for(n, H);
  RGP_REQUIRE((long long)n * B.bands <= INT_MAX, "%s: n = %d: too many maps for one call", fn, n);
  if (a->out) {
    RGP_REQUIRE(a->frames != nullptr, "%s: frames is NULL", fn);
    const uintptr_t o0 = (uintptr_t)a->out, o1 = o0 + (size_t)n * H * W * 3;
    const uintptr_t f0 = (uintptr_t)a->frames, f1 = f0 + (size_t)a->n_src * H * W * 3;
    RGP_REQUIRE(o1 <= f0 || f1 <= o0, "%s: out must not alias frames", fn);
  }
  const size_t need = rgp_overlay_workspace_bytes(n, h, w, H, W);
  RGP_TRY(require_workspace(fn, workspace, workspace_bytes, need, RGP_EWORKSPACE));

  OverlayParams p{};
  p.frames = a->frames; p.frame_idx = a->frame_idx; p.maps = a->maps; p.limits = a->limits; p.lut = a->lut;
  p.out = a->out; p.heat = a->heat_u8; p.alpha = a->alpha;
  p.n = n; p.n_src = a->n_src; p.h = h; p.w = w; p.H = H; p.W = W;
  p.bands = B.bands; p.rows_per_band = B.rows; p.identity = identity; p.shared = shared;
  char* ws = (char*)workspace;
  p.status = (int*)ws;
  size_t off = kStatusBytes;
  hipStream_t s = (hipStream_t)stream;
  if (!identity) {
    p.sc = spline_consts(h, w);
    p.inv_w = 1.0f / (float)w;
    RGP_TRY(upload_tables(h, w, H, W, ws + off, s, &p.tab_w, &p.tab_i));
    off += spline_tables_bytes(H, W);
  }
  // the caller's limits and a resize: every workgroup of the render sees the whole source map, no first launch
  const bool first = identity || !a->limits;
  p.partial = first ? (float*)(ws + off) : nullptr;
  RGP_TRY(clear_status(workspace, s));
  const dim3 grid((unsigned)(n * B.bands));
  const size_t smem = identity ? 0 : (size_t)h * w * sizeof(double);      // the coefficients: at most 32 KiB
  if (first) {
    hipLaunchKernelGGL(overlay_minmax_kernel, grid, dim3(kThreads), smem, s, p);
    RGP_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(overlay_render_kernel, grid, dim3(kThreads), smem, s, p);
  RGP_HIP(hipGetLastError());
  return RGP_OK;
}

int rgp_overlay_status(const void* workspace, int* refused_out, rgp_stream_t stream) {
  int refused;
  RGP_TRY(read_status("rgp_overlay_status", workspace, refused_out, stream, &refused));
  RGP_REQUIRE(refused == 0,
              "rgp_overlay: %d map(s) refused (a NaN or an Inf in the map, limits that are not finite or descend, or a frame "
              "index out of range): the frame unchanged in out, 0 in heat_u8", refused);
  return RGP_OK;
}

}  // extern "C"
