// librgp_hip.so: ground-truth gaze maps at the frame's own resolution (include/rgp.h, "ground-truth maps at the
// frame's resolution"): the loader's `gazemap_height is None` branch (crc_input_data_seq.py:237-240 with :41-53 and
// :261-288) -- the raw-resolution fixation counts, scipy's Gaussian filter with sigma = 19 on 405 x 720 cells, the
// min-max normalisation per frame.  rgp_gtmaps.hip keeps a whole frame in LDS and stops at 4096 cells; here the planes
// live in HBM and the separable filter is tiled over them.
//
// The rescale of the loader is the identity at out_shape == raw_shape (a * (D - 1) / (D - 1) is exact for every integer
// a < 2^53), so there is no rescale code: a sample (u, a, b) lands in row b, column a.
//
// Launches per call, all on the caller's stream: one hipMemsetAsync over the head of the
// workspace and the mask planes, then
//   1. scatter    one workgroup per frame: every sample is validated, then atomicOr(mask[b * D1 + a], 1 << u) and
//                 atomicOr of the column's bit in the frame's column bitmap.  A bad sample or frame_ptr pair marks the
//                 frame and counts it in the status word.
//   2. pass 1     along the frame's first axis (lines of D2 entries, D1 apart), tiled over (frame, strip of kP1Cols
//                 columns, block of kP1Rows rows): popc / n_observers staged once with the reflected halo, every output
//                 scipy's sum in fp64 rounded once to fp32 into the workspace plane; fixationmaps = popc are written here.
//   3. pass 2     along the second axis into `gazemaps`, tiles of kP2Rows x kP2Cols; each workgroup reduces its min and
//                 max and publishes them with atomicMax on the BIT PATTERNS (max as it is, min complemented): the filtered
//                 values are finite and >= +0, where unsigned order is float order, so the two words are exact and do
//                 not depend on the order the workgroups arrive in.
//   4. normalise  in place from the frame's two words; refused frames are filled with NaN.
// No workgroup waits for another one: what crosses workgroups crosses a launch boundary or is an integer atomic.
//
// Zero skipping.  Every term of every sum is >= +0 and x + (+0.0) == x for x >= +0, so a term whose inputs are both
// +0 may be left out, and a sum all of whose inputs are +0 written as +0 without being formed.  What is left out:
//   * pass 1: a strip without a sample in the frame (column bitmap) reads no mask and writes +0; in the LDS kernel a
//     term both of whose staged rows are +0 across the strip; in the direct kernel a column without a sample;
//   * pass 2: a tile none of whose taps' columns has a sample writes +0; in the LDS kernel a term both of whose columns
//     are without a sample, and a column without a sample is not read at all.
// tests/test_gtmaps_full_cpu.py restates exactly these rules in numpy and holds them to the full oracle.
//
// Radius.  The LDS tiles are sized for radius <= RGP_GTMAPS_FULL_LDS_RADIUS = 76 (sigma = 19).  Above it (up to 256) the
// direct kernels read their taps through the cache hierarchy and form whole sums; same sums, same order.
//
// Exactness: as rgp_gtmaps.hip.  -ffp-contract=off, no fast-math, IEEE division, fp32 denormals kept, host-made weights.
#include <climits>
#include <cmath>

#include "image_shared.hip.h"

using namespace rgp;
using namespace rgp::img;

namespace {

constexpr int kThreads = 256;
constexpr int kLdsRadius = RGP_GTMAPS_FULL_LDS_RADIUS;
constexpr int kP1Cols = 64, kP1Rows = 64;       // pass 1: 64 columns x 64 rows per workgroup, (64 + 2 * 76) x 64 staged
constexpr int kP2Cols = 64, kP2Rows = 64;       // pass 2 in LDS: 64 rows x 64 columns, 64 x (64 + 2 * 76) staged
constexpr int kDirCols = 128, kDirRows = 16;    // pass 2 above kLdsRadius: 16 rows x 128 columns, nothing staged
constexpr int kNormPerThread = 8;
static_assert(RGP_GTMAPS_FULL_TILE_COLS % kP1Cols == 0 && RGP_GTMAPS_FULL_TILE_COLS % kP2Cols == 0 &&
              RGP_GTMAPS_FULL_TILE_COLS % kDirCols == 0, "rgp.h: tile columns");
static_assert(RGP_GTMAPS_FULL_TILE_ROWS % kP1Rows == 0 && RGP_GTMAPS_FULL_TILE_ROWS % kP2Rows == 0 &&
              RGP_GTMAPS_FULL_TILE_ROWS % kDirRows == 0, "rgp.h: tile rows");
static_assert(kP1Cols == 64 && kP2Cols == 64 && kP2Rows == 64 && kDirCols == 128 && kThreads == 256 && kLdsRadius <= 128,
              "the lane-to-cell maps and the two-word pair masks below");

struct FullParams {
  const int *frame_ptr, *samples;
  const double* weights;
  int n_frames, n_obs, d1, d2, radius, col_words;
  float *gaze, *fix;
  int* status;
  unsigned *bad, *max_bits, *negmin_bits, *col_bits, *mask;   // [N], [N], [N], [N][col_words], [N][d2 * d1]
  float* plane;                                                // [N][d2 * d1], between the passes
};

__device__ __forceinline__ bool column_has_sample(const unsigned* bits, int x) { return (bits[x >> 5] >> (x & 31)) & 1u; }

// ---- 1. scatter: every value is checked before it addresses memory
__global__ __launch_bounds__(kThreads) void gtmaps_full_scatter_kernel(const FullParams p) {
  __shared__ int sBad;
  const int tid = threadIdx.x, n = blockIdx.x;
  if (tid == 0) sBad = 0;
  __syncthreads();
  const int beg = p.frame_ptr[n], end = p.frame_ptr[n + 1];
  if (frame_ptr_bad(beg, end)) {
    if (tid == 0) sBad = 1;
  } else {
    unsigned* mask = p.mask + (long long)n * p.d1 * p.d2;
    unsigned* cols = p.col_bits + (long long)n * p.col_words;
    for (int i = beg + tid; i < end; i += kThreads) {
      const int* row = p.samples + (long long)i * 3;
      const int u = row[0], a = row[1], b = row[2];
      if (sample_bad(u, a, b, p.n_obs, p.d1, p.d2)) { atomicOr(&sBad, 1); continue; }
      atomicOr(&mask[b * p.d1 + a], 1u << u);
      atomicOr(&cols[a >> 5], 1u << (a & 31));
    }
  }
  __syncthreads();
  if (tid == 0 && sBad != 0) {
    p.bad[n] = 1u;
    atomicAdd(p.status, 1);
  }
}

// ---- the sums of the LDS path.  The plane ahead of either pass is almost entirely +0 (at most 32 observers, a handful of
// samples), so a workgroup keeps one flag per staged line across its lanes' extent -- pass 1: the staged ROW has a non-zero
// cell within the strip's columns; pass 2: the staged COLUMN has a sample in the frame -- and a wave, whose lanes share the
// output's position along the filtered axis, forms only the terms (line[l+i] + line[l-i]) w[i+r] one of whose lines is
// flagged, in scipy's order i = -r .. -1.  A term left out is (+0 + +0) w = +0 and x + (+0) == x for x >= +0.  The flags
// of the 2 r <= 152 partners of an output are gathered with four ballots into two pairs of 64-bit masks (bit d - 1 of
// word 0: distance d <= 64; bit d - 65 of word 1: d >= 65) that live in scalar registers; the loop walks their set bits
// from the farthest partner inwards, wave-uniformly.
struct PairMasks {
  unsigned long long lo[2], hi[2];   // line l - d / l + d is flagged
};

__device__ __forceinline__ PairMasks pair_masks(const unsigned* flags, int centre, int r, int lane) {
  PairMasks m;
#pragma unroll
  for (int word = 0; word < 2; ++word) {
    const int d = lane + 1 + 64 * word;
    m.lo[word] = __ballot(d <= r && flags[centre - d] != 0u);
    m.hi[word] = __ballot(d <= r && flags[centre + d] != 0u);
  }
  return m;
}

// ---- 2. pass 1, along the first axis, radius <= kLdsRadius: the strip and its reflected halo staged in LDS, lane = column
__global__ __launch_bounds__(kThreads) void gtmaps_full_pass1_lds_kernel(const FullParams p, int tiles_x, int tiles_y) {
  __shared__ float sA[(kP1Rows + 2 * kLdsRadius) * kP1Cols];
  __shared__ unsigned sRow[kP1Rows + 2 * kLdsRadius];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int kWaves = kThreads / 64;
  const int tiles = tiles_x * tiles_y;
  const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
  const int x0 = (t % tiles_x) * kP1Cols, y0 = (t / tiles_x) * kP1Rows;
  const int D1 = p.d1, D2 = p.d2, r = p.radius, x = x0 + lane;
  const long long fo = (long long)n * D1 * D2;
  const int y_end = min(kP1Rows, D2 - y0);
  if (p.bad[n] != 0u) {   // uniform over the block: the frame is refused (gazemaps are filled by the last launch)
    if (p.fix && x < D1)
      for (int ry = wave; ry < y_end; ry += kWaves) p.fix[fo + (y0 + ry) * D1 + x] = quiet_nanf();
    return;
  }
  const bool flagged = x < D1 && column_has_sample(p.col_bits + (long long)n * p.col_words, x);
  if (!__syncthreads_or(flagged)) {   // no sample in the strip: fixationmaps and the plane are +0, no mask is read
    if (x < D1)
      for (int ry = wave; ry < y_end; ry += kWaves) {
        const long long o = fo + (y0 + ry) * D1 + x;
        if (p.fix) p.fix[o] = 0.0f;
        if (p.gaze) p.plane[o] = 0.0f;
      }
    return;
  }
  const unsigned* mask = p.mask + fo;
  const float n_obs = (float)p.n_obs;
  if (p.fix && x < D1)
    for (int ry = wave; ry < y_end; ry += kWaves)
      p.fix[fo + (y0 + ry) * D1 + x] = flagged ? (float)__popc(mask[(y0 + ry) * D1 + x]) : 0.0f;
  if (!p.gaze) return;
  const int staged = kP1Rows + 2 * r;
  for (int s = wave; s < staged; s += kWaves) {   // a column without a sample is +0 and is not read
    const float v = flagged ? (float)__popc(mask[reflect(y0 - r + s, D2) * D1 + x]) / n_obs : 0.0f;
    sA[s * kP1Cols + lane] = v;
    const unsigned long long any = __ballot(v != 0.0f);
    if (lane == 0) sRow[s] = any != 0ull;
  }
  __syncthreads();
  const double* __restrict__ w = p.weights;
  for (int ry = wave; ry < y_end; ry += kWaves) {
    const int c = ry + r;
    const PairMasks m = pair_masks(sRow, c, r, lane);
    const float* s = sA + c * kP1Cols + lane;
    double tmp = (double)s[0] * w[r];
#pragma unroll
    for (int word = 1; word >= 0; --word) {
      unsigned long long pair = m.lo[word] | m.hi[word];
      while (pair != 0ull) {
        const int bit = 63 - __clzll((long long)pair);
        pair &= ~(1ull << bit);
        const int d = bit + 1 + 64 * word;
        tmp += ((double)s[-d * kP1Cols] + (double)s[d * kP1Cols]) * w[r - d];
      }
    }
    if (x < D1) p.plane[fo + (y0 + ry) * D1 + x] = (float)tmp;
  }
}

// ---- 3. pass 2, along the second axis, and the frame's min and max; radius <= kLdsRadius.  lane = row while the sums
// are formed (the lanes of a wave share the output's column), lane = column when the tile is written.
__global__ __launch_bounds__(kThreads) void gtmaps_full_pass2_lds_kernel(const FullParams p, int tiles_x, int tiles_y) {
  constexpr int kPitchMax = (kP2Cols + 2 * kLdsRadius) | 1, kOutPitch = kP2Cols + 1;   // odd pitches: a column of 64 rows hits 64 banks
  __shared__ float sB[kP2Rows * kPitchMax];
  __shared__ float sOut[kP2Rows * kOutPitch];
  __shared__ unsigned sCol[kP2Cols + 2 * kLdsRadius];
  __shared__ float sMinMax[2 * (kThreads / 64)];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int kWaves = kThreads / 64;
  const int tiles = tiles_x * tiles_y;
  const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
  const int x0 = (t % tiles_x) * kP2Cols, y0 = (t / tiles_x) * kP2Rows;
  const int D1 = p.d1, D2 = p.d2, r = p.radius;
  const long long fo = (long long)n * D1 * D2;
  const int y_end = min(kP2Rows, D2 - y0), x_end = min(kP2Cols, D1 - x0);
  if (p.bad[n] != 0u) return;   // uniform over the block
  const int staged = kP2Cols + 2 * r, pitch = staged | 1;
  const unsigned* cols = p.col_bits + (long long)n * p.col_words;
  bool any = false;
  for (int c = tid; c < staged; c += kThreads) {
    const bool f = column_has_sample(cols, reflect(x0 - r + c, D1));
    sCol[c] = f;
    any |= f;
  }
  if (!__syncthreads_or(any)) {   // every staged column is +0: so is the tile, and its min and max
    if (lane < x_end)
      for (int ry = wave; ry < y_end; ry += kWaves) p.gaze[fo + (y0 + ry) * D1 + x0 + lane] = 0.0f;
    if (tid == 0) atomicMax(&p.negmin_bits[n], ~0u);
    return;
  }
  const float* plane = p.plane + fo;
  for (int c = wave; c < staged; c += kWaves)   // only the columns with a sample are read: the others are +0 and never looked at
    if (sCol[c] != 0u) sB[lane * pitch + c] = lane < y_end ? plane[(y0 + lane) * D1 + reflect(x0 - r + c, D1)] : 0.0f;
  __syncthreads();
  const double* __restrict__ w = p.weights;
  for (int j = wave; j < x_end; j += kWaves) {
    const int c = j + r;
    const PairMasks m = pair_masks(sCol, c, r, lane);
    const float* s = sB + lane * pitch + c;
    double tmp = sCol[c] != 0u ? (double)s[0] * w[r] : 0.0;
#pragma unroll
    for (int word = 1; word >= 0; --word) {
      unsigned long long pair = m.lo[word] | m.hi[word];
      while (pair != 0ull) {
        const int bit = 63 - __clzll((long long)pair);
        const unsigned long long one = 1ull << bit;
        pair &= ~one;
        const int d = bit + 1 + 64 * word;
        const float lo = (m.lo[word] & one) ? s[-d] : 0.0f, hi = (m.hi[word] & one) ? s[d] : 0.0f;
        tmp += ((double)lo + (double)hi) * w[r - d];
      }
    }
    sOut[lane * kOutPitch + j] = (float)tmp;
  }
  __syncthreads();
  float mn = pos_inf(), mx = 0.0f;
  if (lane < x_end)
    for (int ry = wave; ry < y_end; ry += kWaves) {
      const float g = sOut[ry * kOutPitch + lane];
      p.gaze[fo + (y0 + ry) * D1 + x0 + lane] = g;
      mn = fminf(mn, g);
      mx = fmaxf(mx, g);
    }
  block_minmax<kThreads / 64>(mn, mx, sMinMax);
  if (tid == 0) {   // every tile holds at least one cell, so mn is finite here
    atomicMax(&p.max_bits[n], __float_as_uint(mx));
    atomicMax(&p.negmin_bits[n], ~__float_as_uint(mn));
  }
}

// ---- 2'. pass 1 at a radius above kLdsRadius: the taps are read through the caches; a column without a sample is +0
__global__ __launch_bounds__(kThreads) void gtmaps_full_pass1_direct_kernel(const FullParams p, int tiles_x, int tiles_y) {
  const int tid = threadIdx.x, tx = tid & (kP1Cols - 1), tg = tid / kP1Cols;
  constexpr int kRowStep = kThreads / kP1Cols;
  const int tiles = tiles_x * tiles_y;
  const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
  const int x0 = (t % tiles_x) * kP1Cols, y0 = (t / tiles_x) * kP1Rows;
  const int D1 = p.d1, D2 = p.d2, r = p.radius, x = x0 + tx;
  const long long fo = (long long)n * D1 * D2;
  const int y_end = min(kP1Rows, D2 - y0);
  if (x >= D1) return;
  if (p.bad[n] != 0u) {
    if (p.fix)
      for (int ry = tg; ry < y_end; ry += kRowStep) p.fix[fo + (y0 + ry) * D1 + x] = quiet_nanf();
    return;
  }
  const bool flagged = column_has_sample(p.col_bits + (long long)n * p.col_words, x);
  const unsigned* mask = p.mask + fo;
  const float n_obs = (float)p.n_obs;
  const double* __restrict__ w = p.weights;
  for (int ry = tg; ry < y_end; ry += kRowStep) {
    const int y = y0 + ry;
    float out = 0.0f, cnt = 0.0f;
    if (flagged) {
      cnt = (float)__popc(mask[y * D1 + x]);
      if (p.gaze) {
        double tmp = (double)(cnt / n_obs) * w[r];
        for (int i = -r; i < 0; ++i) {
          const float lo = (float)__popc(mask[reflect(y + i, D2) * D1 + x]) / n_obs;
          const float hi = (float)__popc(mask[reflect(y - i, D2) * D1 + x]) / n_obs;
          tmp += ((double)lo + (double)hi) * w[i + r];
        }
        out = (float)tmp;
      }
    }
    if (p.fix) p.fix[fo + y * D1 + x] = cnt;
    if (p.gaze) p.plane[fo + y * D1 + x] = out;
  }
}

// ---- 3'. pass 2 at a radius above kLdsRadius; a tile none of whose taps' columns has a sample is +0
__global__ __launch_bounds__(kThreads) void gtmaps_full_pass2_direct_kernel(const FullParams p, int tiles_x, int tiles_y) {
  __shared__ float sMinMax[2 * (kThreads / 64)];
  const int tid = threadIdx.x, tx = tid & (kDirCols - 1), tg = tid / kDirCols;
  constexpr int kRowStep = kThreads / kDirCols;
  const int tiles = tiles_x * tiles_y;
  const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
  const int x0 = (t % tiles_x) * kDirCols, y0 = (t / tiles_x) * kDirRows;
  const int D1 = p.d1, D2 = p.d2, r = p.radius, x = x0 + tx;
  const long long fo = (long long)n * D1 * D2;
  const int y_end = min(kDirRows, D2 - y0);
  if (p.bad[n] != 0u) return;   // uniform over the block
  const int staged = kDirCols + 2 * r;
  const unsigned* cols = p.col_bits + (long long)n * p.col_words;
  bool any = false;
  for (int c = tid; c < staged; c += kThreads) any |= column_has_sample(cols, reflect(x0 - r + c, D1));
  if (!__syncthreads_or(any)) {
    if (x < D1)
      for (int ry = tg; ry < y_end; ry += kRowStep) p.gaze[fo + (y0 + ry) * D1 + x] = 0.0f;
    if (tid == 0) atomicMax(&p.negmin_bits[n], ~0u);
    return;
  }
  const float* plane = p.plane + fo;
  const double* __restrict__ w = p.weights;
  float mn = pos_inf(), mx = 0.0f;
  if (x < D1)
    for (int ry = tg; ry < y_end; ry += kRowStep) {
      const float* line = plane + (y0 + ry) * D1;
      double tmp = (double)line[x] * w[r];
      for (int i = -r; i < 0; ++i) tmp += ((double)line[reflect(x + i, D1)] + (double)line[reflect(x - i, D1)]) * w[i + r];
      const float g = (float)tmp;
      p.gaze[fo + (y0 + ry) * D1 + x] = g;
      mn = fminf(mn, g);
      mx = fmaxf(mx, g);
    }
  block_minmax<kThreads / 64>(mn, mx, sMinMax);
  if (tid == 0) {
    atomicMax(&p.max_bits[n], __float_as_uint(mx));
    atomicMax(&p.negmin_bits[n], ~__float_as_uint(mn));
  }
}

// ---- 4. g -= min(g); g /= max(g) unless the frame is all zero (the filtered values are sums of products of
// non-negative numbers: their sum is 0 exactly when the largest of them is); NaN for a refused frame
__global__ __launch_bounds__(kThreads) void gtmaps_full_normalise_kernel(const FullParams p, int blocks_per_frame) {
  const int n = blockIdx.x / blocks_per_frame, blk = blockIdx.x - n * blocks_per_frame;
  const int n_pix = p.d1 * p.d2;
  float* g = p.gaze + (long long)n * n_pix;
  const int c0 = blk * (kThreads * kNormPerThread) + threadIdx.x;
  if (p.bad[n] != 0u) {
#pragma unroll
    for (int k = 0; k < kNormPerThread; ++k) {
      const int c = c0 + k * kThreads;
      if (c < n_pix) g[c] = quiet_nanf();
    }
    return;
  }
  const float mx = __uint_as_float(p.max_bits[n]), mn = __uint_as_float(~p.negmin_bits[n]);
  if (!(mx > 0.0f)) return;
  const float den = mx - mn;
#pragma unroll
  for (int k = 0; k < kNormPerThread; ++k) {
    const int c = c0 + k * kThreads;
    if (c < n_pix) {
      float v = g[c];
      v = v - mn;
      v = v / den;
      g[c] = v;
    }
  }
}

bool shape_ok(int n_frames, int d1, int d2) {
  return n_frames >= 0 && d1 >= 2 && d2 >= 2 && (long long)d1 * d2 <= RGP_GTMAPS_FULL_MAX_PIX;
}

// bytes of the head: status word, the three per-frame words, the column bitmaps; the mask planes follow it
size_t head_bytes(int n_frames, int d1) {
  const size_t col_words = ((size_t)d1 + 31) / 32;
  return align_up((size_t)kStatusBytes + (size_t)n_frames * 4 * (3 + col_words), 256);
}

}  // namespace

extern "C" {

size_t rgp_gtmaps_full_workspace_bytes(int n_frames, int d1, int d2) {
  if (!shape_ok(n_frames, d1, d2)) return 0;
  // n_frames < 2^31, d1 * d2 <= 2^22, d1 <= 2^21: below 2^57 in all
  return head_bytes(n_frames, d1) + (size_t)n_frames * (size_t)d1 * (size_t)d2 * 8;
}

int rgp_gazemaps_full_from_fixations(const rgp_gtmaps_full_args* a, rgp_stream_t stream) {
  RGP_REQUIRE(a != nullptr, "rgp_gazemaps_full_from_fixations: args is NULL");
  RGP_REQUIRE(a->n_frames >= 0, "rgp_gazemaps_full_from_fixations: n_frames = %d must not be negative", a->n_frames);
  if (a->n_frames == 0) return RGP_OK;
  RGP_REQUIRE(a->frame_ptr != nullptr, "rgp_gazemaps_full_from_fixations: frame_ptr is NULL");
  RGP_REQUIRE(a->samples != nullptr, "rgp_gazemaps_full_from_fixations: samples is NULL");
  RGP_REQUIRE(a->weights != nullptr, "rgp_gazemaps_full_from_fixations: weights is NULL");
  RGP_REQUIRE(a->gazemaps || a->fixationmaps,
              "rgp_gazemaps_full_from_fixations: gazemaps and fixationmaps are both NULL: nothing to compute");
  RGP_REQUIRE(a->n_observers >= 1 && a->n_observers <= RGP_GTMAPS_MAX_OBSERVERS,
              "rgp_gazemaps_full_from_fixations: n_observers = %d must be in [1, RGP_GTMAPS_MAX_OBSERVERS = %d]", a->n_observers,
              RGP_GTMAPS_MAX_OBSERVERS);
  RGP_REQUIRE(a->raw_d1 >= 2 && a->raw_d2 >= 2, "rgp_gazemaps_full_from_fixations: raw_d1 = %d and raw_d2 = %d must be at least 2",
              a->raw_d1, a->raw_d2);
  RGP_REQUIRE((long long)a->raw_d1 * a->raw_d2 <= RGP_GTMAPS_FULL_MAX_PIX,
              "rgp_gazemaps_full_from_fixations: frames of raw_d2 = %d x raw_d1 = %d: more than RGP_GTMAPS_FULL_MAX_PIX = %d cells",
              a->raw_d2, a->raw_d1, RGP_GTMAPS_FULL_MAX_PIX);
  RGP_REQUIRE(a->radius >= 0 && a->radius <= RGP_GTMAPS_FULL_MAX_RADIUS,
              "rgp_gazemaps_full_from_fixations: radius = %d must be in [0, RGP_GTMAPS_FULL_MAX_RADIUS = %d]", a->radius,
              RGP_GTMAPS_FULL_MAX_RADIUS);
  const int N = a->n_frames, D1 = a->raw_d1, D2 = a->raw_d2;
  const size_t need = rgp_gtmaps_full_workspace_bytes(N, D1, D2);
  RGP_TRY(require_workspace("rgp_gazemaps_full_from_fixations", a->workspace, a->workspace_bytes, need));
  const bool lds = a->radius <= kLdsRadius;
  const int p2c = lds ? kP2Cols : kDirCols, p2r = lds ? kP2Rows : kDirRows;
  const int t1x = (D1 + kP1Cols - 1) / kP1Cols, t1y = (D2 + kP1Rows - 1) / kP1Rows;
  const int t2x = (D1 + p2c - 1) / p2c, t2y = (D2 + p2r - 1) / p2r;
  const int norm_blocks = (D1 * D2 + kThreads * kNormPerThread - 1) / (kThreads * kNormPerThread);
  const long long most = std::max({(long long)t1x * t1y, (long long)t2x * t2y, (long long)norm_blocks});
  RGP_REQUIRE((long long)N * most <= INT_MAX,
              "rgp_gazemaps_full_from_fixations: n_frames = %d frames of %d x %d need more than 2^31 - 1 workgroups per launch: "
              "split the call", N, D2, D1);

  const size_t n_pix = (size_t)D1 * D2, head = head_bytes(N, D1);
  char* ws = (char*)a->workspace;
  FullParams p{};
  p.frame_ptr = a->frame_ptr; p.samples = a->samples; p.weights = a->weights;
  p.n_frames = N; p.n_obs = a->n_observers; p.d1 = D1; p.d2 = D2; p.radius = a->radius; p.col_words = (D1 + 31) / 32;
  p.gaze = a->gazemaps; p.fix = a->fixationmaps;
  p.status = (int*)ws;
  p.bad = (unsigned*)(ws + kStatusBytes);
  p.max_bits = p.bad + N;
  p.negmin_bits = p.max_bits + N;
  p.col_bits = p.negmin_bits + N;
  p.mask = (unsigned*)(ws + head);
  p.plane = (float*)(ws + head + (size_t)N * n_pix * 4);
  hipStream_t s = (hipStream_t)stream;
  // the head and the masks start from zero: status 0, no frame bad, max = +0, complemented min = 0 (= the largest value)
  RGP_HIP(hipMemsetAsync(ws, 0, head + (size_t)N * n_pix * 4, s));
  hipLaunchKernelGGL(gtmaps_full_scatter_kernel, dim3(N), dim3(kThreads), 0, s, p);
  RGP_HIP(hipGetLastError());
  hipLaunchKernelGGL(lds ? gtmaps_full_pass1_lds_kernel : gtmaps_full_pass1_direct_kernel, dim3(N * t1x * t1y), dim3(kThreads), 0, s, p,
                     t1x, t1y);
  RGP_HIP(hipGetLastError());
  if (!a->gazemaps) return RGP_OK;
  hipLaunchKernelGGL(lds ? gtmaps_full_pass2_lds_kernel : gtmaps_full_pass2_direct_kernel, dim3(N * t2x * t2y), dim3(kThreads), 0, s, p,
                     t2x, t2y);
  RGP_HIP(hipGetLastError());
  hipLaunchKernelGGL(gtmaps_full_normalise_kernel, dim3(N * norm_blocks), dim3(kThreads), 0, s, p, norm_blocks);
  RGP_HIP(hipGetLastError());
  return RGP_OK;
}

int rgp_gtmaps_full_status(const void* workspace, int* refused_out, rgp_stream_t stream) {
  int refused;
  RGP_TRY(read_status("rgp_gtmaps_full_status", workspace, refused_out, stream, &refused));
  RGP_REQUIRE(refused == 0,
              "rgp_gazemaps_full_from_fixations: %d frame(s) refused (a sample's observer, a or b out of range, or a bad "
              "frame_ptr pair): their outputs are NaN", refused);
  return RGP_OK;
}

}  // extern "C"
