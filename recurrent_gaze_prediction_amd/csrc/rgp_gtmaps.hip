// librgp_hip.so: ground-truth gaze maps from fixation points on the device (include/rgp.h, "ground-truth maps from
// fixation points"): the rescale of raw gaze points to the map grid, the per-observer de-duplication and the sum over
// observers, scipy's Gaussian filter and the min-max normalisation of the reference's loader
// (process_gazemap.py:35-58, crc_input_data_seq.py:41-53, 261-288).
//
// One launch, one 256-thread workgroup per output frame.  The work per frame is tiny (49x49 = 2401 cells, a few
// samples, 2 x 17 taps per cell): the kernel is bound by launch latency and LDS, not by arithmetic; it is not an MFMA
// kernel.  What it buys is that the maps are born where their consumers (the loss, rgp_saliency_scores, the action
// classifier) read them.
//
// Layout.  All working arrays live in LDS: one uint32 observer mask per cell (16 KiB: bit u = observer u hit the
// cell; atomicOr de-duplicates an observer, popc counts observers; integer LDS atomics are order-free, so the result
// does not depend on the order the samples arrive in), two fp32 planes the filter passes ping-pong between
// (2 x 16 KiB), the weights (65 doubles) and the reduction scratch: 48.6 KiB, one workgroup per frame, three per CU.
//
// Exactness.  This file is compiled with -ffp-contract=off and without fast-math; divisions are IEEE.  The weights
// come from the host (the device's exp is not numpy's).  Each filter output is the sum scipy's correlate1d forms for a
// symmetric kernel, in its order, in fp64, rounded once to fp32; min and max are exact whatever the reduction order;
// everything else is element-wise.  So gazemaps and fixationmaps equal the host's bit for bit.  Only the fp64 sum
// behind `labels` has an order of its own (fixed: the same bits on every launch geometry).
#include <cmath>

#include "image_shared.hip.h"

using namespace rgp;
using namespace rgp::img;

namespace {

constexpr int kThreads = 256;
constexpr int kMaxPix = RGP_GTMAPS_MAX_PIX;
constexpr int kMaxRadius = RGP_GTMAPS_MAX_RADIUS;

struct GtmapsParams {
  const int *frame_ptr, *samples;
  const double* weights;
  int n_frames, n_obs, d1, d2, s1, s2, radius;
  float *gaze, *fix, *labels;
  int* status;
};

// one output of correlate1d with a symmetric kernel: entry l of the line src[base + k*stride], k < n
__device__ __forceinline__ float filter_tap_sum(const float* src, int base, int stride, int l, int n, const double* w, int r) {
  double tmp = (double)src[base + l * stride] * w[r];
  for (int i = -r; i < 0; ++i) {
    const double lo = (double)src[base + reflect(l + i, n) * stride], hi = (double)src[base + reflect(l - i, n) * stride];
    tmp += (lo + hi) * w[i + r];
  }
  return (float)tmp;
}

__global__ __launch_bounds__(kThreads) void gazemaps_from_fixations_kernel(const GtmapsParams p) {
  __shared__ unsigned sMask[kMaxPix];
  __shared__ float sA[kMaxPix], sB[kMaxPix];
  __shared__ double sW[2 * kMaxRadius + 1];
  __shared__ double sRed[4];
  __shared__ float sMinMax[2 * (kThreads / 64)];
  __shared__ int sBad;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = blockIdx.x, S1 = p.s1, S2 = p.s2, n_pix = S1 * S2, r = p.radius;
  const long long fo = (long long)n * n_pix;

  for (int c = tid; c < n_pix; c += kThreads) sMask[c] = 0u;
  if (tid <= 2 * r) sW[tid] = p.weights[tid];
  if (tid == 0) sBad = 0;
  __syncthreads();

  // ---- scatter: every value is checked before it addresses LDS
  const int beg = p.frame_ptr[n], end = p.frame_ptr[n + 1];
  if (frame_ptr_bad(beg, end)) {
    if (tid == 0) sBad = 1;
  } else {
    const double f1 = (double)S1 - 1.0, g1 = (double)p.d1 - 1.0, f2 = (double)S2 - 1.0, g2 = (double)p.d2 - 1.0;
    for (int i = beg + tid; i < end; i += kThreads) {
      const int* row = p.samples + (long long)i * 3;
      const int u = row[0], a = row[1], b = row[2];
      if (sample_bad(u, a, b, p.n_obs, p.d1, p.d2)) { atomicOr(&sBad, 1); continue; }
      const int a_ = (int)(rint((double)a * f1 / g1) + 1e-9);
      const int b_ = (int)(rint((double)b * f2 / g2) + 1e-9);
      if (a_ < 0 || a_ >= S1 || b_ < 0 || b_ >= S2) { atomicOr(&sBad, 1); continue; }   // cannot happen for a, b in range
      atomicOr(&sMask[b_ * S1 + a_], 1u << u);
    }
  }
  __syncthreads();
  if (sBad != 0) {   // uniform over the block: the frame is refused
    const float nan = quiet_nanf();
    for (int c = tid; c < n_pix; c += kThreads) {
      if (p.gaze) p.gaze[fo + c] = nan;
      if (p.fix) p.fix[fo + c] = nan;
      if (p.labels) p.labels[fo + c] = nan;
    }
    if (tid == 0) atomicAdd(p.status, 1);
    return;
  }

  // ---- counts and the pre-filter map
  const float n_obs = (float)p.n_obs;
  for (int c = tid; c < n_pix; c += kThreads) {
    const float cnt = (float)__popc(sMask[c]);
    if (p.fix) p.fix[fo + c] = cnt;
    sA[c] = cnt / n_obs;
  }
  if (!p.gaze && !p.labels) return;
  __syncthreads();

  // ---- gaussian_filter: along the frame's first axis (lines of S2 entries, S1 apart), then along its second
  for (int c = tid; c < n_pix; c += kThreads) {
    const int y = c / S1, x = c - y * S1;
    sB[c] = filter_tap_sum(sA, x, S1, y, S2, sW, r);
  }
  __syncthreads();
  float mn = pos_inf(), mx = neg_inf();
  for (int c = tid; c < n_pix; c += kThreads) {
    const int y = c / S1, x = c - y * S1;
    const float g = filter_tap_sum(sB, y * S1, 1, x, S1, sW, r);
    sA[c] = g;
    mn = fminf(mn, g);
    mx = fmaxf(mx, g);
  }
  block_minmax<kThreads / 64>(mn, mx, sMinMax);

  // ---- g -= min(g); g /= max(g) unless the frame sums to 0.  The filtered values are sums of products of
  // non-negative numbers, so their fp32 sum is 0 exactly when the largest of them is.
  const bool empty = !(mx > 0.0f);
  const float den = mx - mn;
  double part = 0.0;
  for (int c = tid; c < n_pix; c += kThreads) {   // each thread touches only the cells it wrote above
    float g = sA[c];
    if (!empty) {
      g = g - mn;
      g = g / den;
    }
    sA[c] = g;
    if (p.gaze) p.gaze[fo + c] = g;
    part += (double)g;
  }
  if (!p.labels) return;

  // ---- labels = g / sum(g): the sum in fp64 (thread partials in cell order, then a fixed tree), rounded once
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
  if (lane == 0) sRed[wave] = part;
  __syncthreads();
  const float total = (float)((sRed[0] + sRed[1]) + (sRed[2] + sRed[3]));
  for (int c = tid; c < n_pix; c += kThreads) p.labels[fo + c] = sA[c] / total;
}

}  // namespace

extern "C" {

size_t rgp_gtmaps_workspace_bytes(void) { return kStatusBytes; }

int rgp_gazemaps_from_fixations(const rgp_gtmaps_args* a, rgp_stream_t stream) {
  RGP_REQUIRE(a != nullptr, "rgp_gazemaps_from_fixations: args is NULL");
  RGP_REQUIRE(a->n_frames >= 0, "rgp_gazemaps_from_fixations: n_frames = %d must not be negative", a->n_frames);
  if (a->n_frames == 0) return RGP_OK;
  RGP_REQUIRE(a->frame_ptr != nullptr, "rgp_gazemaps_from_fixations: frame_ptr is NULL");
  RGP_REQUIRE(a->samples != nullptr, "rgp_gazemaps_from_fixations: samples is NULL");
  RGP_REQUIRE(a->weights != nullptr, "rgp_gazemaps_from_fixations: weights is NULL");
  RGP_REQUIRE(a->gazemaps || a->fixationmaps || a->labels,
              "rgp_gazemaps_from_fixations: gazemaps, fixationmaps and labels are all NULL: nothing to compute");
  RGP_REQUIRE(a->n_observers >= 1 && a->n_observers <= RGP_GTMAPS_MAX_OBSERVERS,
              "rgp_gazemaps_from_fixations: n_observers = %d must be in [1, RGP_GTMAPS_MAX_OBSERVERS = %d]", a->n_observers,
              RGP_GTMAPS_MAX_OBSERVERS);
  RGP_REQUIRE(a->raw_d1 >= 2 && a->raw_d2 >= 2, "rgp_gazemaps_from_fixations: raw_d1 = %d and raw_d2 = %d must be at least 2",
              a->raw_d1, a->raw_d2);
  RGP_REQUIRE(a->out_s1 >= 1 && a->out_s2 >= 1 && (long long)a->out_s1 * a->out_s2 <= RGP_GTMAPS_MAX_PIX,
              "rgp_gazemaps_from_fixations: maps of out_s2 = %d x out_s1 = %d: out_s1*out_s2 must be in [1, RGP_GTMAPS_MAX_PIX = %d]",
              a->out_s2, a->out_s1, RGP_GTMAPS_MAX_PIX);
  RGP_REQUIRE(a->radius >= 0 && a->radius <= RGP_GTMAPS_MAX_RADIUS,
              "rgp_gazemaps_from_fixations: radius = %d must be in [0, RGP_GTMAPS_MAX_RADIUS = %d]", a->radius, RGP_GTMAPS_MAX_RADIUS);
  RGP_TRY(require_workspace("rgp_gazemaps_from_fixations", a->workspace, a->workspace_bytes, kStatusBytes));

  GtmapsParams p{};
  p.frame_ptr = a->frame_ptr; p.samples = a->samples; p.weights = a->weights;
  p.n_frames = a->n_frames; p.n_obs = a->n_observers; p.d1 = a->raw_d1; p.d2 = a->raw_d2;
  p.s1 = a->out_s1; p.s2 = a->out_s2; p.radius = a->radius;
  p.gaze = a->gazemaps; p.fix = a->fixationmaps; p.labels = a->labels;
  p.status = (int*)a->workspace;
  hipStream_t s = (hipStream_t)stream;
  RGP_TRY(clear_status(a->workspace, s));
  hipLaunchKernelGGL(gazemaps_from_fixations_kernel, dim3(a->n_frames), dim3(kThreads), 0, s, p);
  RGP_HIP(hipGetLastError());
  return RGP_OK;
}

int rgp_gtmaps_status(const void* workspace, rgp_stream_t stream) {
  int refused;
  RGP_TRY(read_status("rgp_gtmaps_status", workspace, nullptr, stream, &refused));
  RGP_REQUIRE(refused == 0,
              "rgp_gazemaps_from_fixations: %d frame(s) refused (a sample's observer, a or b out of range, or a bad frame_ptr "
              "pair): their outputs are NaN", refused);
  return RGP_OK;
}

}  // extern "C"
