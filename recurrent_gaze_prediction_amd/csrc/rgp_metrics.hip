// librgp_hip.so: the saliency metrics of evaluation_metrics.py on the device (include/rgp.h, "saliency metrics").
//
// One launch, one 256-thread workgroup per frame, every requested metric of the frame.  The work per frame is tiny
// (49x49 = 2401 pixels, a handful of fixations, 100 repetitions x <= 10 thresholds): the kernel is bound by launch
// latency and LDS, not by arithmetic, and what it removes is a device->host copy and seconds of interpreter time.
//
// Layout.  Thread t owns the `chunk` = ceil(n_pix / 256) consecutive pixels [t*chunk, (t+1)*chunk) and keeps their
// normalised prediction, ground truth and jittered AUC_Judd saliency in registers (<= 16 each).  LDS holds what is
// gathered at random: the normalised map (<= 32 KiB as fp64) for the negatives of AUC_Borji / AUC_shuffled, the
// saliency at the fixations (2 x 2 KiB), AUC_Judd's sorted thresholds and counters (3 KiB) and, for device draws, the
// compacted negative set (8 KiB as uint16): 47 KiB, three workgroups per CU.
//
// Exactness.  This file is compiled with -ffp-contract=off and without fast-math; divisions are IEEE.  The two
// normalisations and the jitter are element-wise, so the device holds bit for bit the saliency values numpy holds,
// every comparison of the ROC sweeps falls the same way (np_less is numpy's sort order, NaN last), the counts
// are integers, and what is left is the order of the sums (<= 4096 terms of magnitude <= 1: about 4096 * 2^-53).
// The arithmetic itself -- numpy's rules, the metric chains, the draws -- is in metrics_shared.hip.h, shared with
// rgp_metrics_scaled.hip; this file holds the ownership of pixels, the compaction and the register-resident passes.
#include <cmath>

#include "metrics_shared.hip.h"

using namespace rgp;

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kMaxPix = RGP_METRICS_MAX_PIX;
constexpr int kMaxFix = RGP_METRICS_MAX_FIX;
constexpr int kChunk = kMaxPix / kThreads;   // pixels a thread owns at most

struct MetricsParams : MetricsCommon {
  const float *fix, *other;
  long long other_stride;
  int n_pix;
};

// exclusive prefix sum of v over the block in thread order; total = the block's sum
__device__ __forceinline__ int block_excl_scan(int v, int* sh, int& total) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o);
    if (lane >= o) inc += t;
  }
  __syncthreads();
  if (lane == 63) sh[wave] = inc;
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wave; ++w) base += sh[w];
  total = sh[0] + sh[1] + sh[2] + sh[3];
  return base + inc - v;
}

__global__ __launch_bounds__(kThreads, 2) void saliency_scores_kernel(const MetricsParams p) {
  __shared__ double sP[kMaxPix];
  __shared__ double sFixP[kMaxFix], sFixJ[kMaxFix], sThr[kMaxFix];
  __shared__ int sCnt[kMaxFix];
  __shared__ unsigned short sOther[kMaxPix];
  __shared__ double sRed[kWaves * 8];
  __shared__ int sScan[kWaves];
  __shared__ int sBad;
  __shared__ double sFixMax;

  const int tid = threadIdx.x, lane = tid & 63;
  const int n = blockIdx.x, n_pix = p.n_pix;
  const int chunk = (n_pix + kThreads - 1) / kThreads, base = tid * chunk;
  const long long fo = (long long)n * n_pix;
  const unsigned long long frame = p.offset + (unsigned long long)n;
  const bool device_draws = (p.flags & RGP_METRICS_DEVICE_DRAWS) != 0;
  const unsigned M = p.metrics;
  const double nan = quiet_nan();
  double score[RGP_METRICS_COUNT] = {nan, nan, nan, nan, nan, nan};
  if (tid == 0) sBad = 0;

  // ---- pred -> normalize_range (saliency_score_single), in the arithmetic numpy uses for the array's dtype
  double pv[kChunk];
  bool own[kChunk];
  {
    double mn = INFINITY, mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < kChunk; ++j) {
      own[j] = j < chunk && base + j < n_pix;
      pv[j] = 0.0;
      if (own[j]) {
        pv[j] = (p.flags & RGP_METRICS_PRED_F64) ? ((const double*)p.pred)[fo + base + j]
                                                 : (double)((const float*)p.pred)[fo + base + j];
        mn = np_min(mn, pv[j]);
        mx = np_max(mx, pv[j]);
      }
    }
    block_minmax<kWaves>(mn, mx, sRed);
    if (p.flags & RGP_METRICS_PRED_F64) {
      const double den = mx - mn;
#pragma unroll
      for (int j = 0; j < kChunk; ++j) pv[j] = (pv[j] - mn) / den;
    } else {
      const float mnf = (float)mn, den = (float)mx - (float)mn;
#pragma unroll
      for (int j = 0; j < kChunk; ++j) pv[j] = (double)(((float)pv[j] - mnf) / den);
    }
#pragma unroll
    for (int j = 0; j < kChunk; ++j)
      if (own[j]) sP[base + j] = pv[j];
  }

  // ---- fixations (and, for device draws, the negative set) compacted in pixel order
  unsigned fmask = 0, omask = 0;
  const bool want_other = device_draws && (M & RGP_METRIC_AUC_SHUFFLED);
#pragma unroll
  for (int j = 0; j < kChunk; ++j)
    if (own[j]) {
      if (p.fix[fo + base + j] > 0.5f) fmask |= 1u << j;
      if (want_other && p.other[(long long)n * p.other_stride + base + j] > 0.5f) omask |= 1u << j;
    }
  int n_fix, n_other = 0;
  const int foff = block_excl_scan(__popc(fmask), sScan, n_fix);
  if (want_other) {
    int o = block_excl_scan(__popc(omask), sScan, n_other);
#pragma unroll
    for (int j = 0; j < kChunk; ++j)
      if (omask >> j & 1) sOther[o++] = (unsigned short)(base + j);
  }
  if (n_fix > p.neg_stride) {   // over the cap: no finite score, the call reports it (uniform over the block)
    if (tid == 0) refuse_frame(p, n);
    return;
  }
  {
    int o = foff;
#pragma unroll
    for (int j = 0; j < kChunk; ++j)
      if (fmask >> j & 1) sFixP[o++] = pv[j];
  }
  if (want_other && tid == 0 && n_fix == 0) p.ws_cnt[n] = 0;
  __syncthreads();

  // ---- sim (:207-218), cc (:221-236), NSS: block sums
  if (M & (RGP_METRIC_SIM | RGP_METRIC_CC | RGP_METRIC_NSS)) {
    double g[kChunk];
    const bool want_gt = (M & (RGP_METRIC_SIM | RGP_METRIC_CC)) != 0;
#pragma unroll
    for (int j = 0; j < kChunk; ++j) {
      g[j] = 0.0;
      if (own[j] && want_gt)
        g[j] = (p.flags & RGP_METRICS_GT_F64) ? ((const double*)p.gt)[fo + base + j] : (double)((const float*)p.gt)[fo + base + j];
    }
    const double dn = (double)n_pix;
    double s1[2] = {0.0, 0.0};
#pragma unroll
    for (int j = 0; j < kChunk; ++j)
      if (own[j]) { s1[0] += g[j]; s1[1] += pv[j]; }
    block_sum<kWaves>(s1, sRed);
    auto sweep = [&](auto&& f) {   // the thread's pixels out of its registers, which end as the standardised maps
#pragma unroll
      for (int j = 0; j < kChunk; ++j) {
        if (!own[j]) break;   // owned pixels are a prefix: one nest of branches (151 VGPRs), not 16 separate ones (203, a wave less)
        f(g[j], pv[j]);
      }
    };
    const ChainResult c = sim_cc_chain<kWaves, true>(sweep, s1[0], s1[1], dn, (M & RGP_METRIC_CC) != 0, sRed);
    score[RGP_METRIC_ROW_SIM] = c.sim;
    score[RGP_METRIC_ROW_CC] = c.cc;
    if ((M & RGP_METRIC_NSS) && n_fix > 0 && tid == 0) score[RGP_METRIC_ROW_NSS] = nss_score(sFixP, n_fix, c, dn);
  }

  // ---- AUC_Judd (:42-98)
  if ((M & RGP_METRIC_AUC_JUDD) && n_fix > 0) {
    const bool jitter = device_draws ? !(p.flags & RGP_METRICS_NO_JITTER) : p.judd_jitter != nullptr;
    double sj[kChunk];
    double mn = INFINITY, mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < kChunk; ++j) {
      sj[j] = 0.0;
      if (own[j]) {
        sj[j] = sP[base + j];   // the normalised prediction out of LDS: the cc passes left the standardised map in pv
        if (jitter) {
          const double u = device_draws ? judd_jitter_u((unsigned)(base + j), frame, p.seed) : p.judd_jitter[fo + base + j];
          sj[j] = sj[j] + u * 1e-7;
        }
        mn = np_min(mn, sj[j]);
        mx = np_max(mx, sj[j]);
      }
    }
    block_minmax<kWaves>(mn, mx, sRed);
    const double den = mx - mn;
    int o = foff;
#pragma unroll
    for (int j = 0; j < kChunk; ++j) {
      sj[j] = (sj[j] - mn) / den;
      if (fmask >> j & 1) sFixJ[o++] = sj[j];
    }
    if (tid < n_fix) sCnt[tid] = 0;
    __syncthreads();
    judd_rank_thresholds(sFixJ, sThr, n_fix);
    __syncthreads();
    for (int k = 0; k < n_fix; ++k) {   // #(S < thr_k), every pixel against every threshold out of the registers
      const double thr = sThr[k];
      int c = 0;
#pragma unroll
      for (int j = 0; j < kChunk; ++j) c += (own[j] && np_less(sj[j], thr)) ? 1 : 0;
#pragma unroll
      for (int o2 = 32; o2 > 0; o2 >>= 1) c += __shfl_xor(c, o2);
      if (lane == 0) atomicAdd(&sCnt[k], c);
    }
    __syncthreads();
    if (tid == 0) score[RGP_METRIC_ROW_AUC_JUDD] = judd_trapezoid(sCnt, n_fix, n_pix);
  }

  // ---- AUC_Borji (:101-164) and AUC_shuffled (:167-204): the same sweep over two kinds of negatives
  if ((M & (RGP_METRIC_AUC_BORJI | RGP_METRIC_AUC_SHUFFLED)) && n_fix > 0) {
    if (tid == 0) sFixMax = np_max_of(sFixP, n_fix);
    __syncthreads();
    const double fix_max = sFixMax;
    double auc[2] = {0.0, 0.0};
    for (int item = tid; item < 2 * p.n_rep; item += kThreads) {
      const int which = item >= p.n_rep ? 1 : 0, rep = item - which * p.n_rep;
      if (!(M & (which ? RGP_METRIC_AUC_SHUFFLED : RGP_METRIC_AUC_BORJI))) continue;
      const long long row_off = ((long long)n * p.n_rep + rep) * p.neg_stride;
      const int* row;
      int cnt;
      if (device_draws) {
        int* wrow = (which ? p.ws_shuf : p.ws_borji) + row_off;
        if (!which) {
          cnt = n_fix;
          draw_borji_row(wrow, cnt, n_pix, rep, frame, p.seed);
        } else {
          cnt = n_fix < n_other ? n_fix : n_other;
          if (rep == 0) p.ws_cnt[n] = cnt;
          draw_floyd_row(wrow, cnt, n_other, rep, frame, p.seed, [&](int i) { return (int)sOther[i]; });
        }
        row = wrow;
      } else {
        row = (which ? p.shuf_neg : p.borji_neg) + row_off;
        cnt = which ? p.shuf_cnt[n] : n_fix;
        if (cnt < 0 || cnt > p.neg_stride) { atomicOr(&sBad, 1); cnt = 0; }
      }
      // the caller's indices are checked where they are used: a bad one reads pixel 0 and refuses the frame.  The flag
      // is a register and the atomic follows the sweep, so that the loads of the threshold loop have no store between them
      bool bad_idx = false;
      auc[which] += roc_auc(sFixP, n_fix, fix_max, cnt, p.step_size, [&](int s) {
        const int idx = row[s];
        const bool ok = idx >= 0 && idx < n_pix;
        bad_idx = bad_idx || !ok;
        return sP[ok ? idx : 0];
      });
      if (bad_idx) atomicOr(&sBad, 1);
    }
    block_sum<kWaves>(auc, sRed);
    score[RGP_METRIC_ROW_AUC_BORJI] = auc[0] / (double)p.n_rep;
    score[RGP_METRIC_ROW_AUC_SHUFFLED] = auc[1] / (double)p.n_rep;
  }

  __syncthreads();
  if (tid == 0) write_scores(p, n, sBad != 0, score);
}

}  // namespace

extern "C" {

size_t rgp_metrics_workspace_bytes(int n_frames, int n_rep, int neg_stride, unsigned flags) {
  if (n_frames <= 0 || n_rep <= 0 || neg_stride <= 0) return 0;
  return align_up(draws_layout_bytes(n_frames, n_rep, neg_stride, flags), 64);
}

int rgp_saliency_scores(const rgp_metrics_args* a, rgp_stream_t stream) {
  const char* fn = "rgp_saliency_scores";
  RGP_REQUIRE(a != nullptr, "%s: args is NULL", fn);
  RGP_REQUIRE(a->n_frames > 0, "%s: n_frames = %d must be positive", fn, a->n_frames);
  RGP_REQUIRE(a->height > 0 && a->width > 0 && (long long)a->height * a->width <= RGP_METRICS_MAX_PIX,
              "%s: maps of %d x %d: height*width must be in [1, RGP_METRICS_MAX_PIX = %d]", fn, a->height, a->width, RGP_METRICS_MAX_PIX);
  const int n_pix = a->height * a->width;
  RGP_TRY(check_common_args(fn, a, RGP_METRICS_DEVICE_DRAWS | RGP_METRICS_NO_JITTER | RGP_METRICS_PRED_F64 | RGP_METRICS_GT_F64));
  RGP_REQUIRE(a->pred && a->fix && a->scores, "%s: pred, fix and scores must not be NULL", fn);
  if ((a->flags & RGP_METRICS_DEVICE_DRAWS) && (a->metrics & RGP_METRIC_AUC_SHUFFLED)) {
    RGP_REQUIRE(a->other != nullptr, "%s: AUC_shuffled with device draws needs the negative map `other`", fn);
    RGP_REQUIRE(a->other_stride == 0 || a->other_stride == n_pix, "%s: other_stride = %lld must be 0 or height*width", fn, a->other_stride);
  }
  RGP_TRY(check_workspace(fn, a->workspace, a->workspace_bytes,
                          rgp_metrics_workspace_bytes(a->n_frames, a->n_rep, a->neg_stride, a->flags)));

  MetricsParams p{};
  fill_common(p, a);
  p.fix = a->fix; p.other = a->other; p.other_stride = a->other_stride; p.n_pix = n_pix;
  hipStream_t s = (hipStream_t)stream;
  RGP_HIP(hipMemsetAsync(a->workspace, 0, kStatusBytes, s));
  hipLaunchKernelGGL(saliency_scores_kernel, dim3(a->n_frames), dim3(kThreads), 0, s, p);
  RGP_HIP(hipGetLastError());
  return RGP_OK;
}

int rgp_metrics_status(const void* workspace, rgp_stream_t stream) {
  RGP_REQUIRE(workspace != nullptr, "rgp_metrics_status: workspace is NULL");
  hipStream_t s = (hipStream_t)stream;
  int refused = 0;
  RGP_HIP(hipMemcpyAsync(&refused, workspace, sizeof(int), hipMemcpyDeviceToHost, s));
  RGP_HIP(hipStreamSynchronize(s));
  RGP_REQUIRE(refused == 0,
              "rgp_saliency_scores: %d frame(s) refused (more fixations than neg_stride <= RGP_METRICS_MAX_FIX = %d, or supplied "
              "indices / counts out of range): their scores are NaN", refused, RGP_METRICS_MAX_FIX);
  return RGP_OK;
}

}  // extern "C"
