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
// every comparison of the ROC sweeps falls the same way (np_less below is numpy's sort order, NaN last), the counts
// are integers, and what is left is the order of the sums (<= 4096 terms of magnitude <= 1: about 4096 * 2^-53).
#include <cmath>

#include "rgp_host.h"
#include "philox.hip.h"

using namespace rgp;

namespace {

constexpr int kThreads = 256;
constexpr int kMaxPix = RGP_METRICS_MAX_PIX;
constexpr int kMaxFix = RGP_METRICS_MAX_FIX;
constexpr int kChunk = kMaxPix / kThreads;   // pixels a thread owns at most
constexpr int kStatusBytes = 64;
enum { kDrawJudd = 0, kDrawBorji = 1, kDrawShuffled = 2 };

struct MetricsParams {
  const void *pred, *gt;
  const float *fix, *other;
  long long other_stride;
  int n_frames, n_pix;
  unsigned metrics, flags;
  int n_rep, neg_stride;
  double step_size;
  const double* judd_jitter;
  const int *borji_neg, *shuf_neg, *shuf_cnt;   // the caller's draws
  int *ws_borji, *ws_shuf, *ws_cnt;             // device draws: written, then read back by the same threads
  unsigned long long seed, offset;
  int* status;
  double* scores;
};

// numpy's order for floating point (sort, searchsorted): a < b, NaN after everything
__device__ __forceinline__ bool np_less(double a, double b) { return a < b || (b != b && a == a); }
// np.max / np.min of two: NaN propagates
__device__ __forceinline__ double np_max(double a, double b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }
__device__ __forceinline__ double np_min(double a, double b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }
__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// every thread gets the K block sums (same bits in every thread: the butterfly adds commute)
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double* sh) {
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < K; ++k) sh[wave * K + k] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = (sh[k] + sh[K + k]) + (sh[2 * K + k] + sh[3 * K + k]);
}

// np.min and np.max over the block (NaN propagates)
__device__ __forceinline__ void block_minmax(double& mn, double& mx, double* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = np_min(mn, __shfl_xor(mn, o));
    mx = np_max(mx, __shfl_xor(mx, o));
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) { sh[wave * 2] = mn; sh[wave * 2 + 1] = mx; }
  __syncthreads();
  mn = np_min(np_min(sh[0], sh[2]), np_min(sh[4], sh[6]));
  mx = np_max(np_max(sh[1], sh[3]), np_max(sh[5], sh[7]));
}

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

// word `sample & 3` of the Philox block (sample / 4, rep, frame, metric)
__device__ __forceinline__ void draw_block(unsigned out[4], unsigned blk, unsigned rep, unsigned long long frame, int what,
                                           unsigned long long seed) {
  out[0] = blk; out[1] = rep; out[2] = (unsigned)frame; out[3] = ((unsigned)(frame >> 32) << 2) | (unsigned)what;
  philox4x32_10(out, (unsigned)seed, (unsigned)(seed >> 32));
}

__global__ __launch_bounds__(kThreads, 2) void saliency_scores_kernel(const MetricsParams p) {
  __shared__ double sP[kMaxPix];
  __shared__ double sFixP[kMaxFix], sFixJ[kMaxFix], sThr[kMaxFix];
  __shared__ int sCnt[kMaxFix];
  __shared__ unsigned short sOther[kMaxPix];
  __shared__ double sRed[4 * 8];
  __shared__ int sScan[4];
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
    block_minmax(mn, mx, sRed);
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
    if (tid == 0) {
      atomicAdd(p.status, 1);
      for (int r = 0; r < RGP_METRICS_COUNT; ++r)
        if (M >> r & 1) p.scores[(long long)r * p.n_frames + n] = nan;
    }
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
    block_sum(s1, sRed);
    const double gsum = s1[0], psum = s1[1], mg = gsum / dn, mp = psum / dn;
    // sim; g - mean, r - mean (their sums, whether their max is > 0); NSS's variance of the prediction
    double s2[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < kChunk; ++j)
      if (own[j]) {
        const double a = g[j] / gsum, b = pv[j] / psum;
        s2[0] += (a != a) ? a : ((b != b) ? b : (a < b ? a : b));     // np.minimum
        const double g1 = g[j] - mg, r1 = pv[j] - mp;
        s2[1] += g1; s2[2] += r1;
        s2[3] += g1 > 0.0 ? 1.0 : 0.0; s2[4] += r1 > 0.0 ? 1.0 : 0.0;
        s2[5] += r1 * r1;
      }
    block_sum(s2, sRed);
    score[RGP_METRIC_ROW_SIM] = s2[0];
    if (M & RGP_METRIC_CC) {
      const double m2g = s2[1] / dn, m2r = s2[2] / dn;
      const bool pos_g = s2[3] > 0.0, pos_r = s2[4] > 0.0;
      double s3[2] = {0.0, 0.0};
#pragma unroll
      for (int j = 0; j < kChunk; ++j)
        if (own[j]) {
          const double a = (g[j] - mg) - m2g, b = (pv[j] - mp) - m2r;
          s3[0] += a * a; s3[1] += b * b;
        }
      block_sum(s3, sRed);
      const double sdg = sqrt(s3[0] / dn), sdr = sqrt(s3[1] / dn);
      double s4[2] = {0.0, 0.0};
#pragma unroll
      for (int j = 0; j < kChunk; ++j) {   // g, pv become the standardised maps np.corrcoef is given
        g[j] = g[j] - mg;
        if (pos_g) g[j] = g[j] / sdg;
        pv[j] = pv[j] - mp;
        if (pos_r) pv[j] = pv[j] / sdr;
        if (own[j]) { s4[0] += g[j]; s4[1] += pv[j]; }
      }
      block_sum(s4, sRed);
      const double ag = s4[0] / dn, ar = s4[1] / dn;
      double s5[3] = {0.0, 0.0, 0.0};
#pragma unroll
      for (int j = 0; j < kChunk; ++j)
        if (own[j]) {
          const double xg = g[j] - ag, xr = pv[j] - ar;
          s5[0] += xr * xr; s5[1] += xg * xg; s5[2] += xr * xg;
        }
      block_sum(s5, sRed);
      const double f = 1.0 / (dn - 1.0);                                   // np.cov: c *= 1 / (n - ddof)
      const double c00 = s5[0] * f, c11 = s5[1] * f, c01 = s5[2] * f;
      double c = (c01 / sqrt(c00)) / sqrt(c11);                            // np.corrcoef, then its clip to [-1, 1]
      c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
      score[RGP_METRIC_ROW_CC] = c;
#pragma unroll
      for (int j = 0; j < kChunk; ++j)
        if (own[j]) pv[j] = sP[base + j];
    }
    if ((M & RGP_METRIC_NSS) && n_fix > 0 && tid == 0) {
      const double sd = sqrt(s2[5] / dn), den = sd > 0.0 ? sd : 1.0;
      double acc = 0.0;
      for (int k = 0; k < n_fix; ++k) acc += (sFixP[k] - mp) / den;
      score[RGP_METRIC_ROW_NSS] = acc / (double)n_fix;
    }
  }

  // ---- AUC_Judd (:42-98)
  if ((M & RGP_METRIC_AUC_JUDD) && n_fix > 0) {
    const bool jitter = device_draws ? !(p.flags & RGP_METRICS_NO_JITTER) : p.judd_jitter != nullptr;
    double sj[kChunk];
    double mn = INFINITY, mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < kChunk; ++j) {
      sj[j] = pv[j];
      if (own[j]) {
        if (jitter) {
          double u;
          if (device_draws) {
            const unsigned pix = (unsigned)(base + j);
            unsigned w[4];
            draw_block(w, pix >> 1, 0u, frame, kDrawJudd, p.seed);
            const unsigned hi = w[(pix & 1) * 2] >> 5, lo = w[(pix & 1) * 2 + 1] >> 6;
            u = (double)(((unsigned long long)hi << 26) | lo) * (1.0 / 9007199254740992.0);
          } else {
            u = p.judd_jitter[fo + base + j];
          }
          sj[j] = pv[j] + u * 1e-7;
        }
        mn = np_min(mn, sj[j]);
        mx = np_max(mx, sj[j]);
      }
    }
    block_minmax(mn, mx, sRed);
    const double den = mx - mn;
    int o = foff;
#pragma unroll
    for (int j = 0; j < kChunk; ++j) {
      sj[j] = (sj[j] - mn) / den;
      if (fmask >> j & 1) sFixJ[o++] = sj[j];
    }
    if (tid < n_fix) sCnt[tid] = 0;
    __syncthreads();
    if (tid < n_fix) {   // thresholds = saliency at the fixations, descending (np.sort(...)[::-1]: NaN first)
      const double v = sFixJ[tid];
      int rank = 0;
      for (int k = 0; k < n_fix; ++k) {
        const double w = sFixJ[k];
        rank += (np_less(v, w) || (!np_less(w, v) && k < tid)) ? 1 : 0;
      }
      sThr[rank] = v;
    }
    __syncthreads();
    for (int k = 0; k < n_fix; ++k) {   // #(S < thr_k): searchsorted(sorted S, thr_k, 'left')
      const double thr = sThr[k];
      int c = 0;
#pragma unroll
      for (int j = 0; j < kChunk; ++j) c += (own[j] && np_less(sj[j], thr)) ? 1 : 0;
#pragma unroll
      for (int o2 = 32; o2 > 0; o2 >>= 1) c += __shfl_xor(c, o2);
      if (lane == 0) atomicAdd(&sCnt[k], c);
    }
    __syncthreads();
    if (tid == 0) {
      double ptp = 0.0, pfp = 0.0, acc = 0.0;
      for (int k = 1; k <= n_fix; ++k) {
        const double tp = (double)k / (double)n_fix;
        const double fp = (double)((n_pix - sCnt[k - 1]) - k) / (double)(n_pix - n_fix);
        acc += (fp - pfp) * (tp + ptp) / 2.0;
        ptp = tp; pfp = fp;
      }
      acc += (1.0 - pfp) * (1.0 + ptp) / 2.0;
      score[RGP_METRIC_ROW_AUC_JUDD] = acc;
    }
  }

  // ---- AUC_Borji (:101-164) and AUC_shuffled (:167-204): the same sweep over two kinds of negatives
  if ((M & (RGP_METRIC_AUC_BORJI | RGP_METRIC_AUC_SHUFFLED)) && n_fix > 0) {
    if (tid == 0) {
      double m = sFixP[0];
      for (int k = 1; k < n_fix; ++k) m = np_max(m, sFixP[k]);
      sFixMax = m;
    }
    __syncthreads();
    const double fix_max = sFixMax, dfix = (double)n_fix;
    double auc[2] = {0.0, 0.0};
    for (int item = tid; item < 2 * p.n_rep; item += kThreads) {
      const int which = item >= p.n_rep ? 1 : 0, rep = item - which * p.n_rep;
      if (!(M & (which ? RGP_METRIC_AUC_SHUFFLED : RGP_METRIC_AUC_BORJI))) continue;
      const long long row_off = ((long long)n * p.n_rep + rep) * p.neg_stride;
      const int* row;
      int cnt;
      if (device_draws) {
        int* wrow = (which ? p.ws_shuf : p.ws_borji) + row_off;
        if (!which) {   // uniform over the map
          cnt = n_fix;
          for (int s = 0; s < cnt; s += 4) {
            unsigned w[4];
            draw_block(w, (unsigned)(s >> 2), (unsigned)rep, frame, kDrawBorji, p.seed);
            for (int q = 0; q < 4 && s + q < cnt; ++q) wrow[s + q] = (int)__umulhi(w[q], (unsigned)n_pix);
          }
        } else {        // Floyd: a uniform subset of cnt distinct members of the negative set
          cnt = n_fix < n_other ? n_fix : n_other;
          if (rep == 0) p.ws_cnt[n] = cnt;
          unsigned w[4] = {0u, 0u, 0u, 0u};
          for (int s = 0; s < cnt; ++s) {
            if ((s & 3) == 0) draw_block(w, (unsigned)(s >> 2), (unsigned)rep, frame, kDrawShuffled, p.seed);
            const int j = n_other - cnt + s;
            int pick = (int)sOther[__umulhi(w[s & 3], (unsigned)(j + 1))];
            bool taken = false;
            for (int q = 0; q < s; ++q) taken = taken || wrow[q] == pick;
            wrow[s] = taken ? (int)sOther[j] : pick;
          }
        }
        row = wrow;
      } else {
        row = (which ? p.shuf_neg : p.borji_neg) + row_off;
        cnt = which ? p.shuf_cnt[n] : n_fix;
        if (cnt < 0 || cnt > p.neg_stride) { atomicOr(&sBad, 1); cnt = 0; }
      }
      // top = max(s_fix.max(), col.max()) as Python's max(a, b) evaluates it; col.max() of no sample: NaN
      double col_max = nan;
      for (int s = 0; s < cnt; ++s) {
        int idx = row[s];
        if (idx < 0 || idx >= n_pix) { atomicOr(&sBad, 1); idx = 0; }
        const double v = sP[idx];
        col_max = s == 0 ? v : np_max(col_max, v);
      }
      const double top = col_max > fix_max ? col_max : fix_max;
      double a = nan;
      if (top == top && cnt > 0) {
        const int n_thr = (int)ceil(top / p.step_size);   // len(np.arange(0, top, step))
        double ptp = 0.0, pfp = 0.0;
        a = 0.0;
        for (int i = n_thr - 1; i >= 0; --i) {
          const double thr = (double)i * p.step_size;
          int lf = 0, lc = 0;
          for (int k = 0; k < n_fix; ++k) lf += np_less(sFixP[k], thr) ? 1 : 0;
          for (int s = 0; s < cnt; ++s) {
            const int idx = row[s];
            lc += np_less(sP[(idx < 0 || idx >= n_pix) ? 0 : idx], thr) ? 1 : 0;
          }
          const double tp = (double)(n_fix - lf) / dfix, fp = (double)(n_fix - lc) / dfix;
          a += (fp - pfp) * (tp + ptp) / 2.0;
          ptp = tp; pfp = fp;
        }
        a += (1.0 - pfp) * (1.0 + ptp) / 2.0;
      }
      auc[which] += a;
    }
    block_sum(auc, sRed);
    score[RGP_METRIC_ROW_AUC_BORJI] = auc[0] / (double)p.n_rep;
    score[RGP_METRIC_ROW_AUC_SHUFFLED] = auc[1] / (double)p.n_rep;
  }

  __syncthreads();
  if (tid == 0) {
    const bool bad = sBad != 0;
    if (bad) atomicAdd(p.status, 1);
    for (int r = 0; r < RGP_METRICS_COUNT; ++r)
      if (M >> r & 1) p.scores[(long long)r * p.n_frames + n] = bad ? nan : score[r];
  }
}

size_t draws_elems(int n_frames, int n_rep, int neg_stride) { return (size_t)n_frames * (size_t)n_rep * (size_t)neg_stride; }

}  // namespace

extern "C" {

size_t rgp_metrics_workspace_bytes(int n_frames, int n_rep, int neg_stride, unsigned flags) {
  if (n_frames <= 0 || n_rep <= 0 || neg_stride <= 0) return 0;
  size_t b = kStatusBytes;
  if (flags & RGP_METRICS_DEVICE_DRAWS) b += (2 * draws_elems(n_frames, n_rep, neg_stride) + (size_t)n_frames) * sizeof(int);
  return align_up(b, 64);
}

int rgp_saliency_scores(const rgp_metrics_args* a, rgp_stream_t stream) {
  RGP_REQUIRE(a != nullptr, "rgp_saliency_scores: args is NULL");
  RGP_REQUIRE(a->n_frames > 0, "rgp_saliency_scores: n_frames = %d must be positive", a->n_frames);
  RGP_REQUIRE(a->height > 0 && a->width > 0 && (long long)a->height * a->width <= RGP_METRICS_MAX_PIX,
              "rgp_saliency_scores: maps of %d x %d: height*width must be in [1, RGP_METRICS_MAX_PIX = %d]", a->height, a->width,
              RGP_METRICS_MAX_PIX);
  const int n_pix = a->height * a->width;
  const unsigned M = a->metrics, F = a->flags;
  RGP_REQUIRE(M != 0 && (M & ~(unsigned)RGP_METRIC_ALL) == 0, "rgp_saliency_scores: metrics mask 0x%x: no or unknown metric bits", M);
  RGP_REQUIRE((F & ~(unsigned)(RGP_METRICS_DEVICE_DRAWS | RGP_METRICS_NO_JITTER | RGP_METRICS_PRED_F64 | RGP_METRICS_GT_F64)) == 0,
              "rgp_saliency_scores: unknown flags 0x%x", F);
  RGP_REQUIRE(a->n_rep > 0, "rgp_saliency_scores: n_rep = %d must be positive", a->n_rep);
  RGP_REQUIRE(a->step_size > 0.0 && 1.0 / a->step_size <= (double)RGP_METRICS_MAX_THRESHOLDS,
              "rgp_saliency_scores: step_size = %g must be positive and at least 1 / RGP_METRICS_MAX_THRESHOLDS", a->step_size);
  RGP_REQUIRE(a->neg_stride > 0 && a->neg_stride <= RGP_METRICS_MAX_FIX,
              "rgp_saliency_scores: neg_stride = %d (fixations per frame) must be in [1, RGP_METRICS_MAX_FIX = %d]", a->neg_stride,
              RGP_METRICS_MAX_FIX);
  RGP_REQUIRE(a->pred && a->fix && a->scores, "rgp_saliency_scores: pred, fix and scores must not be NULL");
  RGP_REQUIRE(a->gt || !(M & (RGP_METRIC_SIM | RGP_METRIC_CC)), "rgp_saliency_scores: sim and cc need gt");
  const bool dev = (F & RGP_METRICS_DEVICE_DRAWS) != 0;
  if (dev) {
    RGP_REQUIRE(!a->judd_jitter && !a->borji_neg && !a->shuf_neg && !a->shuf_cnt,
                "rgp_saliency_scores: RGP_METRICS_DEVICE_DRAWS takes no draws from the caller (the four pointers must be NULL)");
    if (M & RGP_METRIC_AUC_SHUFFLED) {
      RGP_REQUIRE(a->other != nullptr, "rgp_saliency_scores: AUC_shuffled with device draws needs the negative map `other`");
      RGP_REQUIRE(a->other_stride == 0 || a->other_stride == n_pix,
                  "rgp_saliency_scores: other_stride = %lld must be 0 or height*width", a->other_stride);
    }
  } else {
    RGP_REQUIRE(!(F & RGP_METRICS_NO_JITTER), "rgp_saliency_scores: with the caller's draws a NULL judd_jitter means no jitter");
    RGP_REQUIRE(a->borji_neg || !(M & RGP_METRIC_AUC_BORJI), "rgp_saliency_scores: AUC_Borji with the caller's draws needs borji_neg");
    RGP_REQUIRE((a->shuf_neg && a->shuf_cnt) || !(M & RGP_METRIC_AUC_SHUFFLED),
                "rgp_saliency_scores: AUC_shuffled with the caller's draws needs shuf_neg and shuf_cnt");
  }
  const size_t need = rgp_metrics_workspace_bytes(a->n_frames, a->n_rep, a->neg_stride, F);
  if (!a->workspace || a->workspace_bytes < need || ((size_t)a->workspace & 7) != 0)
    return set_err(RGP_EWORKSPACE, "rgp_saliency_scores: workspace missing, misaligned or too small (%zu < %zu bytes)",
                   a->workspace ? a->workspace_bytes : (size_t)0, need);

  MetricsParams p{};
  p.pred = a->pred; p.gt = a->gt; p.fix = a->fix; p.other = a->other; p.other_stride = a->other_stride;
  p.n_frames = a->n_frames; p.n_pix = n_pix; p.metrics = M; p.flags = F;
  p.n_rep = a->n_rep; p.neg_stride = a->neg_stride; p.step_size = a->step_size;
  p.judd_jitter = a->judd_jitter; p.borji_neg = a->borji_neg; p.shuf_neg = a->shuf_neg; p.shuf_cnt = a->shuf_cnt;
  p.seed = a->seed; p.offset = a->offset;
  p.status = (int*)a->workspace;
  p.scores = a->scores;
  if (dev) {
    const size_t e = draws_elems(a->n_frames, a->n_rep, a->neg_stride);
    p.ws_borji = (int*)((char*)a->workspace + kStatusBytes);
    p.ws_shuf = p.ws_borji + e;
    p.ws_cnt = p.ws_shuf + e;
  }
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
