// librgp_hip.so: the saliency metrics at FRAME resolution (include/rgp.h, "saliency metrics at the fixation maps' shape")
// and the cubic-spline resize they rest on.
//
// evaluation_metrics.saliency_score_single upsizes prediction and ground truth (h x w <= 4096 pixels) to the fixation
// map's shape H x W with scipy's order-3 spline (map_coordinates, mode 'reflect') and scores there: 405 x 720 = 291 600
// pixels per frame.  The upsized maps are never stored.  One launch, one 512-thread workgroup per frame:
//   1. the two source maps go to LDS as fp64 and are turned IN PLACE into B-spline coefficients (the recursive
//      prefilter along axis 0, one thread per column, then along axis 1, one thread per row);
//   2. every sweep of the metrics recomputes the full-size values from the coefficients: 16 LDS reads and 20
//      multiply-adds per pixel and map, the per-axis weights and reflected indices from tables the host made;
//   3. AUC_Judd counts by binary search of each pixel among the sorted thresholds and integer LDS counters;
//      AUC_Borji / AUC_shuffled evaluate the spline only at the fixations and at the drawn negatives.
//
// LDS: coefficients 2 x 32 KiB, tables 40 B x (H + W) when H + W <= 1536 (60 KiB; larger targets read them from
// global memory, where they stay cached: they are the same for all frames), 11.5 KiB of small arrays: 135.5 KiB of
// the CU's 160, 124 KiB of them requested as dynamic shared memory.  One workgroup per CU, so the block size is the
// occupancy: 1024 threads would leave 128 VGPRs per thread and the sweeps spill (436 B of scratch per lane); 512
// threads take 179 VGPRs, no scratch, two waves per SIMD behind which the LDS latency of the sweeps hides
// (profiles/metrics_scaled_kernel_resources.txt).
//
// Exactness.  Compiled with -ffp-contract=off, no fast-math, IEEE division.  The resized VALUES are a fixed sequence
// of multiplies and adds (filter_line, spline_at below; tests/spline_ref.py restates them), so they are reproducible
// bit for bit; normalisations, jitter and comparisons are element-wise, counts are integers, and what is left against
// the host is the order of the sums (H W 2^-53).  The order of every sum is fixed by (H, W) alone.
#include <cmath>
#include <vector>

#include "rgp_host.h"
#include "philox.hip.h"
#include "spline.hip.h"

using namespace rgp;

namespace {

constexpr int kThreads = 512, kWaves = kThreads / 64;
constexpr int kMaxSrc = RGP_METRICS_MAX_PIX;
constexpr int kMaxFix = RGP_METRICS_MAX_FIX;
constexpr int kMaxOther = RGP_METRICS_SCALED_MAX_OTHER;
constexpr int kSrcPerThread = kMaxSrc / kThreads;
constexpr int kTabLds = 1536;   // H + W up to which the per-axis tables live in LDS
constexpr int kStatusBytes = 64;
constexpr int kResizeThreads = 256;
enum { kDrawJudd = 0, kDrawBorji = 1, kDrawShuffled = 2 };


struct ScaledParams {
  const void *pred, *gt;
  const int *fix_ptr, *fix_idx, *other_ptr, *other_idx;
  int fix_len, other_len;
  int n_frames, h, w, H, W;
  unsigned metrics, flags;
  int n_rep, neg_stride;
  double step_size;
  const double* judd_jitter;
  const int *borji_neg, *shuf_neg, *shuf_cnt;   // the caller's draws
  int *ws_borji, *ws_shuf, *ws_cnt;             // device draws: written, then read back by the same workgroup
  double* ws_val;                               // [2][n_frames, n_rep, neg_stride]: normalised saliency at the negatives
  const double* tab_w;                          // [H + W][4] weights, rows first
  const unsigned short* tab_i;                  // [H + W][4] reflected source index (rows: times w)
  unsigned long long seed, offset;
  int* status;
  double* scores;
  SplineConsts sc;
};

struct ResizeParams {
  const void* src;
  void* dst;
  int src_f64, dst_f64, h, w, H, W, rows_per_block;
  const double* tab_w;
  const unsigned short* tab_i;
  SplineConsts sc;
};

// numpy's order for floating point (sort, searchsorted): a < b, NaN after everything
__device__ __forceinline__ bool np_less(double a, double b) { return a < b || (b != b && a == a); }
// np.max / np.min of two: NaN propagates
__device__ __forceinline__ double np_max(double a, double b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }
__device__ __forceinline__ double np_min(double a, double b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }
__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// every thread gets the K block sums: wave butterflies, then the waves' sums in wave order
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
  for (int k = 0; k < K; ++k) {
    double s = sh[k];
    for (int wv = 1; wv < kWaves; ++wv) s += sh[wv * K + k];
    v[k] = s;
  }
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
  mn = sh[0]; mx = sh[1];
  for (int wv = 1; wv < kWaves; ++wv) { mn = np_min(mn, sh[wv * 2]); mx = np_max(mx, sh[wv * 2 + 1]); }
}

// word `sample & 3` of the Philox block (sample / 4, rep, frame, metric): the counter of rgp_metrics.hip
__device__ __forceinline__ void draw_block(unsigned out[4], unsigned blk, unsigned rep, unsigned long long frame, int what,
                                           unsigned long long seed) {
  out[0] = blk; out[1] = rep; out[2] = (unsigned)frame; out[3] = ((unsigned)(frame >> 32) << 2) | (unsigned)what;
  philox4x32_10(out, (unsigned)seed, (unsigned)(seed >> 32));
}

// both passes over `n_maps` maps of h x w that lie kMaxSrc apart, by `threads` threads of the block
__device__ __forceinline__ void prefilter(double* maps, int n_maps, int h, int w, const SplineConsts& sc, int threads) {
  for (int l = threadIdx.x; l < n_maps * w; l += threads)
    filter_line(maps + (l / w) * kMaxSrc + l % w, h, w, sc.z, sc.zn[0], sc.gain, sc.k0[0], sc.last);
  __syncthreads();
  for (int l = threadIdx.x; l < n_maps * h; l += threads)
    filter_line(maps + (l / h) * kMaxSrc + (l % h) * w, w, 1, sc.z, sc.zn[1], sc.gain, sc.k0[1], sc.last);
  __syncthreads();
}

// f(pixel, row, column) for the pixels tid, tid + kThreads, ... of the target grid, no division in the loop
template <class F>
__device__ __forceinline__ void for_pixels(int H, int W, F&& f) {
  const int n_pix = H * W, dY = kThreads / W, dX = kThreads % W;
  int Y = (int)threadIdx.x / W, X = (int)threadIdx.x % W;
  for (int pix = threadIdx.x; pix < n_pix; pix += kThreads) {
    f(pix, Y, X);
    X += dX; Y += dY;
    if (X >= W) { X -= W; ++Y; }
  }
}

template <bool kTabInLds>
__global__ __launch_bounds__(kThreads) void scaled_scores_kernel(const ScaledParams p) {
  extern __shared__ double smem[];
  double* sC = smem;                      // coefficients of pred, then (kMaxSrc on) of gt
  double* sCp = sC;
  double* sCg = sC + kMaxSrc;
  __shared__ double sFixRaw[kMaxFix], sFixP[kMaxFix], sFixJ[kMaxFix], sThr[kMaxFix];
  __shared__ int sFixPix[kMaxFix], sHist[kMaxFix + 1], sCnt[kMaxFix];
  __shared__ double sRed[kWaves * 8];
  __shared__ int sBad;
  __shared__ double sFixMax;

  const int tid = threadIdx.x, lane = tid & 63;
  const int n = blockIdx.x, h = p.h, w = p.w, H = p.H, W = p.W;
  const int n_src = h * w, n_pix = H * W;
  const unsigned long long frame = p.offset + (unsigned long long)n;
  const bool device_draws = (p.flags & RGP_METRICS_DEVICE_DRAWS) != 0;
  const unsigned M = p.metrics;
  const double nan = quiet_nan();
  double score[RGP_METRICS_COUNT] = {nan, nan, nan, nan, nan, nan};
  if (tid == 0) sBad = 0;

  const double* tw;
  const unsigned short* ti;
  if constexpr (kTabInLds) {
    double* sTabW = smem + 2 * kMaxSrc;
    unsigned short* sTabI = (unsigned short*)(sTabW + kTabLds * 4);
    for (int i = tid; i < (H + W) * 4; i += kThreads) { sTabW[i] = p.tab_w[i]; sTabI[i] = p.tab_i[i]; }
    tw = sTabW; ti = sTabI;
  } else {
    tw = p.tab_w; ti = p.tab_i;
  }

  // ---- pred -> normalize_range at h x w (saliency_score_single), in the arithmetic numpy uses for the array's dtype; gt widened
  const bool want_gt = (M & (RGP_METRIC_SIM | RGP_METRIC_CC)) != 0;
  {
    const long long so = (long long)n * n_src;
    double pv[kSrcPerThread];
    double mn = INFINITY, mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < kSrcPerThread; ++j) {
      const int i = tid + j * kThreads;
      pv[j] = 0.0;
      if (i < n_src) {
        pv[j] = (p.flags & RGP_METRICS_PRED_F64) ? ((const double*)p.pred)[so + i] : (double)((const float*)p.pred)[so + i];
        mn = np_min(mn, pv[j]);
        mx = np_max(mx, pv[j]);
      }
    }
    block_minmax(mn, mx, sRed);
    const double den = mx - mn;
    const float mnf = (float)mn, denf = (float)mx - (float)mn;
#pragma unroll
    for (int j = 0; j < kSrcPerThread; ++j) {
      const int i = tid + j * kThreads;
      if (i < n_src) {
        sCp[i] = (p.flags & RGP_METRICS_PRED_F64) ? (pv[j] - mn) / den : (double)(((float)pv[j] - mnf) / denf);
        if (want_gt) sCg[i] = (p.flags & RGP_METRICS_GT_F64) ? ((const double*)p.gt)[so + i] : (double)((const float*)p.gt)[so + i];
      }
    }
  }
  __syncthreads();
  prefilter(sC, want_gt ? 2 : 1, h, w, p.sc, kThreads);

  // ---- the frame's fixations and negative set: nothing is used as an address before it is checked
  int n_fix = 0, n_other = 0, o_base = 0;
  {
    const int a = p.fix_ptr[n], b = p.fix_ptr[n + 1];
    const bool ok = a >= 0 && b >= a && b <= p.fix_len && b - a <= p.neg_stride;
    if (!ok) atomicOr(&sBad, 1);
    n_fix = ok ? b - a : 0;
    if (tid < n_fix) {
      const int idx = p.fix_idx[a + tid];
      const bool good = idx >= 0 && idx < n_pix && (tid == 0 || p.fix_idx[a + tid - 1] < idx);
      if (!good) atomicOr(&sBad, 1);
      sFixPix[tid] = good ? idx : 0;
    }
  }
  if ((M & RGP_METRIC_AUC_SHUFFLED) && p.other_ptr != nullptr) {
    const int q = (p.flags & RGP_METRICS_SCALED_OTHER_SHARED) ? 0 : n;
    const int a = p.other_ptr[q], b = p.other_ptr[q + 1];
    const bool ok = a >= 0 && b >= a && b <= p.other_len && b - a <= kMaxOther;
    if (!ok) atomicOr(&sBad, 1);
    n_other = ok ? b - a : 0;
    o_base = a;
    for (int i = tid; i < n_other; i += kThreads) {
      const int idx = p.other_idx[a + i];
      if (!(idx >= 0 && idx < n_pix && (i == 0 || p.other_idx[a + i - 1] < idx))) atomicOr(&sBad, 1);
    }
  }
  int cnt_shuf = device_draws ? (n_fix < n_other ? n_fix : n_other) : 0;
  if (!device_draws && (M & RGP_METRIC_AUC_SHUFFLED)) {
    cnt_shuf = p.shuf_cnt[n];
    if (cnt_shuf < 0 || cnt_shuf > p.neg_stride) { atomicOr(&sBad, 1); cnt_shuf = 0; }
  }
  __syncthreads();
  if (sBad != 0) {   // uniform over the block: no finite score, the call reports it
    if (tid == 0) {
      atomicAdd(p.status, 1);
      for (int r = 0; r < RGP_METRICS_COUNT; ++r)
        if (M >> r & 1) p.scores[(long long)r * p.n_frames + n] = nan;
    }
    return;
  }
  if (device_draws && (M & RGP_METRIC_AUC_SHUFFLED) && tid == 0) p.ws_cnt[n] = n_fix > 0 ? cnt_shuf : 0;

  // ---- first sweep: the sums of both resized maps, and min / max of the resized prediction (normalize_range of the AUCs)
  const double dn = (double)n_pix;
  double gsum = 0.0, psum = 0.0, pmn = nan, pden = nan;
  if (M & (RGP_METRIC_SIM | RGP_METRIC_CC | RGP_METRIC_NSS | RGP_METRIC_AUC_BORJI | RGP_METRIC_AUC_SHUFFLED)) {
    double s1[2] = {0.0, 0.0};
    double mn = INFINITY, mx = -INFINITY;
    for_pixels(H, W, [&](int, int Y, int X) {
      Taps t;
      load_taps(t, tw, ti, H, Y, X);
      const double r = spline_at(sCp, t);
      s1[1] += r;
      mn = np_min(mn, r);
      mx = np_max(mx, r);
      if (want_gt) s1[0] += spline_at(sCg, t);
    });
    block_sum(s1, sRed);
    block_minmax(mn, mx, sRed);
    gsum = s1[0]; psum = s1[1]; pmn = mn; pden = mx - mn;
  }
  if (tid < n_fix) {
    Taps t;
    load_taps(t, tw, ti, H, sFixPix[tid] / W, sFixPix[tid] % W);
    const double r = spline_at(sCp, t);
    sFixRaw[tid] = r;
    sFixP[tid] = (r - pmn) / pden;
  }
  __syncthreads();

  // ---- sim (:207-218), cc (:221-236), NSS: one sweep per dependent statement of the host, every value recomputed
  if (M & (RGP_METRIC_SIM | RGP_METRIC_CC | RGP_METRIC_NSS)) {
    const double mg = gsum / dn, mp = psum / dn;
    double s2[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for_pixels(H, W, [&](int, int Y, int X) {
      Taps t;
      load_taps(t, tw, ti, H, Y, X);
      const double r = spline_at(sCp, t), g = want_gt ? spline_at(sCg, t) : 0.0;
      const double a = g / gsum, b = r / psum;
      s2[0] += (a != a) ? a : ((b != b) ? b : (a < b ? a : b));     // np.minimum
      const double g1 = g - mg, r1 = r - mp;
      s2[1] += g1; s2[2] += r1;
      s2[3] += g1 > 0.0 ? 1.0 : 0.0; s2[4] += r1 > 0.0 ? 1.0 : 0.0;
      s2[5] += r1 * r1;
    });
    block_sum(s2, sRed);
    score[RGP_METRIC_ROW_SIM] = s2[0];
    if (M & RGP_METRIC_CC) {
      const double m2g = s2[1] / dn, m2r = s2[2] / dn;
      const bool pos_g = s2[3] > 0.0, pos_r = s2[4] > 0.0;
      double s3[2] = {0.0, 0.0};
      for_pixels(H, W, [&](int, int Y, int X) {
        Taps t;
        load_taps(t, tw, ti, H, Y, X);
        const double a = (spline_at(sCg, t) - mg) - m2g, b = (spline_at(sCp, t) - mp) - m2r;
        s3[0] += a * a; s3[1] += b * b;
      });
      block_sum(s3, sRed);
      const double sdg = sqrt(s3[0] / dn), sdr = sqrt(s3[1] / dn);
      double s4[2] = {0.0, 0.0};
      for_pixels(H, W, [&](int, int Y, int X) {   // the standardised maps np.corrcoef is given
        Taps t;
        load_taps(t, tw, ti, H, Y, X);
        double g = spline_at(sCg, t) - mg, r = spline_at(sCp, t) - mp;
        if (pos_g) g = g / sdg;
        if (pos_r) r = r / sdr;
        s4[0] += g; s4[1] += r;
      });
      block_sum(s4, sRed);
      const double ag = s4[0] / dn, ar = s4[1] / dn;
      double s5[3] = {0.0, 0.0, 0.0};
      for_pixels(H, W, [&](int, int Y, int X) {
        Taps t;
        load_taps(t, tw, ti, H, Y, X);
        double g = spline_at(sCg, t) - mg, r = spline_at(sCp, t) - mp;
        if (pos_g) g = g / sdg;
        if (pos_r) r = r / sdr;
        const double xg = g - ag, xr = r - ar;
        s5[0] += xr * xr; s5[1] += xg * xg; s5[2] += xr * xg;
      });
      block_sum(s5, sRed);
      const double f = 1.0 / (dn - 1.0);                                   // np.cov: c *= 1 / (n - ddof)
      const double c00 = s5[0] * f, c11 = s5[1] * f, c01 = s5[2] * f;
      double c = (c01 / sqrt(c00)) / sqrt(c11);                            // np.corrcoef, then its clip to [-1, 1]
      c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
      score[RGP_METRIC_ROW_CC] = c;
    }
    if ((M & RGP_METRIC_NSS) && n_fix > 0 && tid == 0) {
      const double sd = sqrt(s2[5] / dn), den = sd > 0.0 ? sd : 1.0;
      double acc = 0.0;
      for (int k = 0; k < n_fix; ++k) acc += (sFixRaw[k] - mp) / den;
      score[RGP_METRIC_ROW_NSS] = acc / (double)n_fix;
    }
  }

  // ---- AUC_Judd (:42-98): jitter per target pixel, normalize_range over the jittered full-size map
  if ((M & RGP_METRIC_AUC_JUDD) && n_fix > 0) {
    const bool jitter = device_draws ? !(p.flags & RGP_METRICS_NO_JITTER) : p.judd_jitter != nullptr;
    const long long jo = (long long)n * n_pix;
    auto jittered = [&](int pix, int Y, int X) -> double {
      Taps t;
      load_taps(t, tw, ti, H, Y, X);
      double r = spline_at(sCp, t);
      if (jitter) {
        double u;
        if (device_draws) {
          unsigned wd[4];
          draw_block(wd, (unsigned)pix >> 1, 0u, frame, kDrawJudd, p.seed);
          const unsigned hi = wd[(pix & 1) * 2] >> 5, lo = wd[(pix & 1) * 2 + 1] >> 6;
          u = (double)(((unsigned long long)hi << 26) | lo) * (1.0 / 9007199254740992.0);
        } else {
          u = p.judd_jitter[jo + pix];
        }
        r = r + u * 1e-7;
      }
      return r;
    };
    double mn = INFINITY, mx = -INFINITY;
    for_pixels(H, W, [&](int pix, int Y, int X) {
      const double r = jittered(pix, Y, X);
      mn = np_min(mn, r);
      mx = np_max(mx, r);
    });
    block_minmax(mn, mx, sRed);
    const double den = mx - mn;
    if (tid < n_fix) sFixJ[tid] = (jittered(sFixPix[tid], sFixPix[tid] / W, sFixPix[tid] % W) - mn) / den;
    if (tid <= n_fix) sHist[tid] = 0;
    __syncthreads();
    if (tid < n_fix) {   // thresholds = saliency at the fixations, descending (np.sort(...)[::-1]: NaN first)
      const double v = sFixJ[tid];
      int rank = 0;
      for (int k = 0; k < n_fix; ++k) {
        const double x = sFixJ[k];
        rank += (np_less(v, x) || (!np_less(x, v) && k < tid)) ? 1 : 0;
      }
      sThr[rank] = v;
    }
    __syncthreads();
    // a pixel is below the first m thresholds (they descend): hist[m]++, and #(S < thr_k) = sum of hist[m], m > k
    int below_all = 0;
    for_pixels(H, W, [&](int pix, int Y, int X) {
      const double s = (jittered(pix, Y, X) - mn) / den;
      int lo = 0, hi = n_fix;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (np_less(s, sThr[mid])) lo = mid + 1; else hi = mid;
      }
      if (lo == n_fix) ++below_all; else atomicAdd(&sHist[lo], 1);
    });
#pragma unroll
    for (int o2 = 32; o2 > 0; o2 >>= 1) below_all += __shfl_xor(below_all, o2);
    if (lane == 0) atomicAdd(&sHist[n_fix], below_all);
    __syncthreads();
    if (tid == 0) {
      int run = 0;
      for (int k = n_fix - 1; k >= 0; --k) { run += sHist[k + 1]; sCnt[k] = run; }
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
    const long long E = (long long)p.n_frames * p.n_rep * p.neg_stride;
    const long long frame_off = (long long)n * p.n_rep * p.neg_stride;
    if (tid == 0) {
      double m = sFixP[0];
      for (int k = 1; k < n_fix; ++k) m = np_max(m, sFixP[k]);
      sFixMax = m;
    }
    // 1. device draws: one thread per (metric, repetition) leaves the indices in the workspace
    if (device_draws)
      for (int item = tid; item < 2 * p.n_rep; item += kThreads) {
        const int which = item >= p.n_rep ? 1 : 0, rep = item - which * p.n_rep;
        if (!(M & (which ? RGP_METRIC_AUC_SHUFFLED : RGP_METRIC_AUC_BORJI))) continue;
        int* wrow = (which ? p.ws_shuf : p.ws_borji) + frame_off + (long long)rep * p.neg_stride;
        if (!which) {   // uniform over the target grid
          for (int s = 0; s < n_fix; s += 4) {
            unsigned wd[4];
            draw_block(wd, (unsigned)(s >> 2), (unsigned)rep, frame, kDrawBorji, p.seed);
            for (int q = 0; q < 4 && s + q < n_fix; ++q) wrow[s + q] = (int)__umulhi(wd[q], (unsigned)n_pix);
          }
        } else {        // Floyd: a uniform subset of cnt_shuf distinct members of the negative set
          unsigned wd[4] = {0u, 0u, 0u, 0u};
          for (int s = 0; s < cnt_shuf; ++s) {
            if ((s & 3) == 0) draw_block(wd, (unsigned)(s >> 2), (unsigned)rep, frame, kDrawShuffled, p.seed);
            const int j = n_other - cnt_shuf + s;
            const int pick = p.other_idx[o_base + (int)__umulhi(wd[s & 3], (unsigned)(j + 1))];
            bool taken = false;
            for (int q = 0; q < s; ++q) taken = taken || wrow[q] == pick;
            wrow[s] = taken ? p.other_idx[o_base + j] : pick;
          }
        }
      }
    __syncthreads();
    // 2. the normalised saliency at every negative, from the coefficients: one thread per (metric, repetition, sample)
    const int per_metric = p.n_rep * p.neg_stride;
    for (int item = tid; item < 2 * per_metric; item += kThreads) {
      const int which = item >= per_metric ? 1 : 0, r = item - which * per_metric, s = r % p.neg_stride;
      if (!(M & (which ? RGP_METRIC_AUC_SHUFFLED : RGP_METRIC_AUC_BORJI))) continue;
      if (s >= (which ? cnt_shuf : n_fix)) continue;
      const int* src = device_draws ? (which ? p.ws_shuf : p.ws_borji) : (which ? p.shuf_neg : p.borji_neg);
      int idx = src[frame_off + r];
      if (idx < 0 || idx >= n_pix) { atomicOr(&sBad, 1); idx = 0; }
      Taps t;
      load_taps(t, tw, ti, H, idx / W, idx % W);
      p.ws_val[which * E + frame_off + r] = (spline_at(sCp, t) - pmn) / pden;
    }
    __syncthreads();
    // 3. the ROC sweep of each repetition
    const double fix_max = sFixMax, dfix = (double)n_fix;
    double auc[2] = {0.0, 0.0};
    for (int item = tid; item < 2 * p.n_rep; item += kThreads) {
      const int which = item >= p.n_rep ? 1 : 0, rep = item - which * p.n_rep;
      if (!(M & (which ? RGP_METRIC_AUC_SHUFFLED : RGP_METRIC_AUC_BORJI))) continue;
      const double* vals = p.ws_val + which * E + frame_off + (long long)rep * p.neg_stride;
      const int cnt = which ? cnt_shuf : n_fix;
      // top = max(s_fix.max(), col.max()) as Python's max(a, b) evaluates it; col.max() of no sample: NaN
      double col_max = nan;
      for (int s = 0; s < cnt; ++s) col_max = s == 0 ? vals[s] : np_max(col_max, vals[s]);
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
          for (int s = 0; s < cnt; ++s) lc += np_less(vals[s], thr) ? 1 : 0;
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

// the resized maps themselves: grid (frames, row blocks); every block prefilters its frame again (a few microseconds)
__global__ __launch_bounds__(kResizeThreads) void spline_resize_kernel(const ResizeParams p) {
  __shared__ double sC[kMaxSrc];
  const int tid = threadIdx.x, n = blockIdx.x, n_src = p.h * p.w;
  const long long so = (long long)n * n_src;
  for (int i = tid; i < n_src; i += kResizeThreads)
    sC[i] = p.src_f64 ? ((const double*)p.src)[so + i] : (double)((const float*)p.src)[so + i];
  __syncthreads();
  prefilter(sC, 1, p.h, p.w, p.sc, kResizeThreads);
  const int y0 = blockIdx.y * p.rows_per_block;
  const int y1 = y0 + p.rows_per_block < p.H ? y0 + p.rows_per_block : p.H;
  const long long dof = (long long)n * p.H * p.W;
  for (int i = tid; i < (y1 - y0) * p.W; i += kResizeThreads) {
    const int Y = y0 + i / p.W, X = i % p.W;
    Taps t;
    load_taps(t, p.tab_w, p.tab_i, p.H, Y, X);
    const double v = spline_at(sC, t);
    const long long o = dof + (long long)Y * p.W + X;
    if (p.dst_f64) ((double*)p.dst)[o] = v; else ((float*)p.dst)[o] = (float)v;
  }
}

size_t draws_elems(int n_frames, int n_rep, int neg_stride) { return (size_t)n_frames * (size_t)n_rep * (size_t)neg_stride; }
int check_shapes(const char* fn, int h, int w, int H, int W) {
  RGP_REQUIRE(h >= 2 && w >= 2 && (long long)h * w <= RGP_METRICS_MAX_PIX,
              "%s: source maps of %d x %d: height and width must be at least 2 and height*width at most RGP_METRICS_MAX_PIX = %d", fn, h, w,
              RGP_METRICS_MAX_PIX);
  RGP_REQUIRE(H >= 1 && W >= 1 && (long long)H * W <= RGP_METRICS_SCALED_MAX_PIX,
              "%s: target of %d x %d: target_height*target_width must be in [1, RGP_METRICS_SCALED_MAX_PIX = %d]", fn, H, W,
              RGP_METRICS_SCALED_MAX_PIX);
  return RGP_OK;
}

}  // namespace

extern "C" {

size_t rgp_metrics_scaled_workspace_bytes(int n_frames, int n_rep, int neg_stride, int height, int width, unsigned flags) {
  if (n_frames <= 0 || n_rep <= 0 || neg_stride <= 0 || height <= 0 || width <= 0) return 0;
  const size_t e = draws_elems(n_frames, n_rep, neg_stride);
  size_t b = kStatusBytes;
  if (flags & RGP_METRICS_DEVICE_DRAWS) b += (2 * e + (size_t)n_frames) * sizeof(int);
  b = align_up(b, 64) + 2 * e * sizeof(double);
  return align_up(b, 64) + spline_tables_bytes(height, width);
}

size_t rgp_spline_resize_workspace_bytes(int H, int W) { return H <= 0 || W <= 0 ? 0 : spline_tables_bytes(H, W); }

int rgp_saliency_scores_scaled(const rgp_metrics_scaled_args* a, rgp_stream_t stream) {
  const char* fn = "rgp_saliency_scores_scaled";
  RGP_REQUIRE(a != nullptr, "%s: args is NULL", fn);
  RGP_REQUIRE(a->n_frames > 0, "%s: n_frames = %d must be positive", fn, a->n_frames);
  RGP_TRY(check_shapes(fn, a->height, a->width, a->target_height, a->target_width));
  const unsigned M = a->metrics, F = a->flags;
  RGP_REQUIRE(M != 0 && (M & ~(unsigned)RGP_METRIC_ALL) == 0, "%s: metrics mask 0x%x: no or unknown metric bits", fn, M);
  RGP_REQUIRE((F & ~(unsigned)(RGP_METRICS_DEVICE_DRAWS | RGP_METRICS_NO_JITTER | RGP_METRICS_PRED_F64 | RGP_METRICS_GT_F64 |
                               RGP_METRICS_SCALED_OTHER_SHARED)) == 0, "%s: unknown flags 0x%x", fn, F);
  RGP_REQUIRE(a->n_rep > 0, "%s: n_rep = %d must be positive", fn, a->n_rep);
  RGP_REQUIRE(a->step_size > 0.0 && 1.0 / a->step_size <= (double)RGP_METRICS_MAX_THRESHOLDS,
              "%s: step_size = %g must be positive and at least 1 / RGP_METRICS_MAX_THRESHOLDS", fn, a->step_size);
  RGP_REQUIRE(a->neg_stride > 0 && a->neg_stride <= RGP_METRICS_MAX_FIX,
              "%s: neg_stride = %d (fixations per frame) must be in [1, RGP_METRICS_MAX_FIX = %d]", fn, a->neg_stride, RGP_METRICS_MAX_FIX);
  RGP_REQUIRE(a->pred && a->fix_ptr && a->fix_idx && a->scores, "%s: pred, fix_ptr, fix_idx and scores must not be NULL", fn);
  RGP_REQUIRE(a->fix_len >= 0 && a->other_len >= 0, "%s: fix_len = %d and other_len = %d must not be negative", fn, a->fix_len, a->other_len);
  RGP_REQUIRE(a->gt || !(M & (RGP_METRIC_SIM | RGP_METRIC_CC)), "%s: sim and cc need gt", fn);
  RGP_REQUIRE((a->other_ptr == nullptr) == (a->other_idx == nullptr), "%s: other_ptr and other_idx go together", fn);
  const bool dev = (F & RGP_METRICS_DEVICE_DRAWS) != 0;
  if (dev) {
    RGP_REQUIRE(!a->judd_jitter && !a->borji_neg && !a->shuf_neg && !a->shuf_cnt,
                "%s: RGP_METRICS_DEVICE_DRAWS takes no draws from the caller (the four pointers must be NULL)", fn);
    RGP_REQUIRE(a->other_ptr || !(M & RGP_METRIC_AUC_SHUFFLED), "%s: AUC_shuffled with device draws needs the negative set other_ptr / other_idx", fn);
  } else {
    RGP_REQUIRE(!(F & RGP_METRICS_NO_JITTER), "%s: with the caller's draws a NULL judd_jitter means no jitter", fn);
    RGP_REQUIRE(a->borji_neg || !(M & RGP_METRIC_AUC_BORJI), "%s: AUC_Borji with the caller's draws needs borji_neg", fn);
    RGP_REQUIRE((a->shuf_neg && a->shuf_cnt) || !(M & RGP_METRIC_AUC_SHUFFLED),
                "%s: AUC_shuffled with the caller's draws needs shuf_neg and shuf_cnt", fn);
  }
  const int H = a->target_height, W = a->target_width;
  const size_t need = rgp_metrics_scaled_workspace_bytes(a->n_frames, a->n_rep, a->neg_stride, H, W, F);
  if (!a->workspace || a->workspace_bytes < need || ((size_t)a->workspace & 7) != 0)
    return set_err(RGP_EWORKSPACE, "%s: workspace missing, misaligned or too small (%zu < %zu bytes)", fn,
                   a->workspace ? a->workspace_bytes : (size_t)0, need);

  ScaledParams p{};
  p.pred = a->pred; p.gt = a->gt; p.fix_ptr = a->fix_ptr; p.fix_idx = a->fix_idx; p.other_ptr = a->other_ptr; p.other_idx = a->other_idx;
  p.fix_len = a->fix_len; p.other_len = a->other_len;
  p.n_frames = a->n_frames; p.h = a->height; p.w = a->width; p.H = H; p.W = W; p.metrics = M; p.flags = F;
  p.n_rep = a->n_rep; p.neg_stride = a->neg_stride; p.step_size = a->step_size;
  p.judd_jitter = a->judd_jitter; p.borji_neg = a->borji_neg; p.shuf_neg = a->shuf_neg; p.shuf_cnt = a->shuf_cnt;
  p.seed = a->seed; p.offset = a->offset;
  p.status = (int*)a->workspace;
  p.scores = a->scores;
  p.sc = spline_consts(a->height, a->width);
  const size_t e = draws_elems(a->n_frames, a->n_rep, a->neg_stride);
  char* ws = (char*)a->workspace;
  size_t off = kStatusBytes;
  if (dev) {
    p.ws_borji = (int*)(ws + off);
    p.ws_shuf = p.ws_borji + e;
    p.ws_cnt = p.ws_shuf + e;
    off += (2 * e + (size_t)a->n_frames) * sizeof(int);
  }
  off = align_up(off, 64);
  p.ws_val = (double*)(ws + off);
  off = align_up(off + 2 * e * sizeof(double), 64);
  hipStream_t s = (hipStream_t)stream;
  RGP_TRY(upload_tables(a->height, a->width, H, W, ws + off, s, &p.tab_w, &p.tab_i));
  RGP_HIP(hipMemsetAsync(a->workspace, 0, kStatusBytes, s));
  const bool in_lds = H + W <= kTabLds;
  const int smem = 2 * kMaxSrc * (int)sizeof(double) + (in_lds ? kTabLds * 4 * (int)(sizeof(double) + sizeof(unsigned short)) : 0);
  auto kern = in_lds ? scaled_scores_kernel<true> : scaled_scores_kernel<false>;
  RGP_TRY(ensure_dyn_smem((const void*)kern, smem));
  hipLaunchKernelGGL(kern, dim3(a->n_frames), dim3(kThreads), smem, s, p);
  RGP_HIP(hipGetLastError());
  return RGP_OK;
}

int rgp_spline_resize(const void* src, int src_f64, int n_frames, int h, int w, void* dst, int dst_f64, int H, int W,
                      void* workspace, size_t workspace_bytes, rgp_stream_t stream) {
  const char* fn = "rgp_spline_resize";
  RGP_REQUIRE(src && dst, "%s: src and dst must not be NULL", fn);
  RGP_REQUIRE(n_frames > 0, "%s: n_frames = %d must be positive", fn, n_frames);
  RGP_TRY(check_shapes(fn, h, w, H, W));
  const size_t need = rgp_spline_resize_workspace_bytes(H, W);
  if (!workspace || workspace_bytes < need || ((size_t)workspace & 7) != 0)
    return set_err(RGP_EWORKSPACE, "%s: workspace missing, misaligned or too small (%zu < %zu bytes)", fn,
                   workspace ? workspace_bytes : (size_t)0, need);
  ResizeParams p{};
  p.src = src; p.dst = dst; p.src_f64 = src_f64 != 0; p.dst_f64 = dst_f64 != 0; p.h = h; p.w = w; p.H = H; p.W = W;
  p.sc = spline_consts(h, w);
  hipStream_t s = (hipStream_t)stream;
  RGP_TRY(upload_tables(h, w, H, W, workspace, s, &p.tab_w, &p.tab_i));
  // nothing is reduced, so the rows of a frame are split freely: enough blocks to fill the chip at few frames
  const int blocks_y = std::max(1, std::min(std::min(H, 64), 1024 / std::min(n_frames, 1024)));
  p.rows_per_block = (H + blocks_y - 1) / blocks_y;
  hipLaunchKernelGGL(spline_resize_kernel, dim3(n_frames, (H + p.rows_per_block - 1) / p.rows_per_block), dim3(kResizeThreads), 0, s, p);
  RGP_HIP(hipGetLastError());
  return RGP_OK;
}

}  // extern "C"
