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
// threads take 177 VGPRs, no scratch, two waves per SIMD behind which the LDS latency of the sweeps hides
// (profiles/metrics_scaled_kernel_resources.txt).
//
// Exactness.  Compiled with -ffp-contract=off, no fast-math, IEEE division.  The resized VALUES are a fixed sequence
// of multiplies and adds (filter_line, spline_at in spline.hip.h; tests/spline_ref.py restates them), so they are reproducible
// bit for bit; normalisations, jitter and comparisons are element-wise, counts are integers, and what is left against
// the host is the order of the sums (H W 2^-53).  The order of every sum is fixed by (H, W) alone.
// The metrics' arithmetic -- numpy's rules, the chains, the draws -- is in metrics_shared.hip.h, shared with
// rgp_metrics.hip; this file holds the table staging, the prefilter, the point lists, the sweeps over the target grid
// (for_pixels), AUC_Judd's histogram count and the staging of the negatives' values (ws_val).
#include <cmath>
#include <vector>

#include "metrics_shared.hip.h"
#include "spline.hip.h"

using namespace rgp;

namespace {

constexpr int kThreads = 512, kWaves = kThreads / 64;
constexpr int kMaxSrc = RGP_METRICS_MAX_PIX;
constexpr int kMaxFix = RGP_METRICS_MAX_FIX;
constexpr int kMaxOther = RGP_METRICS_SCALED_MAX_OTHER;
constexpr int kSrcPerThread = kMaxSrc / kThreads;
constexpr int kTabLds = 1536;   // H + W up to which the per-axis tables live in LDS
constexpr int kResizeThreads = 256;

struct ScaledParams : MetricsCommon {
  const int *fix_ptr, *fix_idx, *other_ptr, *other_idx;
  int fix_len, other_len;
  int h, w, H, W;
  double* ws_val;                               // [2][n_frames, n_rep, neg_stride]: normalised saliency at the negatives
  const double* tab_w;                          // [H + W][4] weights, rows first
  const unsigned short* tab_i;                  // [H + W][4] reflected source index (rows: times w)
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
    block_minmax<kWaves>(mn, mx, sRed);
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
    if (tid == 0) refuse_frame(p, n);
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
    block_sum<kWaves>(s1, sRed);
    block_minmax<kWaves>(mn, mx, sRed);
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
    auto sweep = [&](auto&& f) {   // the thread's pixels, both maps recomputed from the coefficients
      for_pixels(H, W, [&](int, int Y, int X) {
        Taps t;
        load_taps(t, tw, ti, H, Y, X);
        double r = spline_at(sCp, t), g = want_gt ? spline_at(sCg, t) : 0.0;
        f(g, r);
      });
    };
    const ChainResult c = sim_cc_chain<kWaves, false>(sweep, gsum, psum, dn, (M & RGP_METRIC_CC) != 0, sRed);
    score[RGP_METRIC_ROW_SIM] = c.sim;
    score[RGP_METRIC_ROW_CC] = c.cc;
    if ((M & RGP_METRIC_NSS) && n_fix > 0 && tid == 0) score[RGP_METRIC_ROW_NSS] = nss_score(sFixRaw, n_fix, c, dn);
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
        const double u = device_draws ? judd_jitter_u((unsigned)pix, frame, p.seed) : p.judd_jitter[jo + pix];
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
    block_minmax<kWaves>(mn, mx, sRed);
    const double den = mx - mn;
    if (tid < n_fix) sFixJ[tid] = (jittered(sFixPix[tid], sFixPix[tid] / W, sFixPix[tid] % W) - mn) / den;
    if (tid <= n_fix) sHist[tid] = 0;
    __syncthreads();
    judd_rank_thresholds(sFixJ, sThr, n_fix);
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
      score[RGP_METRIC_ROW_AUC_JUDD] = judd_trapezoid(sCnt, n_fix, n_pix);
    }
  }

  // ---- AUC_Borji (:101-164) and AUC_shuffled (:167-204): the same sweep over two kinds of negatives
  if ((M & (RGP_METRIC_AUC_BORJI | RGP_METRIC_AUC_SHUFFLED)) && n_fix > 0) {
    const long long E = (long long)p.n_frames * p.n_rep * p.neg_stride;
    const long long frame_off = (long long)n * p.n_rep * p.neg_stride;
    if (tid == 0) sFixMax = np_max_of(sFixP, n_fix);
    // 1. device draws: one thread per (metric, repetition) leaves the indices in the workspace
    if (device_draws)
      for (int item = tid; item < 2 * p.n_rep; item += kThreads) {
        const int which = item >= p.n_rep ? 1 : 0, rep = item - which * p.n_rep;
        if (!(M & (which ? RGP_METRIC_AUC_SHUFFLED : RGP_METRIC_AUC_BORJI))) continue;
        int* wrow = (which ? p.ws_shuf : p.ws_borji) + frame_off + (long long)rep * p.neg_stride;
        if (!which) draw_borji_row(wrow, n_fix, n_pix, rep, frame, p.seed);
        else draw_floyd_row(wrow, cnt_shuf, n_other, rep, frame, p.seed, [&](int i) { return p.other_idx[o_base + i]; });
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
    const double fix_max = sFixMax;
    double auc[2] = {0.0, 0.0};
    for (int item = tid; item < 2 * p.n_rep; item += kThreads) {
      const int which = item >= p.n_rep ? 1 : 0, rep = item - which * p.n_rep;
      if (!(M & (which ? RGP_METRIC_AUC_SHUFFLED : RGP_METRIC_AUC_BORJI))) continue;
      const double* vals = p.ws_val + which * E + frame_off + (long long)rep * p.neg_stride;
      auc[which] += roc_auc(sFixP, n_fix, fix_max, which ? cnt_shuf : n_fix, p.step_size, [&](int s) { return vals[s]; });
    }
    block_sum<kWaves>(auc, sRed);
    score[RGP_METRIC_ROW_AUC_BORJI] = auc[0] / (double)p.n_rep;
    score[RGP_METRIC_ROW_AUC_SHUFFLED] = auc[1] / (double)p.n_rep;
  }

  __syncthreads();
  if (tid == 0) write_scores(p, n, sBad != 0, score);
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
  const size_t b = align_up(draws_layout_bytes(n_frames, n_rep, neg_stride, flags), 64) + 2 * draws_elems(n_frames, n_rep, neg_stride) * sizeof(double);
  return align_up(b, 64) + spline_tables_bytes(height, width);
}

size_t rgp_spline_resize_workspace_bytes(int H, int W) { return H <= 0 || W <= 0 ? 0 : spline_tables_bytes(H, W); }

int rgp_saliency_scores_scaled(const rgp_metrics_scaled_args* a, rgp_stream_t stream) {
  const char* fn = "rgp_saliency_scores_scaled";
  RGP_REQUIRE(a != nullptr, "%s: args is NULL", fn);
  RGP_REQUIRE(a->n_frames > 0, "%s: n_frames = %d must be positive", fn, a->n_frames);
  RGP_TRY(check_shapes(fn, a->height, a->width, a->target_height, a->target_width));
  RGP_TRY(check_common_args(fn, a, RGP_METRICS_DEVICE_DRAWS | RGP_METRICS_NO_JITTER | RGP_METRICS_PRED_F64 | RGP_METRICS_GT_F64 |
                                       RGP_METRICS_SCALED_OTHER_SHARED));
  RGP_REQUIRE(a->pred && a->fix_ptr && a->fix_idx && a->scores, "%s: pred, fix_ptr, fix_idx and scores must not be NULL", fn);
  RGP_REQUIRE(a->fix_len >= 0 && a->other_len >= 0, "%s: fix_len = %d and other_len = %d must not be negative", fn, a->fix_len, a->other_len);
  RGP_REQUIRE((a->other_ptr == nullptr) == (a->other_idx == nullptr), "%s: other_ptr and other_idx go together", fn);
  RGP_REQUIRE(a->other_ptr || !(a->flags & RGP_METRICS_DEVICE_DRAWS) || !(a->metrics & RGP_METRIC_AUC_SHUFFLED),
              "%s: AUC_shuffled with device draws needs the negative set other_ptr / other_idx", fn);
  const int H = a->target_height, W = a->target_width;
  RGP_TRY(check_workspace(fn, a->workspace, a->workspace_bytes,
                          rgp_metrics_scaled_workspace_bytes(a->n_frames, a->n_rep, a->neg_stride, H, W, a->flags)));

  ScaledParams p{};
  char* ws = (char*)a->workspace;
  size_t off = align_up(fill_common(p, a), 64);
  p.fix_ptr = a->fix_ptr; p.fix_idx = a->fix_idx; p.other_ptr = a->other_ptr; p.other_idx = a->other_idx;
  p.fix_len = a->fix_len; p.other_len = a->other_len;
  p.h = a->height; p.w = a->width; p.H = H; p.W = W;
  p.sc = spline_consts(a->height, a->width);
  p.ws_val = (double*)(ws + off);
  off = align_up(off + 2 * draws_elems(a->n_frames, a->n_rep, a->neg_stride) * sizeof(double), 64);
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
  RGP_TRY(check_workspace(fn, workspace, workspace_bytes, rgp_spline_resize_workspace_bytes(H, W)));
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
