// The metric layer under librgp_hip.so's two saliency scorers (rgp_metrics.hip: maps and fixations of one shape, pixel
// values in registers; rgp_metrics_scaled.hip: fixations at frame resolution, every pixel recomputed from spline
// coefficients).  Every rule of numpy's arithmetic that evaluation_metrics.py rests on is written down here once -- NaN
// ordering, np.minimum, Python's max(a, b), len(np.arange(0, top, step)), np.cov's 1 / (n - 1), corrcoef's clip, the
// Philox counter layout of the draws, Floyd's subset draw -- and the kernels hold only how a value is fetched.
// A file that includes this is compiled with -ffp-contract=off and without fast-math: the scores are a fixed sequence
// of IEEE operations.
#pragma once
#include <cmath>

#include "rgp_host.h"
#include "philox.hip.h"

namespace rgp {

constexpr int kStatusBytes = 64;   // head of the workspace: the count of refused frames (rgp_metrics_status)
enum { kDrawJudd = 0, kDrawBorji = 1, kDrawShuffled = 2 };

// what both kernels are told alike; each kernel's parameter struct derives from it
struct MetricsCommon {
  const void *pred, *gt;
  int n_frames;
  unsigned metrics, flags;
  int n_rep, neg_stride;
  double step_size;
  const double* judd_jitter;
  const int *borji_neg, *shuf_neg, *shuf_cnt;   // the caller's draws
  int *ws_borji, *ws_shuf, *ws_cnt;             // device draws: written, then read back by the same workgroup
  unsigned long long seed, offset;
  int* status;
  double* scores;
};

// numpy's order for floating point (sort, searchsorted): a < b, NaN after everything
__device__ __forceinline__ bool np_less(double a, double b) { return a < b || (b != b && a == a); }
// np.max / np.min of two (np.maximum / np.minimum): NaN propagates
__device__ __forceinline__ double np_max(double a, double b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }
__device__ __forceinline__ double np_min(double a, double b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }
__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// The block reductions.  The wave butterflies commute, so every lane of a wave holds the same bits; how the kWaves wave
// partials are combined is part of each kernel's reproducibility contract: four waves pair up, (s0 + s1) + (s2 + s3),
// any other count goes left to right in wave order.  sh: kWaves * K doubles (block_minmax: kWaves * 2).
template <int kWaves, int K>
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
    if constexpr (kWaves == 4) {
      v[k] = (sh[k] + sh[K + k]) + (sh[2 * K + k] + sh[3 * K + k]);
    } else {
      double s = sh[k];
      for (int wv = 1; wv < kWaves; ++wv) s += sh[wv * K + k];
      v[k] = s;
    }
  }
}

// np.min and np.max over the block (NaN propagates)
template <int kWaves>
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
  if constexpr (kWaves == 4) {
    mn = np_min(np_min(sh[0], sh[2]), np_min(sh[4], sh[6]));
    mx = np_max(np_max(sh[1], sh[3]), np_max(sh[5], sh[7]));
  } else {
    mn = sh[0]; mx = sh[1];
    for (int wv = 1; wv < kWaves; ++wv) { mn = np_min(mn, sh[wv * 2]); mx = np_max(mx, sh[wv * 2 + 1]); }
  }
}

// word `sample & 3` of the Philox block (sample / 4, rep, frame, metric)
__device__ __forceinline__ void draw_block(unsigned out[4], unsigned blk, unsigned rep, unsigned long long frame, int what,
                                           unsigned long long seed) {
  out[0] = blk; out[1] = rep; out[2] = (unsigned)frame; out[3] = ((unsigned)(frame >> 32) << 2) | (unsigned)what;
  philox4x32_10(out, (unsigned)seed, (unsigned)(seed >> 32));
}

// AUC_Judd's jitter of pixel `pix` with device draws: 53 random bits as numpy's random_sample makes a double of two words
__device__ __forceinline__ double judd_jitter_u(unsigned pix, unsigned long long frame, unsigned long long seed) {
  unsigned w[4];
  draw_block(w, pix >> 1, 0u, frame, kDrawJudd, seed);
  const unsigned hi = w[(pix & 1) * 2] >> 5, lo = w[(pix & 1) * 2 + 1] >> 6;
  return (double)(((unsigned long long)hi << 26) | lo) * (1.0 / 9007199254740992.0);
}

// ---- sim (:207-218), cc (:221-236) and what NSS needs, one sweep per dependent statement of the host.
// A sweep is a callable: sweep(f) calls f(g, r) once per pixel the thread owns, in a fixed order, with the ground-truth
// value and the normalised prediction as lvalues.  gsum, psum: the block sums of both over the map (each kernel's
// first pass).  kKeep: the sweep hands out the values it holds (registers), so the fourth pass leaves the standardised
// maps in them and the fifth takes them from there -- after the chain they are no longer the maps; without it every
// pass gets freshly computed values and the fifth standardises again.  The same operations in the same order either way.
struct ChainResult {
  double sim, cc;      // cc: NaN unless want_cc
  double mp, r1_sq;    // NSS: the prediction's mean, and the sum of (r - mean)^2
};

template <int kWaves, bool kKeep, class Sweep>
__device__ __forceinline__ ChainResult sim_cc_chain(Sweep&& sweep, double gsum, double psum, double dn, bool want_cc, double* sh) {
  const double mg = gsum / dn, mp = psum / dn;
  // sim; g - mean, r - mean (their sums, whether their max is > 0); NSS's variance of the prediction
  double s2[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  sweep([&](double g, double r) {
    s2[0] += np_min(g / gsum, r / psum);                            // np.minimum
    const double g1 = g - mg, r1 = r - mp;
    s2[1] += g1; s2[2] += r1;
    s2[3] += g1 > 0.0 ? 1.0 : 0.0; s2[4] += r1 > 0.0 ? 1.0 : 0.0;
    s2[5] += r1 * r1;
  });
  block_sum<kWaves>(s2, sh);
  ChainResult out = {s2[0], quiet_nan(), mp, s2[5]};
  if (!want_cc) return out;
  const double m2g = s2[1] / dn, m2r = s2[2] / dn;
  const bool pos_g = s2[3] > 0.0, pos_r = s2[4] > 0.0;
  double s3[2] = {0.0, 0.0};
  sweep([&](double g, double r) {
    const double a = (g - mg) - m2g, b = (r - mp) - m2r;
    s3[0] += a * a; s3[1] += b * b;
  });
  block_sum<kWaves>(s3, sh);
  const double sdg = sqrt(s3[0] / dn), sdr = sqrt(s3[1] / dn);
  auto standardised = [&](double& g, double& r) {   // the maps np.corrcoef is given
    g = g - mg; r = r - mp;
    if (pos_g) g = g / sdg;
    if (pos_r) r = r / sdr;
  };
  double s4[2] = {0.0, 0.0};
  sweep([&](double& g, double& r) {
    double zg = g, zr = r;
    standardised(zg, zr);
    if constexpr (kKeep) { g = zg; r = zr; }
    s4[0] += zg; s4[1] += zr;
  });
  block_sum<kWaves>(s4, sh);
  const double ag = s4[0] / dn, ar = s4[1] / dn;
  double s5[3] = {0.0, 0.0, 0.0};
  sweep([&](double g, double r) {
    if constexpr (!kKeep) standardised(g, r);
    const double xg = g - ag, xr = r - ar;
    s5[0] += xr * xr; s5[1] += xg * xg; s5[2] += xr * xg;
  });
  block_sum<kWaves>(s5, sh);
  const double f = 1.0 / (dn - 1.0);                                   // np.cov: c *= 1 / (n - ddof)
  const double c00 = s5[0] * f, c11 = s5[1] * f, c01 = s5[2] * f;
  const double c = (c01 / sqrt(c00)) / sqrt(c11);                      // np.corrcoef, then its clip to [-1, 1]
  out.cc = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
  return out;
}

// NSS from the prediction at the fixations (one thread)
__device__ __forceinline__ double nss_score(const double* fix_val, int n_fix, const ChainResult& c, double dn) {
  const double sd = sqrt(c.r1_sq / dn), den = sd > 0.0 ? sd : 1.0;
  double acc = 0.0;
  for (int k = 0; k < n_fix; ++k) acc += (fix_val[k] - c.mp) / den;
  return acc / (double)n_fix;
}

// ---- AUC_Judd (:42-98).  Thresholds = saliency at the fixations, descending (np.sort(...)[::-1]: NaN first): thread
// k < n_fix ranks fix_val[k] into thr; the caller syncs on both sides
__device__ __forceinline__ void judd_rank_thresholds(const double* fix_val, double* thr, int n_fix) {
  const int tid = threadIdx.x;
  if (tid >= n_fix) return;
  const double v = fix_val[tid];
  int rank = 0;
  for (int k = 0; k < n_fix; ++k) {
    const double w = fix_val[k];
    rank += (np_less(v, w) || (!np_less(w, v) && k < tid)) ? 1 : 0;
  }
  thr[rank] = v;
}

// the ROC area from cnt[k] = #(S < thr_k), searchsorted(sorted S, thr_k, 'left') (one thread)
__device__ __forceinline__ double judd_trapezoid(const int* cnt, int n_fix, int n_pix) {
  double ptp = 0.0, pfp = 0.0, acc = 0.0;
  for (int k = 1; k <= n_fix; ++k) {
    const double tp = (double)k / (double)n_fix;
    const double fp = (double)((n_pix - cnt[k - 1]) - k) / (double)(n_pix - n_fix);
    acc += (fp - pfp) * (tp + ptp) / 2.0;
    ptp = tp; pfp = fp;
  }
  acc += (1.0 - pfp) * (1.0 + ptp) / 2.0;
  return acc;
}

// ---- AUC_Borji (:101-164) and AUC_shuffled (:167-204): the draws of one repetition, and its ROC sweep.
// Borji: cnt pixel indices uniform over the map
__device__ __forceinline__ void draw_borji_row(int* wrow, int cnt, int n_pix, int rep, unsigned long long frame, unsigned long long seed) {
  for (int s = 0; s < cnt; s += 4) {
    unsigned w[4];
    draw_block(w, (unsigned)(s >> 2), (unsigned)rep, frame, kDrawBorji, seed);
    for (int q = 0; q < 4 && s + q < cnt; ++q) wrow[s + q] = (int)__umulhi(w[q], (unsigned)n_pix);
  }
}

// shuffled, Floyd: a uniform subset of cnt distinct members of the negative set member(0) .. member(n_other - 1)
template <class Member>
__device__ __forceinline__ void draw_floyd_row(int* wrow, int cnt, int n_other, int rep, unsigned long long frame, unsigned long long seed,
                                               Member&& member) {
  unsigned w[4] = {0u, 0u, 0u, 0u};
  for (int s = 0; s < cnt; ++s) {
    if ((s & 3) == 0) draw_block(w, (unsigned)(s >> 2), (unsigned)rep, frame, kDrawShuffled, seed);
    const int j = n_other - cnt + s;
    const int pick = member((int)__umulhi(w[s & 3], (unsigned)(j + 1)));
    bool taken = false;
    for (int q = 0; q < s; ++q) taken = taken || wrow[q] == pick;
    wrow[s] = taken ? member(j) : pick;
  }
}

__device__ __forceinline__ double np_max_of(const double* v, int n) {
  double m = v[0];
  for (int k = 1; k < n; ++k) m = np_max(m, v[k]);
  return m;
}

// one repetition: fix_val[0 .. n_fix) the saliency at the fixations (fix_max its np.max), neg_value(s), s < cnt, at the negatives
template <class Neg>
__device__ __forceinline__ double roc_auc(const double* fix_val, int n_fix, double fix_max, int cnt, double step_size, Neg&& neg_value) {
  // top = max(s_fix.max(), col.max()) as Python's max(a, b) evaluates it; col.max() of no sample: NaN
  double col_max = quiet_nan();
  for (int s = 0; s < cnt; ++s) {
    const double v = neg_value(s);
    col_max = s == 0 ? v : np_max(col_max, v);
  }
  const double top = col_max > fix_max ? col_max : fix_max;
  if (!(top == top && cnt > 0)) return quiet_nan();
  const int n_thr = (int)ceil(top / step_size);   // len(np.arange(0, top, step))
  const double dfix = (double)n_fix;
  double ptp = 0.0, pfp = 0.0, a = 0.0;
  for (int i = n_thr - 1; i >= 0; --i) {
    const double thr = (double)i * step_size;
    int lf = 0, lc = 0;
    for (int k = 0; k < n_fix; ++k) lf += np_less(fix_val[k], thr) ? 1 : 0;
    for (int s = 0; s < cnt; ++s) lc += np_less(neg_value(s), thr) ? 1 : 0;
    const double tp = (double)(n_fix - lf) / dfix, fp = (double)(n_fix - lc) / dfix;
    a += (fp - pfp) * (tp + ptp) / 2.0;
    ptp = tp; pfp = fp;
  }
  a += (1.0 - pfp) * (1.0 + ptp) / 2.0;
  return a;
}

// ---- the frame's column of the score table (one thread); a refused frame is counted and scores NaN
__device__ __forceinline__ void write_scores(const MetricsCommon& p, int n, bool bad, const double* score) {
  if (bad) atomicAdd(p.status, 1);
  for (int r = 0; r < RGP_METRICS_COUNT; ++r)
    if (p.metrics >> r & 1) p.scores[(long long)r * p.n_frames + n] = bad ? quiet_nan() : score[r];
}
__device__ __forceinline__ void refuse_frame(const MetricsCommon& p, int n) { write_scores(p, n, true, nullptr); }

// ---- host side: the fields rgp_metrics_args and rgp_metrics_scaled_args share
template <class Args>
inline int check_common_args(const char* fn, const Args* a, unsigned allowed_flags) {
  const unsigned M = a->metrics, F = a->flags;
  RGP_REQUIRE(M != 0 && (M & ~(unsigned)RGP_METRIC_ALL) == 0, "%s: metrics mask 0x%x: no or unknown metric bits", fn, M);
  RGP_REQUIRE((F & ~allowed_flags) == 0, "%s: unknown flags 0x%x", fn, F);
  RGP_REQUIRE(a->n_rep > 0, "%s: n_rep = %d must be positive", fn, a->n_rep);
  RGP_REQUIRE(a->step_size > 0.0 && 1.0 / a->step_size <= (double)RGP_METRICS_MAX_THRESHOLDS,
              "%s: step_size = %g must be positive and at least 1 / RGP_METRICS_MAX_THRESHOLDS", fn, a->step_size);
  RGP_REQUIRE(a->neg_stride > 0 && a->neg_stride <= RGP_METRICS_MAX_FIX,
              "%s: neg_stride = %d (fixations per frame) must be in [1, RGP_METRICS_MAX_FIX = %d]", fn, a->neg_stride, RGP_METRICS_MAX_FIX);
  RGP_REQUIRE(a->gt || !(M & (RGP_METRIC_SIM | RGP_METRIC_CC)), "%s: sim and cc need gt", fn);
  if (F & RGP_METRICS_DEVICE_DRAWS) {
    RGP_REQUIRE(!a->judd_jitter && !a->borji_neg && !a->shuf_neg && !a->shuf_cnt,
                "%s: RGP_METRICS_DEVICE_DRAWS takes no draws from the caller (the four pointers must be NULL)", fn);
  } else {
    RGP_REQUIRE(!(F & RGP_METRICS_NO_JITTER), "%s: with the caller's draws a NULL judd_jitter means no jitter", fn);
    RGP_REQUIRE(a->borji_neg || !(M & RGP_METRIC_AUC_BORJI), "%s: AUC_Borji with the caller's draws needs borji_neg", fn);
    RGP_REQUIRE((a->shuf_neg && a->shuf_cnt) || !(M & RGP_METRIC_AUC_SHUFFLED),
                "%s: AUC_shuffled with the caller's draws needs shuf_neg and shuf_cnt", fn);
  }
  return RGP_OK;
}

inline int check_workspace(const char* fn, const void* ws, size_t have, size_t need) {
  if (!ws || have < need || ((size_t)ws & 7) != 0)
    return set_err(RGP_EWORKSPACE, "%s: workspace missing, misaligned or too small (%zu < %zu bytes)", fn, ws ? have : (size_t)0, need);
  return RGP_OK;
}

inline size_t draws_elems(int n_frames, int n_rep, int neg_stride) { return (size_t)n_frames * (size_t)n_rep * (size_t)neg_stride; }

// head of both workspaces: the status word, then (device draws) ws_borji, ws_shuf [n_frames, n_rep, neg_stride] and
// ws_cnt [n_frames] as int.  -> the offset behind them (not aligned)
inline size_t draws_layout_bytes(int n_frames, int n_rep, int neg_stride, unsigned flags) {
  size_t b = kStatusBytes;
  if (flags & RGP_METRICS_DEVICE_DRAWS) b += (2 * draws_elems(n_frames, n_rep, neg_stride) + (size_t)n_frames) * sizeof(int);
  return b;
}

// the shared kernel parameters from the checked arguments, the workspace's head laid out; -> draws_layout_bytes
template <class Args>
inline size_t fill_common(MetricsCommon& p, const Args* a) {
  p.pred = a->pred; p.gt = a->gt;
  p.n_frames = a->n_frames; p.metrics = a->metrics; p.flags = a->flags;
  p.n_rep = a->n_rep; p.neg_stride = a->neg_stride; p.step_size = a->step_size;
  p.judd_jitter = a->judd_jitter; p.borji_neg = a->borji_neg; p.shuf_neg = a->shuf_neg; p.shuf_cnt = a->shuf_cnt;
  p.seed = a->seed; p.offset = a->offset;
  p.status = (int*)a->workspace;
  p.scores = a->scores;
  p.ws_borji = p.ws_shuf = p.ws_cnt = nullptr;
  if (a->flags & RGP_METRICS_DEVICE_DRAWS) {
    const size_t e = draws_elems(a->n_frames, a->n_rep, a->neg_stride);
    p.ws_borji = (int*)((char*)a->workspace + kStatusBytes);
    p.ws_shuf = p.ws_borji + e;
    p.ws_cnt = p.ws_shuf + e;
  }
  return draws_layout_bytes(a->n_frames, a->n_rep, a->neg_stride, a->flags);
}

}  // namespace rgp
