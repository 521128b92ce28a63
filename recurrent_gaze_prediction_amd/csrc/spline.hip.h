// The order-3 spline resize shared by librgp_hip.so's kernels (rgp_metrics_scaled.hip, rgp_overlay.hip): scipy's recursive
// prefilter and the 16-tap evaluation as device functions, and the host side that makes the prefilter constants and the
// per-axis tables in float64.  tests/spline_ref.py restates the arithmetic.  A file that includes this is compiled with
// -ffp-contract=off: the values are a fixed sequence of multiplies and adds.
#pragma once
#include <cmath>
#include <vector>

#include "rgp_host.h"

namespace rgp {

// constants of the order-3 prefilter, made on the host in float64 (axis 0: lines of h samples, axis 1: of w)
struct SplineConsts {
  double z, gain, last;   // the pole sqrt(3) - 2; (1 - z)(1 - 1/z); z / (z - 1)
  double zn[2], k0[2];    // z^n by repeated multiplication; z / (1 - z^n z^n)
};

// scipy's spline_filter1d (order 3, mode 'reflect') on the n samples c[0], c[stride], ...: gain, exact causal
// initialisation, forward and backward recursion.  tests/spline_ref.py restates this statement for statement.
__device__ __forceinline__ void filter_line(double* c, int n, int stride, double z, double zn, double gain, double k0, double last) {
  for (int i = 0; i < n; ++i) c[i * stride] = c[i * stride] * gain;
  const double c0 = c[0];
  double acc = c0 + zn * c[(n - 1) * stride];
  double zi = z;
  for (int i = 1; i < n; ++i) {   // scipy accumulates in c[0] itself: the last term's mirrored sample is the running value
    const double mirrored = i == n - 1 ? acc : c[(n - 1 - i) * stride];
    acc = acc + zi * (c[i * stride] + zn * mirrored);
    zi = zi * z;
  }
  acc = acc * k0;
  acc = acc + c0;
  c[0] = acc;
  for (int i = 1; i < n; ++i) c[i * stride] = c[i * stride] + z * c[(i - 1) * stride];
  c[(n - 1) * stride] = c[(n - 1) * stride] * last;
  for (int i = n - 2; i >= 0; --i) c[i * stride] = z * (c[(i + 1) * stride] - c[i * stride]);
}

struct Taps {
  double wy[4], wx[4];
  int ry[4], cx[4];
};

__device__ __forceinline__ void load_taps(Taps& t, const double* tw, const unsigned short* ti, int H, int Y, int X) {
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    t.wy[a] = tw[Y * 4 + a];
    t.ry[a] = ti[Y * 4 + a];
    t.wx[a] = tw[(H + X) * 4 + a];
    t.cx[a] = ti[(H + X) * 4 + a];
  }
}

// one source row's four column taps, summed left to right: s = wx0 c + wx1 c + wx2 c + wx3 c.  It depends on the source
// row and the target column alone, so a kernel may keep it (rgp_overlay.hip) instead of forming it again per target row
template <class W4, class I4>
__device__ __forceinline__ double spline_row_sum(const double* r, const W4& wx, const I4& cx) {
  double s = wx[0] * r[cx[0]];
  s = s + wx[1] * r[cx[1]];
  s = s + wx[2] * r[cx[2]];
  s = s + wx[3] * r[cx[3]];
  return s;
}

// the resized value: rows outer, v = wy0 s0 + wy1 s1 + wy2 s2 + wy3 s3 with s_a the row sums above
__device__ __forceinline__ double spline_at(const double* C, const Taps& t) {
  double v = 0.0;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const double s = spline_row_sum(C + t.ry[a], t.wx, t.cx);
    v = a == 0 ? t.wy[0] * s : v + t.wy[a] * s;
  }
  return v;
}

inline size_t spline_tables_bytes(int H, int W) { return align_up((size_t)(H + W) * 4 * (sizeof(double) + sizeof(unsigned short)), 64); }

// z^n as n - 1 multiplies: the device's and libm's pow are not numpy's, a product is the same everywhere
inline double pow_by_products(double z, int n) {
  double v = z;
  for (int i = 1; i < n; ++i) v = v * z;
  return v;
}

inline SplineConsts spline_consts(int h, int w) {
  SplineConsts c;
  c.z = std::sqrt(3.0) - 2.0;
  c.gain = (1.0 - c.z) * (1.0 - 1.0 / c.z);
  c.last = c.z / (c.z - 1.0);
  const int n[2] = {h, w};
  for (int a = 0; a < 2; ++a) {
    c.zn[a] = pow_by_products(c.z, n[a]);
    c.k0[a] = c.z / (1.0 - c.zn[a] * c.zn[a]);
  }
  return c;
}

// weights and reflected indices of one axis (n_in samples -> n_out), appended; the indices times `scale`
inline void axis_table(int n_in, int n_out, int scale, std::vector<double>& tw, std::vector<unsigned short>& ti) {
  for (int o = 0; o < n_out; ++o) {
    const double x = ((double)o + 0.5) * ((double)n_in / (double)n_out) - 0.5;
    const double f = std::floor(x), t = x - f, u = 1.0 - t;
    tw.push_back(u * u * u / 6.0);
    tw.push_back((t * t * (t - 2.0) * 3.0 + 4.0) / 6.0);
    tw.push_back((u * u * (u - 2.0) * 3.0 + 4.0) / 6.0);
    tw.push_back(t * t * t / 6.0);
    for (int k = -1; k <= 2; ++k) {
      long long i = (long long)f + k;
      if (i < 0) i = -i - 1;
      i %= 2 * (long long)n_in;
      if (i >= n_in) i = 2 * (long long)n_in - 1 - i;
      ti.push_back((unsigned short)(i * scale));
    }
  }
}

// both axes' tables into `dst` (device, tables_bytes): weights [H + W][4] fp64, then indices [H + W][4] uint16
inline int upload_tables(int h, int w, int H, int W, void* dst, hipStream_t s, const double** tab_w, const unsigned short** tab_i) {
  // kept per host thread and rebuilt only when the shapes change: an asynchronous copy out of pageable memory may still
  // be reading them, so they are rewritten only behind a wait for the stream
  thread_local std::vector<double> tw;
  thread_local std::vector<unsigned short> ti;
  thread_local int key[4] = {0, 0, 0, 0};
  if (key[0] != h || key[1] != w || key[2] != H || key[3] != W) {
    RGP_HIP(hipStreamSynchronize(s));
    tw.clear(); ti.clear();
    axis_table(h, H, w, tw, ti);
    axis_table(w, W, 1, tw, ti);
    key[0] = h; key[1] = w; key[2] = H; key[3] = W;
  }
  char* d = (char*)dst;
  RGP_HIP(hipMemcpyAsync(d, tw.data(), tw.size() * sizeof(double), hipMemcpyHostToDevice, s));
  RGP_HIP(hipMemcpyAsync(d + tw.size() * sizeof(double), ti.data(), ti.size() * sizeof(unsigned short), hipMemcpyHostToDevice, s));
  *tab_w = (const double*)d;
  *tab_i = (const unsigned short*)(d + tw.size() * sizeof(double));
  return RGP_OK;
}

}  // namespace rgp
