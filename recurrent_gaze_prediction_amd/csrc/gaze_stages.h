// Host layer shared by the three gaze-family plans (rgp_grcn*.hip, rgp_c3dconv.hip, rgp_lstm.hip): everything around what
// sits between the projection and the up-sampling head.  Each stage is a plain struct of descriptors and workspace buffers
// plus launches that take the workspace, their operands and the stream explicitly: a stage knows no plan and picks no
// stream, so a plan may run it on a side stream, inside its profiler brackets or between its fork / join events.
//
//   Projection      E = X W + b from NCHW features (via xt) or from conv5b rows (K order d*512+c; reference channel c*2+d)
//   ProjectionBwd   d rows = dE W^T; and the atomics-free d W, d b of gaze_lstm / gaze_c3d_conv (below)
//   FoldedHead      head_fold.hip.h: G -> H -> K at set-weights, Z = A K^T, col2im (+ out_b)
//   FoldedHeadBwd   d loss / d logits, d out_b, the patches Pm of dz, the chain rule through the fold, dA = Pm K
//
// What stays with a model: its gather / scatter tables (padded 9x9 or plain 49-row E; frame images, E rows or clip images
// under the head), the order in which it takes its buffers from the arena (= its workspace layout), which packs share a
// launch, and dK = Pm^T A (a strided atomics wgrad in gaze_grcn and gaze_lstm, a GEMM in gaze_c3d_conv).
//
// GEMM-form filter gradients (no float atomics: two backward calls on the same inputs give the same bits).  A reduction
// over the M = frames x 49 rows, out[r][n] = sum_m A[m][r] B[m][n], runs as a plain GEMM on transposed copies of its
// operands -- AT [rows][Mp], BT [N][Mp] (BT lives in the descriptor's filter area), Mp = M rounded up to 64, zero padded --
// with the igemm kernel, K = Mp split over blockIdx.y: every split STORES its partial sum into a slice of its own
// (EpiStoreSplitF32) and head_fold_sum_kernel adds the slices in a fixed order.
#pragma once
#include <algorithm>

#include "bwd_kernels.hip.h"
#include "head_fold.hip.h"
#include "rgp_host.h"

struct Buf {
  size_t off = 0, bytes = 0;
};

inline Buf take(rgp::Arena& a, size_t bytes) {
  Buf b;
  b.bytes = bytes;
  b.off = a.take(bytes);
  return b;
}

namespace rgp {

// host side: add() regions, flush() = one launch (or a plain memset for a single region)
struct ZeroBatch {
  ZeroTable t;
  hipStream_t s;
  explicit ZeroBatch(hipStream_t stream) : s(stream) { t.n = 0; t.first[0] = 0; }
  int add(void* p, size_t bytes) {
    if (bytes == 0) return RGP_OK;
    if ((bytes & 3) || (((size_t)p) & 3)) return set_err(RGP_EINVAL, "ZeroBatch: region not 4-byte aligned");
    if (t.n == ZERO_MAX_REGIONS) RGP_TRY(flush());
    t.ptr[t.n] = p; t.bytes[t.n] = bytes;
    t.first[t.n + 1] = t.first[t.n] + (int)((bytes + ZERO_BLOCK_BYTES - 1) / ZERO_BLOCK_BYTES);
    ++t.n;
    return RGP_OK;
  }
  int flush() {
    if (t.n == 1) RGP_HIP(hipMemsetAsync(t.ptr[0], 0, t.bytes[0], s));
    else if (t.n > 1) {
      zero_regions_kernel<<<t.first[t.n], 256, 0, s>>>(t);
      RGP_HIP(hipGetLastError());
    }
    t.n = 0; t.first[0] = 0;
    return RGP_OK;
  }
};

// ---- C ABI helpers of the three plans (the error texts are part of the ABI: tests match some of them)

// f<bf16_t>(...) or f<float>(...) by a plan's operand dtype
#define RGP_BY_DTYPE(dtype, f, ...) ((dtype) == RGP_BF16 ? f<bf16_t>(__VA_ARGS__) : f<float>(__VA_ARGS__))

// every pointer of a weights struct (all `const float*`) is set; kind: "weight" / "gradient"
template <class W>
int require_pointers(const W* w, const char* fn, const char* kind) {
  const float* const* ptrs = (const float* const*)w;
  for (size_t i = 0; i < sizeof(W) / sizeof(float*); ++i) RGP_REQUIRE(ptrs[i], "%s: %s pointer %zu is null", fn, kind, i);
  return RGP_OK;
}

template <class Plan>
int check_bind(const char* fn, const Plan* g, const void* workspace, size_t bytes) {
  RGP_REQUIRE(g && workspace, "%s: null argument", fn);
  if (bytes < g->ws_bytes) return set_err(RGP_EWORKSPACE, "workspace %zu < required %zu bytes", bytes, g->ws_bytes);
  RGP_REQUIRE(((size_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
  return RGP_OK;
}

template <class Plan>
int check_bound_and_set(const Plan* g, const char* name) {
  if (!g) return set_err(RGP_EINVAL, "null plan");
  if (!g->ws) return set_err(RGP_EWORKSPACE, "%s: workspace not bound", name);
  if (!g->weights_set) return set_err(RGP_ESTATE, "%s: weights not set", name);
  return RGP_OK;
}

// ---- projection

struct Projection {
  ConvDesc proj, proj_rows;                // from xt (K = channel) / from conv5b rows (K order d*512+c)
  Buf xt;                                  // [F*49][1024] operand dtype, reference channel order: taken by the plan
  // out_tab: where the 49 rows of a frame land in E (plain rows, or the interior of a halo-padded 9x9 image)
  bool plan(int P, int dtype, const std::vector<int>& out_tab, long long out_img_stride) {
    for (ConvDesc* d : {&proj, &proj_rows}) {
      d->Mw = 49; d->N = P;
      d->in_img_stride = 49LL * 1024; d->out_img_stride = out_img_stride;
      for (int p = 0; p < 49; ++p) d->in_tab.push_back(p * 1024);
      d->out_tab = out_tab;
    }
    bool ok = build_k_schedule(proj, {0}, {0}, 1024, dtype);
    proj.s_tap = 0; proj.s_n = 1; proj.s_c = P;
    ok &= build_k_schedule(proj_rows, {0, 512}, {0, 1}, 512, dtype);
    proj_rows.s_tap = P; proj_rows.s_n = 1; proj_rows.s_c = 2LL * P;
    return ok;
  }
  template <typename T>
  int pack(PackBatch<T>& pk, const float* W) {
    RGP_TRY(pk.add(proj, W, proj.N, 0));
    return pk.add(proj_rows, W, proj.N, 0);
  }
  // exactly one of c3d_input [F][1024][7][7] fp32 / rows is set.  keep_xt (training plans): rows are also copied to xt in
  // the reference's channel order, which the projection's filter gradient reads (gaze_rnn.py:494-497)
  template <typename T>
  int forward(char* ws, const float* c3d_input, const void* rows, bool keep_xt, int F, void* E, const float* bias, hipStream_t s) {
    const void* A = rows;
    if (!rows) {
      nchw_to_rows_kernel<T><<<dim3(1024 / 64, F), 256, 0, s>>>(c3d_input, (T*)(ws + xt.off), 1024);
      RGP_HIP(hipGetLastError());
      A = ws + xt.off;
    } else if (keep_xt) {
      const long long total = (long long)F * 49 * 1024;
      rows_to_xt_kernel<T><<<(int)std::min<long long>((total + 255) / 256, 8192), 256, 0, s>>>((const T*)rows, (T*)(ws + xt.off), total);
      RGP_HIP(hipGetLastError());
    }
    const ConvDesc& d = rows ? proj_rows : proj;
    IgemmParams p = make_params(d, A, ws, F);
    EpiParams e = make_epi(d, E, ws);
    e.bias = bias;
    return launch_igemm<T, 1, 1, EpiStore<T, true, false>>(p, e, s);
  }
};

// ---- GEMM-form filter gradients (the comment at the top of the file)

// out[blockIdx.y][row][n0 .. n0+7] = acc: the partial sum of K-split blockIdx.y (e.xpre_img_stride: elements per slice)
struct EpiStoreSplitF32 {
  static __device__ __forceinline__ void apply(const EpiParams& e, int N, int img, int ml, int n0, float* v) {
    apply_at(e, N, img, ml, epi_out_base(e, img, ml), n0, v);
  }
  static __device__ __forceinline__ void apply_at(const EpiParams& e, int N, int, int, long long base, int n0, float* v) {
    const int nvalid = N - n0;
    if (nvalid <= 0) return;
    store8<float>((float*)e.out + (long long)blockIdx.y * e.xpre_img_stride + base + n0, v, nvalid);
  }
};

// dst[c][m] = src[m][c] for m < M, 0 for M <= m < Mp   (src [M][C], dst [C][Mp]; C and Mp multiples of 64)
// grid (Mp / 64, C / 64), 256 threads
template <typename T>
static __global__ __launch_bounds__(256) void transpose_pad_kernel(const T* __restrict__ src, T* __restrict__ dst, long long M, int C,
                                                                   long long Mp) {
  __shared__ T tile[64][65];
  const long long m0 = (long long)blockIdx.x * 64;
  const int c0 = blockIdx.y * 64;
  for (int i = threadIdx.x; i < 4096; i += 256) {
    const int r = i >> 6, c = i & 63;
    tile[r][c] = (m0 + r < M) ? src[(m0 + r) * C + c0 + c] : (T)0;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 4096; i += 256) {
    const int c = i >> 6, r = i & 63;
    dst[(long long)(c0 + c) * Mp + m0 + r] = tile[r][c];
  }
}

template <typename T>
void transpose_pad(const T* src, T* dst, long long M, int C, long long Mp, hipStream_t s) {
  transpose_pad_kernel<T><<<dim3((unsigned)(Mp / 64), C / 64), 256, 0, s>>>(src, dst, M, C, Mp);
}

// out [rows][N] = AT [rows][Mp] x BT [N][Mp]^T
inline bool wgrad_gemm_desc(ConvDesc& d, int rows, int N, long long Mp, int dtype) {
  d.Mw = rows; d.N = N; d.in_img_stride = 0; d.out_img_stride = 0;
  for (int r = 0; r < rows; ++r) { d.in_tab.push_back((int)(r * Mp)); d.out_tab.push_back(r * N); }
  return build_k_schedule(d, {0}, {0}, (int)Mp, dtype);
}

// one filter gradient: K = Mp split ksplit ways into `part` ([ksplit][d.Mw][d.N] fp32), summed in a fixed order into `out`
template <typename T>
int wgrad_gemm(char* ws, const ConvDesc& d, const void* AT, const Buf& part, int ksplit, float* out, hipStream_t s) {
  IgemmParams p = make_params(d, AT, ws, 1);
  EpiParams e = make_epi(d, ws + part.off, ws);
  const long long n = (long long)d.Mw * d.N;
  e.xpre_img_stride = n;
  RGP_TRY((launch_igemm<T, 1, 1, EpiStoreSplitF32>(p, e, s, ksplit)));
  head_fold_sum_kernel<<<(int)((n + 255) / 256), 256, 0, s>>>((const float*)(ws + part.off), out, (int)n, ksplit);
  RGP_HIP(hipGetLastError());
  return RGP_OK;
}

struct ProjectionBwd {
  int P = 0;
  ConvDesc b_px;                           // d rows[m][d*512+c] = sum_p dE[m][p] W[c*2+d][p]   (rows order of rgp_c3d_forward)
  // GEMM-form d proj_c3d_W = X^T dE and d proj_c3d_b = colsum(dE) (gaze_lstm, gaze_c3d_conv; gaze_grcn: its atomics wgrad)
  long long M = 0, Mp = 0;                 // rows = frames x 49, rounded up to 64
  int ksplit = 1;
  ConvDesc wg_w;                           // its "filter" area holds dET [P padded to 128][Mp]
  Buf xT, part;                            // XT [1024][Mp] operand dtype; [ksplit][1024][P] fp32: taken by the plan
  bool plan(int P_, int dtype) {
    P = P_;
    b_px.Mw = 1; b_px.N = 1024; b_px.in_img_stride = P; b_px.out_img_stride = 1024; b_px.in_tab = {0}; b_px.out_tab = {0};
    const bool ok = build_k_schedule(b_px, {0}, {0}, P, dtype);
    b_px.s_tap = 0; b_px.s_n = 2LL * P; b_px.s_c = 1;
    return ok;
  }
  // false: F too large (the transposed operands are indexed with ints)
  bool plan_wgrad(int F, int dtype) {
    M = (long long)F * 49;
    Mp = (M + 63) / 64 * 64;
    ksplit = std::min(16, (int)(Mp / bke(dtype)));
    return Mp * 1024 < (1LL << 31) && wgrad_gemm_desc(wg_w, 1024, P, Mp, dtype);
  }
  size_t xT_bytes(int dtype) const { return (size_t)1024 * Mp * esize(dtype); }
  size_t part_bytes() const { return (size_t)ksplit * 1024 * P * 4; }
  template <typename T>
  int pack(PackBatch<T>& pk, const float* W) {
    RGP_TRY(pk.add(b_px, W, 512, 0));                          // d = 0: feature channels 0, 2, 4, ...
    return pk.add(b_px, W + P, 512, 512);                      // d = 1: feature channels 1, 3, 5, ...
  }
  // dE [n_rows][P] operand dtype -> d_rows [n_rows][1024] fp32
  int backward_input(char* ws, int dtype, const void* dE, long long n_rows, float* d_rows, hipStream_t s) const {
    IgemmParams p = make_params(b_px, dE, ws, (int)n_rows);
    EpiParams e = make_epi(b_px, d_rows, ws);
    return dtype == RGP_BF16 ? launch_igemm<bf16_t, 1, 1, EpiStore<float, false, false>>(p, e, s)
                             : launch_igemm<float, 1, 1, EpiStore<float, false, false>>(p, e, s);
  }
  // xt [M][1024], dE [M][P] -> dW [1024][P], db [P] (= row sums of dE^T: one block per column, fixed tree)
  template <typename T>
  int weight_grads(char* ws, const T* xt, const T* dE, float* dW, float* db, hipStream_t s) {
    T* deT = (T*)(ws + wg_w.w_off);
    transpose_pad<T>(dE, deT, M, P, Mp, s);
    transpose_pad<T>(xt, (T*)(ws + xT.off), M, 1024, Mp, s);
    RGP_HIP(hipGetLastError());
    RGP_TRY(wgrad_gemm<T>(ws, wg_w, ws + xT.off, part, ksplit, dW, s));
    rowsum_kernel<T><<<P, 256, 0, s>>>(deT, db, Mp, M);
    RGP_HIP(hipGetLastError());
    return RGP_OK;
  }
};

// ---- folded head (head_fold.hip.h) on A with C channels: the head as one 19x19 stride-6 transposed convolution

struct FoldedHead {
  int C = 0;
  ConvDesc hfold;                          // Z = A K^T: K = C, N = the 19x19 taps; Mw, tables and strides by the model
  // G [49][32] (+ slack), H [11,11,64], K [k_rows][C] and K's five partial sums, fp32; Z [F*49][384] fp32: taken by the plan
  Buf gfold, hf_h, hf_k, hf_part, hf_z;
  static constexpr size_t G_BYTES = 50 * 32 * 4, H_BYTES = (size_t)HF_HP * HF_HP * 64 * 4;
  // k_rows: HF_KP * HF_KP, or HF_PK (rows 361 .. 383 stay zero)
  size_t k_bytes(int k_rows) const { return (size_t)k_rows * C * 4; }
  size_t part_bytes() const { return (size_t)5 * HF_KP * HF_KP * C * 4; }
  static size_t z_bytes(int F) { return (size_t)F * 49 * HF_PK * 4; }
  const float* k(const char* ws) const { return (const float*)(ws + hf_k.off); }
  // after the model has set hfold's Mw, in_tab / out_tab and image strides
  bool plan(int C_, int dtype) {
    C = C_;
    hfold.N = HF_PK;
    const bool ok = build_k_schedule(hfold, {0}, {0}, C, dtype);
    hfold.s_tap = 0; hfold.s_n = C; hfold.s_c = 1;             // source K [(r,t)][s]
    return ok;
  }
  // G = weight3 o out_W -> H = G o weight2 -> K = H o weight1 (four dependent launches)
  int fold(char* ws, const float* w3, const float* out_W, const float* w2, const float* w1, hipStream_t s) {
    float* gf = (float*)(ws + gfold.off);
    float* hf = (float*)(ws + hf_h.off);
    float* part = (float*)(ws + hf_part.off);
    fold_head_filter_kernel<<<(49 * 32 + 255) / 256, 256, 0, s>>>(w3, out_W, gf, 49, 12, 32);
    head_fold_h_kernel<<<(HF_HP * HF_HP * 64 + 255) / 256, 256, 0, s>>>(gf, w2, hf);
    head_fold_k_kernel<<<dim3(HF_KP * HF_KP, 5), 128, 0, s>>>(hf, w1, part, C);
    head_fold_sum_kernel<<<(HF_KP * HF_KP * C + 255) / 256, 256, 0, s>>>(part, (float*)(ws + hf_k.off), HF_KP * HF_KP * C, 5);
    RGP_HIP(hipGetLastError());
    return RGP_OK;
  }
  template <typename T>
  int pack(PackBatch<T>& pk) { return pk.add(hfold, k(pk.ws), HF_KP * HF_KP, 0); }     // GEMM filter [(r,t)][s]; rows 361 .. 383 stay zero
  // A: `images` GEMM images of operand dtype -> logits [F][49][49]
  template <typename T>
  int forward(char* ws, const void* A, int images, const float* out_b, float* logits, int F, hipStream_t s) {
    IgemmParams p = make_params(hfold, A, ws, images);
    EpiParams e = make_epi(hfold, ws + hf_z.off, ws);
    RGP_TRY((launch_igemm<T, 1, 1, EpiStore<float, false, false>>(p, e, s)));
    const long long total = (long long)F * 2401;
    head_col2im_kernel<<<(int)std::min<long long>((total + 255) / 256, 8192), 256, 0, s>>>((const float*)(ws + hf_z.off), out_b, logits, total);
    RGP_HIP(hipGetLastError());
    return RGP_OK;
  }
};

struct FoldedHeadBwd {
  ConvDesc b_hf;                           // dA[(f,m,n), s] = sum_k Pm[(f,m,n), k] K[k, s]   (K [361][C] fp32, rows 361..383 zero)
  // dz [F][2401], per-frame sums, the patches Pm [F*49][384] (operand dtype), dK [384][C], dH [11,11,64], dH's 25 partial
  // sums, dG: taken by the plan
  Buf dz, frame_sum, pm, dkf, dhf, dhp, dgp;
  static size_t dz_bytes(int F) { return (size_t)F * 2401 * 4; }
  static size_t pm_bytes(int F, int dtype) { return (size_t)F * 49 * HF_PK * esize(dtype); }
  static size_t dk_bytes(int C) { return (size_t)HF_PK * C * 4; }
  static constexpr size_t DH_BYTES = FoldedHead::H_BYTES, DHP_BYTES = 25 * FoldedHead::H_BYTES, DG_BYTES = FoldedHead::G_BYTES;
  bool plan(int C, int dtype) {
    ConvDesc& d = b_hf;
    d.Mw = 49; d.N = C; d.in_img_stride = 49LL * HF_PK; d.out_img_stride = 49LL * C;
    for (int pos = 0; pos < 49; ++pos) { d.in_tab.push_back(pos * HF_PK); d.out_tab.push_back(pos * C); }
    const bool ok = build_k_schedule(d, {0}, {0}, HF_PK, dtype);
    d.cin_src = HF_KP * HF_KP;
    d.s_tap = 0; d.s_n = 1; d.s_c = C;
    return ok;
  }
  template <typename T>
  int pack(PackBatch<T>& pk, const float* kf) { return pk.add(b_hf, kf, b_hf.N, 0); }
  // d loss / d logits -> dz, d out_b
  // loss_frames > 0 (a streaming call's backward): the divisor is the caller's, frames are (b, t) of T_ steps, and the dz rows
  // of the frames t >= n_valid are written as zeros -- everything above the recurrence then contributes nothing for them
  int loss_grad(char* ws, const float* logits, const float* probs, const float* labels, int loss_l2, int F, float* d_out_b, hipStream_t s,
                long long loss_frames = 0, int T_ = 0, int n_valid = 0) {
    if (loss_frames > 0) {
      dlogits_stream_kernel<<<F, 256, 0, s>>>(loss_l2 ? logits : probs, labels, (float*)(ws + dz.off), (float*)(ws + frame_sum.off),
                                              2401, 1.0f / (float)loss_frames, loss_l2, T_, n_valid);
    } else {
      dlogits_kernel<<<F, 256, 0, s>>>(loss_l2 ? logits : probs, labels, (float*)(ws + dz.off), (float*)(ws + frame_sum.off), 2401,
                                       1.0f / (float)F, loss_l2);
    }
    sum_kernel<<<1, 256, 0, s>>>((const float*)(ws + frame_sum.off), d_out_b, F, 1.0f);
    RGP_HIP(hipGetLastError());
    return RGP_OK;
  }
  template <typename T>
  int patches(char* ws, int F, hipStream_t s) {
    const long long M = (long long)F * 49, tot = M * HF_PK;
    head_fold_patches_kernel<T><<<(int)std::min<long long>((tot + 255) / 256, 8192), 256, 0, s>>>((const float*)(ws + dz.off), (T*)(ws + pm.off), M);
    RGP_HIP(hipGetLastError());
    return RGP_OK;
  }
  // the chain rule through the fold, from dK (dkf): d weight1, dH -> d weight2, dG -> d weight3, d out_W (six dependent
  // launches).  w1 .. out_W: the forward weights, d_*: their gradients
  int unfold_chain(char* ws, const FoldedHead& h, const float* w1, const float* w2, const float* w3, const float* out_W, float* d_w1,
                   float* d_w2, float* d_w3, float* d_out_W, hipStream_t s) {
    auto Fp = [&](const Buf& x) { return (float*)(ws + x.off); };
    const int C = h.C;
    head_unfold_f1_kernel<<<(25 * 64 * C + 255) / 256, 256, 0, s>>>(Fp(dkf), Fp(h.hf_h), d_w1, C);
    head_unfold_h_kernel<<<dim3(HF_HP * HF_HP, 25), 256, 0, s>>>(Fp(dkf), w1, Fp(dhp), C);
    head_fold_sum_kernel<<<(HF_HP * HF_HP * 64 + 255) / 256, 256, 0, s>>>(Fp(dhp), Fp(dhf), HF_HP * HF_HP * 64, 25);
    head_unfold_f2_kernel<<<(25 * 32 * 64 + 255) / 256, 256, 0, s>>>(Fp(dhf), Fp(h.gfold), d_w2);
    head_unfold_g_kernel<<<49, 256, 0, s>>>(Fp(dhf), w2, Fp(dgp));
    head_unfold_grads_kernel<<<1, 256, 0, s>>>(Fp(dgp), w3, out_W, d_w3, d_out_W);
    RGP_HIP(hipGetLastError());
    return RGP_OK;
  }
  // dst [F*49][C] (Out: fp32 or the operand dtype) = Pm K
  template <typename T, typename Out>
  int dgrad(char* ws, int F, Out* dst, hipStream_t s) {
    IgemmParams p = make_params(b_hf, ws + pm.off, ws, F);
    EpiParams e = make_epi(b_hf, dst, ws);
    return launch_igemm<T, 1, 1, EpiStore<Out, false, false>>(p, e, s);
  }
};

}  // namespace rgp
