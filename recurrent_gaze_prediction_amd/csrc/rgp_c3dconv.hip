// librgp_hip.so: gaze_c3d_conv, the no-recurrence baseline of the gaze family -- plan object, the fold of the whole
// network into one 1024 -> 384 filter (c3dconv_fused.hip.h), the fused inference launch and the staged path.
// Reference graph: /root/reference/models/gaze_c3d_conv.py:105-218.
//
// Two implementations of the same forward:
//   fused  (bf16 plans): [nchw_to_rows] -> c3dconv_fused_kernel: rows -> logits (+ softmax), Z never leaves the CU
//   staged (any dtype):  [nchw_to_rows] -> projection GEMM (+ bias) -> E -> folded head GEMM E x K^T -> Z -> head_col2im
//                        (+ out_b) -> rgp_softmax_xent_fwd: existing kernels only, the one the tests compare the fused with
// Training plans (RGP_C3DCONV_SAVE_FOR_BACKWARD) run the staged path and keep X and E; their backward is c3dconv_bwd.hip.h.
#include <algorithm>
#include <string>

#include "bwd_kernels.hip.h"
#include "rgp_grcn_plan.h"
#include "c3dconv_fused.hip.h"
#include "c3dconv_bwd.hip.h"

using namespace rgp;

struct rgp_c3dconv {
  int B = 0, T = 0, P = 0, dtype = RGP_BF16, F = 0;
  bool fused = false, save = false, fwd_done = false, bwd_done = false;
  ConvDesc proj, proj_rows, hfold;         // staged path: E = X W (+ b), Z = E K^T
  Buf xt, E, hf_z;                         // transposed placeholder input; staged intermediates
  Buf gfold, hf_h, hf_k, hf_part;          // the head's fold (head_fold.hip.h): G, H, K [361][P] and K's five partial sums, fp32
  Buf m2n, m2r, beta, plane;               // the network's fold: M2 in both K orders (operand dtype), bias row, bias plane
  size_t ws_bytes = 0;
  char* ws = nullptr;
  bool weights_set = false;
  const float *proj_b = nullptr, *out_b = nullptr;
  // ---- training plans (c3dconv_bwd.hip.h)
  long long M = 0, Mp = 0;                 // rows = frames x 49, rounded up to 64
  int ksplit = 1;
  ConvDesc b_hf, b_px;                     // dE = Pm K; d rows = dE W^T
  ConvDesc wg_k, wg_w;                     // the filter gradients as GEMMs over the rows: dK = PmT ET^T, dW = XT dET^T; their
                                           // "filter" areas hold ET / dET [P padded to 128][Mp]
  Buf dz, frame_sum, pm, pmT, xT, dE, part, dkf, dhf, dhp, dgp;
  rgp_c3dconv_weights w;                   // forward weights (device fp32) as last set
};

namespace {

template <typename T>
__global__ __launch_bounds__(256) void c3dconv_to_f32_kernel(const T* __restrict__ src, float* __restrict__ dst, long long n) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) dst[i] = Elem<T>::from(src[i]);
}

template <typename T>
int set_weights_impl(rgp_c3dconv* g, const rgp_c3dconv_weights* w, hipStream_t s) {
  char* ws = g->ws;
  const int P = g->P;
  float* gf = (float*)(ws + g->gfold.off);
  float* hf = (float*)(ws + g->hf_h.off);
  float* kf = (float*)(ws + g->hf_k.off);
  float* part = (float*)(ws + g->hf_part.off);
  // the head as one 19x19 stride-6 transposed convolution on E: G = weight3 o out_W -> H = G o weight2 -> K = H o weight1
  fold_head_filter_kernel<<<(49 * 32 + 255) / 256, 256, 0, s>>>(w->up_weight3, w->out_W, gf, 49, 12, 32);
  head_fold_h_kernel<<<(HF_HP * HF_HP * 64 + 255) / 256, 256, 0, s>>>(gf, w->up_weight2, hf);
  head_fold_k_kernel<<<dim3(HF_KP * HF_KP, 5), 128, 0, s>>>(hf, w->up_weight1, part, P);
  head_fold_sum_kernel<<<(HF_KP * HF_KP * P + 255) / 256, 256, 0, s>>>(part, kf, HF_KP * HF_KP * P, 5);
  RGP_HIP(hipGetLastError());
  // ... and the projection folded in: M2 = K W^T (both K orders), beta = K b, the bias plane (inference plans: a
  // training plan re-folds after every optimizer step and runs the staged path, which reads none of the three)
  if (!g->save) {
  c3dconv_fold_m2_kernel<T><<<HF_PK, 256, P * 4, s>>>(w->proj_c3d_W, kf, (T*)(ws + g->m2n.off), (T*)(ws + g->m2r.off), P);
  c3dconv_fold_beta_kernel<<<(HF_PK + 127) / 128, 128, 0, s>>>(w->proj_c3d_b, kf, (float*)(ws + g->beta.off), P);
  c3dconv_bias_plane_kernel<<<(2401 + 255) / 256, 256, 0, s>>>((const float*)(ws + g->beta.off), w->out_b, (float*)(ws + g->plane.off));
  }
  RGP_HIP(hipGetLastError());
  if (!g->fused) {
    PackBatch<T> pk(ws, s);
    RGP_TRY(pk.add(g->proj, w->proj_c3d_W, P, 0));
    RGP_TRY(pk.add(g->proj_rows, w->proj_c3d_W, P, 0));
    RGP_TRY(pk.add(g->hfold, kf, HF_KP * HF_KP, 0));           // GEMM filter [(r,t)][s]; rows 361 .. 383 stay zero
    RGP_TRY(pk.flush());
  }
  if (g->save) {
    PackBatch<T> pk(ws, s);
    RGP_TRY(pk.add(g->b_px, w->proj_c3d_W, 512, 0));            // d = 0: feature channels 0, 2, 4, ...
    RGP_TRY(pk.add(g->b_px, w->proj_c3d_W + P, 512, 512));      // d = 1: feature channels 1, 3, 5, ...
    RGP_TRY(pk.add(g->b_hf, kf, P, 0));
    RGP_TRY(pk.flush());
    g->w = *w;
  }
  g->proj_b = w->proj_c3d_b;
  g->out_b = w->out_b;
  g->weights_set = true;
  g->fwd_done = g->bwd_done = false;
  return RGP_OK;
}

template <typename T>
int forward_impl(rgp_c3dconv* g, const float* c3d_input, const void* rows, float* logits, float* probs, hipStream_t s) {
  char* ws = g->ws;
  const void* A = rows;
  if (!rows) {
    nchw_to_rows_kernel<T><<<dim3(1024 / 64, g->F), 256, 0, s>>>(c3d_input, (T*)(ws + g->xt.off), 1024);
    RGP_HIP(hipGetLastError());
    A = ws + g->xt.off;
  } else if (g->save) {
    // the backward's projection filter gradient reads X in the reference's channel order c*2+d (gaze_rnn.py:494-497)
    const long long total = (long long)g->F * 49 * 1024;
    rows_to_xt_kernel<T><<<(int)std::min<long long>((total + 255) / 256, 8192), 256, 0, s>>>((const T*)rows, (T*)(ws + g->xt.off), total);
    RGP_HIP(hipGetLastError());
  }
  if constexpr (sizeof(T) == 2) {
    if (g->fused) {
      RGP_TRY(ensure_dyn_smem((const void*)c3dconv_fused_kernel, CF_SMEM));
      c3dconv_fused_kernel<<<(g->F + 1) / 2, CF_NT, CF_SMEM, s>>>((const bf16_t*)A, (const bf16_t*)(ws + (rows ? g->m2r.off : g->m2n.off)),
                                                                 (const float*)(ws + g->plane.off), logits, probs, g->F);
      RGP_HIP(hipGetLastError());
      return RGP_OK;
    }
  }
  {
    const ConvDesc& d = rows ? g->proj_rows : g->proj;
    IgemmParams p = make_params(d, A, ws, g->F);
    EpiParams e = make_epi(d, ws + g->E.off, ws);
    e.bias = g->proj_b;
    RGP_TRY((launch_igemm<T, 1, 1, EpiStore<T, true, false>>(p, e, s)));
  }
  {
    IgemmParams p = make_params(g->hfold, ws + g->E.off, ws, g->F);
    EpiParams e = make_epi(g->hfold, ws + g->hf_z.off, ws);
    RGP_TRY((launch_igemm<T, 1, 1, EpiStore<float, false, false>>(p, e, s)));
  }
  const long long total = (long long)g->F * 2401;
  head_col2im_kernel<<<(int)std::min<long long>((total + 255) / 256, 8192), 256, 0, s>>>((const float*)(ws + g->hf_z.off), g->out_b, logits, total);
  RGP_HIP(hipGetLastError());
  if (probs) RGP_TRY(rgp_softmax_xent_fwd(logits, nullptr, probs, nullptr, nullptr, g->F, 2401, (rgp_stream_t)s));
  g->fwd_done = true;
  g->bwd_done = false;
  return RGP_OK;
}

// one filter gradient: out[r][n] = sum_m AT[r][m] BT[n][m] (BT = the desc's filter area), K = Mp split ksplit ways into
// g->part, summed in a fixed order
template <typename T>
int wgrad_gemm(rgp_c3dconv* g, const ConvDesc& d, const void* AT, float* out, hipStream_t s) {
  char* ws = g->ws;
  IgemmParams p = make_params(d, AT, ws, 1);
  EpiParams e = make_epi(d, ws + g->part.off, ws);
  const long long n = (long long)d.Mw * g->P;
  e.xpre_img_stride = n;
  RGP_TRY((launch_igemm<T, 1, 1, EpiStoreSplitF32>(p, e, s, g->ksplit)));
  head_fold_sum_kernel<<<(int)((n + 255) / 256), 256, 0, s>>>((const float*)(ws + g->part.off), out, (int)n, g->ksplit);
  RGP_HIP(hipGetLastError());
  return RGP_OK;
}

template <typename T>
int backward_impl(rgp_c3dconv* g, const float* logits, const float* probs, const float* labels, const rgp_c3dconv_weights* gr,
                  int loss_l2, hipStream_t s) {
  char* ws = g->ws;
  const int P = g->P, F = g->F;
  const long long M = g->M, Mp = g->Mp;
  auto Fp = [&](const Buf& x) { return (float*)(ws + x.off); };
  auto Tp = [&](const Buf& x) { return (T*)(ws + x.off); };
  T* eT = (T*)(ws + g->wg_k.w_off);
  T* deT = (T*)(ws + g->wg_w.w_off);
  // 1. d loss / d logits, d out_b
  dlogits_kernel<<<F, 256, 0, s>>>(loss_l2 ? logits : probs, labels, Fp(g->dz), Fp(g->frame_sum), 2401, 1.0f / (float)F, loss_l2);
  sum_kernel<<<1, 256, 0, s>>>(Fp(g->frame_sum), (float*)gr->out_b, F, 1.0f);
  // 2. patches of dz; dK = Pm^T E
  const long long tot = M * HF_PK;
  head_fold_patches_kernel<T><<<(int)std::min<long long>((tot + 255) / 256, 8192), 256, 0, s>>>(Fp(g->dz), Tp(g->pm), M);
  c3dconv_transpose_kernel<T><<<dim3((unsigned)(Mp / 64), HF_PK / 64), 256, 0, s>>>(Tp(g->pm), Tp(g->pmT), M, HF_PK, Mp);
  c3dconv_transpose_kernel<T><<<dim3((unsigned)(Mp / 64), P / 64), 256, 0, s>>>(Tp(g->E), eT, M, P, Mp);
  RGP_HIP(hipGetLastError());
  RGP_TRY(wgrad_gemm<T>(g, g->wg_k, Tp(g->pmT), Fp(g->dkf), s));
  // 3. the chain rule through the fold (head_fold.hip.h): d weight1, dH -> d weight2, dG -> d weight3, d out_W
  const float* hf = (const float*)(ws + g->hf_h.off);
  const float* gf = (const float*)(ws + g->gfold.off);
  head_unfold_f1_kernel<<<(25 * 64 * P + 255) / 256, 256, 0, s>>>(Fp(g->dkf), hf, (float*)gr->up_weight1, P);
  head_unfold_h_kernel<<<dim3(HF_HP * HF_HP, 25), 256, 0, s>>>(Fp(g->dkf), g->w.up_weight1, Fp(g->dhp), P);
  head_fold_sum_kernel<<<(HF_HP * HF_HP * 64 + 255) / 256, 256, 0, s>>>(Fp(g->dhp), Fp(g->dhf), HF_HP * HF_HP * 64, 25);
  head_unfold_f2_kernel<<<(25 * 32 * 64 + 255) / 256, 256, 0, s>>>(Fp(g->dhf), gf, (float*)gr->up_weight2);
  head_unfold_g_kernel<<<49, 256, 0, s>>>(Fp(g->dhf), g->w.up_weight2, Fp(g->dgp));
  head_unfold_grads_kernel<<<1, 256, 0, s>>>(Fp(g->dgp), g->w.up_weight3, g->w.out_W, (float*)gr->up_weight3, (float*)gr->out_W);
  RGP_HIP(hipGetLastError());
  // 4. dE = Pm K
  {
    IgemmParams p = make_params(g->b_hf, Tp(g->pm), ws, F);
    EpiParams e = make_epi(g->b_hf, Tp(g->dE), ws);
    RGP_TRY((launch_igemm<T, 1, 1, EpiStore<T, false, false>>(p, e, s)));
  }
  // 5. d proj_c3d_W = X^T dE, d proj_c3d_b = column sums of dE (= row sums of dE^T: one block per column, fixed tree)
  c3dconv_transpose_kernel<T><<<dim3((unsigned)(Mp / 64), P / 64), 256, 0, s>>>(Tp(g->dE), deT, M, P, Mp);
  c3dconv_transpose_kernel<T><<<dim3((unsigned)(Mp / 64), 1024 / 64), 256, 0, s>>>(Tp(g->xt), Tp(g->xT), M, 1024, Mp);
  RGP_HIP(hipGetLastError());
  RGP_TRY(wgrad_gemm<T>(g, g->wg_w, Tp(g->xT), (float*)gr->proj_c3d_W, s));
  rowsum_kernel<T><<<P, 256, 0, s>>>(deT, (float*)gr->proj_c3d_b, Mp, M);
  RGP_HIP(hipGetLastError());
  g->bwd_done = true;
  return RGP_OK;
}

int check_ready(rgp_c3dconv* g) {
  if (!g) return set_err(RGP_EINVAL, "null plan");
  if (!g->ws) return set_err(RGP_EWORKSPACE, "rgp_c3dconv: workspace not bound");
  if (!g->weights_set) return set_err(RGP_ESTATE, "rgp_c3dconv: weights not set");
  return RGP_OK;
}

// fp32 elements of a named buffer; *off / *operand: where it lives and whether it is stored in the operand dtype
size_t find_buffer(const rgp_c3dconv* g, const char* name, size_t* off, bool* operand) {
  const std::string n(name ? name : "");
  if (n == "c3d_embedded" && !g->fused) { *off = g->E.off; *operand = true; return (size_t)g->F * 49 * g->P; }
  if (g->save && (n == "folded_filter" || n == "bias_plane")) return 0;      // training plans do not build them
  if (n == "folded_filter") { *off = g->m2n.off; *operand = true; return (size_t)HF_PK * 1024; }
  if (n == "bias_plane") { *off = g->plane.off; *operand = false; return 2401; }
  return 0;
}

}  // namespace

extern "C" {

int rgp_c3dconv_create(rgp_c3dconv_t** plan, int batch, int n_steps, int dim_proj, int dtype, int flags) {
  RGP_REQUIRE(plan, "rgp_c3dconv_create: null out pointer");
  RGP_REQUIRE((flags & ~(RGP_C3DCONV_SAVE_FOR_BACKWARD | RGP_C3DCONV_STAGED | RGP_C3DCONV_FUSED)) == 0,
              "rgp_c3dconv_create: unknown flags 0x%x", flags);
  RGP_REQUIRE(batch > 0 && n_steps > 0, "rgp_c3dconv_create: batch=%d n_steps=%d", batch, n_steps);
  RGP_REQUIRE(dtype == RGP_F32 || dtype == RGP_BF16, "rgp_c3dconv_create: dtype %d", dtype);
  RGP_REQUIRE(dim_proj > 0 && dim_proj % 64 == 0, "rgp_c3dconv_create: dim_proj=%d must be a multiple of 64", dim_proj);
  RGP_REQUIRE((long long)batch * n_steps * 2401 < (1LL << 31), "rgp_c3dconv_create: B*T too large");
  RGP_REQUIRE((flags & (RGP_C3DCONV_STAGED | RGP_C3DCONV_FUSED)) != (RGP_C3DCONV_STAGED | RGP_C3DCONV_FUSED),
              "rgp_c3dconv_create: flags name both paths");
  RGP_REQUIRE(!(flags & RGP_C3DCONV_FUSED) || dtype == RGP_BF16, "rgp_c3dconv_create: the fused kernel (flags) takes bf16 plans only");
  RGP_REQUIRE(!(flags & RGP_C3DCONV_FUSED) || !(flags & RGP_C3DCONV_SAVE_FOR_BACKWARD),
              "rgp_c3dconv_create: the fused kernel (flags) keeps nothing for a backward: training plans run the staged path");
  rgp_c3dconv* g = new rgp_c3dconv();
  g->B = batch; g->T = n_steps; g->P = dim_proj; g->dtype = dtype; g->F = batch * n_steps;
  // default: the fused kernel for bf16 plans ("gaze_c3d_conv": measured against the staged path at both shapes)
  g->save = (flags & RGP_C3DCONV_SAVE_FOR_BACKWARD) != 0;
  g->fused = dtype == RGP_BF16 && !(flags & RGP_C3DCONV_STAGED) && !g->save;
  const int P = g->P, F = g->F, es = esize(dtype);
  Arena a;
  if (!g->fused) {
    bool ok = true;
    for (ConvDesc* d : {&g->proj, &g->proj_rows}) {            // E = X W + b (gaze_c3d_conv.py:124-138), rows [F*49][P]
      d->Mw = 49; d->N = P;
      d->in_img_stride = 49LL * 1024; d->out_img_stride = 49LL * P;
      for (int p = 0; p < 49; ++p) { d->in_tab.push_back(p * 1024); d->out_tab.push_back(p * P); }
    }
    ok &= build_k_schedule(g->proj, {0}, {0}, 1024, dtype);
    g->proj.s_tap = 0; g->proj.s_n = 1; g->proj.s_c = P;
    // rows from C3D carry K order d*512+c; reference channel = c*2+d
    ok &= build_k_schedule(g->proj_rows, {0, 512}, {0, 1}, 512, dtype);
    g->proj_rows.s_tap = P; g->proj_rows.s_n = 1; g->proj_rows.s_c = 2LL * P;
    {
      ConvDesc& d = g->hfold;                                  // the folded head on E: K = P, N = the 19x19 taps
      d.Mw = 49; d.N = HF_PK; d.in_img_stride = 49LL * P; d.out_img_stride = 49LL * HF_PK;
      for (int p = 0; p < 49; ++p) { d.in_tab.push_back(p * P); d.out_tab.push_back(p * HF_PK); }
      ok &= build_k_schedule(d, {0}, {0}, P, dtype);
      d.s_tap = 0; d.s_n = P; d.s_c = 1;                       // source K [(r,t)][s]
    }
    if (!ok) { delete g; return set_err(RGP_EINVAL, "rgp_c3dconv_create: unsupported channel geometry P=%d", P); }
    for (ConvDesc* d : {&g->proj, &g->proj_rows, &g->hfold}) d->reserve(a, dtype);
    g->E = take(a, (size_t)F * 49 * P * es);
    g->hf_z = take(a, (size_t)F * 49 * HF_PK * 4);
  }
  g->xt = take(a, (size_t)F * 49 * 1024 * es);
  g->gfold = take(a, 50 * 32 * 4);
  g->hf_h = take(a, (size_t)HF_HP * HF_HP * 64 * 4);
  g->hf_k = take(a, (size_t)HF_PK * P * 4);                    // (rows 361 .. 383 stay zero)
  g->hf_part = take(a, (size_t)5 * HF_KP * HF_KP * P * 4);
  g->m2n = take(a, (size_t)HF_PK * 1024 * es);
  g->m2r = take(a, (size_t)HF_PK * 1024 * es);
  g->beta = take(a, (size_t)HF_PK * 4);
  g->plane = take(a, 2401 * 4);
  if (g->save) {
    g->M = (long long)F * 49;
    g->Mp = (g->M + 63) / 64 * 64;
    const int nk = (int)(g->Mp / bke(dtype));
    g->ksplit = std::min(16, nk);
    bool ok = g->Mp * 1024 < (1LL << 31);
    {  // d rows[m][d*512+c] = sum_p dE[m][p] W[c*2+d][p]   (rows order of rgp_c3d_forward)
      ConvDesc& d = g->b_px;
      d.Mw = 1; d.N = 1024; d.in_img_stride = P; d.out_img_stride = 1024; d.in_tab = {0}; d.out_tab = {0};
      ok &= build_k_schedule(d, {0}, {0}, P, dtype);
      d.s_tap = 0; d.s_n = 2LL * P; d.s_c = 1;
    }
    {  // dE[(f,m,n), s] = sum_k Pm[(f,m,n), k] K[k, s]   (K [361][P] fp32, rows 361..383 zero)
      ConvDesc& d = g->b_hf;
      d.Mw = 49; d.N = P; d.in_img_stride = 49LL * HF_PK; d.out_img_stride = 49LL * P;
      for (int pos = 0; pos < 49; ++pos) { d.in_tab.push_back(pos * HF_PK); d.out_tab.push_back(pos * P); }
      ok &= build_k_schedule(d, {0}, {0}, HF_PK, dtype);
      d.cin_src = HF_KP * HF_KP;
      d.s_tap = 0; d.s_n = 1; d.s_c = P;
    }
    auto wgrad_desc = [&](ConvDesc& d, int rows) {               // out [rows][P] = AT [rows][Mp] x BT [P][Mp]^T
      d.Mw = rows; d.N = P; d.in_img_stride = 0; d.out_img_stride = 0;
      for (int r = 0; r < rows; ++r) { d.in_tab.push_back((int)(r * g->Mp)); d.out_tab.push_back(r * P); }
      return build_k_schedule(d, {0}, {0}, (int)g->Mp, dtype);
    };
    if (ok) ok &= wgrad_desc(g->wg_k, HF_PK);
    if (ok) ok &= wgrad_desc(g->wg_w, 1024);
    if (!ok) { delete g; return set_err(RGP_EINVAL, "rgp_c3dconv_create: B*T too large for the backward plan"); }
    for (ConvDesc* d : {&g->b_px, &g->b_hf, &g->wg_k, &g->wg_w}) d->reserve(a, dtype);
    g->dz = take(a, (size_t)F * 2401 * 4);
    g->frame_sum = take(a, (size_t)F * 4);
    g->pm = take(a, (size_t)g->M * HF_PK * es);
    g->pmT = take(a, (size_t)HF_PK * g->Mp * es);
    g->xT = take(a, (size_t)1024 * g->Mp * es);
    g->dE = take(a, (size_t)g->M * P * es);
    g->part = take(a, (size_t)g->ksplit * 1024 * P * 4);
    g->dkf = take(a, (size_t)HF_PK * P * 4);
    g->dhf = take(a, (size_t)HF_HP * HF_HP * 64 * 4);
    g->dhp = take(a, (size_t)25 * HF_HP * HF_HP * 64 * 4);
    g->dgp = take(a, 50 * 32 * 4);
  }
  g->ws_bytes = a.off;
  *plan = g;
  return RGP_OK;
}

int rgp_c3dconv_destroy(rgp_c3dconv_t* plan) {
  delete plan;
  return RGP_OK;
}

size_t rgp_c3dconv_workspace_bytes(const rgp_c3dconv_t* plan) { return plan ? plan->ws_bytes : 0; }

const char* rgp_c3dconv_path(const rgp_c3dconv_t* plan) { return plan ? (plan->fused ? "fused" : "staged") : ""; }

int rgp_c3dconv_bind_workspace(rgp_c3dconv_t* g, void* workspace, size_t bytes, rgp_stream_t stream) {
  RGP_REQUIRE(g && workspace, "rgp_c3dconv_bind_workspace: null argument");
  if (bytes < g->ws_bytes) return set_err(RGP_EWORKSPACE, "workspace %zu < required %zu bytes", bytes, g->ws_bytes);
  RGP_REQUIRE(((size_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  g->ws = (char*)workspace;
  g->weights_set = false;
  RGP_HIP(hipMemsetAsync(g->ws, 0, g->ws_bytes, s));           // (packed-filter padding stays zero: a pack writes the same positions every time)
  if (!g->fused)
    for (ConvDesc* d : {&g->proj, &g->proj_rows, &g->hfold}) RGP_TRY(upload_desc(*d, g->ws, s));
  if (g->save)
    for (ConvDesc* d : {&g->b_px, &g->b_hf, &g->wg_k, &g->wg_w}) RGP_TRY(upload_desc(*d, g->ws, s));
  return RGP_OK;
}

int rgp_c3dconv_set_weights(rgp_c3dconv_t* g, const rgp_c3dconv_weights* w, rgp_stream_t stream) {
  RGP_REQUIRE(g && w, "rgp_c3dconv_set_weights: null argument");
  if (!g->ws) return set_err(RGP_EWORKSPACE, "rgp_c3dconv: workspace not bound");
  const float* const* ptrs = (const float* const*)w;
  for (size_t i = 0; i < sizeof(rgp_c3dconv_weights) / sizeof(float*); ++i)
    RGP_REQUIRE(ptrs[i], "rgp_c3dconv_set_weights: weight pointer %zu is null", i);
  RGP_REQUIRE(((size_t)w->proj_c3d_W & 15) == 0, "rgp_c3dconv_set_weights: proj_c3d_W must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  return g->dtype == RGP_BF16 ? set_weights_impl<bf16_t>(g, w, s) : set_weights_impl<float>(g, w, s);
}

int rgp_c3dconv_forward(rgp_c3dconv_t* g, const float* c3d_input, float* logits, float* probs, rgp_stream_t stream) {
  RGP_TRY(check_ready(g));
  RGP_REQUIRE(c3d_input && logits, "rgp_c3dconv_forward: null argument");
  hipStream_t s = (hipStream_t)stream;
  return g->dtype == RGP_BF16 ? forward_impl<bf16_t>(g, c3d_input, nullptr, logits, probs, s)
                              : forward_impl<float>(g, c3d_input, nullptr, logits, probs, s);
}

int rgp_c3dconv_forward_rows(rgp_c3dconv_t* g, const void* c3d_rows, float* logits, float* probs, rgp_stream_t stream) {
  RGP_TRY(check_ready(g));
  RGP_REQUIRE(c3d_rows && logits, "rgp_c3dconv_forward_rows: null argument");
  RGP_REQUIRE(((size_t)c3d_rows & 15) == 0, "rgp_c3dconv_forward_rows: rows must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  return g->dtype == RGP_BF16 ? forward_impl<bf16_t>(g, nullptr, c3d_rows, logits, probs, s)
                              : forward_impl<float>(g, nullptr, c3d_rows, logits, probs, s);
}

int rgp_c3dconv_backward(rgp_c3dconv_t* g, const float* logits, const float* probs, const float* labels,
                         const rgp_c3dconv_weights* grads, int loss_type, rgp_stream_t stream) {
  RGP_TRY(check_ready(g));
  RGP_REQUIRE(labels && grads && (loss_type == 0 || loss_type == 1), "rgp_c3dconv_backward: bad arguments");
  RGP_REQUIRE(loss_type == 1 ? logits != nullptr : probs != nullptr, "rgp_c3dconv_backward: the loss needs %s", loss_type == 1 ? "logits" : "probs");
  if (!g->save) return set_err(RGP_ESTATE, "rgp_c3dconv_backward: the plan was not created with RGP_C3DCONV_SAVE_FOR_BACKWARD");
  if (!g->fwd_done) return set_err(RGP_ESTATE, "rgp_c3dconv_backward: no forward since the weights were set");
  const float* const* ptrs = (const float* const*)grads;
  for (size_t i = 0; i < sizeof(rgp_c3dconv_weights) / sizeof(float*); ++i)
    RGP_REQUIRE(ptrs[i], "rgp_c3dconv_backward: gradient pointer %zu is null", i);
  hipStream_t s = (hipStream_t)stream;
  return g->dtype == RGP_BF16 ? backward_impl<bf16_t>(g, logits, probs, labels, grads, loss_type, s)
                              : backward_impl<float>(g, logits, probs, labels, grads, loss_type, s);
}

int rgp_c3dconv_backward_input(rgp_c3dconv_t* g, float* d_rows, rgp_stream_t stream) {
  RGP_REQUIRE(g && d_rows, "rgp_c3dconv_backward_input: null argument");
  if (!g->ws || !g->save || !g->weights_set || !g->bwd_done) return set_err(RGP_ESTATE, "rgp_c3dconv_backward_input: call after rgp_c3dconv_backward");
  hipStream_t s = (hipStream_t)stream;
  IgemmParams p = make_params(g->b_px, g->ws + g->dE.off, g->ws, (int)g->M);
  EpiParams e = make_epi(g->b_px, d_rows, g->ws);
  return g->dtype == RGP_BF16 ? launch_igemm<bf16_t, 1, 1, EpiStore<float, false, false>>(p, e, s)
                              : launch_igemm<float, 1, 1, EpiStore<float, false, false>>(p, e, s);
}

size_t rgp_c3dconv_buffer_elems(const rgp_c3dconv_t* g, const char* name) {
  size_t off; bool operand;
  return g ? find_buffer(g, name, &off, &operand) : 0;
}

int rgp_c3dconv_read_buffer(rgp_c3dconv_t* g, const char* name, float* dst, rgp_stream_t stream) {
  RGP_REQUIRE(g && g->ws && name && dst, "rgp_c3dconv_read_buffer: null argument");
  size_t off = 0; bool operand = false;
  const size_t n = find_buffer(g, name, &off, &operand);
  if (!n) return set_err(RGP_EINVAL, "rgp_c3dconv_read_buffer: unknown buffer '%s'", name);
  hipStream_t s = (hipStream_t)stream;
  const int blocks = (int)std::min<size_t>((n + 255) / 256, 8192);
  if (operand && g->dtype == RGP_BF16) c3dconv_to_f32_kernel<bf16_t><<<blocks, 256, 0, s>>>((const bf16_t*)(g->ws + off), dst, (long long)n);
  else c3dconv_to_f32_kernel<float><<<blocks, 256, 0, s>>>((const float*)(g->ws + off), dst, (long long)n);
  RGP_HIP(hipGetLastError());
  return RGP_OK;
}

}  // extern "C"
