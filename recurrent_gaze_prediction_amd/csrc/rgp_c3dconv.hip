// librgp_hip.so: gaze_c3d_conv, the no-recurrence baseline of the gaze family -- plan object, the fold of the whole
// network into one 1024 -> 384 filter (c3dconv_fused.hip.h), the fused inference launch and the staged path.
// Reference graph: /root/reference/models/gaze_c3d_conv.py:105-218.
//
// Two implementations of the same forward:
//   fused  (bf16 plans): [nchw_to_rows] -> c3dconv_fused_kernel: rows -> logits (+ softmax), Z never leaves the CU
//   staged (any dtype):  [nchw_to_rows] -> projection GEMM (+ bias) -> E -> folded head GEMM E x K^T -> Z -> head_col2im
//                        (+ out_b) -> rgp_softmax_xent_fwd: existing kernels only, the one the tests compare the fused with
// Training plans (RGP_C3DCONV_SAVE_FOR_BACKWARD) run the staged path and keep X and E.  Their backward is the chain rule
// head_fold.hip.h documents with y := E, with NO float atomics: both filter gradients are GEMM-form (gaze_stages.h),
//   dK[(r,t),s] = sum_m Pm[m,(r,t)] E[m,s]    d proj_c3d_W[k,s] = sum_m X[m,k] dE[m,s]    d proj_c3d_b = colsum(dE)
// The projection, the folded head and their backward are the gaze family's shared stages (gaze_stages.h).
#include <algorithm>
#include <string>

#include "gaze_stages.h"
#include "c3dconv_fused.hip.h"

using namespace rgp;

struct rgp_c3dconv {
  int B = 0, T = 0, P = 0, dtype = RGP_BF16, F = 0;
  bool fused = false, save = false, fwd_done = false, bwd_done = false;
  Projection pj;                           // staged path: E = X W (+ b) ...
  FoldedHead head;                         // ... Z = E K^T; the head's fold
  Buf E;
  Buf m2n, m2r, beta, plane;               // the network's fold: M2 in both K orders (operand dtype), bias row, bias plane
  size_t ws_bytes = 0;
  char* ws = nullptr;
  bool weights_set = false;
  const float *proj_b = nullptr, *out_b = nullptr;
  // ---- training plans
  FoldedHeadBwd hb;                        // dE = Pm K
  ProjectionBwd pb;                        // d rows = dE W^T; dW = XT dET^T
  ConvDesc wg_k;                           // dK = PmT ET^T as a GEMM over the rows: its "filter" area holds ET [P padded to 128][Mp]
  Buf pmT, dE;
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
  const float* kf = g->head.k(ws);
  // the head as one 19x19 stride-6 transposed convolution on E
  RGP_TRY(g->head.fold(ws, w->up_weight3, w->out_W, w->up_weight2, w->up_weight1, s));
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
    RGP_TRY(g->pj.pack(pk, w->proj_c3d_W));
    RGP_TRY(g->head.pack(pk));
    RGP_TRY(pk.flush());
  }
  if (g->save) {
    PackBatch<T> pk(ws, s);
    RGP_TRY(g->pb.pack(pk, w->proj_c3d_W));
    RGP_TRY(g->hb.pack(pk, kf));
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
  if constexpr (sizeof(T) == 2) {
    if (g->fused) {
      const void* A = rows;
      if (!rows) {
        nchw_to_rows_kernel<T><<<dim3(1024 / 64, g->F), 256, 0, s>>>(c3d_input, (T*)(ws + g->pj.xt.off), 1024);
        RGP_HIP(hipGetLastError());
        A = ws + g->pj.xt.off;
      }
      RGP_TRY(ensure_dyn_smem((const void*)c3dconv_fused_kernel, CF_SMEM));
      c3dconv_fused_kernel<<<(g->F + 1) / 2, CF_NT, CF_SMEM, s>>>((const bf16_t*)A, (const bf16_t*)(ws + (rows ? g->m2r.off : g->m2n.off)),
                                                                 (const float*)(ws + g->plane.off), logits, probs, g->F);
      RGP_HIP(hipGetLastError());
      return RGP_OK;
    }
  }
  RGP_TRY(g->pj.forward<T>(ws, c3d_input, rows, g->save, g->F, ws + g->E.off, g->proj_b, s));
  RGP_TRY(g->head.forward<T>(ws, ws + g->E.off, g->F, g->out_b, logits, g->F, s));
  if (probs) RGP_TRY(rgp_softmax_xent_fwd(logits, nullptr, probs, nullptr, nullptr, g->F, 2401, (rgp_stream_t)s));
  g->fwd_done = true;
  g->bwd_done = false;
  return RGP_OK;
}

template <typename T>
int backward_impl(rgp_c3dconv* g, const float* logits, const float* probs, const float* labels, const rgp_c3dconv_weights* gr,
                  int loss_l2, hipStream_t s) {
  char* ws = g->ws;
  const int P = g->P, F = g->F;
  const long long M = g->pb.M, Mp = g->pb.Mp;
  auto Fp = [&](const Buf& x) { return (float*)(ws + x.off); };
  auto Tp = [&](const Buf& x) { return (T*)(ws + x.off); };
  // 1. d loss / d logits, d out_b
  RGP_TRY(g->hb.loss_grad(ws, logits, probs, labels, loss_l2, F, (float*)gr->out_b, s));
  // 2. patches of dz; dK = Pm^T E
  RGP_TRY(g->hb.patches<T>(ws, F, s));
  transpose_pad<T>(Tp(g->hb.pm), Tp(g->pmT), M, HF_PK, Mp, s);
  transpose_pad<T>(Tp(g->E), (T*)(ws + g->wg_k.w_off), M, P, Mp, s);
  RGP_HIP(hipGetLastError());
  RGP_TRY(wgrad_gemm<T>(ws, g->wg_k, Tp(g->pmT), g->pb.part, g->pb.ksplit, Fp(g->hb.dkf), s));
  // 3. the chain rule through the fold
  RGP_TRY(g->hb.unfold_chain(ws, g->head, g->w.up_weight1, g->w.up_weight2, g->w.up_weight3, g->w.out_W, (float*)gr->up_weight1,
                             (float*)gr->up_weight2, (float*)gr->up_weight3, (float*)gr->out_W, s));
  // 4. dE = Pm K
  RGP_TRY((g->hb.dgrad<T, T>(ws, F, Tp(g->dE), s)));
  // 5. d proj_c3d_W = X^T dE, d proj_c3d_b = column sums of dE
  RGP_TRY(g->pb.weight_grads<T>(ws, Tp(g->pj.xt), Tp(g->dE), (float*)gr->proj_c3d_W, (float*)gr->proj_c3d_b, s));
  g->bwd_done = true;
  return RGP_OK;
}

int check_ready(rgp_c3dconv* g) { return check_bound_and_set(g, "rgp_c3dconv"); }

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
    std::vector<int> rows49, z49;
    for (int p = 0; p < 49; ++p) { rows49.push_back(p * P); z49.push_back(p * HF_PK); }
    bool ok = g->pj.plan(P, dtype, rows49, 49LL * P);           // E = X W + b (gaze_c3d_conv.py:124-138), rows [F*49][P]
    {
      ConvDesc& d = g->head.hfold;                             // the folded head on E: a GEMM image is a frame's 49 rows
      d.Mw = 49; d.in_img_stride = 49LL * P; d.out_img_stride = 49LL * HF_PK;
      d.in_tab = rows49; d.out_tab = z49;
    }
    ok &= g->head.plan(P, dtype);
    if (!ok) { delete g; return set_err(RGP_EINVAL, "rgp_c3dconv_create: unsupported channel geometry P=%d", P); }
    for (ConvDesc* d : {&g->pj.proj, &g->pj.proj_rows, &g->head.hfold}) d->reserve(a, dtype);
    g->E = take(a, (size_t)F * 49 * P * es);
    g->head.hf_z = take(a, FoldedHead::z_bytes(F));
  }
  g->head.C = P;                                               // (fused plans fold the head too)
  g->pj.xt = take(a, (size_t)F * 49 * 1024 * es);
  g->head.gfold = take(a, FoldedHead::G_BYTES);
  g->head.hf_h = take(a, FoldedHead::H_BYTES);
  g->head.hf_k = take(a, g->head.k_bytes(HF_PK));
  g->head.hf_part = take(a, g->head.part_bytes());
  g->m2n = take(a, (size_t)HF_PK * 1024 * es);
  g->m2r = take(a, (size_t)HF_PK * 1024 * es);
  g->beta = take(a, (size_t)HF_PK * 4);
  g->plane = take(a, 2401 * 4);
  if (g->save) {
    bool ok = g->pb.plan(P, dtype);
    ok &= g->hb.plan(P, dtype);
    ok = ok && g->pb.plan_wgrad(F, dtype) && wgrad_gemm_desc(g->wg_k, HF_PK, P, g->pb.Mp, dtype);
    if (!ok) { delete g; return set_err(RGP_EINVAL, "rgp_c3dconv_create: B*T too large for the backward plan"); }
    for (ConvDesc* d : {&g->pb.b_px, &g->hb.b_hf, &g->wg_k, &g->pb.wg_w}) d->reserve(a, dtype);
    g->hb.dz = take(a, FoldedHeadBwd::dz_bytes(F));
    g->hb.frame_sum = take(a, (size_t)F * 4);
    g->hb.pm = take(a, FoldedHeadBwd::pm_bytes(F, dtype));
    g->pmT = take(a, (size_t)HF_PK * g->pb.Mp * es);
    g->pb.xT = take(a, g->pb.xT_bytes(dtype));
    g->dE = take(a, (size_t)g->pb.M * P * es);
    g->pb.part = take(a, g->pb.part_bytes());
    g->hb.dkf = take(a, FoldedHeadBwd::dk_bytes(P));
    g->hb.dhf = take(a, FoldedHeadBwd::DH_BYTES);
    g->hb.dhp = take(a, FoldedHeadBwd::DHP_BYTES);
    g->hb.dgp = take(a, FoldedHeadBwd::DG_BYTES);
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
  RGP_TRY(check_bind("rgp_c3dconv_bind_workspace", g, workspace, bytes));
  hipStream_t s = (hipStream_t)stream;
  g->ws = (char*)workspace;
  g->weights_set = false;
  RGP_HIP(hipMemsetAsync(g->ws, 0, g->ws_bytes, s));           // (packed-filter padding stays zero: a pack writes the same positions every time)
  if (!g->fused)
    for (ConvDesc* d : {&g->pj.proj, &g->pj.proj_rows, &g->head.hfold}) RGP_TRY(upload_desc(*d, g->ws, s));
  if (g->save)
    for (ConvDesc* d : {&g->pb.b_px, &g->hb.b_hf, &g->wg_k, &g->pb.wg_w}) RGP_TRY(upload_desc(*d, g->ws, s));
  return RGP_OK;
}

int rgp_c3dconv_set_weights(rgp_c3dconv_t* g, const rgp_c3dconv_weights* w, rgp_stream_t stream) {
  RGP_REQUIRE(g && w, "rgp_c3dconv_set_weights: null argument");
  if (!g->ws) return set_err(RGP_EWORKSPACE, "rgp_c3dconv: workspace not bound");
  RGP_TRY(require_pointers(w, "rgp_c3dconv_set_weights", "weight"));
  RGP_REQUIRE(((size_t)w->proj_c3d_W & 15) == 0, "rgp_c3dconv_set_weights: proj_c3d_W must be 16-byte aligned");
  return RGP_BY_DTYPE(g->dtype, set_weights_impl, g, w, (hipStream_t)stream);
}

int rgp_c3dconv_forward(rgp_c3dconv_t* g, const float* c3d_input, float* logits, float* probs, rgp_stream_t stream) {
  RGP_TRY(check_ready(g));
  RGP_REQUIRE(c3d_input && logits, "rgp_c3dconv_forward: null argument");
  return RGP_BY_DTYPE(g->dtype, forward_impl, g, c3d_input, nullptr, logits, probs, (hipStream_t)stream);
}

int rgp_c3dconv_forward_rows(rgp_c3dconv_t* g, const void* c3d_rows, float* logits, float* probs, rgp_stream_t stream) {
  RGP_TRY(check_ready(g));
  RGP_REQUIRE(c3d_rows && logits, "rgp_c3dconv_forward_rows: null argument");
  RGP_REQUIRE(((size_t)c3d_rows & 15) == 0, "rgp_c3dconv_forward_rows: rows must be 16-byte aligned");
  return RGP_BY_DTYPE(g->dtype, forward_impl, g, nullptr, c3d_rows, logits, probs, (hipStream_t)stream);
}

int rgp_c3dconv_backward(rgp_c3dconv_t* g, const float* logits, const float* probs, const float* labels,
                         const rgp_c3dconv_weights* grads, int loss_type, rgp_stream_t stream) {
  RGP_TRY(check_ready(g));
  RGP_REQUIRE(labels && grads && (loss_type == 0 || loss_type == 1), "rgp_c3dconv_backward: bad arguments");
  RGP_REQUIRE(loss_type == 1 ? logits != nullptr : probs != nullptr, "rgp_c3dconv_backward: the loss needs %s", loss_type == 1 ? "logits" : "probs");
  if (!g->save) return set_err(RGP_ESTATE, "rgp_c3dconv_backward: the plan was not created with RGP_C3DCONV_SAVE_FOR_BACKWARD");
  if (!g->fwd_done) return set_err(RGP_ESTATE, "rgp_c3dconv_backward: no forward since the weights were set");
  RGP_TRY(require_pointers(grads, "rgp_c3dconv_backward", "gradient"));
  return RGP_BY_DTYPE(g->dtype, backward_impl, g, logits, probs, labels, grads, loss_type, (hipStream_t)stream);
}

int rgp_c3dconv_backward_input(rgp_c3dconv_t* g, float* d_rows, rgp_stream_t stream) {
  RGP_REQUIRE(g && d_rows, "rgp_c3dconv_backward_input: null argument");
  if (!g->ws || !g->save || !g->weights_set || !g->bwd_done) return set_err(RGP_ESTATE, "rgp_c3dconv_backward_input: call after rgp_c3dconv_backward");
  return g->pb.backward_input(g->ws, g->dtype, g->ws + g->dE.off, g->pb.M, d_rows, (hipStream_t)stream);
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
