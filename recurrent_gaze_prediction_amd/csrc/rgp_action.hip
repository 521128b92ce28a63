// librgp_hip.so: the action classifier on gaze-attended C3D features -- plan object and launches (kernels: action_fc.hip.h).
// Reference graph: models/action_classification.py:210-292, basic_graphs.py:149-166.
//
//   [a = gazemap Wg]  ->  action_fc1_fwd: per-slab partial sums of x W1, x = c3d * a applied on load
//                     ->  action_tail (one workgroup): slab sum in order, + b1, the rest of the network, loss, small gradients
//   training:         ->  action_fc1_update: dx, g = x^T d h1, Adam / SGD+L2 and the operand copy in ONE pass over W1 (m, v)
//                     ->  d a, d Wg  ->  the small variables' optimizer step (rgp_adam_clip_step without clipping / plain SGD)
//
// Second implementation (RGP_ACTION_UNFUSED): x is materialised, the same fc1 kernel runs on it without the attention
// fusion, dW1 and dx come from plain kernels and W1 takes rgp_adam_clip_step (SVM: its SGD + L2 kernel) followed by a
// re-pack of the operand copy.  No float atomics anywhere: two runs of a plan give the same bits.
//
// The plan keeps the fp32 master pointers of set_weights (and the Adam slots of bind_slots) and updates them in place.
#include <algorithm>
#include <cmath>
#include <string>

#include "gaze_stages.h"
#include "action_fc.hip.h"

using namespace rgp;

namespace {
constexpr int N_SMALL = 6;      // Wg, b1, W2, b2, W3, b3: the variables behind W1 in rgp_action_weights
}

struct rgp_action {
  int B = 0, C = 0, K = 0, N = 0, Npad = 0, mode = RGP_ACTION_NN, dtype = RGP_BF16, nslab = 0, MT = 1;
  bool gaze = false, save = false, unfused = false;
  bool weights_set = false, slots_set = false, fc1_done = false;
  size_t ws_bytes = 0;
  char* ws = nullptr;
  rgp_action_weights w{}, sm{}, sv{};      // masters as last set; Adam slots
  Buf w1op, a, part, wsq, h1, h2, logits, ypred, dlog, dh2, dh1, loss, dx, da, gsmall, adam_ws, c3dbuf, xbuf, dw1;
  long long small_n[N_SMALL] = {0, 0, 0, 0, 0, 0}, small_off[N_SMALL] = {0, 0, 0, 0, 0, 0}, small_total = 0;
};

namespace {

float* const* small_ptrs(const rgp_action_weights* w) { return (float* const*)&w->Wg; }
float* F(const rgp_action* g, const Buf& b) { return (float*)(g->ws + b.off); }

int check_ready(rgp_action* g) { return check_bound_and_set(g, "rgp_action"); }

int run_proj(rgp_action* g, const float* gazemap, hipStream_t s) {
  action_gaze_proj_kernel<<<g->B, 1024, 0, s>>>(gazemap, g->w.Wg, F(g, g->a));
  RGP_HIP(hipGetLastError());
  return RGP_OK;
}

template <typename T, int MT>
int launch_fwd(rgp_action* g, const float* x, const float* a, hipStream_t s) {
  const bool svm = g->mode == RGP_ACTION_SVM;
  action_fc1_fwd_kernel<T, MT><<<dim3(g->nslab, (g->Npad + 63) / 64), 256, 0, s>>>(
      x, a, (const T*)(g->ws + g->w1op.off), F(g, g->part), svm ? g->w.W1 : nullptr, svm ? F(g, g->wsq) : nullptr, g->B, g->K, g->N,
      g->Npad);
  RGP_HIP(hipGetLastError());
  return RGP_OK;
}

// fc1 forward from c3d [B][C][49] fp32: [a] -> [x] -> per-slab partial sums
template <typename T>
int fc1_fwd_impl(rgp_action* g, const float* c3d, const float* gazemap, hipStream_t s) {
  const float *x = c3d, *a = nullptr;
  if (g->gaze) {
    RGP_TRY(run_proj(g, gazemap, s));
    a = F(g, g->a);
    if (g->unfused) {
      const long long total = (long long)g->B * g->K;
      action_x_kernel<<<(int)std::min<long long>((total + 255) / 256, 8192), 256, 0, s>>>(c3d, a, F(g, g->xbuf), g->K, total);
      RGP_HIP(hipGetLastError());
      x = F(g, g->xbuf);
      a = nullptr;
    }
  }
  int rc;
  switch (g->MT) {
    case 1: rc = launch_fwd<T, 1>(g, x, a, s); break;
    case 2: rc = launch_fwd<T, 2>(g, x, a, s); break;
    case 3: rc = launch_fwd<T, 3>(g, x, a, s); break;
    default: rc = launch_fwd<T, 4>(g, x, a, s); break;
  }
  RGP_TRY(rc);
  g->fc1_done = true;
  return RGP_OK;
}

int run_tail(rgp_action* g, const float* labels, bool train, float* logits_out, float* ypred_out, float* loss_out, hipStream_t s) {
  ActionTailArgs p;
  memset(&p, 0, sizeof(p));
  p.part = F(g, g->part); p.wsq = F(g, g->wsq); p.nslab = g->nslab; p.B = g->B; p.train = train ? 1 : 0;
  p.b1 = g->w.b1; p.W2 = g->w.W2; p.b2 = g->w.b2; p.W3 = g->w.W3; p.b3 = g->w.b3; p.labels = labels;
  p.h1 = F(g, g->h1); p.h2 = F(g, g->h2); p.logits = F(g, g->logits); p.ypred = F(g, g->ypred); p.dlog = F(g, g->dlog);
  p.dh2 = F(g, g->dh2); p.dh1 = F(g, g->dh1); p.loss = F(g, g->loss);
  p.logits_out = logits_out; p.ypred_out = ypred_out; p.loss_out = loss_out;
  float* gs = F(g, g->gsmall);
  p.g_b1 = gs + g->small_off[1]; p.g_W2 = gs + g->small_off[2]; p.g_b2 = gs + g->small_off[3]; p.g_W3 = gs + g->small_off[4];
  p.g_b3 = gs + g->small_off[5];
  if (g->mode == RGP_ACTION_SVM) action_svm_tail_kernel<<<1, 1024, 0, s>>>(p);
  else action_tail_kernel<<<1, 1024, 0, s>>>(p);
  RGP_HIP(hipGetLastError());
  return RGP_OK;
}

template <typename T, int MT>
int launch_update(rgp_action* g, const float* c3d, const float* a, const float* dh1, float* dx, float lr_t, hipStream_t s) {
  auto kern = action_fc1_update_kernel<T, MT>;
  constexpr int smem = 16 * MT * (ACT_LDD + ACT_UPD_ROWS) * 4;      // (constant per instantiation: ensure_dyn_smem sets the limit once)
  RGP_TRY(ensure_dyn_smem((const void*)kern, smem));
  kern<<<(g->K + ACT_UPD_ROWS - 1) / ACT_UPD_ROWS, 256, smem, s>>>(c3d, a, dh1, g->w.W1, g->sm.W1, g->sv.W1, (T*)(g->ws + g->w1op.off), dx,
                                                                   g->B, g->K, lr_t, 0.9f, 0.999f, (float)(1.0 - 0.9), (float)(1.0 - 0.999), 1e-8f);
  RGP_HIP(hipGetLastError());
  return RGP_OK;
}

// lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t), t = step + 1, in double from beta1 = 0.9, beta2 = 0.999 (rgp_adam_clip_step raises its
// fp32 betas: its lr_t differs in the sixth digit)
float adam_lr_t(int step, float lr) {
  const double t = (double)step + 1.0;
  return (float)((double)lr * sqrt(1.0 - pow(0.999, t)) / (1.0 - pow(0.9, t)));
}

// The pass over W1 (+ d a, d Wg on plans with a gaze map); `a` must be current.
template <typename T>
int fc1_update_impl(rgp_action* g, const float* c3d, const float* gazemap, const float* dh1, int step, float lr, hipStream_t s) {
  const bool svm = g->mode == RGP_ACTION_SVM;
  const float* a = g->gaze ? F(g, g->a) : nullptr;
  float* dx = g->gaze ? F(g, g->dx) : nullptr;
  T* wop = (T*)(g->ws + g->w1op.off);
  const long long nW = (long long)g->K * g->N;
  if (!g->unfused) {
    if (svm) {
      action_svm_update_kernel<T><<<(g->K + 255) / 256, 256, 0, s>>>(c3d, a, dh1, g->w.W1, wop, dx, g->B, g->K, lr);
      RGP_HIP(hipGetLastError());
    } else {
      const float lr_t = adam_lr_t(step, lr);
      int rc;
      switch (g->MT) {
        case 1: rc = launch_update<T, 1>(g, c3d, a, dh1, dx, lr_t, s); break;
        case 2: rc = launch_update<T, 2>(g, c3d, a, dh1, dx, lr_t, s); break;
        case 3: rc = launch_update<T, 3>(g, c3d, a, dh1, dx, lr_t, s); break;
        default: rc = launch_update<T, 4>(g, c3d, a, dh1, dx, lr_t, s); break;
      }
      RGP_TRY(rc);
    }
  } else {
    const float* x = c3d;
    if (g->gaze) {
      const long long total = (long long)g->B * g->K;
      action_x_kernel<<<(int)std::min<long long>((total + 255) / 256, 8192), 256, 0, s>>>(c3d, a, F(g, g->xbuf), g->K, total);
      x = F(g, g->xbuf);
      action_dx_plain_kernel<<<(g->K + 3) / 4, 256, 0, s>>>(g->w.W1, dh1, dx, g->B, g->K, g->N, svm ? ACT_SVM_C : 1.f);
    }
    const int blocks = (int)std::min<long long>((nW + 255) / 256, 8192);
    action_dw1_plain_kernel<<<blocks, 256, 0, s>>>(x, dh1, F(g, g->dw1), g->B, g->K, g->N);
    RGP_HIP(hipGetLastError());
    if (svm) action_sgd_l2_kernel<<<blocks, 256, 0, s>>>(g->w.W1, F(g, g->dw1), nW, lr);
    else RGP_TRY(rgp_adam_clip_step(g->w.W1, F(g, g->dw1), g->sm.W1, g->sv.W1, nW, F(g, g->adam_ws), step, lr, 0.9f, 0.999f, 1e-8f, 0.f,
                                    nullptr, (rgp_stream_t)s));
    action_pack_kernel<T><<<blocks, 256, 0, s>>>(g->w.W1, wop, nW, g->N, g->Npad);
    RGP_HIP(hipGetLastError());
  }
  if (g->gaze) {
    action_da_kernel<<<g->B, 1024, 0, s>>>(c3d, dx, F(g, g->da), g->C);
    action_dwg_kernel<<<(ACT_GM * ACT_P + 255) / 256, 256, 0, s>>>(gazemap, F(g, g->da), F(g, g->gsmall) + g->small_off[0], g->B);
    RGP_HIP(hipGetLastError());
  }
  return RGP_OK;
}

// The small variables: one rgp_adam_clip_step over their range of the caller's flat buffer when they (and their slots)
// lie back to back in the order of rgp_action_weights, one call per variable otherwise.  SVM: plain SGD.
int small_step(rgp_action* g, int step, float lr, hipStream_t s) {
  float* const* p = small_ptrs(&g->w);
  float* const* m = small_ptrs(&g->sm);
  float* const* v = small_ptrs(&g->sv);
  float* gs = F(g, g->gsmall);
  if (g->mode == RGP_ACTION_SVM) {
    for (int i = 0; i < 2; ++i)
      if (g->small_n[i]) action_sgd_kernel<<<(int)std::min<long long>((g->small_n[i] + 255) / 256, 1024), 256, 0, s>>>(p[i], gs + g->small_off[i], g->small_n[i], lr);
    RGP_HIP(hipGetLastError());
    return RGP_OK;
  }
  int first = g->gaze ? 0 : 1;
  bool contig = true;
  for (int i = first; i + 1 < N_SMALL; ++i)
    contig &= p[i + 1] == p[i] + g->small_n[i] && m[i + 1] == m[i] + g->small_n[i] && v[i + 1] == v[i] + g->small_n[i];
  if (contig)
    return rgp_adam_clip_step(p[first], gs + g->small_off[first], m[first], v[first], g->small_total - g->small_off[first], F(g, g->adam_ws),
                              step, lr, 0.9f, 0.999f, 1e-8f, 0.f, nullptr, (rgp_stream_t)s);
  for (int i = first; i < N_SMALL; ++i)
    RGP_TRY(rgp_adam_clip_step(p[i], gs + g->small_off[i], m[i], v[i], g->small_n[i], F(g, g->adam_ws), step, lr, 0.9f, 0.999f, 1e-8f, 0.f,
                               nullptr, (rgp_stream_t)s));
  return RGP_OK;
}

int check_struct(const rgp_action* g, const rgp_action_weights* w, const char* fn, const char* kind) {
  RGP_REQUIRE(w->W1 && w->b1, "%s: %s pointer W1 / b1 is null", fn, kind);
  RGP_REQUIRE(!g->gaze || w->Wg, "%s: %s pointer Wg is null (the plan uses the gaze map)", fn, kind);
  if (g->mode == RGP_ACTION_NN) RGP_REQUIRE(w->W2 && w->b2 && w->W3 && w->b3, "%s: a %s pointer of the NN layers is null", fn, kind);
  RGP_REQUIRE(((size_t)w->W1 & 15) == 0, "%s: W1 must be 16-byte aligned", fn);
  return RGP_OK;
}

template <typename T>
int pack_impl(rgp_action* g, hipStream_t s) {
  const long long nW = (long long)g->K * g->N;
  action_pack_kernel<T><<<(int)std::min<long long>((nW + 255) / 256, 8192), 256, 0, s>>>(g->w.W1, (T*)(g->ws + g->w1op.off), nW, g->N, g->Npad);
  RGP_HIP(hipGetLastError());
  return RGP_OK;
}

template <typename T>
int rows_impl(rgp_action* g, const void* rows, hipStream_t s) {
  const long long n = (long long)g->B * g->K;
  action_rows_to_c3d_kernel<T><<<(int)std::min<long long>((n + 255) / 256, 8192), 256, 0, s>>>((const T*)rows, F(g, g->c3dbuf), n);
  RGP_HIP(hipGetLastError());
  return RGP_OK;
}

size_t find_buffer(const rgp_action* g, const char* name, size_t* off) {
  const std::string n(name ? name : "");
  const size_t B = g->B, N = g->N;
  const bool nn = g->mode == RGP_ACTION_NN;
  if (n == "a" && g->gaze) { *off = g->a.off; return B * ACT_P; }
  if (n == "h1") { *off = g->h1.off; return B * N; }
  if (n == "h2" && nn) { *off = g->h2.off; return B * ACT_NH; }
  if (n == "loss") { *off = g->loss.off; return 1; }
  if (!g->save) return 0;
  if (n == "d_h1") { *off = g->dh1.off; return B * N; }
  if (n == "d_h2" && nn) { *off = g->dh2.off; return B * ACT_NH; }
  if (n == "d_logits" && nn) { *off = g->dlog.off; return B * ACT_NC; }
  if (n == "dx" && g->gaze) { *off = g->dx.off; return B * (size_t)g->K; }
  if (n == "d_a" && g->gaze) { *off = g->da.off; return B * ACT_P; }
  static const char* small[N_SMALL] = {"d_Wg", "d_b1", "d_W2", "d_b2", "d_W3", "d_b3"};
  for (int i = 0; i < N_SMALL; ++i)
    if (n == small[i] && g->small_n[i]) { *off = g->gsmall.off + (size_t)g->small_off[i] * 4; return (size_t)g->small_n[i]; }
  return 0;
}

}  // namespace

extern "C" {

int rgp_action_create(rgp_action_t** plan, int batch, int dim_feat, int mode, int dtype, int flags) {
  RGP_REQUIRE(plan, "rgp_action_create: null out pointer");
  RGP_REQUIRE((flags & ~(RGP_ACTION_USE_GAZEMAP | RGP_ACTION_SAVE_FOR_BACKWARD | RGP_ACTION_UNFUSED)) == 0,
              "rgp_action_create: unknown flags 0x%x", flags);
  RGP_REQUIRE(batch >= 1 && batch <= 64, "rgp_action_create: batch=%d outside [1, 64]", batch);
  RGP_REQUIRE(dim_feat >= 1 && dim_feat <= 8192, "rgp_action_create: dim_feat=%d", dim_feat);
  RGP_REQUIRE(mode == RGP_ACTION_NN || mode == RGP_ACTION_SVM, "rgp_action_create: mode %d", mode);
  RGP_REQUIRE(dtype == RGP_F32 || dtype == RGP_BF16, "rgp_action_create: dtype %d", dtype);
  rgp_action* g = new rgp_action();
  g->B = batch; g->C = dim_feat; g->K = ACT_P * dim_feat; g->mode = mode; g->dtype = dtype;
  g->N = mode == RGP_ACTION_NN ? ACT_NH : ACT_NC;
  g->Npad = mode == RGP_ACTION_NN ? ACT_NH : 16;
  g->nslab = (g->K + ACT_KS - 1) / ACT_KS;
  g->MT = (batch + 15) / 16;
  g->gaze = (flags & RGP_ACTION_USE_GAZEMAP) != 0;
  g->save = (flags & RGP_ACTION_SAVE_FOR_BACKWARD) != 0;
  g->unfused = (flags & RGP_ACTION_UNFUSED) != 0;
  const size_t B = batch, K = g->K, N = g->N;
  const bool nn = mode == RGP_ACTION_NN;
  const long long sn[N_SMALL] = {g->gaze ? ACT_GM * ACT_P : 0, (long long)N, nn ? ACT_NH * ACT_NH : 0, nn ? ACT_NH : 0,
                                 nn ? ACT_NH * ACT_NC : 0, nn ? ACT_NC : 0};
  for (int i = 0; i < N_SMALL; ++i) { g->small_n[i] = sn[i]; g->small_off[i] = g->small_total; g->small_total += sn[i]; }
  Arena a;
  g->w1op = take(a, (size_t)g->nslab * ACT_KS * g->Npad * esize(dtype));
  g->a = take(a, B * ACT_P * 4);
  g->part = take(a, (size_t)g->nslab * B * N * 4);
  g->wsq = take(a, (size_t)g->nslab * 4);
  g->h1 = take(a, B * N * 4);
  g->h2 = take(a, B * ACT_NH * 4);
  g->logits = take(a, B * ACT_NC * 4);
  g->ypred = take(a, B * ACT_NC * 4);
  g->dlog = take(a, B * ACT_NC * 4);
  g->dh2 = take(a, B * ACT_NH * 4);
  g->dh1 = take(a, B * N * 4);
  g->loss = take(a, 4);
  g->gsmall = take(a, (size_t)g->small_total * 4);
  g->adam_ws = take(a, RGP_SQNORM_PARTIALS * 4);
  if (dim_feat == 1024) g->c3dbuf = take(a, B * K * 4);
  if (g->gaze && g->save) { g->dx = take(a, B * K * 4); g->da = take(a, B * ACT_P * 4); }
  if (g->gaze && g->unfused) g->xbuf = take(a, B * K * 4);
  if (g->save && g->unfused) g->dw1 = take(a, K * N * 4);
  g->ws_bytes = a.off;
  *plan = g;
  return RGP_OK;
}

int rgp_action_destroy(rgp_action_t* plan) {
  delete plan;
  return RGP_OK;
}

size_t rgp_action_workspace_bytes(const rgp_action_t* plan) { return plan ? plan->ws_bytes : 0; }

int rgp_action_bind_workspace(rgp_action_t* g, void* workspace, size_t bytes, rgp_stream_t stream) {
  RGP_TRY(check_bind("rgp_action_bind_workspace", g, workspace, bytes));
  g->ws = (char*)workspace;
  g->weights_set = g->fc1_done = false;
  RGP_HIP(hipMemsetAsync(g->ws, 0, g->ws_bytes, (hipStream_t)stream));   // (the operand copy's padding stays zero)
  return RGP_OK;
}

int rgp_action_set_weights(rgp_action_t* g, const rgp_action_weights* w, rgp_stream_t stream) {
  RGP_REQUIRE(g && w, "rgp_action_set_weights: null argument");
  if (!g->ws) return set_err(RGP_EWORKSPACE, "rgp_action: workspace not bound");
  RGP_TRY(check_struct(g, w, "rgp_action_set_weights", "weight"));
  g->w = *w;
  RGP_TRY(RGP_BY_DTYPE(g->dtype, pack_impl, g, (hipStream_t)stream));
  g->weights_set = true;
  g->fc1_done = false;
  return RGP_OK;
}

int rgp_action_get_weights(rgp_action_t* g, const rgp_action_weights* dst, rgp_stream_t stream) {
  RGP_TRY(check_ready(g));
  RGP_REQUIRE(dst, "rgp_action_get_weights: null argument");
  RGP_TRY(check_struct(g, dst, "rgp_action_get_weights", "destination"));
  const float* const* src = (const float* const*)&g->w;
  float* const* d = (float* const*)dst;
  const long long n[1 + N_SMALL] = {(long long)g->K * g->N, g->small_n[0], g->small_n[1], g->small_n[2], g->small_n[3], g->small_n[4],
                                    g->small_n[5]};
  for (int i = 0; i < 1 + N_SMALL; ++i)
    if (n[i] && d[i] != src[i]) RGP_HIP(hipMemcpyAsync(d[i], src[i], (size_t)n[i] * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return RGP_OK;
}

int rgp_action_bind_slots(rgp_action_t* g, const rgp_action_weights* m, const rgp_action_weights* v) {
  RGP_REQUIRE(g && m && v, "rgp_action_bind_slots: null argument");
  RGP_REQUIRE(g->mode == RGP_ACTION_NN, "rgp_action_bind_slots: SVM plans train with plain SGD and have no slots");
  RGP_TRY(check_struct(g, m, "rgp_action_bind_slots", "m slot"));
  RGP_TRY(check_struct(g, v, "rgp_action_bind_slots", "v slot"));
  g->sm = *m;
  g->sv = *v;
  g->slots_set = true;
  return RGP_OK;
}

int rgp_action_fc1_fwd(rgp_action_t* g, const float* c3d, const float* gazemap, rgp_stream_t stream) {
  RGP_TRY(check_ready(g));
  RGP_REQUIRE(c3d && (gazemap || !g->gaze), "rgp_action_fc1_fwd: null argument");
  return RGP_BY_DTYPE(g->dtype, fc1_fwd_impl, g, c3d, gazemap, (hipStream_t)stream);
}

int rgp_action_tail(rgp_action_t* g, const float* labels, rgp_stream_t stream) {
  RGP_TRY(check_ready(g));
  if (!g->fc1_done) return set_err(RGP_ESTATE, "rgp_action_tail: no rgp_action_fc1_fwd since the weights were set");
  RGP_REQUIRE(labels || !g->save, "rgp_action_tail: a training plan needs labels");
  return run_tail(g, labels, g->save, nullptr, nullptr, nullptr, (hipStream_t)stream);
}

int rgp_action_fc1_update(rgp_action_t* g, const float* c3d, const float* gazemap, const float* d_h1, int step, float lr,
                          rgp_stream_t stream) {
  RGP_TRY(check_ready(g));
  RGP_REQUIRE(c3d && d_h1 && (gazemap || !g->gaze) && step >= 0, "rgp_action_fc1_update: bad arguments");
  if (!g->save) return set_err(RGP_ESTATE, "rgp_action_fc1_update: the plan was not created with RGP_ACTION_SAVE_FOR_BACKWARD");
  if (g->mode == RGP_ACTION_NN && !g->slots_set) return set_err(RGP_ESTATE, "rgp_action_fc1_update: no Adam slots bound (rgp_action_bind_slots)");
  hipStream_t s = (hipStream_t)stream;
  if (g->gaze) RGP_TRY(run_proj(g, gazemap, s));
  g->fc1_done = false;                    // W1 changes: the partial sums are stale
  return RGP_BY_DTYPE(g->dtype, fc1_update_impl, g, c3d, gazemap, d_h1, step, lr, s);
}

int rgp_action_forward(rgp_action_t* g, const float* c3d, const float* gazemap, float* logits, float* y_pred, rgp_stream_t stream) {
  RGP_TRY(check_ready(g));
  RGP_REQUIRE(c3d && (gazemap || !g->gaze), "rgp_action_forward: null argument");
  hipStream_t s = (hipStream_t)stream;
  RGP_TRY(RGP_BY_DTYPE(g->dtype, fc1_fwd_impl, g, c3d, gazemap, s));
  return run_tail(g, nullptr, false, logits, y_pred, nullptr, s);
}

int rgp_action_forward_rows(rgp_action_t* g, const void* c3d_rows, const float* gazemap, float* logits, float* y_pred,
                            rgp_stream_t stream) {
  RGP_TRY(check_ready(g));
  RGP_REQUIRE(c3d_rows && (gazemap || !g->gaze), "rgp_action_forward_rows: null argument");
  RGP_REQUIRE(g->C == 1024, "rgp_action_forward_rows: conv5b rows have 1024 channels, the plan has %d", g->C);
  RGP_TRY(RGP_BY_DTYPE(g->dtype, rows_impl, g, c3d_rows, (hipStream_t)stream));
  return rgp_action_forward(g, F(g, g->c3dbuf), gazemap, logits, y_pred, stream);
}

int rgp_action_loss(rgp_action_t* g, const float* labels, float* loss_dev, rgp_stream_t stream) {
  RGP_TRY(check_ready(g));
  RGP_REQUIRE(labels && loss_dev, "rgp_action_loss: null argument");
  if (!g->fc1_done) return set_err(RGP_ESTATE, "rgp_action_loss: no forward since the weights were set");
  return run_tail(g, labels, false, nullptr, nullptr, loss_dev, (hipStream_t)stream);
}

int rgp_action_train_step(rgp_action_t* g, const float* c3d, const float* gazemap, const float* labels, int step, float lr,
                          float* loss_dev, rgp_stream_t stream) {
  RGP_TRY(check_ready(g));
  RGP_REQUIRE(c3d && labels && (gazemap || !g->gaze) && step >= 0, "rgp_action_train_step: bad arguments");
  if (!g->save) return set_err(RGP_ESTATE, "rgp_action_train_step: the plan was not created with RGP_ACTION_SAVE_FOR_BACKWARD");
  if (g->mode == RGP_ACTION_NN && !g->slots_set) return set_err(RGP_ESTATE, "rgp_action_train_step: no Adam slots bound (rgp_action_bind_slots)");
  hipStream_t s = (hipStream_t)stream;
  RGP_TRY(RGP_BY_DTYPE(g->dtype, fc1_fwd_impl, g, c3d, gazemap, s));
  RGP_TRY(run_tail(g, labels, true, nullptr, nullptr, loss_dev, s));
  RGP_TRY(RGP_BY_DTYPE(g->dtype, fc1_update_impl, g, c3d, gazemap, (const float*)F(g, g->dh1), step, lr, s));
  RGP_TRY(small_step(g, step, lr, s));
  g->fc1_done = false;                                   // (the intermediates of this step stay readable; W1 has moved on)
  return RGP_OK;
}

size_t rgp_action_buffer_elems(const rgp_action_t* g, const char* name) {
  size_t off;
  return g ? find_buffer(g, name, &off) : 0;
}

int rgp_action_read_buffer(rgp_action_t* g, const char* name, float* dst, rgp_stream_t stream) {
  RGP_REQUIRE(g && g->ws && name && dst, "rgp_action_read_buffer: null argument");
  size_t off = 0;
  const size_t n = find_buffer(g, name, &off);
  if (!n) return set_err(RGP_EINVAL, "rgp_action_read_buffer: unknown buffer '%s'", name);
  RGP_HIP(hipMemcpyAsync(dst, g->ws + off, n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return RGP_OK;
}

}  // extern "C"
