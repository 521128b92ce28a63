// librgp_hip.so: gaze_grcn77 -- gaze_grcn's projection and ConvGRU with a per-pixel 128 -> 1 read-out on the 7x7 state
// instead of the up-sampling head.  Reference graph: /root/reference/models/gaze_grcn77.py:77-218.
//
// The plan owns an rgp_grcn sub-plan (512, 128), as rgp_cascade owns its bottom level: identity batch-norm parameters,
// scratch for the head fields the sub-plan's ABI asks for, its stage calls for the forward and
// rgp_grcn_backward_from_states for the backward.  The sub-plan's up-sampling head never runs; what runs behind the
// recurrence is head_point.hip.h on the sub-plan's fp32 states.
#include <cstring>
#include <string>

#include "rgp_grcn_plan.h"
#include "head_point.hip.h"

using namespace rgp;

struct rgp_grcn77 {
  int B = 0, T = 0, F = 0, dtype = RGP_BF16, save = 0;
  static constexpr int P = 512, S = 128;
  rgp_grcn* inner = nullptr;
  size_t off_inner = 0;
  Buf bn_id;         // [T*S] gamma = sqrt(1 + eps) | [T*S] beta = 0 | zeros for the sub-plan's unused head filters
  Buf scratch;       // the sub-plan's gradients of those fields (never read)
  Buf d_h;           // [F][49][S] fp32: the head's state gradient ("d_rcn_outputs")
  Buf part_W, part_b;
  size_t ws_bytes = 0;
  char* ws = nullptr;
  bool weights_set = false, fwd_done = false, bwd_done = false;
  const float *out_W = nullptr, *out_b = nullptr;
};

namespace {

constexpr size_t kHeadZeros = (size_t)25 * 64 * 128;          // the largest unused head filter (up_weight1)

__global__ void fill_kernel(float* p, float v, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

int check_ready(rgp_grcn77* g) {
  RGP_TRY(check_bound_and_set(g, "rgp_grcn77"));
  return grcn_check_error(g->inner);
}

int launch_head_fwd(const float* states, long long stride_b, long long stride_t, const rgp_grcn77* g, float* logits, float* probs,
                    hipStream_t s) {
  const int blocks = (g->F + HP_FRAMES_PER_BLOCK - 1) / HP_FRAMES_PER_BLOCK;
  head_point_fwd_kernel<<<blocks, 256, 0, s>>>(states, stride_b, stride_t, g->out_W, g->out_b, logits, probs, g->F, g->T);
  RGP_HIP(hipGetLastError());
  return RGP_OK;
}

// the sub-plan's states: time-major [T+1][B][49][S], frame (b, t) in slot t + 1
const float* plan_states(const rgp_grcn77* g) {
  return (const float*)(g->inner->ws + g->inner->hall.off) + (size_t)g->B * 49 * rgp_grcn77::S;
}

int tail(rgp_grcn77* g, float* logits, float* probs, rgp_stream_t stream) {
  RGP_TRY(rgp_convgru_xconv_fwd(g->inner, stream));
  RGP_TRY(rgp_convgru_seq_fwd(g->inner, stream));
  g->fwd_done = !g->inner->stream.on;
  g->bwd_done = false;
  return launch_head_fwd(plan_states(g), 49LL * rgp_grcn77::S, (long long)g->B * 49 * rgp_grcn77::S, g, logits, probs,
                         (hipStream_t)stream);
}

}  // namespace

extern "C" {

int rgp_grcn77_create(rgp_grcn77_t** plan, int batch, int n_steps, int dtype, int flags) {
  RGP_REQUIRE(plan, "rgp_grcn77_create: null out pointer");
  RGP_REQUIRE((flags & ~(RGP_GRCN77_SAVE_FOR_BACKWARD | RGP_GRCN77_PER_STEP)) == 0, "rgp_grcn77_create: unknown flags 0x%x", flags);
  RGP_REQUIRE(batch > 0 && n_steps > 0, "rgp_grcn77_create: batch=%d n_steps=%d", batch, n_steps);
  RGP_REQUIRE(dtype == RGP_F32 || dtype == RGP_BF16, "rgp_grcn77_create: dtype %d", dtype);
  rgp_grcn77* g = new rgp_grcn77();
  g->B = batch; g->T = n_steps; g->F = batch * n_steps; g->dtype = dtype;
  g->save = (flags & RGP_GRCN77_SAVE_FOR_BACKWARD) != 0;
  // (the flag values are those of RGP_GRCN_*; the sub-plan's own head is never run: no fold)
  const int rc = rgp_grcn_create(&g->inner, batch, n_steps, rgp_grcn77::P, rgp_grcn77::S, dtype,
                                 (g->save ? RGP_GRCN_SAVE_FOR_BACKWARD : 0) | ((flags & RGP_GRCN77_PER_STEP) ? RGP_GRCN_PER_STEP : 0) |
                                     RGP_GRCN_UNFOLDED_HEAD);
  if (rc != RGP_OK) { delete g; return rc; }
  const size_t nbn = (size_t)n_steps * rgp_grcn77::S;
  Arena a;
  g->off_inner = a.take(rgp_grcn_workspace_bytes(g->inner));
  g->bn_id = take(a, (2 * nbn + kHeadZeros) * 4);
  if (g->save) {
    g->scratch = take(a, (2 * nbn + kHeadZeros + 25 * 32 * 64 + 49 * 12 * 32 + 16 + 16) * 4);
    g->d_h = take(a, (size_t)g->F * 49 * rgp_grcn77::S * 4);
    g->part_W = take(a, (size_t)g->F * rgp_grcn77::S * 4);
    g->part_b = take(a, (size_t)g->F * 4);
  }
  g->ws_bytes = a.off;
  *plan = g;
  return RGP_OK;
}

int rgp_grcn77_destroy(rgp_grcn77_t* g) {
  if (g) {
    if (g->inner) rgp_grcn_destroy(g->inner);
    delete g;
  }
  return RGP_OK;
}

size_t rgp_grcn77_workspace_bytes(const rgp_grcn77_t* plan) { return plan ? plan->ws_bytes : 0; }

int rgp_grcn77_bind_workspace(rgp_grcn77_t* g, void* workspace, size_t bytes, rgp_stream_t stream) {
  RGP_TRY(check_bind("rgp_grcn77_bind_workspace", g, workspace, bytes));
  hipStream_t s = (hipStream_t)stream;
  g->ws = (char*)workspace;
  g->weights_set = g->fwd_done = g->bwd_done = false;
  RGP_HIP(hipMemsetAsync(g->ws + g->bn_id.off, 0, g->ws_bytes - g->bn_id.off, s));
  RGP_TRY(rgp_grcn_bind_workspace(g->inner, g->ws + g->off_inner, rgp_grcn_workspace_bytes(g->inner), stream));
  // the sub-plan's per-timestep batch-norm as the identity: gamma = sqrt(1 + eps), beta = 0 (rgp_cascade.hip does the same)
  const int nbn = g->T * rgp_grcn77::S;
  fill_kernel<<<(nbn + 255) / 256, 256, 0, s>>>((float*)(g->ws + g->bn_id.off), sqrtf(1.0f + 1e-3f), nbn);
  RGP_HIP(hipGetLastError());
  return RGP_OK;
}

int rgp_grcn77_set_weights(rgp_grcn77_t* g, const rgp_grcn77_weights* w, rgp_stream_t stream) {
  RGP_REQUIRE(g && w, "rgp_grcn77_set_weights: null argument");
  if (!g->ws) return set_err(RGP_EWORKSPACE, "rgp_grcn77: workspace not bound");
  RGP_TRY(require_pointers(w, "rgp_grcn77_set_weights", "weight"));
  RGP_REQUIRE(((size_t)w->out_W & 15) == 0, "rgp_grcn77_set_weights: out_W must be 16-byte aligned");
  rgp_grcn_weights iw;
  memset(&iw, 0, sizeof(iw));
  iw.proj_c3d_W = w->proj_c3d_W; iw.proj_c3d_b = w->proj_c3d_b;
  iw.gru_Wz = w->gru_Wz; iw.gru_Uz = w->gru_Uz; iw.gru_Wr = w->gru_Wr; iw.gru_Ur = w->gru_Ur; iw.gru_W = w->gru_W; iw.gru_U = w->gru_U;
  const float* bn = (const float*)(g->ws + g->bn_id.off);
  const size_t nbn = (size_t)g->T * rgp_grcn77::S;
  iw.bn_gamma = bn; iw.bn_beta = bn + nbn;
  const float* zeros = bn + 2 * nbn;
  iw.up_weight1 = zeros; iw.up_weight2 = zeros; iw.up_weight3 = zeros; iw.out_W = zeros; iw.out_b = zeros;
  RGP_TRY(rgp_grcn_set_weights(g->inner, &iw, stream));
  g->out_W = w->out_W;
  g->out_b = w->out_b;
  g->weights_set = true;
  g->fwd_done = g->bwd_done = false;
  return RGP_OK;
}

int rgp_grcn77_forward(rgp_grcn77_t* g, const float* c3d_input, float* logits, float* probs, rgp_stream_t stream) {
  RGP_TRY(check_ready(g));
  RGP_REQUIRE(c3d_input && logits, "rgp_grcn77_forward: null argument");
  RGP_TRY(rgp_proj_fwd(g->inner, c3d_input, stream));
  return tail(g, logits, probs, stream);
}

int rgp_grcn77_forward_rows(rgp_grcn77_t* g, const void* c3d_rows, float* logits, float* probs, rgp_stream_t stream) {
  RGP_TRY(check_ready(g));
  RGP_REQUIRE(c3d_rows && logits, "rgp_grcn77_forward_rows: null argument");
  RGP_REQUIRE(((size_t)c3d_rows & 15) == 0, "rgp_grcn77_forward_rows: rows must be 16-byte aligned");
  RGP_TRY(grcn_proj_rows_fwd(g->inner, c3d_rows, (hipStream_t)stream));
  return tail(g, logits, probs, stream);
}

size_t rgp_grcn77_state_elems(const rgp_grcn77_t* g) { return g ? rgp_grcn_state_elems(g->inner) : 0; }

// The state goes through the sub-plan (its batch-norm is the identity in every slot: no phase); head_point reads the states as ever.
int rgp_grcn77_forward_stream(rgp_grcn77_t* g, const float* c3d_input, const void* c3d_rows, const float* state_in, float* state_out,
                              int n_valid, float* logits, float* probs, rgp_stream_t stream) {
  RGP_REQUIRE(g, "rgp_grcn77_forward_stream: null plan");
  RGP_TRY(check_stream_args("rgp_grcn77_forward_stream", g->T, c3d_input, c3d_rows, state_in, state_out, n_valid, 0, logits));
  RGP_TRY(check_ready(g));
  rgp_grcn* in = g->inner;
  StreamScope call(in->stream, state_in, state_out, n_valid);
  g->fwd_done = false;                                     // no backward behind a started streaming call (RGP_ESTATE)
  RGP_TRY(c3d_input ? rgp_proj_fwd(in, c3d_input, stream) : grcn_proj_rows_fwd(in, c3d_rows, (hipStream_t)stream));
  RGP_TRY(tail(g, logits, probs, stream));
  return grcn_state_out(in, (hipStream_t)stream);
}

int rgp_grcn77_head_fwd(rgp_grcn77_t* g, const float* states, float* logits, float* probs, rgp_stream_t stream) {
  RGP_TRY(check_ready(g));
  RGP_REQUIRE(logits, "rgp_grcn77_head_fwd: null logits");
  if (!states) {
    if (!g->fwd_done) return set_err(RGP_ESTATE, "rgp_grcn77_head_fwd: no forward since the weights were set");
    return launch_head_fwd(plan_states(g), 49LL * rgp_grcn77::S, (long long)g->B * 49 * rgp_grcn77::S, g, logits, probs,
                           (hipStream_t)stream);
  }
  RGP_REQUIRE(((size_t)states & 15) == 0, "rgp_grcn77_head_fwd: states must be 16-byte aligned");
  return launch_head_fwd(states, (long long)g->T * 49 * rgp_grcn77::S, 49LL * rgp_grcn77::S, g, logits, probs, (hipStream_t)stream);
}

int rgp_grcn77_backward(rgp_grcn77_t* g, const float* logits, const float* probs, const float* labels,
                        const rgp_grcn77_weights* grads, int loss_type, rgp_stream_t stream) {
  RGP_TRY(check_ready(g));
  RGP_REQUIRE(labels && grads && (loss_type == 0 || loss_type == 1), "rgp_grcn77_backward: bad arguments");
  RGP_REQUIRE(loss_type == 1 ? logits != nullptr : probs != nullptr, "rgp_grcn77_backward: the loss needs %s", loss_type == 1 ? "logits" : "probs");
  if (!g->save) return set_err(RGP_ESTATE, "rgp_grcn77_backward: the plan was not created with RGP_GRCN77_SAVE_FOR_BACKWARD");
  if (!g->fwd_done) return set_err(RGP_ESTATE, "rgp_grcn77_backward: no forward since the weights were set (a streaming call is none: no truncated BPTT)");
  RGP_TRY(require_pointers(grads, "rgp_grcn77_backward", "gradient"));
  hipStream_t s = (hipStream_t)stream;
  constexpr int S = rgp_grcn77::S;
  float* d_h = (float*)(g->ws + g->d_h.off);
  float* part_W = (float*)(g->ws + g->part_W.off);
  float* part_b = (float*)(g->ws + g->part_b.off);
  const int blocks = (g->F + HP_FRAMES_PER_BLOCK - 1) / HP_FRAMES_PER_BLOCK;
  head_point_bwd_kernel<<<blocks, 256, 0, s>>>(plan_states(g), 49LL * S, (long long)g->B * 49 * S, g->out_W, loss_type == 1 ? logits : probs,
                                               labels, loss_type, 1.0f / (float)g->F, d_h, part_W, part_b, g->F, g->T);
  head_point_sum_kernel<<<S / 16 + 1, 256, 0, s>>>(part_W, part_b, (float*)grads->out_W, (float*)grads->out_b, g->F);
  RGP_HIP(hipGetLastError());
  rgp_grcn_weights ig;
  float* sc = (float*)(g->ws + g->scratch.off);
  const size_t nbn = (size_t)g->T * S;
  ig.proj_c3d_W = grads->proj_c3d_W; ig.proj_c3d_b = grads->proj_c3d_b;
  ig.gru_Wz = grads->gru_Wz; ig.gru_Uz = grads->gru_Uz; ig.gru_Wr = grads->gru_Wr; ig.gru_Ur = grads->gru_Ur;
  ig.gru_W = grads->gru_W; ig.gru_U = grads->gru_U;
  ig.bn_gamma = sc; sc += nbn;
  ig.bn_beta = sc; sc += nbn;
  ig.up_weight1 = sc; sc += kHeadZeros;
  ig.up_weight2 = sc; sc += 25 * 32 * 64;
  ig.up_weight3 = sc; sc += 49 * 12 * 32;
  ig.out_W = sc; sc += 16;
  ig.out_b = sc;
  RGP_TRY(rgp_grcn_backward_from_states(g->inner, d_h, &ig, stream));
  g->bwd_done = true;
  return RGP_OK;
}

int rgp_grcn77_backward_input(rgp_grcn77_t* g, float* d_rows, rgp_stream_t stream) {
  RGP_REQUIRE(g && d_rows, "rgp_grcn77_backward_input: null argument");
  if (!g->ws || !g->save || !g->weights_set || !g->bwd_done) return set_err(RGP_ESTATE, "rgp_grcn77_backward_input: call after rgp_grcn77_backward");
  return rgp_grcn_backward_input(g->inner, d_rows, stream);
}

int rgp_grcn77_status(rgp_grcn77_t* g, rgp_stream_t stream) {
  RGP_REQUIRE(g, "rgp_grcn77_status: null plan");
  return rgp_grcn_status(g->inner, stream);
}

int rgp_grcn77_persistent_workgroups(const rgp_grcn77_t* g) { return g ? rgp_grcn_persistent_workgroups(g->inner) : 0; }

size_t rgp_grcn77_buffer_elems(const rgp_grcn77_t* g, const char* name) {
  if (!g || !name) return 0;
  const std::string n(name);
  if (n == "c3d_embedded" || n == "rcn_outputs") return rgp_grcn_buffer_elems(g->inner, name);
  if (n == "d_rcn_outputs" && g->save) return (size_t)g->F * 49 * rgp_grcn77::S;
  return 0;
}

int rgp_grcn77_read_buffer(rgp_grcn77_t* g, const char* name, float* dst, rgp_stream_t stream) {
  RGP_REQUIRE(g && g->ws && name && dst, "rgp_grcn77_read_buffer: null argument");
  if (rgp_grcn77_buffer_elems(g, name) == 0) return set_err(RGP_EINVAL, "rgp_grcn77_read_buffer: unknown buffer '%s'", name);
  if (std::string(name) == "d_rcn_outputs") {
    if (!g->bwd_done) return set_err(RGP_ESTATE, "rgp_grcn77_read_buffer: 'd_rcn_outputs' exists after rgp_grcn77_backward");
    RGP_HIP(hipMemcpyAsync(dst, g->ws + g->d_h.off, g->d_h.bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return RGP_OK;
  }
  return rgp_grcn_read_buffer(g->inner, name, dst, stream);
}

}  // extern "C"
