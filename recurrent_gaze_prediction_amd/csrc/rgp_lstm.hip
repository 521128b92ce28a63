// librgp_hip.so: gaze_lstm, the ConvLSTM member of the gaze family -- plan object, forward (persistent sequence kernel or
// per-timestep launches) and the backward (BPTT as one persistent launch or as per-timestep launches).
// Reference graph: /root/reference/models/gaze_lstm.py:178-353, cell :103-133 (three quirks kept as written: g reuses
// W_hi, o reads the OLD c, W_hc is a variable nothing reads).
//
//   [nchw_to_rows] -> projection GEMM (+ bias) -> E (halo-padded) -> hoisted x convolution, ONE GEMM with N = 512
//   (column 4 c + {i, f, g, o}) -> recurrence -> h_t images -> folded head GEMM (head_fold.hip.h, identity batch-norm)
//   -> col2im (+ out_b) -> softmax
// recurrence, two implementations:
//   persistent (bf16, <= 64 clips, enough CUs): convlstm_seq.hip.h, all T steps in one launch
//   per step   (any plan; RGP_LSTM_PER_STEP):   one igemm launch per step on h_{t-1} with the EpiLstm epilogue
// BPTT, two implementations (the rest of the backward is common to both and reads the same dpre image):
//   persistent (RGP_LSTM_BPTT_PERSISTENT; bf16 training plans, <= 64 clips, enough CUs): convlstm_bptt.hip.h, one launch
//   per step   (every other plan):                 lstm_bwd_step_kernel + the step's input-gradient GEMM, 2 T - 1 launches
// h_t lives as halo-padded operand images [B][T+1][81][S] (slot 0 = the zero state): step t's GEMM reads slot t and writes
// slot t+1, the head reads slots 1..T (its GEMM "image" is a clip), and the backward's filter gradients read slots 0..T-1.
#include <algorithm>
#include <string>

#include "gaze_stages.h"
#include "wgrad_launch.h"
#include "convlstm_seq.hip.h"
#include "convlstm_bptt.hip.h"
#include "lstm_kernels.hip.h"

using namespace rgp;

struct rgp_lstm {
  int B = 0, T = 0, P = 512, S = 128, dtype = RGP_BF16, F = 0;
  bool save = false, fwd_done = false, bwd_done = false, weights_set = false;
  StreamCall stream;                       // rgp_lstm_forward_stream; slot 0 = that of hall / call / the h images
  Projection pj;                           // gaze_stages.h
  FoldedHead head;                         // on h_t: a GEMM "image" is a clip
  ConvDesc xconv, grec;
  Buf E, xpre, hall, call, gates, hseq, peep;
  Buf xch, seq_cnt, bptt_xch, bptt_cnt;
  SeqGroupPlan sg;                         // groups of the persistent kernels (none = per-step launches), error word, fault bits
  bool fwd_persistent = false;             // the plan selected convlstm_seq_kernel ...
  bool bptt_persistent = false;            // ... convlstm_bptt_kernel (each runs only where sg.resident() holds)
  size_t ws_bytes = 0;
  char* ws = nullptr;
  const float *proj_b = nullptr, *out_b = nullptr;
  // ---- training plans
  FoldedHeadBwd hb;
  ProjectionBwd pb;                        // with the GEMM-form weight gradients, as gaze_c3d_conv
  ConvDesc b_rec, b_x;
  std::vector<int> koff_c;
  size_t o_koff_c = 0;
  Buf dy, dh_carry, dc_carry, dpre, dE;
  rgp_lstm_weights w;
};

namespace {

// What flags = 0 selects for plans the persistent kernel can run (bf16, <= 64 clips).  The rule ("gaze_lstm"): the
// persistent kernel only if scripts/bench_lstm.py measures it faster than the per-step path at both of its shapes on one box.
constexpr bool LSTM_DEFAULT_PERSISTENT = true;
// The same for the BPTT of training plans without RGP_LSTM_BPTT_PERSISTENT, by the same rule: the persistent BPTT only if
// scripts/bench_lstm.py measures it faster than the per-step loop at both of its shapes on one box.  (Flipping it changes
// which path the gradient tests of tests/test_lstm_gpu.py cover: a change of its own.)
constexpr bool LSTM_DEFAULT_BPTT_PERSISTENT = false;

std::vector<int> pad_tab9(int C) {
  std::vector<int> t;
  for (int y = 0; y < 7; ++y)
    for (int x = 0; x < 7; ++x) t.push_back(((y + 1) * 9 + x + 1) * C);
  return t;
}

int lstm_check_error(rgp_lstm* g) {
  return g->sg.check_err("rgp_lstm: a persistent ConvLSTM launch of this plan lost a group member (another launch was "
                         "resident on the device?): its outputs were NaN-poisoned");
}

int check_ready(rgp_lstm* g) {
  RGP_TRY(check_bound_and_set(g, "rgp_lstm"));
  return lstm_check_error(g);
}

template <typename T>
int set_weights_impl(rgp_lstm* g, const rgp_lstm_weights* w, hipStream_t s) {
  char* ws = g->ws;
  const int P = g->P, S = g->S;
  PackBatch<T> pk(ws, s);
  RGP_TRY(g->pj.pack(pk, w->proj_c3d_W));
  // gate-interleaved columns 4 c + q (lstm_kernels.hip.h): x parts q = i, f, g, o; recurrent q = 0 W_hi, 1 W_hf, 3 W_ho
  RGP_TRY(pk.add(g->xconv, w->W_xi, S, 0, 0, 0, 4));
  RGP_TRY(pk.add(g->xconv, w->W_xf, S, 1, 0, 0, 4));
  RGP_TRY(pk.add(g->xconv, w->W_xc, S, 2, 0, 0, 4));
  RGP_TRY(pk.add(g->xconv, w->W_xo, S, 3, 0, 0, 4));
  RGP_TRY(pk.add(g->grec, w->W_hi, S, 0, 0, 0, 4));
  RGP_TRY(pk.add(g->grec, w->W_hf, S, 1, 0, 0, 4));
  RGP_TRY(pk.add(g->grec, w->W_ho, S, 3, 0, 0, 4));
  if (g->save) {
    RGP_TRY(g->pb.pack(pk, w->proj_c3d_W));
    RGP_TRY(pk.add(g->b_rec, w->W_hi, S, 0, 0, 1));             // rotated filters on [d(i+g) | df | do]
    RGP_TRY(pk.add(g->b_rec, w->W_hf, S, 0, S, 1));
    RGP_TRY(pk.add(g->b_rec, w->W_ho, S, 0, 2 * S, 1));
    RGP_TRY(pk.add(g->b_x, w->W_xc, P, 0, LSTM_DG * S, 1));     // on [dg | di | (i+g: zero rows) | df | do]
    RGP_TRY(pk.add(g->b_x, w->W_xi, P, 0, LSTM_DI * S, 1));
    RGP_TRY(pk.add(g->b_x, w->W_xf, P, 0, LSTM_DF * S, 1));
    RGP_TRY(pk.add(g->b_x, w->W_xo, P, 0, LSTM_DO * S, 1));
  }
  RGP_TRY(pk.flush());
  // the peephole planes side by side (kernels index one array)
  float* pp = (float*)(ws + g->peep.off);
  const size_t pb = (size_t)49 * S * 4;
  RGP_HIP(hipMemcpyAsync(pp, w->W_ci, pb, hipMemcpyDeviceToDevice, s));
  RGP_HIP(hipMemcpyAsync(pp + 49 * S, w->W_cf, pb, hipMemcpyDeviceToDevice, s));
  RGP_HIP(hipMemcpyAsync(pp + 98 * S, w->W_co, pb, hipMemcpyDeviceToDevice, s));
  // the head as one 19x19 stride-6 transposed convolution on h_t (head_fold.hip.h; no batch-norm in this graph)
  RGP_TRY(g->head.fold(ws, w->up_weight3, w->out_W, w->up_weight2, w->up_weight1, s));
  PackBatch<T> pk2(ws, s);
  RGP_TRY(g->head.pack(pk2));
  if (g->save) RGP_TRY(g->hb.pack(pk2, g->head.k(ws)));
  RGP_TRY(pk2.flush());
  g->proj_b = w->proj_c3d_b;
  g->out_b = w->out_b;
  g->w = *w;
  g->weights_set = true;
  g->fwd_done = g->bwd_done = false;
  return RGP_OK;
}

// All T steps in one persistent launch (convlstm_seq.hip.h)
int seq_persistent(rgp_lstm* g, bool carry, hipStream_t s) {
  char* ws = g->ws;
  RGP_HIP(hipMemsetAsync(ws + g->seq_cnt.off, 0, g->seq_cnt.bytes, s));       // phase counters: zeroed EVERY call
  LstmSeqParams p;
  p.w_rec = (const bf16_t*)(ws + g->grec.w_off);
  p.xpre = (const float*)(ws + g->xpre.off);
  p.peep = (const float*)(ws + g->peep.off);
  p.hall = (float*)(ws + g->hall.off);
  p.call = (float*)(ws + g->call.off);
  p.gates = g->save ? (float*)(ws + g->gates.off) : nullptr;
  p.hseq = (bf16_t*)(ws + g->hseq.off);
  p.xch = (bf16_t*)(ws + g->xch.off);
  p.g = g->sg.args(g->B, (unsigned*)(ws + g->seq_cnt.off), RGP_FAULT_SEQ_LOST_MEMBER);
  p.T = g->T; p.K = g->grec.K;
  p.carry = carry ? 1 : 0;
  RGP_REQUIRE(g->grec.K == 9 * g->S && g->grec.chunk_major == 0, "convlstm_seq: unexpected filter packing");
  if (carry) return launch_seq_group(g->sg, convlstm_seq_kernel<4, true>, convlstm_seq_kernel<7, true>, p, LSQ_SMEM, s);
  return launch_seq_group(g->sg, convlstm_seq_kernel<4, false>, convlstm_seq_kernel<7, false>, p, LSQ_SMEM, s);
}

template <typename T>
int seq_impl(rgp_lstm* g, hipStream_t s) {
  char* ws = g->ws;
  const int B = g->B, T_ = g->T, S = g->S;
  const bool persistent = sizeof(T) == 2 && g->fwd_persistent && g->sg.resident();
  const bool carry = g->stream.carry();
  // A streaming call seeds slot 0 with its state (both paths: [h | c] -> hall, call, the padded h image; the persistent
  // kernel's exchange image of parity 1), by StreamCall's rule
  if (g->stream.needs_seed()) {
    const float* si = g->stream.seed_src();
    SeqSeedArgs a{si, si ? si + (size_t)B * 49 * S : nullptr, (float*)(ws + g->hall.off), (float*)(ws + g->call.off), ws + g->hseq.off,
                  (long long)(T_ + 1) * 81 * S, persistent ? (bf16_t*)(ws + g->xch.off) : nullptr, g->sg.groups, std::max(g->sg.nc, 1), B, S};
    RGP_TRY(launch_seq_seed<T>(a, s));
    g->stream.seed_done();
  }
  if constexpr (sizeof(T) == 2) {
    if (persistent) return seq_persistent(g, carry, s);
  }
  const size_t st = (size_t)B * 49 * S;
  float* hall = (float*)(ws + g->hall.off);
  float* call = (float*)(ws + g->call.off);
  for (int t = 0; t < T_; ++t) {
    IgemmParams p = make_params(g->grec, (const T*)(ws + g->hseq.off) + (size_t)t * 81 * S, ws, B);
    EpiParams e = make_epi(g->grec, ws + g->hseq.off, ws);
    e.out_extra = (long long)(t + 1) * 81 * S;
    e.xpre = (const float*)(ws + g->xpre.off) + (size_t)t * 49 * 4 * S;
    e.xpre_img_stride = (long long)T_ * 49 * 4 * S;
    e.xpre_ld = 4 * S;
    e.S = S;
    e.state_rows = 49;
    e.h_prev = call + (size_t)t * st;
    e.h_next = call + (size_t)(t + 1) * st;
    e.u_gate = hall + (size_t)(t + 1) * st;
    e.r_save = g->save ? (float*)(ws + g->gates.off) + (size_t)t * st : nullptr;
    e.out2_img_mul = (long long)T_ * st;
    e.bn_gamma = (const float*)(ws + g->peep.off);
    RGP_TRY((launch_igemm<T, 1, 1, EpiLstm<T>>(p, e, s)));
  }
  return RGP_OK;
}

// All T backward steps in one persistent launch (convlstm_bptt.hip.h)
int bptt_persistent(rgp_lstm* g, hipStream_t s) {
  char* ws = g->ws;
  RGP_HIP(hipMemsetAsync(ws + g->bptt_cnt.off, 0, g->bptt_cnt.bytes, s));     // phase counters: zeroed EVERY call
  LstmBpttParams p;
  p.w_rec = (const bf16_t*)(ws + g->b_rec.w_off);
  p.dh_head = (const float*)(ws + g->dy.off);
  p.gates = (const float*)(ws + g->gates.off);
  p.call = (const float*)(ws + g->call.off);
  p.peep = (const float*)(ws + g->peep.off);
  p.dpre = (bf16_t*)(ws + g->dpre.off);
  p.xch = (bf16_t*)(ws + g->bptt_xch.off);
  p.g = g->sg.args(g->B, (unsigned*)(ws + g->bptt_cnt.off), RGP_FAULT_BPTT_LOST_MEMBER);
  p.T = g->T; p.K = g->b_rec.K;
  RGP_REQUIRE(g->b_rec.K == 27 * g->S && g->b_rec.chunk_major == 0, "convlstm_bptt: unexpected filter packing");
  return launch_seq_group(g->sg, convlstm_bptt_kernel<4>, convlstm_bptt_kernel<7>, p, LBP_SMEM, s);
}

template <typename T>
int forward_impl(rgp_lstm* g, const float* c3d_input, const void* rows, float* logits, float* probs, hipStream_t s) {
  char* ws = g->ws;
  RGP_TRY(g->pj.forward<T>(ws, c3d_input, rows, g->save, g->F, ws + g->E.off, g->proj_b, s));
  {
    IgemmParams p = make_params(g->xconv, ws + g->E.off, ws, g->F);
    EpiParams e = make_epi(g->xconv, ws + g->xpre.off, ws);
    RGP_TRY((launch_igemm<T, 1, 1, EpiStore<float, false, false>>(p, e, s)));
  }
  RGP_TRY(seq_impl<T>(g, s));
  RGP_TRY(g->head.forward<T>(ws, ws + g->hseq.off, g->B, g->out_b, logits, g->F, s));
  if (probs) RGP_TRY(rgp_softmax_xent_fwd(logits, nullptr, probs, nullptr, nullptr, g->F, 2401, (rgp_stream_t)s));
  g->fwd_done = !g->stream.on;                                // no backward behind a streaming call (no truncated BPTT)
  g->bwd_done = false;
  return RGP_OK;
}

template <typename T>
int backward_impl(rgp_lstm* g, const float* logits, const float* probs, const float* labels, const rgp_lstm_weights* gr,
                  int loss_l2, hipStream_t s) {
  char* ws = g->ws;
  const int B = g->B, T_ = g->T, S = g->S, P = g->P, F = g->F;
  const long long M = g->pb.M;
  const size_t st = (size_t)B * 49 * S;
  auto Fp = [&](const Buf& x) { return (float*)(ws + x.off); };
  auto Tp = [&](const Buf& x) { return (T*)(ws + x.off); };
  auto I = [&](size_t off) { return (const int*)(ws + off); };
  auto wg_params = []() { WgradParams p; memset(&p, 0, sizeof(p)); p.nz = 1; return p; };
  {
    // the wgrad kernel accumulates: clear its outputs (one launch); W_hc has no path to the loss (gaze_lstm.py:80): zeros
    ZeroBatch zb(s);
    for (const float* q : {gr->W_xi, gr->W_xf, gr->W_xc, gr->W_xo}) RGP_TRY(zb.add((void*)q, (size_t)9 * P * S * 4));
    for (const float* q : {gr->W_hi, gr->W_hf, gr->W_ho, gr->W_hc}) RGP_TRY(zb.add((void*)q, (size_t)9 * S * S * 4));
    RGP_TRY(zb.add(ws + g->hb.dkf.off, g->hb.dkf.bytes));
    RGP_TRY(zb.flush());
  }
  // 1. d loss / d logits, d out_b
  RGP_TRY(g->hb.loss_grad(ws, logits, probs, labels, loss_l2, F, (float*)gr->out_b, s));
  // 2. the folded head with y := h (head_fold.hip.h): patches of dz -> dK -> chain rule; dh_head = Pm x K
  RGP_TRY(g->hb.patches<T>(ws, F, s));
  {
    WgradParams p = wg_params();
    p.X = Tp(g->hb.pm); p.dY = Tp(g->hseq); p.dW = Fp(g->hb.dkf);
    wgrad_grid(p, T_, 7, 7);                                    // image = clip, z = step: h_t is slot t+1 of the clip's images
    p.x_sx = HF_PK; p.x_sy = 7 * HF_PK; p.x_sz = 49 * HF_PK; p.x_img_stride = (long long)T_ * 49 * HF_PK;
    p.y_sx = S; p.y_sy = 9 * S; p.y_sz = 81 * S; p.y_org = (81 + 10) * S; p.y_img_stride = (long long)(T_ + 1) * 81 * S;
    p.koff = I(g->o_koff_c); p.M = M; p.N = S; p.nk = HF_PK / Elem<T>::BKE; p.ldw = S; p.k_valid = HF_PK;
    RGP_TRY((launch_wgrad<T, 1>(p, s)));
  }
  RGP_TRY(g->hb.unfold_chain(ws, g->head, g->w.up_weight1, g->w.up_weight2, g->w.up_weight3, g->w.out_W, (float*)gr->up_weight1,
                             (float*)gr->up_weight2, (float*)gr->up_weight3, (float*)gr->out_W, s));
  RGP_TRY((g->hb.dgrad<T, float>(ws, F, Fp(g->dy), s)));
  // 3. BPTT, t = T-1 .. 0: element-wise step, then dh_{t-1} = rotated [W_hi | W_hf | W_ho] on [d(i+g) | df | do]
  bool bptt_one_launch = false;
  if constexpr (sizeof(T) == 2) {
    if (g->bptt_persistent && g->sg.resident()) {
      RGP_TRY(bptt_persistent(g, s));
      bptt_one_launch = true;
    }
  }
  const int ew_blocks = (int)std::min<size_t>((st + 255) / 256, 4096);
  for (int t = T_ - 1; t >= 0 && !bptt_one_launch; --t) {
    lstm_bwd_step_kernel<T><<<ew_blocks, 256, 0, s>>>(Fp(g->dy), Fp(g->dh_carry), Fp(g->dc_carry), Fp(g->gates), Fp(g->call),
                                                      Fp(g->peep), Tp(g->dpre), B, T_, t, S, t == T_ - 1);
    RGP_HIP(hipGetLastError());
    if (t == 0) break;                                         // (nothing reads d h_0: the zero state)
    IgemmParams p = make_params(g->b_rec, Tp(g->dpre) + ((size_t)t * 81 * 5 + LSTM_DIG) * S, ws, B);
    EpiParams e = make_epi(g->b_rec, Fp(g->dh_carry), ws);
    RGP_TRY((launch_igemm<T, 1, 1, EpiStore<float, false, false>>(p, e, s)));
  }
  // 4. peephole gradients (fixed-order sums over the frames)
  lstm_peephole_grad_kernel<T><<<(3 * 49 * S + 255) / 256, 256, 0, s>>>(Tp(g->dpre), Fp(g->call), (float*)gr->W_ci, (float*)gr->W_cf,
                                                                         (float*)gr->W_co, B, T_, S);
  RGP_HIP(hipGetLastError());
  // 5. filter gradients of the cell, hoisted over all steps (wgrad_kernel on the padded operand images)
  {
    WgradParams p = wg_params();
    p.N = S; p.ldw = S; p.M = M;
    p.y_sx = 5 * S; p.y_sy = 45 * S; p.y_org = 50 * S;
    // input filters: rows = frames x 7x7, X = the padded projected features E
    wgrad_grid(p, 1, 7, 7);
    p.X = Tp(g->E); p.x_sx = P; p.x_sy = 9 * P; p.x_img_stride = 81LL * P; p.y_img_stride = 81LL * 5 * S;
    p.koff = I(g->xconv.koff_off); p.nk = g->xconv.nk; p.k_valid = 9 * P;
    float* dWx[4] = {(float*)gr->W_xi, (float*)gr->W_xf, (float*)gr->W_xc, (float*)gr->W_xo};
    const int bx[4] = {LSTM_DI, LSTM_DF, LSTM_DG, LSTM_DO};
    p.dY = Tp(g->dpre); p.dW = dWx[0]; p.nz = 4;
    for (int q = 0; q < 4; ++q) { p.zy[q] = (long long)bx[q] * S * sizeof(T); p.zw[q] = dWx[q] - dWx[0]; }
    RGP_TRY((launch_wgrad<T, 1>(p, s)));
  }
  {
    // recurrent filters: image = clip, z = step; X = h_{t-1} = slot t of the clip's images; d W_hi from d i_pre + d g_pre
    WgradParams p = wg_params();
    p.N = S; p.ldw = S; p.M = M; p.dY = Tp(g->dpre);
    p.y_sx = 5 * S; p.y_sy = 45 * S; p.y_org = 50 * S;
    wgrad_grid(p, T_, 7, 7);
    p.X = Tp(g->hseq); p.x_sx = S; p.x_sy = 9 * S; p.x_sz = 81 * S; p.x_img_stride = (long long)(T_ + 1) * 81 * S;
    p.y_sz = 81 * 5 * S; p.y_img_stride = (long long)T_ * 81 * 5 * S;
    p.koff = I(g->grec.koff_off); p.nk = g->grec.nk; p.k_valid = 9 * S;
    float* dWh[3] = {(float*)gr->W_hi, (float*)gr->W_hf, (float*)gr->W_ho};
    const int bh[3] = {LSTM_DIG, LSTM_DF, LSTM_DO};
    p.dW = dWh[0]; p.nz = 3;
    for (int q = 0; q < 3; ++q) { p.zx[q] = 0; p.zy[q] = (long long)bh[q] * S * sizeof(T); p.zw[q] = dWh[q] - dWh[0]; }
    RGP_TRY((launch_wgrad<T, 1>(p, s)));
  }
  // 6. dE through the four input filters, then the projection's gradients as gaze_c3d_conv's (no atomics)
  {
    IgemmParams p = make_params(g->b_x, Tp(g->dpre), ws, F);
    EpiParams e = make_epi(g->b_x, Tp(g->dE), ws);
    RGP_TRY((launch_igemm<T, 1, 1, EpiStore<T, false, false>>(p, e, s)));
  }
  RGP_TRY(g->pb.weight_grads<T>(ws, Tp(g->pj.xt), Tp(g->dE), (float*)gr->proj_c3d_W, (float*)gr->proj_c3d_b, s));
  g->bwd_done = true;
  return RGP_OK;
}

// kind 0: [T][B] fp32 states -> [B][T]; 1: E (padded, operand dtype); 2: column block `off` of dpre (padded, operand dtype)
struct View { size_t off; int kind; size_t elems; };

bool find_view(const rgp_lstm* g, const char* name, View& v) {
  const std::string n(name ? name : "");
  const size_t st = (size_t)g->B * 49 * g->S, all = st * g->T;
  if (n == "h") v = {g->hall.off + st * 4, 0, all};
  else if (n == "c") v = {g->call.off + st * 4, 0, all};
  else if (n == "emb") v = {g->E.off, 1, (size_t)g->F * 49 * g->P};
  else if (g->save && (n == "i" || n == "f" || n == "g" || n == "o"))
    v = {g->gates.off + (n == "i" ? 0 : n == "f" ? 1 : n == "g" ? 2 : 3) * all * 4, 0, all};
  else if (g->save && (n == "d_i" || n == "d_f" || n == "d_g" || n == "d_o"))
    v = {(size_t)(n == "d_i" ? LSTM_DI : n == "d_f" ? LSTM_DF : n == "d_g" ? LSTM_DG : LSTM_DO), 2, all};
  else return false;
  return true;
}

}  // namespace

extern "C" {

int rgp_lstm_create(rgp_lstm_t** plan, int batch, int n_steps, int dtype, int flags) {
  RGP_REQUIRE(plan, "rgp_lstm_create: null out pointer");
  RGP_REQUIRE((flags & ~(RGP_LSTM_SAVE_FOR_BACKWARD | RGP_LSTM_PER_STEP | RGP_LSTM_PERSISTENT | RGP_LSTM_BPTT_PERSISTENT)) == 0,
              "rgp_lstm_create: unknown flags 0x%x", flags);
  RGP_REQUIRE((flags & (RGP_LSTM_PER_STEP | RGP_LSTM_PERSISTENT)) != (RGP_LSTM_PER_STEP | RGP_LSTM_PERSISTENT),
              "rgp_lstm_create: flags name both recurrence paths");
  RGP_REQUIRE(batch > 0 && n_steps > 0, "rgp_lstm_create: batch=%d n_steps=%d", batch, n_steps);
  RGP_REQUIRE(dtype == RGP_F32 || dtype == RGP_BF16, "rgp_lstm_create: dtype %d", dtype);
  RGP_REQUIRE((long long)batch * n_steps * 2401 < (1LL << 31) && (long long)batch * (n_steps + 1) * 81 * 5 * 128 < (1LL << 31),
              "rgp_lstm_create: B*T too large");
  RGP_REQUIRE(!(flags & RGP_LSTM_PERSISTENT) || (dtype == RGP_BF16 && batch <= 64),
              "rgp_lstm_create: the persistent kernel (flags) takes bf16 plans of at most 64 clips");
  RGP_REQUIRE(!(flags & RGP_LSTM_BPTT_PERSISTENT) || (flags & RGP_LSTM_SAVE_FOR_BACKWARD),
              "rgp_lstm_create: flags name RGP_LSTM_BPTT_PERSISTENT without RGP_LSTM_SAVE_FOR_BACKWARD (the persistent BPTT needs a training plan)");
  RGP_REQUIRE(!(flags & RGP_LSTM_BPTT_PERSISTENT) || (dtype == RGP_BF16 && batch <= 64),
              "rgp_lstm_create: the persistent BPTT kernel (flags) takes bf16 plans of at most 64 clips");
  rgp_lstm* g = new rgp_lstm();
  g->B = batch; g->T = n_steps; g->dtype = dtype; g->F = batch * n_steps;
  g->save = (flags & RGP_LSTM_SAVE_FOR_BACKWARD) != 0;
  const int P = g->P, S = g->S, F = g->F, T_ = n_steps, es = esize(dtype);
  bool ok = true;
  ok &= g->pj.plan(P, dtype, pad_tab9(P), 81LL * P);           // E = X W + b (gaze_lstm.py:238-244), halo-padded 9x9xP
  auto conv3x3 = [&](ConvDesc& d, int Cin) {                   // 3x3 SAME on a padded 9x9 image, N = 4 S interleaved columns
    d.Mw = 49; d.N = 4 * S;
    for (int y = 0; y < 7; ++y) for (int x = 0; x < 7; ++x) d.in_tab.push_back((y * 9 + x) * Cin);
    std::vector<int> tapoff, fidx;
    for (int ky = 0; ky < 3; ++ky) for (int kx = 0; kx < 3; ++kx) { tapoff.push_back((ky * 9 + kx) * Cin); fidx.push_back(ky * 3 + kx); }
    const bool r = build_k_schedule(d, tapoff, fidx, Cin, dtype);
    d.s_tap = (long long)Cin * S; d.s_n = 1; d.s_c = S;        // HWIO [3,3,Cin,S]
    return r;
  };
  ok &= conv3x3(g->xconv, P);
  g->xconv.in_img_stride = 81LL * P; g->xconv.out_img_stride = 49LL * 4 * S;
  for (int p = 0; p < 49; ++p) g->xconv.out_tab.push_back(p * 4 * S);
  ok &= conv3x3(g->grec, S);
  g->grec.in_img_stride = (long long)(T_ + 1) * 81 * S; g->grec.out_img_stride = g->grec.in_img_stride;
  g->grec.out_tab = pad_tab9(S);
  {
    ConvDesc& d = g->head.hfold;                               // folded head: a GEMM "image" is a clip, rows = (step, 7x7 position)
    d.Mw = T_ * 49; d.in_img_stride = (long long)(T_ + 1) * 81 * S; d.out_img_stride = (long long)T_ * 49 * HF_PK;
    for (int t = 0; t < T_; ++t)
      for (int m = 0; m < 7; ++m) for (int n = 0; n < 7; ++n) {
        d.in_tab.push_back(((t + 1) * 81 + (m + 1) * 9 + n + 1) * S);
        d.out_tab.push_back((t * 49 + m * 7 + n) * HF_PK);
      }
    ok &= g->head.plan(S, dtype);
  }
  if (!ok) { delete g; return set_err(RGP_EINVAL, "rgp_lstm_create: K schedule failed"); }
  Arena a;
  for (ConvDesc* d : {&g->pj.proj, &g->pj.proj_rows, &g->xconv, &g->grec, &g->head.hfold}) d->reserve(a, dtype);
  const size_t st = (size_t)batch * 49 * S * 4;
  g->pj.xt = take(a, (size_t)F * 49 * 1024 * es);
  g->E = take(a, (size_t)F * 81 * P * es);
  g->xpre = take(a, (size_t)F * 49 * 4 * S * 4);
  g->hall = take(a, st * (T_ + 1));
  g->call = take(a, st * (T_ + 1));
  if (g->save) g->gates = take(a, st * T_ * 4);
  g->hseq = take(a, (size_t)batch * (T_ + 1) * 81 * S * es);
  g->peep = take(a, (size_t)3 * 49 * S * 4);
  g->head.gfold = take(a, FoldedHead::G_BYTES);
  g->head.hf_h = take(a, FoldedHead::H_BYTES);
  g->head.hf_k = take(a, g->head.k_bytes(HF_PK));
  g->head.hf_z = take(a, FoldedHead::z_bytes(F));
  g->head.hf_part = take(a, g->head.part_bytes());
  // persistent kernels: bf16 operands, up to 2 clips per group of 8 workgroups, at most 32 groups.  The forward's flags and
  // the BPTT's are independent of each other; the groups are sized if either kernel is selected.
  const bool eligible = dtype == RGP_BF16 && batch <= 64;
  g->fwd_persistent = eligible && ((flags & RGP_LSTM_PERSISTENT) || (LSTM_DEFAULT_PERSISTENT && !(flags & RGP_LSTM_PER_STEP)));
  g->bptt_persistent = eligible && g->save && ((flags & RGP_LSTM_BPTT_PERSISTENT) || LSTM_DEFAULT_BPTT_PERSISTENT);
  if (g->fwd_persistent || g->bptt_persistent) g->sg.size(batch);
  if (g->fwd_persistent) {
    g->xch = take(a, (size_t)2 * g->sg.groups * 98 * 128 * 2);
    g->seq_cnt = take(a, (size_t)g->sg.groups * T_ * 4);
  }
  if (g->bptt_persistent) {
    g->bptt_xch = take(a, (size_t)2 * 3 * g->sg.groups * 98 * 128 * 2);
    g->bptt_cnt = take(a, (size_t)g->sg.groups * T_ * 4);
  }
  if (g->save) {
    bool okb = true;
    // 3x3 SAME input gradients: correlation of the padded gradient image (pixel stride 5 S) with the rotated, in/out-swapped filters
    auto dgrad3x3 = [&](ConvDesc& d, int Cgrad, int Nout, int filt_cin, long long in_stride) {
      d.Mw = 49; d.N = Nout; d.in_img_stride = in_stride; d.out_img_stride = 49LL * Nout;
      std::vector<int> tapoff, fidx;
      for (int y = 0; y < 7; ++y) for (int x = 0; x < 7; ++x) { d.in_tab.push_back((y * 9 + x) * 5 * S); d.out_tab.push_back((y * 7 + x) * Nout); }
      for (int t = 0; t < 9; ++t) { tapoff.push_back(((t / 3) * 9 + (t % 3)) * 5 * S); fidx.push_back(8 - t); }
      const bool r = build_k_schedule(d, tapoff, fidx, Cgrad, dtype);
      d.cin_src = S;
      d.s_tap = (long long)filt_cin * S; d.s_n = S; d.s_c = 1;
      return r;
    };
    okb &= dgrad3x3(g->b_rec, 3 * S, S, S, (long long)T_ * 81 * 5 * S);
    okb &= dgrad3x3(g->b_x, 5 * S, P, P, 81LL * 5 * S);
    okb &= g->pb.plan(P, dtype);
    okb &= g->hb.plan(S, dtype);                               // dh[(f,m,n), s] = sum_k Pm[(f,m,n), k] K[k, s]
    okb = okb && g->pb.plan_wgrad(F, dtype);                   // d proj_c3d_W [1024][P] = XT [1024][Mp] x dET [P][Mp]^T
    if (!okb) { delete g; return set_err(RGP_EINVAL, "rgp_lstm_create: B*T too large for the backward plan"); }
    for (ConvDesc* d : {&g->b_rec, &g->b_x, &g->pb.b_px, &g->hb.b_hf, &g->pb.wg_w}) d->reserve(a, dtype);
    for (int k = 0; k < HF_PK / bke(dtype); ++k) g->koff_c.push_back(k * bke(dtype));
    g->o_koff_c = a.take(g->koff_c.size() * 4);
    g->hb.dz = take(a, FoldedHeadBwd::dz_bytes(F));
    g->hb.frame_sum = take(a, (size_t)F * 4);
    g->hb.pm = take(a, FoldedHeadBwd::pm_bytes(F, dtype));
    g->hb.dkf = take(a, FoldedHeadBwd::dk_bytes(S));
    g->hb.dhf = take(a, FoldedHeadBwd::DH_BYTES);
    g->hb.dhp = take(a, FoldedHeadBwd::DHP_BYTES);
    g->hb.dgp = take(a, FoldedHeadBwd::DG_BYTES);
    g->dy = take(a, (size_t)g->pb.M * S * 4);
    g->dh_carry = take(a, st);
    g->dc_carry = take(a, st);
    g->dpre = take(a, (size_t)F * 81 * 5 * S * es);
    g->dE = take(a, (size_t)g->pb.M * P * es);
    g->pb.xT = take(a, g->pb.xT_bytes(dtype));
    g->pb.part = take(a, g->pb.part_bytes());
  }
  g->ws_bytes = a.off;
  *plan = g;
  return RGP_OK;
}

int rgp_lstm_destroy(rgp_lstm_t* plan) {
  if (plan) plan->sg.free_err();
  delete plan;
  return RGP_OK;
}

size_t rgp_lstm_workspace_bytes(const rgp_lstm_t* plan) { return plan ? plan->ws_bytes : 0; }

int rgp_lstm_bind_workspace(rgp_lstm_t* g, void* workspace, size_t bytes, rgp_stream_t stream) {
  RGP_TRY(check_bind("rgp_lstm_bind_workspace", g, workspace, bytes));
  hipStream_t s = (hipStream_t)stream;
  RGP_TRY(g->sg.alloc_err());
  g->ws = (char*)workspace;
  g->weights_set = false;
  g->stream = StreamCall();
  // zero everything once: the halos of E / h images / dpre, slot 0 of the states and the unused filter rows stay zero,
  // because kernels only ever write interiors and a pack writes the same positions every time
  RGP_HIP(hipMemsetAsync(g->ws, 0, g->ws_bytes, s));
  for (ConvDesc* d : {&g->pj.proj, &g->pj.proj_rows, &g->xconv, &g->grec, &g->head.hfold}) RGP_TRY(upload_desc(*d, g->ws, s));
  if (g->save) {
    for (ConvDesc* d : {&g->b_rec, &g->b_x, &g->pb.b_px, &g->hb.b_hf, &g->pb.wg_w}) RGP_TRY(upload_desc(*d, g->ws, s));
    RGP_HIP(hipMemcpyAsync(g->ws + g->o_koff_c, g->koff_c.data(), g->koff_c.size() * 4, hipMemcpyHostToDevice, s));
  }
  return RGP_OK;
}

int rgp_lstm_set_weights(rgp_lstm_t* g, const rgp_lstm_weights* w, rgp_stream_t stream) {
  RGP_REQUIRE(g && w, "rgp_lstm_set_weights: null argument");
  if (!g->ws) return set_err(RGP_EWORKSPACE, "rgp_lstm: workspace not bound");
  RGP_TRY(require_pointers(w, "rgp_lstm_set_weights", "weight"));
  return RGP_BY_DTYPE(g->dtype, set_weights_impl, g, w, (hipStream_t)stream);
}

int rgp_lstm_forward(rgp_lstm_t* g, const float* c3d_input, float* logits, float* probs, rgp_stream_t stream) {
  RGP_TRY(check_ready(g));
  RGP_REQUIRE(c3d_input && logits, "rgp_lstm_forward: null argument");
  return RGP_BY_DTYPE(g->dtype, forward_impl, g, c3d_input, nullptr, logits, probs, (hipStream_t)stream);
}

int rgp_lstm_forward_rows(rgp_lstm_t* g, const void* c3d_rows, float* logits, float* probs, rgp_stream_t stream) {
  RGP_TRY(check_ready(g));
  RGP_REQUIRE(c3d_rows && logits, "rgp_lstm_forward_rows: null argument");
  RGP_REQUIRE(((size_t)c3d_rows & 15) == 0, "rgp_lstm_forward_rows: rows must be 16-byte aligned");
  return RGP_BY_DTYPE(g->dtype, forward_impl, g, nullptr, c3d_rows, logits, probs, (hipStream_t)stream);
}

size_t rgp_lstm_state_elems(const rgp_lstm_t* g) { return g ? (size_t)2 * g->B * 49 * g->S : 0; }

int rgp_lstm_forward_stream(rgp_lstm_t* g, const float* c3d_input, const void* c3d_rows, const float* state_in, float* state_out,
                            int n_valid, float* logits, float* probs, rgp_stream_t stream) {
  RGP_REQUIRE(g, "rgp_lstm_forward_stream: null plan");
  RGP_TRY(check_stream_args("rgp_lstm_forward_stream", g->T, c3d_input, c3d_rows, state_in, state_out, n_valid, 0, logits));
  RGP_TRY(check_ready(g));
  hipStream_t s = (hipStream_t)stream;
  StreamScope call(g->stream, state_in, state_out, n_valid);
  g->fwd_done = false;                                       // ... nor behind one that fails half-way
  RGP_TRY(RGP_BY_DTYPE(g->dtype, forward_impl, g, c3d_input, c3d_rows, logits, probs, s));
  return stream_state_out(g->stream, {g->ws + g->hall.off, g->ws + g->call.off}, (size_t)g->B * 49 * g->S * 4, s);   // [h | c]
}

int rgp_lstm_backward(rgp_lstm_t* g, const float* logits, const float* probs, const float* labels, const rgp_lstm_weights* grads,
                      int loss_type, rgp_stream_t stream) {
  RGP_TRY(check_ready(g));
  RGP_REQUIRE(labels && grads && (loss_type == 0 || loss_type == 1), "rgp_lstm_backward: bad arguments");
  RGP_REQUIRE(loss_type == 1 ? logits != nullptr : probs != nullptr, "rgp_lstm_backward: the loss needs %s", loss_type == 1 ? "logits" : "probs");
  if (!g->save) return set_err(RGP_ESTATE, "rgp_lstm_backward: the plan was not created with RGP_LSTM_SAVE_FOR_BACKWARD");
  if (!g->fwd_done) return set_err(RGP_ESTATE, "rgp_lstm_backward: no forward since the weights were set (a streaming call is none: no truncated BPTT)");
  RGP_TRY(require_pointers(grads, "rgp_lstm_backward", "gradient"));
  return RGP_BY_DTYPE(g->dtype, backward_impl, g, logits, probs, labels, grads, loss_type, (hipStream_t)stream);
}

int rgp_lstm_backward_input(rgp_lstm_t* g, float* d_rows, rgp_stream_t stream) {
  RGP_REQUIRE(g && d_rows, "rgp_lstm_backward_input: null argument");
  if (!g->ws || !g->save || !g->weights_set || !g->bwd_done) return set_err(RGP_ESTATE, "rgp_lstm_backward_input: call after rgp_lstm_backward");
  return g->pb.backward_input(g->ws, g->dtype, g->ws + g->dE.off, g->pb.M, d_rows, (hipStream_t)stream);
}

int rgp_lstm_status(rgp_lstm_t* g, rgp_stream_t stream) {
  RGP_REQUIRE(g, "rgp_lstm_status: null plan");
  RGP_HIP(hipStreamSynchronize((hipStream_t)stream));
  return lstm_check_error(g);
}

int rgp_lstm_inject_fault(rgp_lstm_t* g, int kind) {
  RGP_REQUIRE(g && (kind == RGP_FAULT_SEQ_LOST_MEMBER || kind == RGP_FAULT_BPTT_LOST_MEMBER), "rgp_lstm_inject_fault: bad arguments");
  const bool selected = kind == RGP_FAULT_SEQ_LOST_MEMBER ? g->fwd_persistent : g->bptt_persistent;
  if (g->dtype != RGP_BF16 || !selected || !g->sg.resident())
    return set_err(RGP_ESTATE, "rgp_lstm_inject_fault: the plan does not use the persistent ConvLSTM %s kernel",
                   kind == RGP_FAULT_SEQ_LOST_MEMBER ? "sequence" : "BPTT");
  g->sg.fault |= kind;
  return RGP_OK;
}

int rgp_lstm_persistent_workgroups(const rgp_lstm_t* g) {
  return (g && g->dtype == RGP_BF16 && g->fwd_persistent && g->sg.resident()) ? g->sg.groups * 8 : 0;
}

int rgp_lstm_bptt_persistent_workgroups(const rgp_lstm_t* g) {
  return (g && g->dtype == RGP_BF16 && g->bptt_persistent && g->sg.resident()) ? g->sg.groups * 8 : 0;
}

size_t rgp_lstm_buffer_elems(const rgp_lstm_t* g, const char* name) {
  View v;
  return (g && find_view(g, name, v)) ? v.elems : 0;
}

int rgp_lstm_read_buffer(rgp_lstm_t* g, const char* name, float* dst, rgp_stream_t stream) {
  RGP_REQUIRE(g && g->ws && name && dst, "rgp_lstm_read_buffer: null argument");
  View v;
  if (!find_view(g, name, v)) return set_err(RGP_EINVAL, "rgp_lstm_read_buffer: unknown buffer '%s'", name);
  hipStream_t s = (hipStream_t)stream;
  if (v.kind == 0) {
    lstm_tb_to_bt_kernel<<<1024, 256, 0, s>>>((const float*)(g->ws + v.off), dst, g->T, g->B, 49LL * g->S);
  } else if (v.kind == 2) {
    const long long total = (long long)v.elems;
    const int blocks = (int)std::min<long long>((total + 255) / 256, 8192);
    if (g->dtype == RGP_BF16) lstm_dpre_block_kernel<bf16_t><<<blocks, 256, 0, s>>>((const bf16_t*)(g->ws + g->dpre.off), dst, (int)v.off, g->S, total);
    else lstm_dpre_block_kernel<float><<<blocks, 256, 0, s>>>((const float*)(g->ws + g->dpre.off), dst, (int)v.off, g->S, total);
  } else {
    const long long total = (long long)v.elems;
    const int blocks = (int)std::min<long long>((total + 255) / 256, 8192);
    const int* tab = (const int*)(g->ws + g->pj.proj.out_tab_off);
    if (g->dtype == RGP_BF16) unpad_kernel<bf16_t><<<blocks, 256, 0, s>>>((const bf16_t*)(g->ws + v.off), dst, tab, 49, g->P, 81LL * g->P, total);
    else unpad_kernel<float><<<blocks, 256, 0, s>>>((const float*)(g->ws + v.off), dst, tab, 49, g->P, 81LL * g->P, total);
  }
  RGP_HIP(hipGetLastError());
  return RGP_OK;
}

}  // extern "C"
