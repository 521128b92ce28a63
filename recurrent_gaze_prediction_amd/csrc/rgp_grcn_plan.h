// Plan object of the gaze_grcn path, shared by the forward (rgp_grcn.hip) and backward
// (rgp_grcn_bwd.hip) translation units.
#pragma once
#include "gaze_stages.h"

struct rgp_grcn {
  // (owner: a cascade plan) step_ev[t] is recorded on the launch stream behind step t of the per-timestep recurrence: lets
  // another stream consume state t while the later steps run (rgp_cascade.hip).  Null = nothing recorded
  hipEvent_t* step_ev = nullptr;
  // (same owner) backward from external state gradients with per-timestep BPTT: the launch stream waits for bwd_step_ev[t]
  // before step t reads frame (b, t) of the gradient -- its producer runs one step ahead on another stream.  Null = the whole
  // gradient is complete when the call is made
  hipEvent_t* bwd_step_ev = nullptr;
  int B = 0, T = 0, P = 0, S = 0, dtype = RGP_BF16, save = 0, F = 0;
  rgp::Projection pj;                // gaze_stages.h: E halo-padded 9x9xP
  rgp::ConvDesc xconv, gzr, gc, d3;
  rgp::ConvDesc d3t;   // the folded 7x7 conv as a row-Toeplitz GEMM: 16 output pixels of a row per GEMM row (d3: x = 48 only)
  std::vector<rgp::ConvDesc> d1, d2;            // transposed convolutions: one problem per row phase py, N = (px, channel)
  std::vector<rgp::ConvDesc> d1_pack, d2_pack;  // their filter-packing aliases (one per (py, px): a tap table of its own)
  // read_buffer tables (host copies + offsets)
  std::vector<int> tab_pad9_P, tab_pad9_S, tab_pad27, tab_pad55, tab_lin49_3S, tab_lin49_S;
  size_t o_pad9_P = 0, o_pad9_S = 0, o_pad27 = 0, o_pad55 = 0, o_lin49_3S = 0, o_lin49_S = 0;
  Buf E, xpre, hall, uall, rall, call, hp, rhp, hbn, D1, D2, frame_loss, gtoep, bias16;
  // unless RGP_GRCN_UNFOLDED_HEAD: the three transposed convolutions + out_W folded into ONE 19x19 stride-6 transposed
  // convolution on BN(h), run as GEMM + col2im (head_fold.hip.h), forward and backward
  bool fold_head = false;
  rgp::FoldedHead head;            // (unfolded plans use its gfold only: G = weight3 o out_W)
  Buf xch_h, xch_rh, seq_cnt;   // persistent ConvGRU sequence kernel: exchange images [groups][98][128] + phase counters
  rgp::SeqGroupPlan sg;             // ... its groups, error word and fault bits (rgp_grcn_inject_fault: bit 0 the next sequence launch, bit 1 the next BPTT launch)
  size_t ws_bytes = 0;
  char* ws = nullptr;
  bool weights_set = false;
  bool fwd_done = false;           // the last public forward of either kind enqueued all its stages (rgp_grcn_backward_stream)
  const float *bn_gamma = nullptr, *bn_beta = nullptr, *proj_b = nullptr, *out_b = nullptr;
  rgp::StageProfiler prof;
  rgp::StreamCall stream;   // rgp_grcn_forward_stream, or the call of the plan that owns this one (rgp_grcn77, rgp_cascade)
  struct GrcnBwd* bwd = nullptr;   // backward plan (save_for_backward only), rgp_grcn_bwd.hip
};

// rgp_grcn.hip: the plan's persistent BPTT launch leaves RGP_RCCL_CU_RESERVE CUs free (the TOP gradient group may leave before it)
bool grads_top_early(const rgp_grcn* g);
// rgp_grcn.hip: the projection from conv5b rows as a stage of its own (what rgp_grcn_forward_rows runs first)
int grcn_proj_rows_fwd(rgp_grcn* g, const void* c3d_rows, hipStream_t s);
// the state behind step n_valid of the plan's streaming call = slot n_valid of hall
inline int grcn_state_out(rgp_grcn* g, hipStream_t s) {
  return rgp::stream_state_out(g->stream, {g->ws + g->hall.off}, (size_t)g->B * 49 * g->S * 4, s);
}
// rgp_grcn_bwd.hip
// returns RGP_ETIMEOUT (and clears the word) if a persistent launch of this plan reported a lost group member
int grcn_check_error(rgp_grcn* g);
int grcn_bwd_plan(rgp_grcn* g, rgp::Arena& a);
int grcn_bwd_upload(rgp_grcn* g, hipStream_t s);
int grcn_bwd_pack(rgp_grcn* g, const rgp_grcn_weights* w, hipStream_t s, hipStream_t sc);   // sc: the stream the head's fold ran on
int grcn_bwd_fork_fold(rgp_grcn* g, hipStream_t s, hipStream_t* sc);
int grcn_bwd_join_fold(rgp_grcn* g, hipStream_t s);
void grcn_bwd_destroy(rgp_grcn* g);
// workspace offset of a backward buffer rgp_grcn_read_buffer shows ("dxpre", "dh_head"); false = no such buffer
bool grcn_bwd_view(const rgp_grcn* g, const char* name, size_t* off);
