// The per-step GRU recurrence of gaze_grcn, the fc-GRU and the cascade's top cell: two launches per step (EpiGruZR, EpiGruC) on
// a descriptor of where step t reads and writes, and the seed / hand-out of the two dense-row cells' streaming state.
#pragma once
#include "rgp_host.h"

namespace rgp {

// Where step t works, as strides: 0 = one buffer, rewritten every step.
struct GruSteps {
  const ConvDesc *zr = nullptr, *c = nullptr;   // the gate GEMM on h_{t-1} and the candidate GEMM on r * h_{t-1}
  int B = 0, T = 0, S = 0, rows = 0;            // clips, steps, state channels (padded), state rows per clip
  const float* xpre = nullptr;                  // hoisted x-parts [B][T][rows][3 S]
  float* hall = nullptr;                        // fp32 states: slot t -> slot t + 1, of h_ring slots (0: one per step, T + 1)
  int h_ring = 0;
  float *u = nullptr, *r = nullptr, *cand = nullptr;   // gates kept per step (r, cand: or null), gate_step elements apart
  size_t gate_step = 0;
  char *hp = nullptr, *rh = nullptr;            // operand images of h and r * h: step t at + t * step bytes, clips img elements apart
  size_t hp_step = 0, rh_step = 0;
  long long hp_img = 0, rh_img = 0;
  const int *zr_out_tab = nullptr, *c_out_tab = nullptr;   // rows of rh / of the next h operand, if not zr's / c's own table
  void* out2 = nullptr;                         // BN(h_t) as frame (b, t) of the consumer's images, rows by c's own table
  long long out2_img = 0;
  const float *bn_gamma = nullptr, *bn_beta = nullptr;   // step t reads slot (t + bn_phase) % T, bn_step elements apart
  size_t bn_step = 0;
  int bn_phase = 0;
  float bn_inv_std = 1.0f;
};

// before(t) runs ahead of step t's launches, after(t, h_next) behind them (h_next: the fp32 state the step wrote); both return
// an RGP code.  What is a caller's own goes there: event waits and records, the state hand-out of a streaming call.
template <typename T, int G16, class Before, class After>
int run_gru_steps(const GruSteps& d, char* ws, hipStream_t s, Before before, After after) {
  const size_t st = (size_t)d.B * d.rows * d.S;
  const int* c_tab = (const int*)(ws + d.c->out_tab_off);
  for (int t = 0; t < d.T; ++t) {
    RGP_TRY(before(t));
    char* rh_buf = d.rh + t * d.rh_step;
    EpiParams e = make_epi(*d.zr, rh_buf, ws);
    if (d.zr_out_tab) e.out_tab = d.zr_out_tab;
    e.out_img_stride = d.rh_img;
    e.xpre = d.xpre + (size_t)t * d.rows * 3 * d.S;
    e.xpre_img_stride = (long long)d.T * d.rows * 3 * d.S;
    e.xpre_ld = 3 * d.S;
    e.xpre_col = 0;
    e.S = d.S;
    e.state_rows = d.rows;
    e.h_prev = d.hall + (size_t)(d.h_ring ? t % d.h_ring : t) * st;
    e.h_next = d.hall + (size_t)(d.h_ring ? (t + 1) % d.h_ring : t + 1) * st;
    e.u_gate = d.u + t * d.gate_step;
    e.r_save = d.r ? d.r + t * d.gate_step : nullptr;
    e.c_save = d.cand ? d.cand + t * d.gate_step : nullptr;
    IgemmParams p = make_params(*d.zr, d.hp + t * d.hp_step, ws, d.B);
    p.in_img_stride = d.hp_img;
    RGP_TRY((launch_igemm<T, G16, 1, EpiGruZR<T>>(p, e, s)));
    // candidate conv on r*h, blend, BN -> next operand + frame (b, t) of out2
    e.out = d.hp + (t + 1) * d.hp_step;
    e.out_tab = d.c_out_tab ? d.c_out_tab : c_tab;
    e.out_img_stride = d.hp_img;
    e.xpre_col = 2 * d.S;
    e.out2 = d.out2;
    e.out2_tab = c_tab;
    e.out2_img_stride = d.out2_img;
    e.out2_img_mul = d.T;
    e.out2_img_add = t;
    e.bn_gamma = d.bn_gamma + (size_t)((t + d.bn_phase) % d.T) * d.bn_step;
    e.bn_beta = d.bn_beta + (size_t)((t + d.bn_phase) % d.T) * d.bn_step;
    e.bn_inv_std = d.bn_inv_std;
    IgemmParams pc = make_params(*d.c, rh_buf, ws, d.B);
    pc.in_img_stride = d.rh_img;
    RGP_TRY((launch_igemm<T, G16, 1, EpiGruC<T>>(pc, e, s)));
    RGP_TRY(after(t, e.h_next));
  }
  return RGP_OK;
}

// Streaming, the dense-row cells (fc-GRU: rows = 1; cascade top: the 49x49 interior of a 53x53 image): h_0 from a caller's
// state.  src [B][rows][n] dense fp32, or null = zeros -> h0 [B][rows][S] fp32 (slot 0 of the state snapshots) and the operand
// of step 0, clip b at pad + b * img, row p at tab[p] (null: p * S).  Channels >= n are written as zeros; what the table skips
// (a halo) is not touched.  The conversion is the epilogues' (Elem<T>::to = f2bf, as EpiGruC rounds hp_out and fcs_pack8 the
// exchange rows), so the operand of a cut stream is bit for bit what an uncut recurrence publishes at that step.
template <typename T>
__global__ __launch_bounds__(256) void gru_seed_kernel(const float* __restrict__ src, float* __restrict__ h0, T* __restrict__ pad,
                                                       const int* __restrict__ tab, long long img, int B, int rows, int n, int S) {
  const int total = B * rows * S;                        // (below 2^31 for every plan that fits a device)
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int row = i / S, c = i - row * S;              // row = rows b + p
    const int b = row / rows, p = row - b * rows;
    const float v = (src && c < n) ? src[(long long)row * n + c] : 0.f;
    h0[i] = v;
    pad[b * img + (tab ? tab[p] : p * S) + c] = Elem<T>::to(v);
  }
}

// h_{-1} of a dense-row cell ahead of its steps (both paths of the fc-GRU read it where this puts it): the zeros of two memsets,
// or one seed launch by StreamCall's rule.  save: the operand is slot (b, 0) of T + 1 kept images, which no memset covers.
// src: this cell's part of c.in.
template <typename T>
int gru_seed_or_zero(StreamCall& c, const float* src, const GruSteps& d, int n, const int* tab, bool save, hipStream_t s) {
  const size_t st = (size_t)d.B * d.rows * d.S;
  if (c.needs_seed()) {
    gru_seed_kernel<T><<<(int)std::min<size_t>((st + 255) / 256, 4096), 256, 0, s>>>(c.carry() ? src : nullptr, d.hall, (T*)d.hp, tab, d.hp_img,
                                                                                    d.B, d.rows, n, d.S);
    RGP_HIP(hipGetLastError());
    c.seed_done(save);
    return RGP_OK;
  }
  if (!save) RGP_HIP(hipMemsetAsync(d.hp, 0, (size_t)d.B * d.hp_img * sizeof(T), s));
  RGP_HIP(hipMemsetAsync(d.hall, 0, st * 4, s));
  return RGP_OK;
}

// The way out: dst [B][rows][n] dense = the first n channels of the fp32 state rows at src (one strided copy)
inline int gru_state_out(const float* src, float* dst, const int* tab, const GruSteps& d, int n, hipStream_t s) {
  if (!dst) return RGP_OK;
  const long long total = (long long)d.B * d.rows * n;
  unpad_kernel<float><<<(int)std::min<long long>((total + 255) / 256, 8192), 256, 0, s>>>(src, dst, tab, d.rows, n, (long long)d.rows * d.S, total);
  RGP_HIP(hipGetLastError());
  return RGP_OK;
}

}  // namespace rgp
