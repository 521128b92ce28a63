/* librgp_hip.so -- C ABI of the MI355X-native recurrent gaze-prediction path.
 *
 * The reference (yj-yu/Recurrent_Gaze_Prediction) has no FFI/plugin boundary: its
 * seam is the Python graph builder `create_gazeprediction_network(frame_images,
 * c3d_input, dropout_keep_prob, net)` (models/gaze_grcn.py:173-188) executed by a
 * single `session.run(feed_dict)` (models/gaze_rnn.py:523-531, 603-611).  This
 * header is the boundary a maintainer would bind in its place: each entry point
 * cites the reference lines whose computation it replaces.
 *
 * Conventions
 *  - every function returns 0 (RGP_OK) or a negative RGP_E* code; the message is in
 *    rgp_last_error() (thread-local);
 *  - every tensor argument is a caller-owned DEVICE pointer (fp32 unless stated);
 *    the library never allocates device memory: the caller provides one workspace
 *    of rgp_*_workspace_bytes() bytes per plan;
 *  - every call is asynchronous on the given HIP stream (a hipStream_t passed as
 *    void*); a plan may be used from one stream at a time.  Training plans (and the
 *    cascade's forward) run independent parts of a call -- weight gradients beside the
 *    data-gradient chain, the cascade's two cells one time step apart -- on streams of
 *    the library's own (three per device, shared by every plan of the process), forked
 *    behind `stream` and joined into it before the call returns: to the caller the call
 *    is ordered on `stream` as if it ran there alone.  The same holds inside a stream
 *    capture (the forks become branches of the graph once the library's streams exist,
 *    i.e. after one eager call; before that the call is serial).  Because those streams
 *    are shared, they join a capture for its duration: while one host thread captures
 *    calls of this library, no other thread may issue training calls on that device;
 *  - layouts are the reference's: c3d_input [B,T,1024,7,7], maps [B,T,49,49],
 *    conv filters HWIO / DHWIO, transposed-conv filters [kh,kw,out,in];
 *  - dtype selects the MFMA operand type of the contractions (RGP_BF16:
 *    v_mfma_f32_16x16x32_bf16, RGP_F32: v_mfma_f32_16x16x4_f32); accumulation,
 *    gate math, recurrent state, logits and losses are always fp32.
 */
#ifndef RGP_H_
#define RGP_H_
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RGP_OK 0
#define RGP_EINVAL (-1)   /* bad argument / unsupported shape */
#define RGP_EHIP (-2)     /* a HIP runtime call failed */
#define RGP_EWORKSPACE (-3) /* workspace missing or too small */
#define RGP_ESTATE (-4)   /* call order violated (e.g. forward before set_weights) */
#define RGP_ETIMEOUT (-5) /* a persistent ConvGRU launch lost a group member: its outputs are NaN-poisoned (rgp_grcn_status) */

#define RGP_F32 0
#define RGP_BF16 1

typedef void* rgp_stream_t; /* hipStream_t */

const char* rgp_last_error(void);
int rgp_version(void);
/* Writes the gcnArchName of the current device ("gfx950...") into buf. */
int rgp_device_arch(char* buf, int buflen);

/* ------------------------------------------------------------------ gaze_grcn */
typedef struct rgp_grcn rgp_grcn_t;

/* fp32 device pointers, reference variable names:
 * proj_c3d_W [1024,P] proj_c3d_b [P]                    gaze_grcn.py:234-237
 * gru_W{z,r,}  [3,3,P,S]   gru_U{z,r,} [3,3,S,S]        gaze_grcn.py:64-81
 * bn_gamma, bn_beta [T,S] (one BN layer per timestep)   gaze_grcn.py:325
 * up_weight1 [5,5,64,S] up_weight2 [5,5,32,64] up_weight3 [7,7,12,32]   gaze_grcn.py:292-310
 * out_W [12,1] out_b [1]                                gaze_grcn.py:311-314 */
typedef struct rgp_grcn_weights {
  const float *proj_c3d_W, *proj_c3d_b;
  const float *gru_Wz, *gru_Uz, *gru_Wr, *gru_Ur, *gru_W, *gru_U;
  const float *bn_gamma, *bn_beta;
  const float *up_weight1, *up_weight2, *up_weight3;
  const float *out_W, *out_b;
} rgp_grcn_weights;

/* Plan for GazePredictionGRCN.create_gazeprediction_network (gaze_grcn.py:173-376)
 * at fixed batch B, timesteps T, dim_cnn_proj P (512), rnn_state_size S (128). */
int rgp_grcn_create(rgp_grcn_t** plan, int batch, int n_steps, int dim_proj, int dim_state, int dtype,
                    int flags);
/* flags (0 / 1 keep the meaning of the former `save_for_backward` argument):
 *  RGP_GRCN_SAVE_FOR_BACKWARD  training plan (gates, states and operand images kept for rgp_grcn_backward);
 *  RGP_GRCN_PER_STEP           run the ConvGRU recurrence and its BPTT as per-timestep launches even where the
 *                              persistent kernels apply (bf16, 128 state channels, <= 64 clips): the library's second
 *                              implementation of the recurrence, always used by f32 plans;
 *  RGP_GRCN_UNFOLDED_HEAD      by default a plan runs the saliency head (gaze_grcn.py:326-361) folded: the three transposed
 *                              convolutions and out_W have no bias or non-linearity between them and are combined, exactly,
 *                              into one 19x19 stride-6 transposed convolution on BN(h_t) when the weights are set (GEMM +
 *                              col2im forward; the backward is the chain rule through the fold and returns the gradients of
 *                              weight1 / weight2 / weight3 / out_W themselves).  With this flag the plan runs the three
 *                              stages one by one, forward and backward: the library's second implementation of the head;
 *                              the buffers "d1" / "d2" of rgp_grcn_read_buffer exist only then. */
#define RGP_GRCN_SAVE_FOR_BACKWARD 1
#define RGP_GRCN_PER_STEP 2
#define RGP_GRCN_UNFOLDED_HEAD 4
/* The persistent ConvGRU kernels (one launch for all T steps, forward and BPTT) need all their workgroups resident
 * together: keep ONE of them in flight per device.  Launches issued through this library from one process are
 * serialised against each other automatically (any stream, any plan, any host thread: the wait for the previous
 * launch, the launch and its record are one critical section); a launch that nevertheless loses a group member
 * -- another process running the same kernels on the device -- gives up after about a second, NaN-poisons everything
 * computed from it (logits, maps, states, gradients) and raises the plan's error state: the next call on the plan
 * returns RGP_ETIMEOUT, and so does rgp_grcn_status, which first waits for `stream`.  The state is cleared by being
 * reported. */
int rgp_grcn_status(rgp_grcn_t* plan, rgp_stream_t stream);
/* Test hook: the next persistent sequence (kind 1) / BPTT (kind 2) launch of the plan runs without one member of its
 * first group, i.e. exercises the time-out path above (about one second).  RGP_ESTATE if the plan uses per-step launches. */
#define RGP_FAULT_SEQ_LOST_MEMBER 1
#define RGP_FAULT_BPTT_LOST_MEMBER 2
int rgp_grcn_inject_fault(rgp_grcn_t* plan, int kind);
int rgp_grcn_destroy(rgp_grcn_t* plan);
size_t rgp_grcn_workspace_bytes(const rgp_grcn_t* plan);
/* Uploads the offset tables and zeroes the halos.  Once per workspace. */
int rgp_grcn_bind_workspace(rgp_grcn_t* plan, void* workspace, size_t bytes, rgp_stream_t stream);
/* Packs the fp32 weights into MFMA operand form ([N][K], operand dtype). Call after
 * every weight update. */
int rgp_grcn_set_weights(rgp_grcn_t* plan, const rgp_grcn_weights* w, rgp_stream_t stream);

/* Whole graph: c3d_input [B,T,1024,7,7] -> logits [B,T,49,49]
 * (gaze_grcn.py:173-376) and, if probs != NULL, the per-frame softmax that
 * build_model applies for loss_type xentropy (gaze_rnn.py:149-159). */
int rgp_grcn_forward(rgp_grcn_t* plan, const float* c3d_input, float* logits, float* probs, rgp_stream_t stream);
/* Same graph fed by C3D conv5b rows produced by rgp_c3d_forward (operand dtype,
 * [B*T*49][1024] with K order d*512+c), skipping the transpose of gaze_grcn.py:225-227. */
int rgp_grcn_forward_rows(rgp_grcn_t* plan, const void* c3d_rows, float* logits, float* probs, rgp_stream_t stream);

/* Streaming inference: the same graph with the recurrent state carried across calls, so that a video longer than the
 * plan's T steps is one recurrence and not a row of unrelated clips.  Streaming is a call, not a plan property.
 *   c3d_input / c3d_rows  exactly one is non-NULL; laid out as for rgp_grcn_forward / _forward_rows, always [B,T,...]
 *   state_in   fp32 [B][49][S] (16-byte aligned), NULL = the zero state; never written
 *   state_out  may be NULL; must not alias state_in; receives the state behind step n_valid
 *   n_valid    1..T: the recurrence is defined for steps 0..n_valid-1.  The outputs of later steps are unspecified; their
 *              inputs are read, but influence neither the first n_valid outputs nor state_out
 *   bn_phase   0..T-1: step t of the call uses batch-norm slot (bn_phase + t) % T.  A caller that passes its stream
 *              position mod T gets results that do not depend on where the stream was cut; with cuts at multiples of T
 *              this is the reference's chunked evaluation plus a carried state.
 * rgp_grcn_forward_stream(.., NULL, state_out, T, 0, ..) computes what rgp_grcn_forward computes.  Argument errors are
 * RGP_EINVAL and are reported ahead of the plan's bound / weights state.  A training plan accepts the call; a following
 * rgp_grcn_backward / _from_states returns RGP_ESTATE until a plain forward has run (they differentiate a recurrence from the
 * zero state over all T steps with batch-norm slot t), and rgp_grcn_backward_stream below differentiates the call.
 * A persistent launch that times out (rgp_grcn_status) NaN-poisons state_out of its clips along with the maps; state_in
 * being read-only, the caller repeats the call.
 * rgp_grcn_state_elems: B*49*S, the fp32 elements of a state; host-only, works on an unbound plan. */
size_t rgp_grcn_state_elems(const rgp_grcn_t* plan);
int rgp_grcn_forward_stream(rgp_grcn_t* plan, const float* c3d_input, const void* c3d_rows, const float* state_in, float* state_out,
                            int n_valid, int bn_phase, float* logits, float* probs, rgp_stream_t stream);
/* Training across the carried state: the backward of the plan's LAST forward of either kind, on a training plan, either BPTT
 * path.  Behind rgp_grcn_forward_stream(.., state_in, .., n_valid, bn_phase, ..) it differentiates that call: steps
 * 0 .. n_valid-1, the recurrence started at state_in, step t through batch-norm slot (bn_phase + t) % T (its gamma is read and
 * its gradient slot written; the slots of the steps behind n_valid receive zeros).  Behind rgp_grcn_forward / _forward_rows:
 * all T steps from the zero state, slot t.
 *   loss         that of rgp_grcn_backward, summed over the frames of the valid steps and divided by loss_frames (> 0): the
 *                caller's divisor, so that the gradients of a film's chunks add up to the gradient of a mean over the film.
 *                logits, probs, labels are full size [B,T,49,49]; what lies behind n_valid reaches no output
 *   d_state_out  fp32 [B][49][S], 16-byte aligned: the gradient of whatever comes later w.r.t. the state_out the forward handed
 *                out (the state behind step n_valid); NULL = zeros (truncated BPTT, or a film's last chunk); never written
 *   d_state_in   fp32 [B][49][S], 16-byte aligned, may be NULL, must not be d_state_out: receives d loss / d state_in.  A
 *                persistent BPTT launch that times out poisons the gate-gradient rows of the valid steps and this: NaN, never
 *                finite and wrong
 *   grads        written, not accumulated, as rgp_grcn_backward writes them; rgp_grcn_wait_grads works as behind it
 * The inputs of the forward must be finite over all T steps, also behind n_valid: the gradient rows of those steps are zero,
 * and the hoisted filter gradients multiply them with what the forward saved there.
 * rgp_grcn_backward_input behind this call returns d_rows with the rows of the steps >= n_valid exactly zero.
 * Argument errors are RGP_EINVAL, name the argument, and come ahead of the bound / weights checks; an inference plan, or a plan
 * with no forward yet, is RGP_ESTATE.  rgp_grcn_backward and rgp_grcn_backward_from_states are unchanged and keep refusing
 * behind a streaming forward.  Not captured into HIP graphs (not tested). */
int rgp_grcn_backward_stream(rgp_grcn_t* plan, const float* logits, const float* probs, const float* labels,
                             const float* d_state_out, float* d_state_in, long long loss_frames,
                             const rgp_grcn_weights* grads, int loss_type, rgp_stream_t stream);

/* Stages of the same graph on the plan's workspace (for tests / profiling):
 * rgp_proj_fwd          transpose + xw_plus_b                  gaze_grcn.py:225-254
 * rgp_convgru_xconv_fwd W_z,W_r,W convs of all T steps at once gaze_grcn.py:108-109,112-113,122-123
 * rgp_convgru_seq_fwd   T x { U convs, gates, blend } + BN     gaze_grcn.py:110-127,259-288,325
 * rgp_head_fwd          3 transposed convs + 12->1             gaze_grcn.py:326-366 */
int rgp_proj_fwd(rgp_grcn_t* plan, const float* c3d_input, rgp_stream_t stream);
int rgp_convgru_xconv_fwd(rgp_grcn_t* plan, rgp_stream_t stream);
int rgp_convgru_seq_fwd(rgp_grcn_t* plan, rgp_stream_t stream);
int rgp_head_fwd(rgp_grcn_t* plan, float* logits, rgp_stream_t stream);

/* Copies an intermediate, un-padded and widened to fp32, into dst:
 * "c3d_embedded" [B,T,7,7,P]   "xpre" [B,T,7,7,3S] (z|r|c pre-activations of W*x)
 * "rcn_outputs" [B,T,7,7,S] (h_t)   "bn" [B,T,7,7,S]   "d1" [B*T,23,23,64]   "d2" [B*T,49,49,32]
 * "u" / "r" / "c" [T,B,7,7,S] (r,c only with save_for_backward).
 * Of the last backward of a save_for_backward plan (read-only, for tests): "dxpre" [B,T,7,7,3S] (gradients of the z|r|c
 * pre-activations)   "dh_head" [T,B,7,7,S] (gradient reaching h_t from the head, behind the batch-norm backward). */
int rgp_grcn_read_buffer(rgp_grcn_t* plan, const char* name, float* dst, rgp_stream_t stream);
/* Number of fp32 elements rgp_grcn_read_buffer writes for name (0 if unknown). */
size_t rgp_grcn_buffer_elems(const rgp_grcn_t* plan, const char* name);

/* Per-frame softmax (model_util.py:61-64) and cross entropy with summed/averaged
 * loss (model_util.py:66-72, gaze_rnn.py:390-407): logits, labels [frames, npix];
 * probs, frame_loss [frames], loss [1] may each be NULL.  loss = sum(frame_loss)/frames. */
int rgp_softmax_xent_fwd(const float* logits, const float* labels, float* probs, float* frame_loss, float* loss,
                         int frames, int npix, rgp_stream_t stream);

/* Backward of the same graph under the loss of gaze_rnn.py:363-408 (what tf.gradients builds,
 * base.py:278-281).  Needs a plan created with save_for_backward=1 and a preceding
 * rgp_grcn_forward on the same inputs (its saved states live in the workspace).
 * logits / probs: outputs of that forward; labels: per-frame-normalised ground-truth maps
 * [B,T,49,49] (normalize_probability_map, model_util.py:40-58).  loss_type 0 = xentropy,
 * 1 = l2.  grads: fp32 device arrays shaped like the weights; fully overwritten. */
int rgp_grcn_backward(rgp_grcn_t* plan, const float* logits, const float* probs, const float* labels,
                      const rgp_grcn_weights* grads, int loss_type, rgp_stream_t stream);

/* Backward of the projection + ConvGRU only, for a network that stacks its own layers on the states
 * (the cascade, gaze_grcn_cascade.py:289-336): d_states [B*T*49, S] fp32 is the gradient w.r.t. the
 * batch-normalised states in frame order b*T+t; the head fields of grads receive zeros. */
int rgp_grcn_backward_from_states(rgp_grcn_t* plan, const float* d_states, const rgp_grcn_weights* grads,
                                  rgp_stream_t stream);

/* Data-parallel training: rgp_grcn_backward / _from_states record an event on their stream once a group
 * of gradients is final, in this order -- RGP_GRCN_GRADS_TOP: bn_gamma, bn_beta, up_weight1..3, out_W, out_b (before
 * the BPTT starts); RGP_GRCN_GRADS_GRU: the six ConvGRU filters; RGP_GRCN_GRADS_PROJ: proj_c3d_W / _b (the end of the
 * backward).  rgp_grcn_wait_grads makes `waiting_stream` wait for that event, so the host can issue the all-reduce
 * of the group's slice there while the rest of the backward is still running.  RGP_ESTATE before the first backward,
 * and after a backward that was captured into a HIP graph (nothing is recorded during capture; a replay has no events). */
#define RGP_GRCN_GRADS_TOP 0
#define RGP_GRCN_GRADS_GRU 1
#define RGP_GRCN_GRADS_PROJ 2
int rgp_grcn_wait_grads(rgp_grcn_t* plan, int group, rgp_stream_t waiting_stream);
/* Co-residency rule for that overlap.  The persistent BPTT launch occupies one CU per workgroup (8 per group of 1 - 2
 * clips; 157 KB of LDS each, so nothing else fits beside one) and cannot make progress until ALL of them are resident.
 * A collective started before it may hold CUs for as long as the slowest peer rank takes.  Therefore the TOP group's
 * event is recorded ahead of the BPTT launch only when that launch needs at most (CUs of the device -
 * RGP_RCCL_CU_RESERVE) workgroups (on a 256-CU MI355X: up to 24 clips per GPU, e.g. BASELINE config 4's 8); larger
 * per-GPU batches (config 3's 64 clips = 256 workgroups) record it BEHIND the launch, so no collective of this step can
 * run next to it.  Per-step plans (RGP_GRCN_PER_STEP, f32) always release it early.  rgp_grcn_grads_top_early reports
 * which of the two the plan does on the current device: 1 = before the BPTT, 0 = behind it. */
#define RGP_RCCL_CU_RESERVE 64
int rgp_grcn_grads_top_early(const rgp_grcn_t* plan);
/* Workgroups (= CUs) a persistent ConvGRU / BPTT launch of this plan occupies on the current device; 0 if the plan runs
 * the recurrence as per-timestep launches (RGP_GRCN_PER_STEP, f32, other widths, more clips than the device has CUs for). */
int rgp_grcn_persistent_workgroups(const rgp_grcn_t* plan);

/* After rgp_grcn_backward: the gradient w.r.t. the network input, d_rows [B*T*49, 1024] fp32 in the column
 * order of the conv5b rows (d*512 + c) -- what rgp_c3d_backward takes when the conv stack is fine-tuned
 * end to end (BASELINE config 5). */
int rgp_grcn_backward_input(rgp_grcn_t* plan, float* d_rows, rgp_stream_t stream);

/* tf.clip_by_global_norm + tf.train.AdamOptimizer.apply_gradients on one flat fp32 parameter
 * buffer (base.py:286-297; TF form: lr_t = lr*sqrt(1-b2^t)/(1-b1^t), theta -= lr_t*m/(sqrt(v)+eps),
 * t = step+1).  workspace: 256 floats.  grad_norm_out (optional, device): the global norm.
 * max_grad_norm <= 0 disables clipping. */
int rgp_adam_clip_step(float* params, const float* grads, float* m, float* v, long long n, float* workspace,
                       int step, float lr, float beta1, float beta2, float eps, float max_grad_norm,
                       float* grad_norm_out, rgp_stream_t stream);

/* The same step when the variables live in several flat buffers (conv stack + head, config 5): the clip
 * norm is global over ALL of them (base.py:286-292).  rgp_global_sqnorm writes RGP_SQNORM_PARTIALS partial
 * sums of squares of one buffer; rgp_adam_clip_step_ext applies the step to one buffer given the
 * concatenated partials of all buffers. */
#define RGP_SQNORM_PARTIALS 256
int rgp_global_sqnorm(const float* grads, long long n, float* partials, rgp_stream_t stream);
int rgp_adam_clip_step_ext(float* params, const float* grads, float* m, float* v, long long n, const float* partials,
                           int n_partials, int step, float lr, float beta1, float beta2, float eps, float max_grad_norm,
                           float* grad_norm_out, rgp_stream_t stream);

/* Graph-replayable optimizer step: the learning-rate schedule (gaze_rnn.py:436-444: lr0 * decay^floor(step /
 * decay_steps)) and Adam's bias correction are evaluated ON THE DEVICE from a device-resident step counter, so a
 * whole training step captured in a HIP graph replays correctly.  rgp_lr_schedule_step writes lr_t and advances
 * the counter (once per training step); rgp_adam_clip_step_dev is rgp_adam_clip_step_ext reading lr_t. */
int rgp_lr_schedule_step(int* step_dev, float lr0, float decay, int decay_steps, float beta1, float beta2, float* lr_t_dev,
                         rgp_stream_t stream);
int rgp_adam_clip_step_dev(float* params, const float* grads, float* m, float* v, long long n, const float* partials,
                           int n_partials, const float* lr_t_dev, float beta1, float beta2, float eps, float max_grad_norm,
                           float* grad_norm_out, rgp_stream_t stream);

/* The other two optimizers of create_train_op (base.py:268-273), same clip-then-apply contract and the same
 * `partials` (rgp_global_sqnorm of every flat buffer, concatenated) as rgp_adam_clip_step_ext:
 *  rgp_momentum_clip_step : tf.train.MomentumOptimizer(lr, momentum=0.9)   accum = momentum*accum + g; var -= lr*accum
 *  rgp_rmsprop_clip_step  : tf.train.RMSPropOptimizer(lr, decay=0.9, momentum=0.9, epsilon=1e-10)
 *                           ms = decay*ms + (1-decay)*g^2; mom = momentum*mom + lr*g/sqrt(ms+eps); var -= mom
 *                           (TF initialises the ms slot to ones, mom to zeros: the caller owns the slots). */
int rgp_momentum_clip_step(float* params, const float* grads, float* accum, long long n, const float* partials, int n_partials,
                           float lr, float momentum, float max_grad_norm, float* grad_norm_out, rgp_stream_t stream);
int rgp_rmsprop_clip_step(float* params, const float* grads, float* ms, float* mom, long long n, const float* partials,
                          int n_partials, float lr, float decay, float momentum, float eps, float max_grad_norm,
                          float* grad_norm_out, rgp_stream_t stream);

/* l2 loss (gaze_rnn.py:387-389, gaze_grcn_cascade.py:428-441): loss[0] = sum 0.5 (maps - labels)^2 / frames over
 * n elements; workspace: RGP_SQNORM_PARTIALS floats (deterministic two-stage sum). */
int rgp_l2_loss_fwd(const float* maps, const float* labels, long long n, int frames, float* workspace, float* loss,
                    rgp_stream_t stream);

/* Inverted dropout as an op (tf.nn.dropout: keep element i iff floor(keep_prob + u_i) = 1, kept values / keep_prob).
 * rgp_dropout_mask draws the keep mask (1 byte per element, 0 / 1) on the device with Philox-4x32-10 keyed by `seed`;
 * element i uses word i&3 of counter block offset + i/4, so the draw is independent of the launch geometry and a
 * caller advances `offset` by ceil(n/4) per training step.  The mask is the caller's: the training forward of a plan
 * with a dropout site reads it (rgp_fcgru_set_dropout, rgp_cascade_set_dropout) and the backward gates with the same
 * bytes.  rgp_dropout_apply is the op on a dense fp32 vector, in place (also its own backward). */
int rgp_dropout_mask(unsigned char* mask, long long n, float keep_prob, unsigned long long seed, unsigned long long offset,
                     rgp_stream_t stream);
int rgp_dropout_apply(float* x, const unsigned char* mask, long long n, float keep_prob, rgp_stream_t stream);

/* Stage timing (HIP events recorded on the caller's stream around each stage launch
 * group; costs two hipEventRecord per stage).  Stages: 0 proj (incl. transpose),
 * 1 xconv, 2 convgru sequence, 3 head (transposed convs), 4 softmax.
 * rgp_grcn_profile_read synchronises on the recorded events, writes the accumulated
 * milliseconds and launch-group counts since the last read, and resets them. */
#define RGP_GRCN_STAGES 5
int rgp_grcn_profile_enable(rgp_grcn_t* plan, int enable);
int rgp_grcn_profile_read(rgp_grcn_t* plan, double ms[RGP_GRCN_STAGES], long long calls[RGP_GRCN_STAGES]);

/* ------------------------------------------------------------------ fc-GRU (gaze_rnn) */
typedef struct rgp_fcgru rgp_fcgru_t;

/* GazePredictionGRU.create_gazeprediction_network (models/gaze_rnn.py:211-360), fp32 device
 * pointers: proj_c3d_W [1024,32] proj_c3d_b [32] (gaze_rnn.py:294-295); TF-1.x GRUCell(1617)
 * variables gates_kernel [1568+1617, 2*1617] (columns [r | u]), gates_bias [2*1617],
 * candidate_kernel [1568+1617, 1617], candidate_bias [1617] (gaze_rnn.py:315);
 * proj_out_W [1617, GH*GW], proj_out_b [GH*GW] (gaze_rnn.py:319-320). */
typedef struct rgp_fcgru_weights {
  const float *proj_c3d_W, *proj_c3d_b;
  const float *gates_kernel, *gates_bias, *candidate_kernel, *candidate_bias;
  const float *proj_out_W, *proj_out_b;
} rgp_fcgru_weights;

int rgp_fcgru_create(rgp_fcgru_t** plan, int batch, int n_steps, int gazemap_h, int gazemap_w, int dtype);
int rgp_fcgru_destroy(rgp_fcgru_t* plan);
size_t rgp_fcgru_workspace_bytes(const rgp_fcgru_t* plan);
int rgp_fcgru_bind_workspace(rgp_fcgru_t* plan, void* workspace, size_t bytes, rgp_stream_t stream);
int rgp_fcgru_set_weights(rgp_fcgru_t* plan, const rgp_fcgru_weights* w, rgp_stream_t stream);
/* c3d_input [B,T,1024,7,7] -> logits [B,T,GH,GW]; probs (optional) = per-frame softmax. */
int rgp_fcgru_forward(rgp_fcgru_t* plan, const float* c3d_input, float* logits, float* probs, rgp_stream_t stream);

/* Training (config 2): a plan created with save_for_backward = 1 keeps the gates and operand rows of every step;
 * rgp_fcgru_backward then differentiates the loss of gaze_rnn.py:363-408 (loss_type 0 xentropy, 1 l2) w.r.t.
 * all eight variables (grads: arrays shaped like the weights, fully overwritten), as rgp_grcn_backward does. */
int rgp_fcgru_create_ex(rgp_fcgru_t** plan, int batch, int n_steps, int gazemap_h, int gazemap_w, int dtype,
                        int save_for_backward);
int rgp_fcgru_backward(rgp_fcgru_t* plan, const float* logits, const float* probs, const float* labels,
                       const rgp_fcgru_weights* grads, int loss_type, rgp_stream_t stream);

/* Training-time dropout on the projected features c3d_embedded [B*T*49, 32] (gaze_rnn.py:302-303; single_step feeds
 * keep 0.5 when training, :529).  mask: device bytes [B*T*49*32] from rgp_dropout_mask (or the caller's own draw), read
 * by every following forward AND backward until changed; keep_prob = 1 or mask = NULL switches the site off
 * (inference, the default). */
int rgp_fcgru_set_dropout(rgp_fcgru_t* plan, float keep_prob, const unsigned char* mask);

/* rgp_fcgru_create with flags (rgp_fcgru_create = flags 0, rgp_fcgru_create_ex = RGP_FCGRU_SAVE_FOR_BACKWARD or 0):
 *   RGP_FCGRU_SAVE_FOR_BACKWARD  training plan (gates, states and operand rows of every step kept for rgp_fcgru_backward);
 *   RGP_FCGRU_PER_STEP           run the recurrence as two launches per timestep (what every plan did so far);
 *   RGP_FCGRU_PERSISTENT         run all T steps of the recurrence in ONE persistent launch with the h-side kernels
 *                                resident in registers (csrc/fcgru_seq.hip.h).  Refused with RGP_EINVAL, the reason in
 *                                rgp_last_error(): f32 plans, batch > 64, n_steps > 16384, and -- asked of the current
 *                                device at create -- a device with fewer CUs than the launch has workgroups (203).
 *   RGP_FCGRU_BPTT_PERSISTENT    run the backward-through-time pass of rgp_fcgru_backward in ONE persistent launch with the
 *                                transposed h-side kernels resident in registers (csrc/fcgru_bptt.hip.h), whatever path the
 *                                forward takes; without it the pass is four launches per timestep, as on every plan so
 *                                far.  Refused with RGP_EINVAL, the reason in rgp_last_error(): without
 *                                RGP_FCGRU_SAVE_FOR_BACKWARD, f32 plans, batch > 64, (batch * n_steps + 1) * 3 * 1664 * 2
 *                                bytes (the gate-gradient rows, which the kernel addresses with 32-bit offsets; batch
 *                                rounded up to a multiple of 16) not below 2^32 (batch 64: n_steps <= 6721) -- these four
 *                                need no device -- and a device with fewer than 203 CUs.
 *   RGP_FCGRU_PERSISTENT_F32     RGP_FCGRU_PERSISTENT for f32 plans: all T steps in ONE persistent launch with the fp32 h-side
 *                                kernels resident in registers and fp32 MFMAs on the plan's own fp32 operand rows
 *                                (csrc/fcgru_seq_f32.hip.h).  A flag of its own because RGP_FCGRU_PERSISTENT keeps refusing
 *                                f32 plans.  Refused with RGP_EINVAL, the reason in rgp_last_error(): plans that are not f32,
 *                                batch > 64, together with RGP_FCGRU_PER_STEP or RGP_FCGRU_PERSISTENT, n_steps > 8192
 *                                (64 * n_steps * 1664 * 4 bytes of exchange rows are addressed with 32-bit offsets) -- these
 *                                need no device -- and a device with fewer than 203 CUs.  The backward behind it is the
 *                                per-step one unless RGP_FCGRU_BPTT_PERSISTENT_F32 is set (RGP_FCGRU_BPTT_PERSISTENT stays
 *                                bf16 only).
 *   RGP_FCGRU_BPTT_PERSISTENT_F32  RGP_FCGRU_BPTT_PERSISTENT for f32 plans: the backward-through-time pass in ONE persistent
 *                                launch with the transposed fp32 h-side kernels resident in registers and LDS and fp32
 *                                MFMAs on the plan's own fp32 gate-gradient rows (csrc/fcgru_bptt_f32.hip.h), whatever path
 *                                the forward takes.  A flag of its own because RGP_FCGRU_BPTT_PERSISTENT keeps refusing f32
 *                                plans.  Refused with RGP_EINVAL, the reason in rgp_last_error(): without
 *                                RGP_FCGRU_SAVE_FOR_BACKWARD, plans that are not f32, batch > 64, together with
 *                                RGP_FCGRU_BPTT_PERSISTENT, (batch16 * n_steps + 1) * 3 * 1664 * 4 bytes (batch16 = batch
 *                                rounded up to a multiple of 16) not below 2^32 (batch 64: n_steps <= 3360) -- these need
 *                                no device -- and a device with fewer than 203 CUs.
 * With no path flag the library's choice is per step.  Unknown bits and two path flags together are RGP_EINVAL.  All
 * paths fill the same buffers in the same layouts: rgp_fcgru_backward runs behind any of them. */
#define RGP_FCGRU_SAVE_FOR_BACKWARD 1
#define RGP_FCGRU_PER_STEP 2
#define RGP_FCGRU_PERSISTENT 4
#define RGP_FCGRU_BPTT_PERSISTENT 8
#define RGP_FCGRU_PERSISTENT_F32 16
#define RGP_FCGRU_BPTT_PERSISTENT_F32 32
int rgp_fcgru_create_flags(rgp_fcgru_t** plan, int batch, int n_steps, int gazemap_h, int gazemap_w, int dtype, int flags);
/* Workgroups (= CUs) a persistent recurrence launch of this plan occupies; 0: the plan runs per-step launches. */
int rgp_fcgru_persistent_workgroups(const rgp_fcgru_t* plan);
/* The same for the persistent BPTT launch of rgp_fcgru_backward: 203, or 0 (plans without RGP_FCGRU_BPTT_PERSISTENT
 * or RGP_FCGRU_BPTT_PERSISTENT_F32). */
int rgp_fcgru_bptt_persistent_workgroups(const rgp_fcgru_t* plan);
/* Time-out of the persistent launch, as for the other recurrent families: all its workgroups must be resident together
 * (keep ONE such launch in flight per device).  A launch that waits about a second for a missing member stops waiting,
 * NaN-poisons the h rows of every step and clip (NaN logits) and the fp32 states, and sets the plan's error word: the
 * next rgp_fcgru_forward, or rgp_fcgru_status, which first waits for `stream`, returns RGP_ETIMEOUT once.  RGP_OK on
 * per-step plans.  A persistent BPTT launch that times out NaN-poisons its units of all three parts of every gate-gradient
 * row ("dxpre" below) and of the final carry ("dh0"): every filter gradient and the projection's input gradient are then
 * NaN; rgp_fcgru_status, or the next rgp_fcgru_forward / rgp_fcgru_backward of the plan, returns RGP_ETIMEOUT once. */
int rgp_fcgru_status(rgp_fcgru_t* plan, rgp_stream_t stream);
/* Intermediates of the last forward of a TRAINING plan as fp32 (padding columns dropped, bf16 buffers widened), either
 * recurrence path: "xpre" [B,T,3,1617] hoisted x parts + biases, column blocks u, r, c; "h" [T+1,B,1617] fp32 states,
 * slot 0 = h_0; "u", "r", "c" [T,B,1617] gates; "hp" [B,T+1,1617] the operand rows of h (slot t = h_{t-1} of step t);
 * "rh" [B,T,1617] the operand rows r * h_{t-1}.  rgp_fcgru_buffer_elems: their sizes (0: unknown name, or an inference
 * plan).  Errors: RGP_EINVAL for an unknown name; RGP_ESTATE on an inference plan or before the first forward.
 * Of the last BACKWARD, either BPTT path (RGP_ESTATE before the first one): "dxpre" [B,T,3,1617] the gate-gradient operand
 * rows d loss / d pre-activation, parts [u | r | c] (row 0 of the buffer, all zero, is skipped); "dh_head" [B,T,1617] fp32
 * d loss / d h_t through the read-out alone; "dh0" [B,1617] fp32 the final carry, d loss / d h_{-1}. */
int rgp_fcgru_read_buffer(rgp_fcgru_t* plan, const char* name, float* dst_fp32, rgp_stream_t stream);
size_t rgp_fcgru_buffer_elems(const rgp_fcgru_t* plan, const char* name);
/* Streaming inference, as rgp_grcn_forward_stream without bn_phase (this graph has no per-timestep batch-norm) and without
 * a rows entry.  Streaming is a call, not a plan property: any plan takes it, on either recurrence path.
 *   state_in   fp32 [B][1617], dense (the layout of a slot of "h" above, not the padded 1664); NULL = the zero state;
 *              never written
 *   state_out  may be NULL; must not be state_in; receives h behind step n_valid
 *   n_valid    1..T.  All T steps are computed; the outputs of steps behind n_valid are unspecified, their inputs are read
 *              but reach nothing the caller keeps (projection, x-GEMM, read-out and softmax are per frame, the recurrence
 *              is causal)
 * rgp_fcgru_forward_stream(.., NULL, state_out, T, ..) computes exactly what rgp_fcgru_forward computes.  Argument errors
 * are RGP_EINVAL, name the argument, and come ahead of the bound / weights checks.  The dropout site behaves as in
 * rgp_fcgru_forward (it is frame-local).  A training plan accepts the call; rgp_fcgru_backward then returns RGP_ESTATE
 * until a plain forward has run (it differentiates a recurrence from the zero state over all T steps), and
 * rgp_fcgru_backward_stream below differentiates the call.  A persistent launch that times out NaN-poisons state_out along with
 * what it poisons anyway; state_in being read-only, the caller repeats the call.
 * rgp_fcgru_state_elems: B*1617, the fp32 elements of a state; host-only, works on an unbound plan. */
size_t rgp_fcgru_state_elems(const rgp_fcgru_t* plan);
int rgp_fcgru_forward_stream(rgp_fcgru_t* plan, const float* c3d_input, const float* state_in, float* state_out, int n_valid,
                             float* logits, float* probs, rgp_stream_t stream);
/* Training across the carried state: the backward of the plan's LAST forward of either kind, on a training plan, either BPTT
 * path.  Behind rgp_fcgru_forward_stream(.., state_in, .., n_valid, ..) it differentiates that call: the first n_valid steps, the
 * recurrence started at state_in.  Behind rgp_fcgru_forward: all T steps from the zero state.
 *   loss         that of rgp_fcgru_backward, summed over the frames of the valid steps and divided by loss_frames (> 0): the
 *                caller's divisor, so that the gradients of a film's chunks add up to the gradient of a mean over the film.
 *                logits, probs, labels are full size [B,T,G]; what lies behind n_valid reaches no output
 *   d_state_out  fp32 [B][1617] dense, the gradient of whatever comes later w.r.t. the state_out the forward handed out;
 *                NULL = zeros (truncated BPTT, or a film's last chunk); never written
 *   d_state_in   fp32 [B][1617] dense, may be NULL, must not be d_state_out: d loss / d state_in, what "dh0" of
 *                rgp_fcgru_read_buffer shows.  A persistent BPTT launch that times out poisons the gate-gradient rows of the
 *                valid steps and this: NaN, never finite and wrong
 *   grads        written, not accumulated, as rgp_fcgru_backward writes them
 * c3d_input of the forward must be finite over all T steps, also behind n_valid: the gradient rows of those steps are zero, and
 * the hoisted filter gradients multiply them with the rows the forward saved there.
 * Argument errors are RGP_EINVAL, name the argument, and come ahead of the bound / weights checks; an inference plan, or a plan
 * with no forward yet, is RGP_ESTATE.  rgp_fcgru_backward itself is unchanged. */
int rgp_fcgru_backward_stream(rgp_fcgru_t* plan, const float* logits, const float* probs, const float* labels,
                              const float* d_state_out, float* d_state_in, long long loss_frames,
                              const rgp_fcgru_weights* grads, int loss_type, rgp_stream_t stream);
/* ------------------------------------------------------------------ gaze_c3d_conv (the no-recurrence baseline) */
typedef struct rgp_c3dconv rgp_c3dconv_t;

/* GazePredictionConv.create_gazeprediction_network (models/gaze_c3d_conv.py:105-218): gaze_grcn's projection and
 * three-stage up-sampling head with the ConvGRU taken out; no batch-norm, no state, both dropout sites inert.  fp32
 * device pointers (proj_c3d_W 16-byte aligned): proj_c3d_W [1024,P] proj_c3d_b [P] (:124-125); up_weight1 [5,5,64,P]
 * up_weight2 [5,5,32,64] up_weight3 [7,7,12,32] out_W [12,1] out_b [1] (:153-173).  The graph is linear per frame:
 * set_weights folds it, in fp32 with sums in a fixed order (equal weights give equal bits), into one 1024 -> 384 filter
 * and a 49x49 bias plane (csrc/c3dconv_fused.hip.h). */
typedef struct rgp_c3dconv_weights {
  const float *proj_c3d_W, *proj_c3d_b, *up_weight1, *up_weight2, *up_weight3, *out_W, *out_b;
} rgp_c3dconv_weights;

/* flags: 0 = the library's choice (bf16 inference plans: the fused kernel -- rows to logits and softmax in one launch;
 * everything else: the staged path -- projection GEMM, folded head GEMM, col2im, softmax).  RGP_C3DCONV_STAGED forces
 * the staged path, RGP_C3DCONV_FUSED the fused kernel (bf16 without SAVE_FOR_BACKWARD only, RGP_EINVAL otherwise).
 * RGP_C3DCONV_SAVE_FOR_BACKWARD: a training plan, keeps the input rows and the projected features.
 * dim_proj: a multiple of 64 (the reference: 512). */
#define RGP_C3DCONV_SAVE_FOR_BACKWARD 1
#define RGP_C3DCONV_STAGED 2
#define RGP_C3DCONV_FUSED 4
int rgp_c3dconv_create(rgp_c3dconv_t** plan, int batch, int n_steps, int dim_proj, int dtype, int flags);
int rgp_c3dconv_destroy(rgp_c3dconv_t* plan);
size_t rgp_c3dconv_workspace_bytes(const rgp_c3dconv_t* plan);
int rgp_c3dconv_bind_workspace(rgp_c3dconv_t* plan, void* workspace, size_t bytes, rgp_stream_t stream);
int rgp_c3dconv_set_weights(rgp_c3dconv_t* plan, const rgp_c3dconv_weights* w, rgp_stream_t stream);
/* c3d_input [B,T,1024,7,7] fp32 (the placeholder layout) -> logits [B,T,49,49]; probs (optional) = per-frame softmax.
 * No atomics on either path: two calls on the same input give the same bits. */
int rgp_c3dconv_forward(rgp_c3dconv_t* plan, const float* c3d_input, float* logits, float* probs, rgp_stream_t stream);
/* c3d_rows: [B*T*49, 1024] in the plan's operand dtype, column d*512+c, 16-byte aligned (what rgp_c3d_forward writes) */
int rgp_c3dconv_forward_rows(rgp_c3dconv_t* plan, const void* c3d_rows, float* logits, float* probs, rgp_stream_t stream);
/* Training plans, after a forward: gradients of the loss of gaze_rnn.py:363-408 (loss_type 0 xentropy: probs and labels
 * are read; 1 l2: logits and labels) w.r.t. the seven variables (grads: arrays shaped like the weights, fully
 * overwritten).  No float atomics: every reduction runs in a fixed order, two calls on the same inputs give the same bits. */
int rgp_c3dconv_backward(rgp_c3dconv_t* plan, const float* logits, const float* probs, const float* labels,
                         const rgp_c3dconv_weights* grads, int loss_type, rgp_stream_t stream);
/* After rgp_c3dconv_backward: d loss / d input as conv5b rows [B*T*49, 1024] fp32 (column d*512+c), the gradient
 * rgp_c3d_backward consumes when the conv stack is fine-tuned beneath this model. */
int rgp_c3dconv_backward_input(rgp_c3dconv_t* plan, float* d_rows, rgp_stream_t stream);
/* fp32 copies of "c3d_embedded" [B*T*49, P] (staged plans, after a forward), "folded_filter" [384, 1024] (row = tap
 * (r+3)*19+t+3 of the 19x19 stride-6 filter, rows 361..383 zero; column = placeholder channel) and "bias_plane" [49,49]
 * (both after set_weights, inference plans).  buffer_elems: the element count, 0 = this plan has no such buffer. */
int rgp_c3dconv_read_buffer(rgp_c3dconv_t* plan, const char* name, float* dst, rgp_stream_t stream);
size_t rgp_c3dconv_buffer_elems(const rgp_c3dconv_t* plan, const char* name);
/* "fused" or "staged": what forward will run */
const char* rgp_c3dconv_path(const rgp_c3dconv_t* plan);
/* ------------------------------------------------------------------ gaze_lstm (the ConvLSTM model) */
typedef struct rgp_lstm rgp_lstm_t;

/* GazePredictionLSTM.create_gazeprediction_network (models/gaze_lstm.py:178-353): projection 1024 -> 512, LSTM_RCN_Cell
 * (:48-148; 128 state channels, 3x3 SAME on 7x7, zero state for c and h, no batch-norm), gaze_grcn's up-sampling head
 * on h_t.  The cell as the reference writes it (:114-131):
 *   i = sigmoid(W_xi*x + W_hi*h + W_ci.c)   f = sigmoid(W_xf*x + W_hf*h + W_cf.c)   g = tanh(W_xc*x + W_hi*h)
 *   c' = f.c + i.g   o = sigmoid(W_xo*x + W_ho*h + W_co.c)   h' = tanh(c').o
 * -- g reuses W_hi, o reads the OLD c, and W_hc [3,3,128,128] is a variable nothing reads: it is carried (checkpoints),
 * its gradient is written as zeros, and the optimizer must leave it out (tf.gradients gives None for it).
 * All fp32 device pointers: W_x* [3,3,512,128], W_h* [3,3,128,128], peepholes W_c* [7,7,128] (per position);
 * the others as in rgp_grcn_weights. */
typedef struct rgp_lstm_weights {
  const float *proj_c3d_W, *proj_c3d_b;
  const float *W_xi, *W_hi, *W_ci, *W_xf, *W_hf, *W_cf, *W_xc, *W_hc, *W_xo, *W_ho, *W_co;
  const float *up_weight1, *up_weight2, *up_weight3, *out_W, *out_b;
} rgp_lstm_weights;

/* flags: RGP_LSTM_SAVE_FOR_BACKWARD  training plan (gates, states and operand images kept for rgp_lstm_backward);
 *        RGP_LSTM_PER_STEP           run the recurrence as one launch per timestep even where the persistent kernel
 *                                    applies: the library's second implementation, always used by f32 plans and by
 *                                    plans with more than 64 clips;
 *        RGP_LSTM_PERSISTENT         ask for the persistent kernel (all T steps in one launch, csrc/convlstm_seq.hip.h):
 *                                    bf16 plans of at most 64 clips, RGP_EINVAL otherwise.  On a device with fewer
 *                                    than 8 CUs per group the plan still runs per step
 *                                    (rgp_lstm_persistent_workgroups tells).
 *        RGP_LSTM_BPTT_PERSISTENT    run the backward-through-time pass of rgp_lstm_backward as one persistent launch
 *                                    (csrc/convlstm_bptt.hip.h) instead of two launches per timestep: only together with
 *                                    RGP_LSTM_SAVE_FOR_BACKWARD, on bf16 plans of at most 64 clips, RGP_EINVAL otherwise.
 *                                    Independent of the two flags of the forward; on a device with too few CUs the plan
 *                                    still runs per step (rgp_lstm_bptt_persistent_workgroups tells).
 *        0                           the library's choice for plans both paths can run: the persistent kernel for the
 *                                    forward, measured faster than per-step launches at both benchmark shapes
 *                                    (DESIGN.md); per-step launches for the BPTT. */
#define RGP_LSTM_SAVE_FOR_BACKWARD 1
#define RGP_LSTM_PER_STEP 2
#define RGP_LSTM_PERSISTENT 4
#define RGP_LSTM_BPTT_PERSISTENT 8
int rgp_lstm_create(rgp_lstm_t** plan, int batch, int n_steps, int dtype, int flags);
int rgp_lstm_destroy(rgp_lstm_t* plan);
size_t rgp_lstm_workspace_bytes(const rgp_lstm_t* plan);
int rgp_lstm_bind_workspace(rgp_lstm_t* plan, void* workspace, size_t bytes, rgp_stream_t stream);
int rgp_lstm_set_weights(rgp_lstm_t* plan, const rgp_lstm_weights* w, rgp_stream_t stream);
/* c3d_input [B,T,1024,7,7] fp32 -> logits [B,T,49,49]; probs (optional) = per-frame softmax.  No float atomics: two
 * calls on the same input give the same bits.  The persistent recurrence kernel computes a clip with the same bits
 * whatever its group slot and the batch size; for the whole forward that also needs the GEMMs around it to pick tiles
 * with one accumulation order, which is tested for clips of a 64 x 16 call against 2 x 16 calls only. */
int rgp_lstm_forward(rgp_lstm_t* plan, const float* c3d_input, float* logits, float* probs, rgp_stream_t stream);
/* c3d_rows: [B*T*49, 1024] in the plan's operand dtype, column d*512+c, 16-byte aligned (what rgp_c3d_forward writes) */
int rgp_lstm_forward_rows(rgp_lstm_t* plan, const void* c3d_rows, float* logits, float* probs, rgp_stream_t stream);
/* Streaming inference, as rgp_grcn_forward_stream without bn_phase (this graph has no per-timestep batch-norm).  The
 * state is [2][B][49][128] fp32: h, then c.  rgp_lstm_state_elems: 2*B*49*128.  After the call rgp_lstm_backward returns
 * RGP_ESTATE until a plain forward has run. */
size_t rgp_lstm_state_elems(const rgp_lstm_t* plan);
int rgp_lstm_forward_stream(rgp_lstm_t* plan, const float* c3d_input, const void* c3d_rows, const float* state_in, float* state_out,
                            int n_valid, float* logits, float* probs, rgp_stream_t stream);
/* Training plans, after a forward: gradients of the loss of gaze_rnn.py:363-408 (loss_type 0 xentropy, 1 l2) w.r.t. the
 * 18 variables (grads: arrays shaped like the weights).  BPTT runs as per-timestep launches, or as one persistent launch
 * on plans created with RGP_LSTM_BPTT_PERSISTENT; grads->W_hc is zeroed. */
int rgp_lstm_backward(rgp_lstm_t* plan, const float* logits, const float* probs, const float* labels,
                      const rgp_lstm_weights* grads, int loss_type, rgp_stream_t stream);
/* After rgp_lstm_backward: d loss / d input as conv5b rows [B*T*49, 1024] fp32 (column d*512+c) */
int rgp_lstm_backward_input(rgp_lstm_t* plan, float* d_rows, rgp_stream_t stream);
/* The persistent kernel fails as the ConvGRU kernels do (rgp_grcn_status): a group that misses a member gives up after
 * about a second, NaN-poisons its clips and raises the plan's error state -- the next call on the plan and
 * rgp_lstm_status (which first waits for `stream`) return RGP_ETIMEOUT once.  The persistent BPTT poisons the
 * pre-activation gradients of step 0 of its clips, and with them every gradient of the call.  rgp_lstm_inject_fault
 * (RGP_FAULT_SEQ_LOST_MEMBER: the forward's kernel, RGP_FAULT_BPTT_LOST_MEMBER: the BPTT's): test hook, the next such
 * launch runs without one member of its first group; RGP_ESTATE on a plan that does not run that kernel. */
int rgp_lstm_status(rgp_lstm_t* plan, rgp_stream_t stream);
int rgp_lstm_inject_fault(rgp_lstm_t* plan, int kind);
/* Workgroups (= CUs) a persistent launch of this plan occupies on the current device; 0 = per-timestep launches */
int rgp_lstm_persistent_workgroups(const rgp_lstm_t* plan);
/* The same for the persistent BPTT launch of rgp_lstm_backward; 0 = the per-timestep loop */
int rgp_lstm_bptt_persistent_workgroups(const rgp_lstm_t* plan);
/* fp32 copies of "h", "c" (and, training plans, the gates "i", "f", "g", "o") as [B,T,7,7,128], and of "emb", the
 * projected features [B*T*49, 512], after a forward; training plans, after a backward: "d_i", "d_f", "d_g", "d_o", the
 * gradients of the gates' pre-activations [B,T,7,7,128] as the BPTT (either path) left them in the operand dtype.
 * buffer_elems: the element count, 0 = no such buffer. */
int rgp_lstm_read_buffer(rgp_lstm_t* plan, const char* name, float* dst, rgp_stream_t stream);
size_t rgp_lstm_buffer_elems(const rgp_lstm_t* plan, const char* name);
/* ------------------------------------------------------------------ gaze_grcn77 (the 7x7-map ConvGRU model) */
typedef struct rgp_grcn77 rgp_grcn77_t;

/* GazePredictionGRCN.create_gazeprediction_network of models/gaze_grcn77.py:77-218: gaze_grcn's projection 1024 -> 512 and
 * GRU_RCN_Cell (128 state channels, 3x3 SAME on 7x7, zero initial state), no batch-norm and no up-sampling: the logit of a
 * pixel is h_t[b,y,x,:] . out_W + out_b (:206-208), the maps are [B,T,7,7] and the softmax / the loss run over 49 pixels.
 * Both dropout sites (:160-161, :209) are inert.  All fp32 device pointers: proj_c3d_W [1024,512] proj_c3d_b [512];
 * gru_W{z,r,} [3,3,512,128] gru_U{z,r,} [3,3,128,128]; out_W [128,1] (16-byte aligned) out_b [1].  The plan reads the
 * biases and out_W / out_b in place on every call: they stay the caller's and must outlive the plan's use of them.
 * The read-out (csrc/head_point.hip.h) is fp32 arithmetic on the fp32 state in both plan dtypes: one launch forward
 * (logits and softmax), one launch plus a fixed-order sum backward.  No float atomics in it: two calls on the same
 * states give the same bits, and a frame's logits depend on that frame's states only. */
typedef struct rgp_grcn77_weights {
  const float *proj_c3d_W, *proj_c3d_b;
  const float *gru_Wz, *gru_Uz, *gru_Wr, *gru_Ur, *gru_W, *gru_U;
  const float *out_W, *out_b;
} rgp_grcn77_weights;

/* flags: the meaning of the RGP_GRCN_* flags of the same value */
#define RGP_GRCN77_SAVE_FOR_BACKWARD 1
#define RGP_GRCN77_PER_STEP 2
int rgp_grcn77_create(rgp_grcn77_t** plan, int batch, int n_steps, int dtype, int flags);
int rgp_grcn77_destroy(rgp_grcn77_t* plan);
size_t rgp_grcn77_workspace_bytes(const rgp_grcn77_t* plan);
int rgp_grcn77_bind_workspace(rgp_grcn77_t* plan, void* workspace, size_t bytes, rgp_stream_t stream);
int rgp_grcn77_set_weights(rgp_grcn77_t* plan, const rgp_grcn77_weights* w, rgp_stream_t stream);
/* c3d_input [B,T,1024,7,7] fp32 -> logits [B,T,7,7]; probs (optional) = per-frame softmax over the 49 pixels */
int rgp_grcn77_forward(rgp_grcn77_t* plan, const float* c3d_input, float* logits, float* probs, rgp_stream_t stream);
/* c3d_rows: [B*T*49, 1024] in the plan's operand dtype, column d*512+c, 16-byte aligned (what rgp_c3d_forward writes) */
int rgp_grcn77_forward_rows(rgp_grcn77_t* plan, const void* c3d_rows, float* logits, float* probs, rgp_stream_t stream);
/* Streaming inference, as rgp_grcn_forward_stream without bn_phase (this graph has no per-timestep batch-norm): the
 * state [B][49][128] goes through the plan's rgp_grcn sub-plan.  After the call rgp_grcn77_backward returns RGP_ESTATE
 * until a plain forward has run. */
size_t rgp_grcn77_state_elems(const rgp_grcn77_t* plan);
int rgp_grcn77_forward_stream(rgp_grcn77_t* plan, const float* c3d_input, const void* c3d_rows, const float* state_in, float* state_out,
                              int n_valid, float* logits, float* probs, rgp_stream_t stream);
/* Training plans, after a forward: gradients of the loss of gaze_rnn.py:363-408 over 49 pixels (loss_type 0 xentropy: probs
 * and labels are read; 1 l2: logits and labels; labels [B,T,7,7]) w.r.t. the ten variables (grads: arrays shaped like
 * the weights, fully overwritten).  The recurrence is differentiated by rgp_grcn_backward_from_states of the plan's
 * ConvGRU: persistent or per-step as the forward. */
int rgp_grcn77_backward(rgp_grcn77_t* plan, const float* logits, const float* probs, const float* labels,
                        const rgp_grcn77_weights* grads, int loss_type, rgp_stream_t stream);
/* After rgp_grcn77_backward: d loss / d input as conv5b rows [B*T*49, 1024] fp32 (column d*512+c) */
int rgp_grcn77_backward_input(rgp_grcn77_t* plan, float* d_rows, rgp_stream_t stream);
/* The persistent ConvGRU launches fail as rgp_grcn's do (rgp_grcn_status): the next call on the plan and rgp_grcn77_status
 * (which first waits for `stream`) return RGP_ETIMEOUT once; the poisoned states give NaN logits. */
int rgp_grcn77_status(rgp_grcn77_t* plan, rgp_stream_t stream);
/* Workgroups (= CUs) a persistent launch of this plan occupies on the current device; 0 = per-timestep launches */
int rgp_grcn77_persistent_workgroups(const rgp_grcn77_t* plan);
/* fp32 copies of "c3d_embedded" [B,T,7,7,512] and "rcn_outputs" [B,T,7,7,128] (h_t) after a forward and, training plans
 * after a backward, "d_rcn_outputs" [B,T,7,7,128], the read-out's gradient w.r.t. the states.  buffer_elems: the element
 * count, 0 = no such buffer. */
int rgp_grcn77_read_buffer(rgp_grcn77_t* plan, const char* name, float* dst, rgp_stream_t stream);
size_t rgp_grcn77_buffer_elems(const rgp_grcn77_t* plan, const char* name);
/* The read-out as a stage (for tests / profiling).  states = NULL: the plan's own states of the last forward; otherwise
 * the caller's fp32 [B,T,7,7,128], 16-byte aligned. */
int rgp_grcn77_head_fwd(rgp_grcn77_t* plan, const float* states, float* logits, float* probs, rgp_stream_t stream);
/* ------------------------------------------------------------------ frame-wise ShallowNet */
typedef struct rgp_shallownet rgp_shallownet_t;

/* SaliencyModel.create_shallownet variables (models/saliency_shallownet.py:90-185), fp32 device
 * pointers: conv1_w [5,5,3,32] conv2_w [3,3,32,64] conv3_w [3,3,64,32] (HWIO) + biases;
 * fc1_w [n_flat, 4802] (n_flat = 3872 at 98x98, 4608 at 112x112), fc2_w [2401, 4802] + biases. */
typedef struct rgp_shallownet_weights {
  const float *conv1_w, *conv1_b, *conv2_w, *conv2_b, *conv3_w, *conv3_b;
  const float *fc1_w, *fc1_b, *fc2_w, *fc2_b;
} rgp_shallownet_weights;

int rgp_shallownet_create(rgp_shallownet_t** plan, int max_frames, int image_hw, int dtype);
int rgp_shallownet_destroy(rgp_shallownet_t* plan);
size_t rgp_shallownet_workspace_bytes(const rgp_shallownet_t* plan);
int rgp_shallownet_bind_workspace(rgp_shallownet_t* plan, void* workspace, size_t bytes, rgp_stream_t stream);
int rgp_shallownet_set_weights(rgp_shallownet_t* plan, const rgp_shallownet_weights* w, rgp_stream_t stream);
/* frames [n,H,W,3] fp32 in [0,1] -> saliency [n,49,49] (saliency_shallownet.py:213); saliency7
 * (optional) [n,7,7] = its 7x7 average pool (gaze_rnn.py:262-269). */
int rgp_shallownet_forward(rgp_shallownet_t* plan, const float* frames, int n_frames, float* saliency,
                           float* saliency7, rgp_stream_t stream);

/* Training (FramewiseShallowNet trains every variable, gaze_framewise_shallownet.py:43-57): with a plan created
 * by rgp_shallownet_create_ex(save_for_backward = 1), rgp_shallownet_backward takes d loss / d saliency
 * [n_frames,49,49] fp32 for the frames of the last forward and overwrites grads (arrays shaped like the weights). */
int rgp_shallownet_create_ex(rgp_shallownet_t** plan, int max_frames, int image_hw, int dtype, int save_for_backward);
int rgp_shallownet_backward(rgp_shallownet_t* plan, int n_frames, const float* d_saliency, const rgp_shallownet_weights* grads,
                            rgp_stream_t stream);
/* Training-time dropout on fc1's ReLU output, before the maxout (saliency_shallownet.py:152-158; SaliencyModel feeds
 * keep 0.4 when training, :330).  mask: device bytes [n_frames, 4802] in the layer's own unit order (unit j and j + 2401
 * are maxout partners), the caller's; keep_prob in (0, 1]; keep_prob = 1 or NULL = off, and the plan then launches
 * exactly what it launches without the site.  The backward gates with the same draw and 1 / keep_prob. */
int rgp_shallownet_set_dropout(rgp_shallownet_t* plan, float keep_prob, const unsigned char* mask);
/* fp32 copies of the plan's intermediates for the n frames of the last forward, un-padded, in the reference's layouts
 * (c1 = H - 4, p1 = c1 / 2, c2 = p1 - 2, p2 = ceil(c2 / 2), c3 = p2 - 2, p3 = ceil(c3 / 2), n_flat = p3 p3 32):
 *   after a forward     "frames4" [n,H,H,3] (the frames in the operand dtype), "pool1" [n,p1,p1,32], "act2" [n,c2,c2,64],
 *                       "pool2" [n,p2,p2,64], "act3" [n,c3,c3,32], "pool3" [n,n_flat], "mo1" [n,2401] (fc1 after its maxout);
 *   training plans      "amax1" [n,p1,p1,32] (member 2 dy + dx of conv1's 2x2 window that held the first maximum),
 *                       "amax2" [n,p2,p2,64], "amax3" [n,p3,p3,32] (place 3 a + b of the first maximum in the 3x3 window,
 *                       counted from the window's corner, padding cells included), "mask1", "mask2" [n,2401] (maxout: 1 =
 *                       unit j, 2 = unit j + 2401, 0 = both ReLU-gated): the codes as floats;
 *   after a backward    "dz2", "dz1" [n,4802] (gradients of the FC pre-activations, natural unit order), "dmo1" [n,2401],
 *                       "dpool3" [n,n_flat], "dy3" [n,c3,c3,32], "dpool2" [n,p2,p2,64], "dy2" [n,c2,c2,64], "dpool1"
 *                       [n,p1,p1,32], "dy1" [n,c1,c1,32] (dy: gradients of the conv pre-activations).
 * RGP_EINVAL for an unknown name; RGP_ESTATE before the first forward, for a training-plan buffer of an inference plan and
 * for a gradient buffer when no backward has run since the last forward.  buffer_elems: the element count for the frames
 * of the last forward (max_frames before the first), 0 = this plan has no such buffer. */
int rgp_shallownet_read_buffer(rgp_shallownet_t* plan, const char* name, float* dst, rgp_stream_t stream);
size_t rgp_shallownet_buffer_elems(const rgp_shallownet_t* plan, const char* name);

/* ------------------------------------------------------------------ two-level cascade (config 5) */
typedef struct rgp_cascade rgp_cascade_t;

/* Variables of GazePredictionGRCN in models/gaze_grcn_cascade.py (fp32 device pointers):
 * proj_c3d_W [1,1,1024,512] + b (:269-275); bottom cell filters GRU_Conv_* (3x3, 512 -> 256, :290-303);
 * Upsampling/weight [11,11,64,256] (:317-321); top cell filters (5x5, x: [5,5,65,3], h: [5,5,3,3],
 * :346-357, input = concat(upsampled [64], ShallowNet saliency [1]));
 * fc1_w [7203,4802] fc2_w [2401,4802] + biases (:383-423); the ShallowNet's own variables. */
typedef struct rgp_cascade_weights {
  const float *proj_c3d_W, *proj_c3d_b;
  const float *bottom_Wz, *bottom_Uz, *bottom_Wr, *bottom_Ur, *bottom_W, *bottom_U;
  const float* upsampling_weight;
  const float *top_Wz, *top_Uz, *top_Wr, *top_Ur, *top_W, *top_U;
  const float *fc1_w, *fc1_b, *fc2_w, *fc2_b;
  rgp_shallownet_weights shallownet;
} rgp_cascade_weights;

int rgp_cascade_create(rgp_cascade_t** plan, int batch, int n_steps, int image_hw, int dtype);
int rgp_cascade_destroy(rgp_cascade_t* plan);
size_t rgp_cascade_workspace_bytes(const rgp_cascade_t* plan);
int rgp_cascade_bind_workspace(rgp_cascade_t* plan, void* workspace, size_t bytes, rgp_stream_t stream);
int rgp_cascade_set_weights(rgp_cascade_t* plan, const rgp_cascade_weights* w, rgp_stream_t stream);
/* frame_images [B*T,H,W,3] fp32 in [0,1], c3d_input [B,T,1024,7,7] -> gazemaps [B,T,49,49]
 * (predicted_gazemaps of gaze_grcn_cascade.py:423, trained with loss_type l2). */
int rgp_cascade_forward(rgp_cascade_t* plan, const float* frame_images, const float* c3d_input, float* gazemaps,
                        rgp_stream_t stream);
/* Streaming inference, as rgp_grcn_forward_stream without bn_phase (the bottom level's batch-norm is the identity for
 * every step) and without a rows entry: BOTH recurrent states are carried across calls.
 *   state      one flat fp32 buffer (16-byte aligned): the bottom state [B][49][256], which is what rgp_grcn_state_elems of
 *              the sub-plan describes, then the top state [B][49][49][3], the dense layout of "gaze_rcn_outputs"
 *   state_in   NULL = zeros for both; never written
 *   state_out  may be NULL; must not alias state_in; receives both states behind step n_valid
 *   n_valid    1..T.  All T steps are computed; the outputs of later steps are unspecified; their inputs, frame images
 *              included, are read, but influence neither the first n_valid maps nor state_out
 * rgp_cascade_forward_stream(.., NULL, state_out, T, ..) computes exactly what rgp_cascade_forward computes.  Argument
 * errors are RGP_EINVAL and are reported ahead of the plan's bound / weights state.  Inference and training plans both
 * accept the call; behind it rgp_cascade_backward returns RGP_ESTATE (no truncated BPTT) until a plain forward has run.
 * Every recurrence launch of this plan is a per-step launch: there is no time-out path.  Streaming inside a stream
 * capture is not supported: RGP_EINVAL if `stream` is capturing.  This one refusal asks the runtime about the stream, so it
 * comes BEHIND the bound / weights checks (an unbound plan on a capturing stream reports RGP_EWORKSPACE).
 * rgp_cascade_state_elems: B*(49*256 + 2401*3), the fp32 elements of a state; host-only, works on an unbound plan. */
size_t rgp_cascade_state_elems(const rgp_cascade_t* plan);
int rgp_cascade_forward_stream(rgp_cascade_t* plan, const float* frame_images, const float* c3d_input, const float* state_in,
                               float* state_out, int n_valid, float* gazemaps, rgp_stream_t stream);
/* Training (BASELINE config 5).  rgp_cascade_create_ex(save_for_backward = 1) keeps the gates, states and
 * maxout masks of the forward.  rgp_cascade_backward differentiates the l2 loss of gaze_grcn_cascade.py:428-441
 * (sum_t 0.5 ||maps - gt||^2 / (B*T)) w.r.t. every non-ShallowNet variable (the ShallowNet has learning rate
 * 0, base.py:264-265): grads is shaped like the weights, every listed array is fully overwritten, the
 * shallownet sub-struct is ignored.  d_rows (optional, [B*T*49, 1024] fp32) receives the gradient w.r.t. the
 * C3D conv5b rows for rgp_c3d_backward (end-to-end fine-tune). */
int rgp_cascade_create_ex(rgp_cascade_t** plan, int batch, int n_steps, int image_hw, int dtype, int save_for_backward);
int rgp_cascade_backward(rgp_cascade_t* plan, const float* gazemaps, const float* gt_gazemap, const rgp_cascade_weights* grads,
                         float* d_rows, rgp_stream_t stream);
/* Training-time dropout on fc1's ReLU output, before the maxout (gaze_grcn_cascade.py:401-402).  mask: device bytes
 * [B*T, 4802] in the layer's own unit order (unit j and j + 2401 are maxout partners); keep_prob = 1 or NULL = off. */
int rgp_cascade_set_dropout(rgp_cascade_t* plan, float keep_prob, const unsigned char* mask);
/* Intermediates of the last forward as dense fp32 (net[...] keys of gaze_grcn_cascade.py):
 * "frm_sal" [B*T,49,49], "rcn_outputs" [B,T,7,7,256], "rcn_upsampled_outputs" [B*T,49,49,64],
 * "gaze_rcn_outputs" [B*T,49,49,3] (top-cell states). */
int rgp_cascade_read_buffer(rgp_cascade_t* plan, const char* name, float* dst, rgp_stream_t stream);

/* ------------------------------------------------------------------ C3D conv stack */
typedef struct rgp_c3d rgp_c3d_t;

/* conv1a..conv5b (prototxt:22-342): w[i] DHWIO [3,3,3,Cin,Cout] fp32, b[i] [Cout]. */
typedef struct rgp_c3d_weights {
  const float* w[8];
  const float* b[8];
} rgp_c3d_weights;

/* Plan for up to max_windows 16x112x112x3 windows per call. */
int rgp_c3d_create(rgp_c3d_t** plan, int max_windows, int dtype);
int rgp_c3d_destroy(rgp_c3d_t* plan);
size_t rgp_c3d_workspace_bytes(const rgp_c3d_t* plan);
int rgp_c3d_bind_workspace(rgp_c3d_t* plan, void* workspace, size_t bytes, rgp_stream_t stream);
int rgp_c3d_set_weights(rgp_c3d_t* plan, const rgp_c3d_weights* w, rgp_stream_t stream);
/* video [n,16,112,112,3] fp32 (mean-subtracted, channels last) -> conv5b after ReLU.
 * features (optional): [n,1024,7,7] fp32, channel = c*2+d (gaze_rnn.py:494-497).
 * rows (optional): [n*49][1024] in the plan's operand dtype, K order d*512+c, the
 * form rgp_grcn_forward_rows consumes. */
int rgp_c3d_forward(rgp_c3d_t* plan, const float* video, int n_windows, float* features, void* rows,
                    rgp_stream_t stream);
/* The VIDEO_DATA layer (feature_extration.prototxt:3-21) + rgp_c3d_forward in one call: frames is a
 * device stack [n_frames, frame_h, frame_w, 3] of 8-bit pixels in the channel order the weights were
 * trained with (OpenCV BGR for the Sports-1M model); window w is the 16 consecutive frames from
 * window_starts[w] (HOST int32 array; extract_C3D_features.py:866 uses 0, 16, 32, ...).  Each frame is
 * resized to 128x171 (bilinear), centre-cropped to 112x112 and mean_cube [3,16,128,171] (device fp32,
 * the parsed sport1m_train16_128_mean.binaryproto; NULL = no subtraction) is subtracted. */
int rgp_c3d_forward_frames(rgp_c3d_t* plan, const unsigned char* frames, int n_frames, int frame_h, int frame_w,
                           const int* window_starts, int n_windows, const float* mean_cube, float* features, void* rows,
                           rgp_stream_t stream);
/* Only the VIDEO_DATA step: writes video [n_windows,16,112,112,3] fp32 (what rgp_c3d_forward takes). */
int rgp_c3d_frames_to_video(rgp_c3d_t* plan, const unsigned char* frames, int n_frames, int frame_h, int frame_w,
                            const int* window_starts, int n_windows, const float* mean_cube, float* video,
                            rgp_stream_t stream);
/* Copies layer i's (0..7) pooled, post-ReLU output, un-padded fp32 NDHWC, into dst. */
int rgp_c3d_read_layer(rgp_c3d_t* plan, int layer, int n_windows, float* dst, rgp_stream_t stream);
size_t rgp_c3d_layer_elems(const rgp_c3d_t* plan, int layer, int n_windows);

/* ---- end-to-end fine-tune of the conv stack (BASELINE config 5; tf.gradients, base.py:278-281) ----
 * rgp_c3d_create_ex(save_for_backward = 1) makes the forward record the pooling arg-max and reserves the
 * gradient images.  After ONE forward of n_windows <= max_windows windows, rgp_c3d_backward takes the
 * gradient w.r.t. the conv5b feature -- d_features [n,1024,7,7] fp32 (layout of `features`) or d_rows
 * [n*49,1024] fp32 (layout of `rows`), exactly one non-NULL -- and ACCUMULATES (+=) the parameter
 * gradients into grads, a flat fp32 vector laid out w[0] (DHWIO), b[0], w[1], b[1], ... (the caller zeroes
 * it; rgp_c3d_param_offset gives each piece's element offset, rgp_c3d_param_elems the total). */
int rgp_c3d_create_ex(rgp_c3d_t** plan, int max_windows, int dtype, int flags);
/* flags of rgp_c3d_create_ex (0 / 1 keep the meaning of the former `save_for_backward` argument):
 *  RGP_C3D_SAVE_FOR_BACKWARD  training plan (arg-max codes, gradient images).
 *  RGP_C3D_KERNELS_IGEMM      bf16 plans: conv2a..conv4b (forward and input gradients) run through the general
 *                             implicit-GEMM kernels and their filter gradients through the general filter-gradient
 *                             kernel instead of the layer-specific patch kernels -- the library's second, independent
 *                             implementation of those layers (tile chosen by problem size: 256x256 / 512x128 /
 *                             staggered 256x128 / 128x128), kept for cross-checking the default path.
 *  RGP_C3D_KERNELS_TILE128    with RGP_C3D_KERNELS_IGEMM: every implicit GEMM of the plan on the 128x128 tile loop.
 *  RGP_C3D_CONV2A_ROWWISE     inference plans on the patch kernels: conv2a + pool2 through conv_patch_bf16_kernel of
 *                             conv_patch.hip.h instead of conv_patch_slab_bf16_kernel of conv_patch_slab.hip.h (both
 *                             skip the halo-plane tap groups); bit-identical results (a cross-check and A/B switch).
 *  RGP_C3D_CONV3_TWOPLANE     inference plans on the patch kernels: conv3a and conv3b + pool3 through the body of
 *                             conv_patch.hip.h whose block tile holds both output planes of a pooled plane (what every
 *                             plan ran before, and what training plans run) instead of its plane-pure form;
 *                             bit-identical results (a cross-check and A/B switch).  (Value 16 is not a flag.) */
#define RGP_C3D_SAVE_FOR_BACKWARD 1
#define RGP_C3D_KERNELS_IGEMM 2
#define RGP_C3D_KERNELS_TILE128 4
#define RGP_C3D_CONV2A_ROWWISE 8
#define RGP_C3D_CONV3_TWOPLANE 32
/* Name of the kernel instantiation the plan launches for layer i's forward at n_windows windows ("" if unknown):
 * what a profiler shows for the stage rgp_c3d_profile_read times as index i. */
const char* rgp_c3d_layer_kernel_name(const rgp_c3d_t* plan, int layer, int n_windows);
size_t rgp_c3d_param_elems(const rgp_c3d_t* plan);
size_t rgp_c3d_param_offset(const rgp_c3d_t* plan, int layer, int is_bias);
int rgp_c3d_backward(rgp_c3d_t* plan, const float* d_features, const float* d_rows, int n_windows, float* grads,
                     rgp_stream_t stream);
/* Data-parallel fine-tune (gradient buckets launched as their wgrads complete, late layers first).
 * rgp_c3d_backward records an event on its stream once layer i's slice of `grads` (w[i] then b[i], see
 * rgp_c3d_param_offset) is final; rgp_c3d_wait_layer_grads makes `waiting_stream` wait for that event, so the
 * host can issue the RCCL all-reduce of the slice there while the backward of layers i-1..0 is still running. */
int rgp_c3d_wait_layer_grads(rgp_c3d_t* plan, int layer, rgp_stream_t waiting_stream);
/* After rgp_c3d_backward: the gradient w.r.t. layer i's conv output before ReLU/pooling (what dgrad and
 * wgrad of that layer consumed) as dense fp32 [n, D, H, W, Cout].  Valid until the next forward/backward of
 * the plan.  (bf16 layer 0: the backward pass works from the pooled gradient and never builds this image; the
 * call expands it on demand from the pooled gradient and arg-max codes the pass left behind.) */
int rgp_c3d_read_grad_image(rgp_c3d_t* plan, int layer, int n_windows, float* dst, rgp_stream_t stream);

/* Per-layer timing, as rgp_grcn_profile_*: index 0..7 = conv1a..conv5b (one fused
 * conv+bias+ReLU+pool kernel launch each), 8 = video_prep. */
#define RGP_C3D_STAGES 9
int rgp_c3d_profile_enable(rgp_c3d_t* plan, int enable);
int rgp_c3d_profile_read(rgp_c3d_t* plan, double ms[RGP_C3D_STAGES], long long calls[RGP_C3D_STAGES]);

/* ------------------------------------------------------------------ saliency metrics
 * evaluation_metrics.py:15-297 scored on the device: ONE launch scores n_frames frames on every requested metric, one
 * workgroup per frame.  The semantics are those of this package's evaluation_metrics.py (itself pinned to the
 * reference's file by tests/golden/metrics_ref.npz) for maps of one common shape height x width, where its `resize`
 * is the identity: pred is min-max normalised first (saliency_score_single, :239-272) and
 *   sim (:207-218)  cc (:221-236)  AUC_Judd (:42-98)  AUC_Borji (:101-164)  AUC_shuffled (:167-204)  NSS (not in the
 *   reference: mean z-scored saliency at the fixations)
 * are computed in fp64 with IEEE division and no contraction, comparisons included, so every `>=` of the ROC sweeps
 * falls as it does on the host and only the order of summation differs.  pred is fp32 unless RGP_METRICS_PRED_F64 is
 * set; an fp32 pred is normalised in fp32 and then widened, which is what numpy does with an fp32 array, an fp64 pred
 * in fp64.  NaN follows numpy too (np.min / np.max propagate it, sort and searchsorted place it last).
 * Where the host raises instead of returning (a prediction without contrast or an empty negative set in AUC_Borji /
 * AUC_shuffled) the score is NaN.
 *
 * scores [RGP_METRICS_COUNT, n_frames] fp64, row RGP_METRIC_ROW_* per metric; rows of metrics that were not
 * requested are left untouched.  A frame without fixations scores NaN on NSS and the three AUCs.  The mean over
 * frames is the caller's.
 *
 * Random draws, two forms:
 *  - the caller's (default): judd_jitter [n_frames, height*width] fp64 uniform draws (NULL: AUC_Judd without jitter);
 *    borji_neg / shuf_neg [n_frames, n_rep, neg_stride] int32 PIXEL INDICES of each repetition's negatives, of which
 *    AUC_Borji reads the first n_fix of a row and AUC_shuffled the first shuf_cnt[frame] (= min(n_fix, size of the
 *    frame's negative set), what `permutation(M)[:n_fix]` yields); `other` is not read;
 *  - RGP_METRICS_DEVICE_DRAWS: the four pointers are NULL and the draws come from Philox-4x32-10 keyed by `seed`, the
 *    counter made of (offset + frame, metric, repetition, sample): scores do not depend on the launch geometry, and
 *    frames [a, b) of a call with offset o are frames [0, b-a) of a call with offset o+a.  AUC_Borji negatives are
 *    uniform over the map, AUC_shuffled negatives min(n_fix, M) DISTINCT members of the frame's negative set `other`
 *    (Floyd's subset sampling), AUC_Judd is jittered unless RGP_METRICS_NO_JITTER.  The drawn indices are left in the
 *    workspace in the caller's-draws layout (see below), where a test can read them.
 *
 * fix / other: a pixel belongs to the set iff its value > 0.5.  other_stride is the distance in elements between two
 * frames' negative maps: 0 (one map for all frames, saliency_score :275-295) or height*width (one per frame,
 * evaluate_gaze.py:116-135).
 *
 * Limits: height*width <= RGP_METRICS_MAX_PIX, at most neg_stride <= RGP_METRICS_MAX_FIX fixations per frame,
 * 1/step_size <= RGP_METRICS_MAX_THRESHOLDS.  The host refuses what it can see (RGP_EINVAL before any launch).  The
 * number of fixations is only known on the device: a frame with more than neg_stride of them, or one whose supplied
 * indices / counts are out of range, gets NaN in all its requested scores and is counted in the workspace's status
 * word, which rgp_metrics_status reports.
 *
 * workspace (device, 8-byte aligned, rgp_metrics_workspace_bytes): bytes [0, 64) status; with
 * RGP_METRICS_DEVICE_DRAWS then borji_neg, shuf_neg (int32 [n_frames, n_rep, neg_stride] each) and shuf_cnt
 * (int32 [n_frames]).  rgp_saliency_scores clears the status word on the stream before its launch. */
#define RGP_METRICS_MAX_PIX 4096
#define RGP_METRICS_MAX_FIX 256
#define RGP_METRICS_MAX_THRESHOLDS 1024
#define RGP_METRICS_COUNT 6
#define RGP_METRIC_SIM 1
#define RGP_METRIC_CC 2
#define RGP_METRIC_AUC_JUDD 4
#define RGP_METRIC_AUC_BORJI 8
#define RGP_METRIC_AUC_SHUFFLED 16
#define RGP_METRIC_NSS 32
#define RGP_METRIC_ALL 63
/* row of `scores` = bit position of the metric */
#define RGP_METRIC_ROW_SIM 0
#define RGP_METRIC_ROW_CC 1
#define RGP_METRIC_ROW_AUC_JUDD 2
#define RGP_METRIC_ROW_AUC_BORJI 3
#define RGP_METRIC_ROW_AUC_SHUFFLED 4
#define RGP_METRIC_ROW_NSS 5
#define RGP_METRICS_DEVICE_DRAWS 1
#define RGP_METRICS_NO_JITTER 2
#define RGP_METRICS_PRED_F64 4
#define RGP_METRICS_GT_F64 8

typedef struct rgp_metrics_args {
  const void* pred;            /* [n_frames, height, width] fp32 (fp64 with RGP_METRICS_PRED_F64) */
  const void* gt;              /* same shape, fp32 (fp64 with RGP_METRICS_GT_F64); read by sim and cc only */
  const float* fix;            /* same shape */
  const float* other;          /* negative set of AUC_shuffled; read with RGP_METRICS_DEVICE_DRAWS only */
  long long other_stride;      /* 0 or height*width */
  int n_frames, height, width;
  unsigned metrics;            /* RGP_METRIC_* bits */
  unsigned flags;              /* RGP_METRICS_* bits */
  int n_rep;                   /* repetitions of AUC_Borji / AUC_shuffled (the reference: 100) */
  int neg_stride;              /* ints per (frame, repetition) row of the negatives = fixation cap of this call */
  double step_size;            /* threshold step of AUC_Borji / AUC_shuffled (the reference: 0.1) */
  const double* judd_jitter;
  const int *borji_neg, *shuf_neg, *shuf_cnt;
  unsigned long long seed, offset;
  void* workspace;
  size_t workspace_bytes;
  double* scores;              /* [RGP_METRICS_COUNT, n_frames] */
} rgp_metrics_args;

size_t rgp_metrics_workspace_bytes(int n_frames, int n_rep, int neg_stride, unsigned flags);
int rgp_saliency_scores(const rgp_metrics_args* args, rgp_stream_t stream);
/* Waits for `stream`, reads the status word of the last rgp_saliency_scores that used `workspace`: RGP_OK, or
 * RGP_EINVAL with the number of refused frames in rgp_last_error(). */
int rgp_metrics_status(const void* workspace, rgp_stream_t stream);

/* ------------------------------------------------------------------ saliency metrics at the fixation maps' shape
 * What evaluate_gaze.py runs (fixation_original_scale=True): saliency_score_single (:239-272) min-max normalises the
 * prediction at its own shape height x width, upsizes prediction and ground truth to the fixation map's shape
 * target_height x target_width with an order-3 spline resize, and scores there.  ONE launch, one workgroup per frame; the
 * upsized maps are never stored: the kernel keeps each frame's B-spline coefficients in LDS and evaluates the spline
 * inside every sweep of the metrics.
 *
 * The resize is scipy.ndimage.map_coordinates(order=3, mode='reflect') at the coordinates
 * (arange(o) + 0.5) * (float(i) / o) - 0.5 per axis (this package's evaluation_metrics.resize): the recursive prefilter
 * with pole sqrt(3) - 2 and exact 'reflect' initialisation along axis 0, then axis 1, then per target pixel the 16-term
 * sum of wy wx c over the taps floor(x) - 1 .. floor(x) + 2 with reflected indices, rows outer.  The pole's powers and
 * the per-axis weight / index tables are made on the host in float64; the device only multiplies and adds (no fused
 * multiply-add), so the resized values are a fixed sequence of IEEE operations (tests/spline_ref.py restates it) that
 * agrees with scipy to about 2e-15.  At equal shapes the host's resize is the identity and rgp_saliency_scores is the
 * entry point; this one applies the spline whatever the shapes.
 *
 * pred, gt [n_frames, height, width] fp32 / fp64 as for rgp_saliency_scores (an fp32 pred is normalised in fp32, then
 * widened).  Fixations are POINTS: frame n owns fix_idx[fix_ptr[n] .. fix_ptr[n + 1]), flat pixel indices
 * row * target_width + col on the target grid, strictly increasing within a frame (the order of np.nonzero(F.ravel()));
 * fix_len = the length of fix_idx.  The negative set of AUC_shuffled in the same form, other_ptr [n_frames + 1], or [2]
 * with RGP_METRICS_SCALED_OTHER_SHARED (one set for all frames, saliency_score :275-295); read for device draws, and
 * checked whenever given.  Draws: both forms of rgp_saliency_scores with the same layout and Philox counters, the
 * indices on the TARGET grid, judd_jitter [n_frames, target_height * target_width].
 *
 * Semantics per metric as rgp_saliency_scores, on the target_height * target_width resized values: AUC_Judd normalises
 * the jittered full-size map, AUC_Borji / AUC_shuffled the resized map (the spline overshoots [0, 1]) and evaluate it
 * only at the fixations and the drawn negatives.  Every sum has an order fixed by the shapes alone: frames [a, b) of a
 * call with offset o equal frames [0, b - a) of a call with offset o + a bit for bit.
 *
 * Limits: 2 <= height, width and height*width <= RGP_METRICS_MAX_PIX; target_height*target_width <=
 * RGP_METRICS_SCALED_MAX_PIX; neg_stride <= RGP_METRICS_MAX_FIX; 1/step_size <= RGP_METRICS_MAX_THRESHOLDS: refused
 * by the host with RGP_EINVAL before any launch.  Seen by the device only, and answered with NaN in every requested
 * score of that frame and a count in the status word (rgp_metrics_status, the first 64 workspace bytes): an index outside
 * [0, target_height*target_width), indices that do not increase, a fix_ptr / other_ptr pair that decreases or leaves
 * [0, fix_len] / [0, other_len], more fixations than neg_stride, more negatives than RGP_METRICS_SCALED_MAX_OTHER, a
 * draw index or shuf_cnt out of range.  Nothing out of range is used as an address.
 *
 * workspace (device, 8-byte aligned, rgp_metrics_scaled_workspace_bytes): bytes [0, 64) status; with
 * RGP_METRICS_DEVICE_DRAWS borji_neg, shuf_neg, shuf_cnt as rgp_saliency_scores leaves them; then the kernel's own
 * (the saliency at the negatives, the resize tables).
 *
 * rgp_spline_resize writes the resized maps themselves, [n_frames, H, W] fp64 (dst_f64) or fp32 (rounded once), from
 * src [n_frames, h, w] fp32 or fp64 (src_f64): the frame-size map for overlays and dumps; no normalisation.  Its
 * workspace (rgp_spline_resize_workspace_bytes) holds the tables. */
#define RGP_METRICS_SCALED_MAX_PIX   (1 << 22)     /* target pixels per frame: covers 1080 x 1920 */
#define RGP_METRICS_SCALED_MAX_OTHER 4096          /* members of a frame's AUC_shuffled negative set */
#define RGP_METRICS_SCALED_OTHER_SHARED 16         /* flag: other_ptr is [2], one negative set for all frames */

typedef struct rgp_metrics_scaled_args {
  const void* pred;            /* [n_frames, height, width] fp32 (fp64 with RGP_METRICS_PRED_F64) */
  const void* gt;              /* same shape, fp32 (fp64 with RGP_METRICS_GT_F64); read by sim and cc only */
  const int* fix_ptr;          /* [n_frames + 1] */
  const int* fix_idx;          /* [fix_len] */
  const int* other_ptr;        /* [n_frames + 1], or [2] with RGP_METRICS_SCALED_OTHER_SHARED; may be NULL with the caller's draws */
  const int* other_idx;        /* [other_len] */
  int fix_len, other_len;
  int n_frames, height, width, target_height, target_width;
  unsigned metrics;            /* RGP_METRIC_* bits */
  unsigned flags;              /* RGP_METRICS_* bits */
  int n_rep, neg_stride;
  double step_size;
  const double* judd_jitter;   /* [n_frames, target_height * target_width] */
  const int *borji_neg, *shuf_neg, *shuf_cnt;
  unsigned long long seed, offset;
  void* workspace;
  size_t workspace_bytes;
  double* scores;              /* [RGP_METRICS_COUNT, n_frames] */
} rgp_metrics_scaled_args;

size_t rgp_metrics_scaled_workspace_bytes(int n_frames, int n_rep, int neg_stride, int height, int width, unsigned flags);
int rgp_saliency_scores_scaled(const rgp_metrics_scaled_args* args, rgp_stream_t stream);
size_t rgp_spline_resize_workspace_bytes(int H, int W);
int rgp_spline_resize(const void* src, int src_f64, int n_frames, int h, int w, void* dst, int dst_f64, int H, int W,
                      void* workspace, size_t workspace_bytes, rgp_stream_t stream);

/* ------------------------------------------------------------------ ground-truth maps from fixation points
 * The arithmetic of the reference's loader (process_gazemap.py:35-58, crc_input_data_seq.py:41-53, 261-288) on the
 * device: ONE launch builds n_frames frames, one workgroup per frame.  Per frame n, whose samples are rows
 * frame_ptr[n] .. frame_ptr[n+1] of `samples` (int32 [n_samples][3] = observer u, raw coordinates a, b):
 *   a_ = (int)(rint((double)a * (out_s1 - 1.0) / (raw_d1 - 1.0)) + 1e-9), b_ likewise with out_s2 / raw_d2 (rint: half
 *   to even, np.round); the cell is row b_, column a_ of a frame [out_s2][out_s1] (the loader's swapaxes, :280).  An
 *   observer who hits a cell twice counts once, different observers add:
 *   fixationmaps = the count as fp32 (what rgp_metrics_args.fix takes);
 *   gazemaps     = count / n_observers in fp32, then scipy.ndimage.gaussian_filter on an fp32 frame (first along the
 *                  frame's first axis, then along its second; boundary `reflect`; every output
 *                  tmp = c w[r]; for i = -r .. -1: tmp += (line[l+i] + line[l-i]) w[i+r] in fp64, rounded to fp32, the
 *                  intermediate frame between the passes being fp32), then, unless the frame is all zero,
 *                  g -= min(g); g /= max(g) in fp32 (a constant non-zero frame: NaN, as numpy);
 *   labels       = gazemaps / their sum (normalize_probability_map, model_util.py:40-58): the sum accumulated in fp64 in
 *                  a fixed order and rounded once to fp32; an all-zero frame gives NaN as the host helper does.
 * weights: DEVICE double [2 radius + 1], made by the HOST (w = exp(-0.5 / sigma^2 x^2) / sum, x = -radius .. radius,
 * radius = (int)(4 sigma + 0.5)): the device's exp is not numpy's.  No fused multiply-add, no fast-math: with the same
 * weights the maps equal the host's bit for bit.
 *
 * Limits: out_s1*out_s2 <= RGP_GTMAPS_MAX_PIX, 1 <= n_observers <= RGP_GTMAPS_MAX_OBSERVERS, 0 <= radius <=
 * RGP_GTMAPS_MAX_RADIUS, raw_d1, raw_d2 >= 2; the host refuses what it can see (RGP_EINVAL before any device call).  A
 * sample with u outside [0, n_observers), a outside [0, raw_d1) or b outside [0, raw_d2), or a frame whose frame_ptr
 * pair is negative or decreasing, refuses its frame on the device: NaN in every requested output of that frame, the
 * frame counted in the workspace's status word (rgp_gtmaps_status); the other frames are unaffected.  n_frames == 0:
 * RGP_OK, nothing is launched.  The original-scale path of the loader (sigma = 19 on the raw frame) has an entry of its
 * own: rgp_gazemaps_full_from_fixations, below.
 *
 * workspace (device, 8-byte aligned, rgp_gtmaps_workspace_bytes): the status word, cleared on the stream before the
 * launch. */
#define RGP_GTMAPS_MAX_PIX 4096
#define RGP_GTMAPS_MAX_OBSERVERS 32
#define RGP_GTMAPS_MAX_RADIUS 32

typedef struct rgp_gtmaps_args {
  const int* frame_ptr;        /* [n_frames + 1] */
  const int* samples;          /* [n_samples][3] */
  const double* weights;       /* [2 radius + 1] */
  int n_frames, n_observers, raw_d1, raw_d2, out_s1, out_s2, radius;
  float *gazemaps, *fixationmaps, *labels;   /* [n_frames][out_s2][out_s1]; any may be NULL, not all three */
  void* workspace;
  size_t workspace_bytes;
} rgp_gtmaps_args;

size_t rgp_gtmaps_workspace_bytes(void);
int rgp_gazemaps_from_fixations(const rgp_gtmaps_args* args, rgp_stream_t stream);
/* Waits for `stream`, reads the status word of the last rgp_gazemaps_from_fixations that used `workspace`: RGP_OK, or
 * RGP_EINVAL with the number of refused frames in rgp_last_error(). */
int rgp_gtmaps_status(const void* workspace, rgp_stream_t stream);

/* ------------------------------------------------------------------ ground-truth maps at the frame's resolution
 * The loader's original-scale path (crc_input_data_seq.py:237-240 with :41-53 and :261-288): the maps above with
 * out_shape = raw_shape, i.e. frames [raw_d2][raw_d1] of up to RGP_GTMAPS_FULL_MAX_PIX cells (405 x 720, 1080 x 1920)
 * and sigma = 19 (radius 76).  Same arithmetic, same weights from the host, same bits as the host: the rescale is the
 * identity, fixationmaps = observers per cell, gazemaps = count / n_observers filtered along the frame's first axis,
 * then its second (scipy's correlate1d sums in fp64, each rounded once to fp32, the plane between the passes fp32,
 * `reflect` at any distance), then g -= min(g); g /= max(g) unless the frame is all zero.  There are no `labels`.
 * The planes live in the workspace; the filter is tiled over them in a fixed number of launches on `stream` (scatter,
 * pass 1, pass 2 with the frame's min and max, normalise), none of which waits for another workgroup.  A filter radius up
 * to RGP_GTMAPS_FULL_LDS_RADIUS stages its taps in LDS; above it they are read through the caches, same sums.
 *
 * Limits: raw_d1, raw_d2 >= 2, raw_d1*raw_d2 <= RGP_GTMAPS_FULL_MAX_PIX, 1 <= n_observers <= RGP_GTMAPS_MAX_OBSERVERS,
 * 0 <= radius <= RGP_GTMAPS_FULL_MAX_RADIUS; the host refuses what it can see (RGP_EINVAL before any device call).  A bad
 * sample or frame_ptr pair refuses its frame on the device as above: NaN in every requested output of that frame, the
 * frame counted in the status word (rgp_gtmaps_full_status), no out-of-range value used as an address, the other frames
 * unaffected.  n_frames == 0: RGP_OK, nothing is launched.
 *
 * workspace (device, 8-byte aligned, rgp_gtmaps_full_workspace_bytes(n_frames, raw_d1, raw_d2): the status word, three
 * words and a column bitmap per frame, then a uint32 observer-mask plane and an fp32 plane per frame -- 8 bytes per cell
 * and frame; 0 for arguments the entry refuses).  Frames are independent: a caller short of memory splits the call.
 * RGP_GTMAPS_FULL_TILE_COLS / _ROWS: every tile extent of either pass divides them (for tests that straddle tiles). */
#define RGP_GTMAPS_FULL_MAX_PIX (1 << 22)
#define RGP_GTMAPS_FULL_MAX_RADIUS 256
#define RGP_GTMAPS_FULL_LDS_RADIUS 76
#define RGP_GTMAPS_FULL_TILE_COLS 128
#define RGP_GTMAPS_FULL_TILE_ROWS 64

typedef struct rgp_gtmaps_full_args {
  const int* frame_ptr;        /* [n_frames + 1] */
  const int* samples;          /* [n_samples][3] */
  const double* weights;       /* [2 radius + 1] */
  int n_frames, n_observers, raw_d1, raw_d2, radius;
  float *gazemaps, *fixationmaps;            /* [n_frames][raw_d2][raw_d1]; either may be NULL, not both */
  void* workspace;
  size_t workspace_bytes;
} rgp_gtmaps_full_args;

size_t rgp_gtmaps_full_workspace_bytes(int n_frames, int raw_d1, int raw_d2);
int rgp_gazemaps_full_from_fixations(const rgp_gtmaps_full_args* args, rgp_stream_t stream);
/* Waits for `stream`, reads the status word of the last rgp_gazemaps_full_from_fixations that used `workspace`: RGP_OK,
 * or RGP_EINVAL with the number of refused frames in rgp_last_error() and, if refused is not NULL, in *refused. */
int rgp_gtmaps_full_status(const void* workspace, int* refused, rgp_stream_t stream);

/* ------------------------------------------------------------------ loader frame images: Pillow's antialiased resize
 * The loader's frame step (crc_input_data_seq.py:186-209) for the ShallowNet branch: selected uint8 RGB frames resized
 * with Image.resize((w, h), Image.ANTIALIAS) -- Pillow's two-pass 8-bit resample -- and scaled by float32(1 / 255).
 * ONE launch; a workgroup owns one output frame and one band of its output rows: it streams the band's input rows from
 * HBM, resamples each horizontally into an 8-bit image of the band in LDS, runs the vertical pass from LDS and stores
 * the fp32 and / or uint8 image.  The 8-bit intermediate never reaches HBM.  Integer arithmetic throughout: the same
 * bits as Pillow with the same tables, whatever the banding.
 *
 * Tables (DEVICE int32, made by the HOST, frames.resample_coeffs): per axis, in -> out, k [out][ksize] the 22-bit
 * fixed-point weights and b [out][2] = (xmin, n): output xx = clamp((2^21 + sum_{x < n} pixel[xmin + x] k[xx][x]) >> 22,
 * 0, 255), arithmetic shift, int32 accumulator (exact while 255 sum|k| + 2^21 < 2^31, which the host builder checks;
 * every |k| must be below 2^23: the products are 24-bit multiplies).  Horizontal first, on the input rows the band's
 * vertical entries touch, then vertical on the 8-bit intermediate.  A pass whose in == out is skipped: its bytes go
 * through unchanged and its tables are not read (they may be NULL, its ksize 0).  images = (float)u8 * 0.003921569f.
 *
 * frame_index (device, [n_out]; NULL = frames 0 .. n_out-1) selects the source frame of every output frame.  An entry
 * outside [0, n_frames) refuses that output frame on the device: NaN in `images`, 0 in `images_u8`, counted in the
 * status word (rgp_frames_status), never used as an address, the other frames unaffected.  The bounds tables are
 * checked the same way before they address anything (xmin >= 0, 0 <= n <= ksize, xmin + n <= in, and a band's input
 * rows within what its LDS image holds): a bad entry refuses every output frame.
 *
 * bands: the least number of bands the output rows are cut into (band i = rows [i out_h / B, (i + 1) out_h / B));
 * 0 = the library's choice (enough workgroups to fill the chip).  The library raises the count until a band's LDS
 * image fits RGP_FRAMES_LDS_BYTES; if not even one output row per band fits: RGP_EINVAL.
 *
 * Limits (the host refuses what it can see with RGP_EINVAL, naming the argument, before any device call): 3 channels;
 * 1 <= out_h, out_w <= RGP_FRAMES_MAX_OUT; ksize <= RGP_FRAMES_MAX_KSIZE; fw <= RGP_FRAMES_MAX_IN_W (four input rows
 * are staged at a time); n_frames * fh * fw * 3 and n_out * out_h * out_w * 3 below RGP_FRAMES_MAX_BYTES; both outputs
 * NULL; bands > out_h; a missing table.  n_out == 0: RGP_OK, nothing is launched.
 * workspace (device, 8-byte aligned, rgp_frames_workspace_bytes()): the status word, cleared on the stream before
 * the launch. */
#define RGP_FRAMES_MAX_OUT 256
#define RGP_FRAMES_MAX_KSIZE 128
#define RGP_FRAMES_MAX_IN_W 2040
#define RGP_FRAMES_MAX_BYTES (1ll << 40)
#define RGP_FRAMES_LDS_BYTES (156 * 1024)     /* the most a workgroup may take */
#define RGP_FRAMES_LDS_TARGET (80 * 1024)     /* the library's own choice of bands keeps two workgroups per CU */
#define RGP_FRAMES_STAGE_BYTES 24576          /* input rows staged per step (and the band's output image) */

typedef struct rgp_frames_args {
  const unsigned char* frames;      /* [n_frames][fh][fw][3] */
  int n_frames, fh, fw;
  const int* frame_index;           /* [n_out] or NULL */
  int n_out, out_h, out_w;
  const int *kh, *bh;               /* [out_w][ksize_h], [out_w][2]; unused when fw == out_w */
  int ksize_h;
  const int *kv, *bv;               /* [out_h][ksize_v], [out_h][2]; unused when fh == out_h */
  int ksize_v;
  int bands;
  float* images;                    /* [n_out][out_h][out_w][3]; either may be NULL, not both */
  unsigned char* images_u8;
  void* workspace;
  size_t workspace_bytes;
} rgp_frames_args;

size_t rgp_frames_workspace_bytes(void);
/* The band count the entry would use (>= bands), the LDS bytes of its workgroups and the input rows a band's LDS image
 * holds; 0 if no banding fits or an argument is out of range.  ksize of a skipped pass: 0.  Host arithmetic only. */
int rgp_frames_plan(int fh, int fw, int out_h, int out_w, int ksize_h, int ksize_v, int n_out, int bands, int* lds_bytes,
                    int* mid_rows);
int rgp_frame_images(const rgp_frames_args* args, rgp_stream_t stream);
/* Waits for `stream`, reads the status word of the last rgp_frame_images that used `workspace`: RGP_OK, or RGP_EINVAL
 * with the number of refused output frames in rgp_last_error() and, if refused is not NULL, in *refused. */
int rgp_frames_status(const void* workspace, int* refused, rgp_stream_t stream);

/* ------------------------------------------------------------------ gaze-map export: scipy's bytescale and imresize
 * extract_map.py:35-41 writes the 7 x 7 map of every step as avg_pool(a) = scipy.misc.imresize(a[i], (7, 7)) / its sum,
 * and scipy.misc.imsave (evaluate_gaze.py:148-152) encodes bytescale(a).  ONE launch for n fp32 maps [n][h][w], one wave
 * per map, any of three outputs.  Per map (scipy <= 1.2, a NumPy before NEP 50):
 *   bytes      cmin, cmax fp32; cscale = cmax - cmin in fp32, 1 if that is 0; scale = float32(255.0 / float64(cscale));
 *              b = (a - cmin) * scale, an fp32 subtract and an fp32 multiply; u = uint8(trunc(clip(b, 0, 255) + 0.5f)).
 *              Where 255 / cscale overflows fp32 (cscale below about 7.5e-37) scale is +inf and the cells equal to cmin
 *              are 0 * inf = NaN: they give byte 0, the x86 conversion's result; the other cells give 255.
 *   pooled_u8  Pillow's 8-bit resample of `bytes` as one channel, h x w -> out_h x out_w, with the tables of "loader
 *              frame images" above (frames.resample_coeffs; made by the HOST, int32 on the DEVICE): horizontal, then
 *              vertical on the 8-bit intermediate; a pass whose in == out is skipped and its tables are not read.
 *   pooled     float64(pooled_u8) / float64(sum of pooled_u8): an exact integer sum, one IEEE division per cell.  A zero
 *              sum (a constant map, a very peaked one) gives NaN in every cell, as NumPy's 0 / 0 does: not an error.
 * With pooled and pooled_u8 both NULL only `bytes` is made and out_h, out_w and the tables are not read.
 *
 * A map that holds a NaN or an Inf is refused on the device: NaN in `pooled`, 0 in `pooled_u8` and `bytes`, counted in
 * the status word (rgp_mapexport_status), the other maps unaffected.  The bounds tables are checked on the device before
 * they address anything (xmin >= 0, 0 <= n <= ksize, xmin + n <= in): a bad entry refuses every map.
 *
 * Limits (the host refuses what it can see with RGP_EINVAL, naming the argument, before any device call): 1 <= h, w <=
 * RGP_MAPEXPORT_MAX_SIDE; 1 <= out_h <= h and 1 <= out_w <= w (no upscale); ksize <= RGP_MAPEXPORT_MAX_KSIZE; all three
 * outputs NULL; a missing table for a pass that runs; the workspace.  n == 0: RGP_OK, nothing is launched.
 * workspace (device, 8-byte aligned, rgp_mapexport_workspace_bytes()): the status word, cleared on the stream before the
 * launch. */
#define RGP_MAPEXPORT_MAX_SIDE 64
#define RGP_MAPEXPORT_MAX_KSIZE 512
#define RGP_MAPEXPORT_LDS_BYTES (152 * 1024)  /* the most a workgroup may take (64 x 64 maps); 49 x 49 -> 7 x 7 takes 50 KB */

typedef struct rgp_mapexport_args {
  const float* maps;                /* [n][h][w] */
  int n, h, w, out_h, out_w;
  const int *kh, *bh;               /* [out_w][ksize_h], [out_w][2]; unused when w == out_w */
  int ksize_h;
  const int *kv, *bv;               /* [out_h][ksize_v], [out_h][2]; unused when h == out_h */
  int ksize_v;
  double* pooled;                   /* [n][out_h][out_w]; any may be NULL, not all three */
  unsigned char* pooled_u8;         /* [n][out_h][out_w] */
  unsigned char* bytes;             /* [n][h][w] */
  void* workspace;
  size_t workspace_bytes;
} rgp_mapexport_args;

size_t rgp_mapexport_workspace_bytes(void);
int rgp_mapexport(const rgp_mapexport_args* args, rgp_stream_t stream);
/* Waits for `stream`, reads the status word of the last rgp_mapexport that used `workspace`: RGP_OK, or RGP_EINVAL with
 * the number of refused maps in rgp_last_error() and, if refused is not NULL, in *refused. */
int rgp_mapexport_status(const void* workspace, int* refused, rgp_stream_t stream);

/* ------------------------------------------------------------------ frame overlays: spline resize, colormap, Pillow's blend
 * n fp32 maps [n][h][w] drawn over uint8 RGB frames [n_src][H][W][3] that are in device memory, two launches, the bytes the
 * host libraries give.  Per map i and its frame (frame_idx[i], or i when frame_idx is NULL):
 *   resize     v[Y][X] = the fp32 value rgp_spline_resize writes (fp64 prefilter and taps, rounded once); the map as it is
 *              where (h, w) == (H, W), as the host's resize is the identity there
 *   bytescale  scipy's, on v at [H][W]: cmin / cmax fp32 from the data (or limits[i][0], limits[i][1]: scipy's
 *              bytescale(data, cmin=, cmax=)); cscale = cmax - cmin, 1 if 0; scale = float32(255.0 / float64(cscale));
 *              b = (v - cmin) * scale, an fp32 subtract and an fp32 multiply; u = uint8(trunc(clip(b, 0, 255) + 0.5f)); a NaN b
 *              (0 * inf) gives 0.  These bytes are heat_u8.
 *   colour     c = lut[u], lut uint8 [256][3] (matplotlib: cmap(u8, bytes=True)[..., :3])
 *   blend      PIL.Image.blend(frame, colour, alpha) per byte: alpha == 0 the frame's byte, alpha == 1 the colour's, otherwise
 *              uint8(trunc(float(f) + alpha * float(c - f))), one fp32 multiply and one fp32 add, not fused.
 * RGP_OVERLAY_SHARED_LIMITS: one (cmin, cmax) for the call, the min and max over all resized maps that are not refused.
 * The resized floats are never stored: the first launch leaves per-band min / max in the workspace, the second evaluates
 * the spline again and renders.  Maps [a, b) of a call with limits equal maps [0, b - a) of a call on that slice.
 *
 * Refused on the device, counted in the status word (rgp_overlay_status), the other maps unaffected: a map that holds a
 * NaN or an Inf, limits that are not finite or with cmax < cmin, a frame_idx entry outside [0, n_src) (checked before it
 * addresses anything).  A refused map's frame goes to `out` unchanged (zeros for a bad frame index) and its heat_u8 is 0;
 * under RGP_OVERLAY_SHARED_LIMITS it does not count towards the limits.
 *
 * The host refuses with RGP_EINVAL, naming the argument, before any device call: NULL maps, lut, frames (when out is set);
 * maps, limits or frame_idx not 4-byte aligned; out and heat_u8 both NULL; h or w below 2, or h*w above
 * RGP_METRICS_MAX_PIX, when a resize is needed; H*W above RGP_METRICS_SCALED_MAX_PIX; alpha outside [0, 1] or NaN; n_src
 * below n without frame_idx; out overlapping frames; unknown flags, limits together with RGP_OVERLAY_SHARED_LIMITS.  A
 * missing, misaligned (8 bytes) or short workspace is RGP_EWORKSPACE.  n == 0: RGP_OK, nothing is launched.  frames, out and
 * heat_u8 need no alignment. */
#define RGP_OVERLAY_SHARED_LIMITS 1

typedef struct rgp_overlay_args {
  const unsigned char* frames;      /* [n_src][H][W][3] */
  const int* frame_idx;             /* [n], or NULL: map i on frame i; repeats and any order allowed */
  const float* maps;                /* [n][h][w] */
  const float* limits;              /* [n][2] (cmin, cmax), or NULL: from the data */
  const unsigned char* lut;         /* [256][3] */
  float alpha;
  unsigned flags;
  unsigned char* out;               /* [n][H][W][3], or NULL */
  unsigned char* heat_u8;           /* [n][H][W], or NULL; not both */
  int n, n_src, h, w, H, W;
} rgp_overlay_args;

size_t rgp_overlay_workspace_bytes(int n, int h, int w, int H, int W);
int rgp_overlay(const rgp_overlay_args* args, void* workspace, size_t workspace_bytes, rgp_stream_t stream);
/* Waits for `stream`, reads the status word of the last rgp_overlay that used `workspace`: RGP_OK, or RGP_EINVAL with the
 * number of refused maps in rgp_last_error() and, if refused is not NULL, in *refused. */
int rgp_overlay_status(const void* workspace, int* refused, rgp_stream_t stream);

/* ------------------------------------------------------------------ action classifier on gaze-attended C3D features */
typedef struct rgp_action rgp_action_t;

/* Classifier.projection + classification_graph_nn / _svm (models/action_classification.py:210-292).  Inputs per batch:
 * c3d [B, C, 49] fp32 (the placeholder layout; C = 1024 in the reference), gazemap [B, 49, 49] fp32 (ground truth or a
 * gaze model's probs), labels [B, 13] in {0, 1}.  With RGP_ACTION_USE_GAZEMAP (:224-238) a = gazemap.reshape(B, 2401) Wg
 * and x[b, c*49+p] = c3d[b, c, p] a[b, p]; without it x is the flattened c3d.  K = 49 C.
 *  RGP_ACTION_NN  (:265-292): h1 = x W1 + b1, h2 = h1 W2 + b2, logits = h2 W3 + b3 -- NO non-linearity between the layers
 *    (use_relu=False) -- y_pred = sigmoid(logits), loss = mean over B x 13 of max(z,0) - z y + log(1 + exp(-|z|)); Adam
 *    in the TF form of rgp_adam_clip_step (beta1 0.9, beta2 0.999, eps 1e-8, no clipping).  The caller passes the
 *    learning rate of the step: 0.002 * 0.96^(step/10), the exponent continuous (tf.train.exponential_decay default).
 *  RGP_ACTION_SVM (:242-263): y = x W1 + b1 (logits and y_pred are both y), loss = 0.5 sum W1^2 + 50 sum max(0, 1 - labels y),
 *    plain SGD (the reference's lr: 0.01).  The labels stay {0, 1} AS THE REFERENCE WRITES THEM: a zero label adds the
 *    constant 1 to the hinge sum and passes no gradient; the hinge passes gradient only where 1 - labels y > 0, strictly.
 * fp32 device pointers: W1 [K, 256] (SVM: [K, 13]; 16-byte aligned), Wg [2401, 49] (gaze-map plans), b1 [256] (SVM: [13]),
 * W2 [256, 256], b2 [256], W3 [256, 13], b3 [13] (NN).  The plan keeps these pointers: a training step updates the arrays
 * IN PLACE, and the operand copy of W1 (the plan's dtype) with them. */
typedef struct rgp_action_weights {
  float *W1, *Wg, *b1, *W2, *b2, *W3, *b3;
} rgp_action_weights;

#define RGP_ACTION_NN 0
#define RGP_ACTION_SVM 1
#define RGP_ACTION_USE_GAZEMAP 1
#define RGP_ACTION_SAVE_FOR_BACKWARD 2   /* a training plan */
#define RGP_ACTION_UNFUSED 4             /* the second implementation: x, dW1 and dx in memory, existing optimizer kernels */
/* dim_feat: C in [1, 8192]; batch in [1, 64]; anything else, or an unknown flag: RGP_EINVAL. */
int rgp_action_create(rgp_action_t** plan, int batch, int dim_feat, int mode, int dtype, int flags);
int rgp_action_destroy(rgp_action_t* plan);
size_t rgp_action_workspace_bytes(const rgp_action_t* plan);
int rgp_action_bind_workspace(rgp_action_t* plan, void* workspace, size_t bytes, rgp_stream_t stream);
int rgp_action_set_weights(rgp_action_t* plan, const rgp_action_weights* w, rgp_stream_t stream);
/* Copies the current values into the arrays of dst (a no-op for an array the plan already updates in place). */
int rgp_action_get_weights(rgp_action_t* plan, const rgp_action_weights* dst, rgp_stream_t stream);
/* NN training plans: Adam's m and v, arrays shaped like the weights, owned and initialised by the caller. */
int rgp_action_bind_slots(rgp_action_t* plan, const rgp_action_weights* m, const rgp_action_weights* v);
/* -> logits [B, 13], y_pred [B, 13] (either may be null).  No float atomics: two calls give the same bits. */
int rgp_action_forward(rgp_action_t* plan, const float* c3d, const float* gazemap, float* logits, float* y_pred, rgp_stream_t stream);
/* c3d_rows: conv5b rows [B*49, 1024] in the plan's operand dtype, column d*512+c (what rgp_c3d_forward writes); C = 1024 plans */
int rgp_action_forward_rows(rgp_action_t* plan, const void* c3d_rows, const float* gazemap, float* logits, float* y_pred,
                            rgp_stream_t stream);
/* After a forward: the loss of its batch against labels -> loss_dev[0]. */
int rgp_action_loss(rgp_action_t* plan, const float* labels, float* loss_dev, rgp_stream_t stream);
/* One training step (training plans): forward, loss (-> loss_dev, optional; the loss BEFORE the update), every gradient, the
 * update of W1 in one pass over W1, m and v (dW1 never exists in memory), and the small variables' optimizer step. */
int rgp_action_train_step(rgp_action_t* plan, const float* c3d, const float* gazemap, const float* labels, int step, float lr,
                          float* loss_dev, rgp_stream_t stream);
/* The stages of a step, for tests.  fc1_fwd: a and the per-slab partial sums of x W1; tail: their sum in slab order and
 * the rest of the network (training plans: with the gradients; labels then required); fc1_update: the pass over W1 with
 * the caller's d_h1 [B, 256] (SVM [B, 13]: d hinge sum / d y, the factor 50 is applied inside), recomputing a. */
int rgp_action_fc1_fwd(rgp_action_t* plan, const float* c3d, const float* gazemap, rgp_stream_t stream);
int rgp_action_tail(rgp_action_t* plan, const float* labels, rgp_stream_t stream);
int rgp_action_fc1_update(rgp_action_t* plan, const float* c3d, const float* gazemap, const float* d_h1, int step, float lr,
                          rgp_stream_t stream);
/* fp32 copies of "a" [B,49], "h1" [B,256] (SVM: y [B,13]), "h2", "loss" [1]; training plans: "d_h1", "d_h2", "d_logits",
 * "dx" [B,K] (SVM: including the factor 50), "d_a", and the small gradients "d_Wg", "d_b1", "d_W2", "d_b2", "d_W3", "d_b3".
 * buffer_elems: the element count, 0 = this plan has no such buffer. */
int rgp_action_read_buffer(rgp_action_t* plan, const char* name, float* dst, rgp_stream_t stream);
size_t rgp_action_buffer_elems(const rgp_action_t* plan, const char* name);

/* ------------------------------------------------------------------ ShallowNet pre-training on SALICON (SaliencyModel)
 * The step of models/saliency_shallownet.py:246-250, :291-332 around rgp_shallownet_forward / _backward.
 *
 * rgp_salicon_batch: the batch of :297-311 from an image set RESIDENT on the device, in ONE launch.  images_u8
 * [n][h][w][3] and maps_u8 [n][49][49] are the decoded set (salicon_input_data.py:95-111); output sample s is image
 * index[s]: images[s] = (float)u8 * 0.003921569f (the loader's np.multiply(x.astype(float32), 1.0 / 255.0), the constant of
 * rgp_frame_images), maps[s] the same.  flip (device, [batch], NULL = none): a non-zero byte mirrors image AND map of
 * that sample along the width axis (:310-311; pixels keep their RGB order).  An index entry outside [0, n) refuses that
 * sample on the device: NaN in both of its outputs, counted in the status word (rgp_salicon_status), never used as an
 * address, the other samples unaffected.  Element offsets are 64-bit.
 * Limits (RGP_EINVAL naming the argument, before any device call): h == w, 98 or 112; map_h == map_w == 49; batch >= 0;
 * n > 0; a NULL array other than flip; outputs 4-byte aligned.  batch == 0: RGP_OK, nothing is launched.
 * workspace (device, 8-byte aligned, rgp_salicon_workspace_bytes()): the status word, cleared on the stream before the
 * launch. */
typedef struct rgp_salicon_batch_args {
  const unsigned char* images_u8;   /* [n][h][w][3] */
  const unsigned char* maps_u8;     /* [n][map_h][map_w] */
  int n, h, w, map_h, map_w;
  const int* index;                 /* [batch], device */
  const unsigned char* flip;        /* [batch], device, or NULL */
  int batch;
  float* images;                    /* [batch][h][w][3] */
  float* maps;                      /* [batch][map_h][map_w] */
  void* workspace;
  size_t workspace_bytes;
} rgp_salicon_batch_args;

size_t rgp_salicon_workspace_bytes(void);
int rgp_salicon_batch(const rgp_salicon_batch_args* args, rgp_stream_t stream);
/* Waits for `stream`, reads the status word of the last rgp_salicon_batch that used `workspace`: RGP_OK, or RGP_EINVAL
 * with the number of refused samples in rgp_last_error() and, if refused is not NULL, in *refused. */
int rgp_salicon_status(const void* workspace, int* refused, rgp_stream_t stream);

/* The target loss of :248-249 and its gradient in one pass: loss[0] = scale / 2 * sum (maps - labels)^2 over n elements,
 * d_maps[i] = (maps[i] - labels[i]) * scale (one fp32 subtract, one fp32 multiply).  scale = 2 / (2401 * config.batch_size),
 * computed by the host in double: the reference divides by the CONFIGURED batch size whatever the number of frames fed.
 * workspace: RGP_SQNORM_PARTIALS floats (deterministic two-stage sum). */
int rgp_euclid_loss_fwd_bwd(const float* maps, const float* labels, long long n, float scale, float* workspace, float* loss,
                            float* d_maps, rgp_stream_t stream);

/* The regulariser of :247 over a flat parameter buffer and its gradient buffer (every variable, biases included):
 * reg_loss[0] = coeff * sum w^2 / 2 (deterministic two-stage sum), grads[i] += coeff * params[i].  Runs after the backward and
 * before the clip: the reference clips the gradient of the total loss.  grads == NULL: the value alone (a validation step).
 * workspace: RGP_SQNORM_PARTIALS floats. */
int rgp_l2_reg(const float* params, float* grads, long long n, float coeff, float* workspace, float* reg_loss, rgp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RGP_H_ */
