"""ctypes binding of librgp_hip.so (the C ABI declared in include/rgp.h).

The product path has NO fallback: if the HIP library is missing or a call fails,
this module raises.  Build it with ``python -c "import __graft_entry__ as g; g.build()"``
(or ``make -C recurrent_gaze_prediction_amd/csrc``).
"""
import ctypes
import os

# torch must be imported BEFORE librgp_hip.so is dlopen'ed: the library's libamdhip64
# dependency then resolves to the HIP runtime torch has already loaded, so device
# pointers, streams and events are shared.  Loading it first would bring in a second
# HIP runtime that sees no context ("no ROCm-capable device is detected").
import torch  # noqa: F401

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'librgp_hip.so')

RGP_F32, RGP_BF16 = 0, 1
RGP_ETIMEOUT = -5
RGP_GRCN_SAVE_FOR_BACKWARD, RGP_GRCN_PER_STEP, RGP_GRCN_UNFOLDED_HEAD = 1, 2, 4
RGP_C3D_SAVE_FOR_BACKWARD, RGP_C3D_KERNELS_IGEMM, RGP_C3D_KERNELS_TILE128, RGP_C3D_CONV2A_ROWWISE = 1, 2, 4, 8
RGP_C3D_CONV3_TWOPLANE = 32
RGP_C3DCONV_SAVE_FOR_BACKWARD, RGP_C3DCONV_STAGED, RGP_C3DCONV_FUSED = 1, 2, 4
RGP_LSTM_SAVE_FOR_BACKWARD, RGP_LSTM_PER_STEP, RGP_LSTM_PERSISTENT, RGP_LSTM_BPTT_PERSISTENT = 1, 2, 4, 8
RGP_GRCN77_SAVE_FOR_BACKWARD, RGP_GRCN77_PER_STEP = 1, 2
RGP_FCGRU_SAVE_FOR_BACKWARD, RGP_FCGRU_PER_STEP, RGP_FCGRU_PERSISTENT, RGP_FCGRU_BPTT_PERSISTENT = 1, 2, 4, 8
RGP_FCGRU_PERSISTENT_F32 = 16       # the persistent recurrence of f32 plans (csrc/fcgru_seq_f32.hip.h)
RGP_FCGRU_BPTT_PERSISTENT_F32 = 32  # the persistent BPTT of f32 plans (csrc/fcgru_bptt_f32.hip.h)
RGP_FAULT_SEQ_LOST_MEMBER, RGP_FAULT_BPTT_LOST_MEMBER = 1, 2
RGP_ACTION_NN, RGP_ACTION_SVM = 0, 1
RGP_ACTION_USE_GAZEMAP, RGP_ACTION_SAVE_FOR_BACKWARD, RGP_ACTION_UNFUSED = 1, 2, 4
RGP_GRCN_GRADS_TOP, RGP_GRCN_GRADS_GRU, RGP_GRCN_GRADS_PROJ = 0, 1, 2
RGP_SQNORM_PARTIALS = 256          # include/rgp.h
# saliency metrics (include/rgp.h): caps, metric bits (row of `scores` = bit position), flags
RGP_METRICS_MAX_PIX, RGP_METRICS_MAX_FIX, RGP_METRICS_MAX_THRESHOLDS, RGP_METRICS_COUNT = 4096, 256, 1024, 6
METRIC_BITS = {'sim': 1, 'cc': 2, 'AUC_Judd': 4, 'AUC_Borji': 8, 'AUC_shuffled': 16, 'NSS': 32}
METRIC_ROWS = {'sim': 0, 'cc': 1, 'AUC_Judd': 2, 'AUC_Borji': 3, 'AUC_shuffled': 4, 'NSS': 5}
RGP_METRICS_DEVICE_DRAWS, RGP_METRICS_NO_JITTER, RGP_METRICS_PRED_F64, RGP_METRICS_GT_F64 = 1, 2, 4, 8
# the same metrics at the fixation maps' shape (include/rgp.h): caps and the flag of a shared negative set
RGP_METRICS_SCALED_MAX_PIX, RGP_METRICS_SCALED_MAX_OTHER, RGP_METRICS_SCALED_OTHER_SHARED = 1 << 22, 4096, 16
# ground-truth maps from fixation points (include/rgp.h): caps
RGP_GTMAPS_MAX_PIX, RGP_GTMAPS_MAX_OBSERVERS, RGP_GTMAPS_MAX_RADIUS = 4096, 32, 32
# the same maps at the frame's resolution (include/rgp.h): caps, the largest radius the LDS tiles hold, and extents every
# tile extent of either filter pass divides
RGP_GTMAPS_FULL_MAX_PIX, RGP_GTMAPS_FULL_MAX_RADIUS, RGP_GTMAPS_FULL_LDS_RADIUS = 1 << 22, 256, 76
RGP_GTMAPS_FULL_TILE_COLS, RGP_GTMAPS_FULL_TILE_ROWS = 128, 64
# loader frame images (include/rgp.h): caps, the LDS a workgroup may take / takes by the library's own choice of bands, and
# the bytes of input rows staged per step
RGP_FRAMES_MAX_OUT, RGP_FRAMES_MAX_KSIZE, RGP_FRAMES_MAX_IN_W, RGP_FRAMES_MAX_BYTES = 256, 128, 2040, 1 << 40
RGP_FRAMES_LDS_BYTES, RGP_FRAMES_LDS_TARGET, RGP_FRAMES_STAGE_BYTES = 156 * 1024, 80 * 1024, 24576
# gaze-map export (include/rgp.h): caps and the LDS a workgroup may take
RGP_MAPEXPORT_MAX_SIDE, RGP_MAPEXPORT_MAX_KSIZE, RGP_MAPEXPORT_LDS_BYTES = 64, 512, 152 * 1024
# frame overlays (include/rgp.h): the flag of one (cmin, cmax) for the whole call
RGP_OVERLAY_SHARED_LIMITS = 1
DTYPES = {'f32': RGP_F32, 'fp32': RGP_F32, 'float32': RGP_F32, 'bf16': RGP_BF16, 'bfloat16': RGP_BF16}

c_void_p, c_int, c_size_t, c_char_p = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_char_p


class RgpError(RuntimeError):
    code = None        # the library's RGP_E* return value, when the error came from a library call


class GrcnWeights(ctypes.Structure):
    FIELDS = ('proj_c3d_W', 'proj_c3d_b', 'gru_Wz', 'gru_Uz', 'gru_Wr', 'gru_Ur', 'gru_W', 'gru_U',
              'bn_gamma', 'bn_beta', 'up_weight1', 'up_weight2', 'up_weight3', 'out_W', 'out_b')
    _fields_ = [(n, c_void_p) for n in FIELDS]


class FcGruWeights(ctypes.Structure):
    FIELDS = ('proj_c3d_W', 'proj_c3d_b', 'gates_kernel', 'gates_bias', 'candidate_kernel', 'candidate_bias',
              'proj_out_W', 'proj_out_b')
    _fields_ = [(n, c_void_p) for n in FIELDS]


class C3dConvWeights(ctypes.Structure):
    FIELDS = ('proj_c3d_W', 'proj_c3d_b', 'up_weight1', 'up_weight2', 'up_weight3', 'out_W', 'out_b')
    _fields_ = [(n, c_void_p) for n in FIELDS]


class LstmWeights(ctypes.Structure):
    FIELDS = ('proj_c3d_W', 'proj_c3d_b', 'W_xi', 'W_hi', 'W_ci', 'W_xf', 'W_hf', 'W_cf', 'W_xc', 'W_hc', 'W_xo', 'W_ho', 'W_co',
              'up_weight1', 'up_weight2', 'up_weight3', 'out_W', 'out_b')
    _fields_ = [(n, c_void_p) for n in FIELDS]


class Grcn77Weights(ctypes.Structure):
    FIELDS = ('proj_c3d_W', 'proj_c3d_b', 'gru_Wz', 'gru_Uz', 'gru_Wr', 'gru_Ur', 'gru_W', 'gru_U', 'out_W', 'out_b')
    _fields_ = [(n, c_void_p) for n in FIELDS]


class ShallowNetWeights(ctypes.Structure):
    FIELDS = ('conv1_w', 'conv1_b', 'conv2_w', 'conv2_b', 'conv3_w', 'conv3_b', 'fc1_w', 'fc1_b', 'fc2_w', 'fc2_b')
    _fields_ = [(n, c_void_p) for n in FIELDS]


class CascadeWeights(ctypes.Structure):
    FIELDS = ('proj_c3d_W', 'proj_c3d_b', 'bottom_Wz', 'bottom_Uz', 'bottom_Wr', 'bottom_Ur', 'bottom_W', 'bottom_U',
              'upsampling_weight', 'top_Wz', 'top_Uz', 'top_Wr', 'top_Ur', 'top_W', 'top_U',
              'fc1_w', 'fc1_b', 'fc2_w', 'fc2_b')
    _fields_ = [(n, c_void_p) for n in FIELDS] + [('shallownet', ShallowNetWeights)]


class ActionWeights(ctypes.Structure):
    FIELDS = ('W1', 'Wg', 'b1', 'W2', 'b2', 'W3', 'b3')
    _fields_ = [(n, c_void_p) for n in FIELDS]


class C3DWeights(ctypes.Structure):
    _fields_ = [('w', c_void_p * 8), ('b', c_void_p * 8)]


class MetricsArgs(ctypes.Structure):
    _fields_ = [('pred', c_void_p), ('gt', c_void_p), ('fix', c_void_p), ('other', c_void_p),
                ('other_stride', ctypes.c_longlong), ('n_frames', c_int), ('height', c_int), ('width', c_int),
                ('metrics', ctypes.c_uint), ('flags', ctypes.c_uint), ('n_rep', c_int), ('neg_stride', c_int),
                ('step_size', ctypes.c_double), ('judd_jitter', c_void_p), ('borji_neg', c_void_p),
                ('shuf_neg', c_void_p), ('shuf_cnt', c_void_p), ('seed', ctypes.c_ulonglong),
                ('offset', ctypes.c_ulonglong), ('workspace', c_void_p), ('workspace_bytes', c_size_t),
                ('scores', c_void_p)]


class MetricsScaledArgs(ctypes.Structure):
    _fields_ = [('pred', c_void_p), ('gt', c_void_p), ('fix_ptr', c_void_p), ('fix_idx', c_void_p), ('other_ptr', c_void_p),
                ('other_idx', c_void_p), ('fix_len', c_int), ('other_len', c_int), ('n_frames', c_int), ('height', c_int),
                ('width', c_int), ('target_height', c_int), ('target_width', c_int), ('metrics', ctypes.c_uint),
                ('flags', ctypes.c_uint), ('n_rep', c_int), ('neg_stride', c_int), ('step_size', ctypes.c_double),
                ('judd_jitter', c_void_p), ('borji_neg', c_void_p), ('shuf_neg', c_void_p), ('shuf_cnt', c_void_p),
                ('seed', ctypes.c_ulonglong), ('offset', ctypes.c_ulonglong), ('workspace', c_void_p),
                ('workspace_bytes', c_size_t), ('scores', c_void_p)]


class GtmapsArgs(ctypes.Structure):
    _fields_ = [('frame_ptr', c_void_p), ('samples', c_void_p), ('weights', c_void_p), ('n_frames', c_int),
                ('n_observers', c_int), ('raw_d1', c_int), ('raw_d2', c_int), ('out_s1', c_int), ('out_s2', c_int),
                ('radius', c_int), ('gazemaps', c_void_p), ('fixationmaps', c_void_p), ('labels', c_void_p),
                ('workspace', c_void_p), ('workspace_bytes', c_size_t)]


class GtmapsFullArgs(ctypes.Structure):
    _fields_ = [('frame_ptr', c_void_p), ('samples', c_void_p), ('weights', c_void_p), ('n_frames', c_int),
                ('n_observers', c_int), ('raw_d1', c_int), ('raw_d2', c_int), ('radius', c_int), ('gazemaps', c_void_p),
                ('fixationmaps', c_void_p), ('workspace', c_void_p), ('workspace_bytes', c_size_t)]


class FramesArgs(ctypes.Structure):
    _fields_ = [('frames', c_void_p), ('n_frames', c_int), ('fh', c_int), ('fw', c_int), ('frame_index', c_void_p),
                ('n_out', c_int), ('out_h', c_int), ('out_w', c_int), ('kh', c_void_p), ('bh', c_void_p), ('ksize_h', c_int),
                ('kv', c_void_p), ('bv', c_void_p), ('ksize_v', c_int), ('bands', c_int), ('images', c_void_p),
                ('images_u8', c_void_p), ('workspace', c_void_p), ('workspace_bytes', c_size_t)]


class MapExportArgs(ctypes.Structure):
    _fields_ = [('maps', c_void_p), ('n', c_int), ('h', c_int), ('w', c_int), ('out_h', c_int), ('out_w', c_int),
                ('kh', c_void_p), ('bh', c_void_p), ('ksize_h', c_int), ('kv', c_void_p), ('bv', c_void_p), ('ksize_v', c_int),
                ('pooled', c_void_p), ('pooled_u8', c_void_p), ('bytes', c_void_p), ('workspace', c_void_p),
                ('workspace_bytes', c_size_t)]


class OverlayArgs(ctypes.Structure):
    _fields_ = [('frames', c_void_p), ('frame_idx', c_void_p), ('maps', c_void_p), ('limits', c_void_p), ('lut', c_void_p),
                ('alpha', ctypes.c_float), ('flags', ctypes.c_uint), ('out', c_void_p), ('heat_u8', c_void_p), ('n', c_int),
                ('n_src', c_int), ('h', c_int), ('w', c_int), ('H', c_int), ('W', c_int)]


class SaliconBatchArgs(ctypes.Structure):
    _fields_ = [('images_u8', c_void_p), ('maps_u8', c_void_p), ('n', c_int), ('h', c_int), ('w', c_int), ('map_h', c_int),
                ('map_w', c_int), ('index', c_void_p), ('flip', c_void_p), ('batch', c_int), ('images', c_void_p),
                ('maps', c_void_p), ('workspace', c_void_p), ('workspace_bytes', c_size_t)]


# name -> (restype, argtypes); every symbol include/rgp.h declares
SIGNATURES = {
    'rgp_last_error': (c_char_p, []),
    'rgp_version': (c_int, []),
    'rgp_device_arch': (c_int, [c_char_p, c_int]),
    'rgp_grcn_create': (c_int, [ctypes.POINTER(c_void_p), c_int, c_int, c_int, c_int, c_int, c_int]),
    'rgp_grcn_destroy': (c_int, [c_void_p]),
    'rgp_grcn_status': (c_int, [c_void_p, c_void_p]),
    'rgp_grcn_inject_fault': (c_int, [c_void_p, c_int]),
    'rgp_c3d_layer_kernel_name': (c_char_p, [c_void_p, c_int, c_int]),
    'rgp_grcn_workspace_bytes': (c_size_t, [c_void_p]),
    'rgp_grcn_bind_workspace': (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    'rgp_grcn_set_weights': (c_int, [c_void_p, ctypes.POINTER(GrcnWeights), c_void_p]),
    'rgp_grcn_forward': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'rgp_grcn_forward_rows': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'rgp_grcn_state_elems': (c_size_t, [c_void_p]),
    'rgp_grcn_forward_stream': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'rgp_grcn_backward_stream': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_longlong,
                                         ctypes.POINTER(GrcnWeights), c_int, c_void_p]),
    'rgp_proj_fwd': (c_int, [c_void_p, c_void_p, c_void_p]),
    'rgp_convgru_xconv_fwd': (c_int, [c_void_p, c_void_p]),
    'rgp_convgru_seq_fwd': (c_int, [c_void_p, c_void_p]),
    'rgp_head_fwd': (c_int, [c_void_p, c_void_p, c_void_p]),
    'rgp_grcn_read_buffer': (c_int, [c_void_p, c_char_p, c_void_p, c_void_p]),
    'rgp_grcn_buffer_elems': (c_size_t, [c_void_p, c_char_p]),
    'rgp_grcn_backward_input': (c_int, [c_void_p, c_void_p, c_void_p]),
    'rgp_grcn_backward_from_states': (c_int, [c_void_p, c_void_p, ctypes.POINTER(GrcnWeights), c_void_p]),
    'rgp_softmax_xent_fwd': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    'rgp_fcgru_create': (c_int, [ctypes.POINTER(c_void_p), c_int, c_int, c_int, c_int, c_int]),
    'rgp_fcgru_destroy': (c_int, [c_void_p]),
    'rgp_fcgru_workspace_bytes': (c_size_t, [c_void_p]),
    'rgp_fcgru_bind_workspace': (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    'rgp_fcgru_set_weights': (c_int, [c_void_p, ctypes.POINTER(FcGruWeights), c_void_p]),
    'rgp_fcgru_forward': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'rgp_fcgru_create_ex': (c_int, [ctypes.POINTER(c_void_p), c_int, c_int, c_int, c_int, c_int, c_int]),
    'rgp_fcgru_backward': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.POINTER(FcGruWeights), c_int, c_void_p]),
    'rgp_fcgru_create_flags': (c_int, [ctypes.POINTER(c_void_p), c_int, c_int, c_int, c_int, c_int, c_int]),
    'rgp_fcgru_persistent_workgroups': (c_int, [c_void_p]),
    'rgp_fcgru_bptt_persistent_workgroups': (c_int, [c_void_p]),
    'rgp_fcgru_status': (c_int, [c_void_p, c_void_p]),
    'rgp_fcgru_read_buffer': (c_int, [c_void_p, c_char_p, c_void_p, c_void_p]),
    'rgp_fcgru_buffer_elems': (c_size_t, [c_void_p, c_char_p]),
    'rgp_fcgru_state_elems': (c_size_t, [c_void_p]),
    'rgp_fcgru_forward_stream': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    'rgp_fcgru_backward_stream': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_longlong,
                                          ctypes.POINTER(FcGruWeights), c_int, c_void_p]),
    'rgp_c3dconv_create': (c_int, [ctypes.POINTER(c_void_p), c_int, c_int, c_int, c_int, c_int]),
    'rgp_c3dconv_destroy': (c_int, [c_void_p]),
    'rgp_c3dconv_workspace_bytes': (c_size_t, [c_void_p]),
    'rgp_c3dconv_bind_workspace': (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    'rgp_c3dconv_set_weights': (c_int, [c_void_p, ctypes.POINTER(C3dConvWeights), c_void_p]),
    'rgp_c3dconv_forward': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'rgp_c3dconv_forward_rows': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'rgp_c3dconv_backward': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.POINTER(C3dConvWeights), c_int, c_void_p]),
    'rgp_c3dconv_backward_input': (c_int, [c_void_p, c_void_p, c_void_p]),
    'rgp_c3dconv_read_buffer': (c_int, [c_void_p, c_char_p, c_void_p, c_void_p]),
    'rgp_c3dconv_buffer_elems': (c_size_t, [c_void_p, c_char_p]),
    'rgp_c3dconv_path': (c_char_p, [c_void_p]),
    'rgp_lstm_create': (c_int, [ctypes.POINTER(c_void_p), c_int, c_int, c_int, c_int]),
    'rgp_lstm_destroy': (c_int, [c_void_p]),
    'rgp_lstm_workspace_bytes': (c_size_t, [c_void_p]),
    'rgp_lstm_bind_workspace': (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    'rgp_lstm_set_weights': (c_int, [c_void_p, ctypes.POINTER(LstmWeights), c_void_p]),
    'rgp_lstm_forward': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'rgp_lstm_forward_rows': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'rgp_lstm_state_elems': (c_size_t, [c_void_p]),
    'rgp_lstm_forward_stream': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    'rgp_lstm_backward': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.POINTER(LstmWeights), c_int, c_void_p]),
    'rgp_lstm_backward_input': (c_int, [c_void_p, c_void_p, c_void_p]),
    'rgp_lstm_status': (c_int, [c_void_p, c_void_p]),
    'rgp_lstm_inject_fault': (c_int, [c_void_p, c_int]),
    'rgp_lstm_persistent_workgroups': (c_int, [c_void_p]),
    'rgp_lstm_bptt_persistent_workgroups': (c_int, [c_void_p]),
    'rgp_lstm_read_buffer': (c_int, [c_void_p, c_char_p, c_void_p, c_void_p]),
    'rgp_lstm_buffer_elems': (c_size_t, [c_void_p, c_char_p]),
    'rgp_grcn77_create': (c_int, [ctypes.POINTER(c_void_p), c_int, c_int, c_int, c_int]),
    'rgp_grcn77_destroy': (c_int, [c_void_p]),
    'rgp_grcn77_workspace_bytes': (c_size_t, [c_void_p]),
    'rgp_grcn77_bind_workspace': (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    'rgp_grcn77_set_weights': (c_int, [c_void_p, ctypes.POINTER(Grcn77Weights), c_void_p]),
    'rgp_grcn77_forward': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'rgp_grcn77_forward_rows': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'rgp_grcn77_state_elems': (c_size_t, [c_void_p]),
    'rgp_grcn77_forward_stream': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    'rgp_grcn77_backward': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.POINTER(Grcn77Weights), c_int, c_void_p]),
    'rgp_grcn77_backward_input': (c_int, [c_void_p, c_void_p, c_void_p]),
    'rgp_grcn77_status': (c_int, [c_void_p, c_void_p]),
    'rgp_grcn77_persistent_workgroups': (c_int, [c_void_p]),
    'rgp_grcn77_read_buffer': (c_int, [c_void_p, c_char_p, c_void_p, c_void_p]),
    'rgp_grcn77_buffer_elems': (c_size_t, [c_void_p, c_char_p]),
    'rgp_grcn77_head_fwd': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'rgp_shallownet_create_ex': (c_int, [ctypes.POINTER(c_void_p), c_int, c_int, c_int, c_int]),
    'rgp_shallownet_backward': (c_int, [c_void_p, c_int, c_void_p, ctypes.POINTER(ShallowNetWeights), c_void_p]),
    'rgp_shallownet_create': (c_int, [ctypes.POINTER(c_void_p), c_int, c_int, c_int]),
    'rgp_shallownet_destroy': (c_int, [c_void_p]),
    'rgp_shallownet_workspace_bytes': (c_size_t, [c_void_p]),
    'rgp_shallownet_bind_workspace': (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    'rgp_shallownet_set_weights': (c_int, [c_void_p, ctypes.POINTER(ShallowNetWeights), c_void_p]),
    'rgp_shallownet_forward': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    'rgp_cascade_create': (c_int, [ctypes.POINTER(c_void_p), c_int, c_int, c_int, c_int]),
    'rgp_cascade_destroy': (c_int, [c_void_p]),
    'rgp_cascade_workspace_bytes': (c_size_t, [c_void_p]),
    'rgp_cascade_bind_workspace': (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    'rgp_cascade_set_weights': (c_int, [c_void_p, ctypes.POINTER(CascadeWeights), c_void_p]),
    'rgp_cascade_forward': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'rgp_cascade_state_elems': (c_size_t, [c_void_p]),
    'rgp_cascade_forward_stream': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    'rgp_cascade_read_buffer': (c_int, [c_void_p, c_char_p, c_void_p, c_void_p]),
    'rgp_cascade_create_ex': (c_int, [ctypes.POINTER(c_void_p), c_int, c_int, c_int, c_int, c_int]),
    'rgp_cascade_backward': (c_int, [c_void_p, c_void_p, c_void_p, ctypes.POINTER(CascadeWeights), c_void_p, c_void_p]),
    'rgp_c3d_create': (c_int, [ctypes.POINTER(c_void_p), c_int, c_int]),
    'rgp_c3d_destroy': (c_int, [c_void_p]),
    'rgp_c3d_workspace_bytes': (c_size_t, [c_void_p]),
    'rgp_c3d_bind_workspace': (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    'rgp_c3d_set_weights': (c_int, [c_void_p, ctypes.POINTER(C3DWeights), c_void_p]),
    'rgp_c3d_forward': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    'rgp_c3d_forward_frames': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, ctypes.POINTER(c_int), c_int, c_void_p,
                                       c_void_p, c_void_p, c_void_p]),
    'rgp_c3d_frames_to_video': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, ctypes.POINTER(c_int), c_int, c_void_p,
                                        c_void_p, c_void_p]),
    'rgp_c3d_create_ex': (c_int, [ctypes.POINTER(c_void_p), c_int, c_int, c_int]),
    'rgp_c3d_param_elems': (c_size_t, [c_void_p]),
    'rgp_c3d_param_offset': (c_size_t, [c_void_p, c_int, c_int]),
    'rgp_c3d_backward': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    'rgp_c3d_read_grad_image': (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    'rgp_c3d_read_layer': (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    'rgp_c3d_layer_elems': (c_size_t, [c_void_p, c_int, c_int]),
    'rgp_grcn_backward': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.POINTER(GrcnWeights), c_int, c_void_p]),
    'rgp_adam_clip_step': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_longlong, c_void_p, c_int,
                                   ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                   c_void_p, c_void_p]),
    'rgp_global_sqnorm': (c_int, [c_void_p, ctypes.c_longlong, c_void_p, c_void_p]),
    'rgp_adam_clip_step_ext': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_longlong, c_void_p, c_int, c_int,
                                       ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                       c_void_p, c_void_p]),
    'rgp_lr_schedule_step': (c_int, [c_void_p, ctypes.c_float, ctypes.c_float, c_int, ctypes.c_float, ctypes.c_float,
                                     c_void_p, c_void_p]),
    'rgp_adam_clip_step_dev': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_longlong, c_void_p, c_int, c_void_p,
                                       ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, c_void_p, c_void_p]),
    'rgp_momentum_clip_step': (c_int, [c_void_p, c_void_p, c_void_p, ctypes.c_longlong, c_void_p, c_int, ctypes.c_float,
                                       ctypes.c_float, ctypes.c_float, c_void_p, c_void_p]),
    'rgp_rmsprop_clip_step': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_longlong, c_void_p, c_int,
                                      ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                      c_void_p, c_void_p]),
    'rgp_l2_loss_fwd': (c_int, [c_void_p, c_void_p, ctypes.c_longlong, c_int, c_void_p, c_void_p, c_void_p]),
    'rgp_dropout_mask': (c_int, [c_void_p, ctypes.c_longlong, ctypes.c_float, ctypes.c_ulonglong, ctypes.c_ulonglong, c_void_p]),
    'rgp_metrics_workspace_bytes': (c_size_t, [c_int, c_int, c_int, ctypes.c_uint]),
    'rgp_saliency_scores': (c_int, [ctypes.POINTER(MetricsArgs), c_void_p]),
    'rgp_metrics_status': (c_int, [c_void_p, c_void_p]),
    'rgp_metrics_scaled_workspace_bytes': (c_size_t, [c_int, c_int, c_int, c_int, c_int, ctypes.c_uint]),
    'rgp_saliency_scores_scaled': (c_int, [ctypes.POINTER(MetricsScaledArgs), c_void_p]),
    'rgp_spline_resize_workspace_bytes': (c_size_t, [c_int, c_int]),
    'rgp_spline_resize': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    'rgp_gtmaps_workspace_bytes': (c_size_t, []),
    'rgp_gazemaps_from_fixations': (c_int, [ctypes.POINTER(GtmapsArgs), c_void_p]),
    'rgp_gtmaps_status': (c_int, [c_void_p, c_void_p]),
    'rgp_gtmaps_full_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
    'rgp_gazemaps_full_from_fixations': (c_int, [ctypes.POINTER(GtmapsFullArgs), c_void_p]),
    'rgp_gtmaps_full_status': (c_int, [c_void_p, ctypes.POINTER(c_int), c_void_p]),
    'rgp_frames_workspace_bytes': (c_size_t, []),
    'rgp_frames_plan': (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    'rgp_frame_images': (c_int, [ctypes.POINTER(FramesArgs), c_void_p]),
    'rgp_frames_status': (c_int, [c_void_p, ctypes.POINTER(c_int), c_void_p]),
    'rgp_mapexport_workspace_bytes': (c_size_t, []),
    'rgp_mapexport': (c_int, [ctypes.POINTER(MapExportArgs), c_void_p]),
    'rgp_mapexport_status': (c_int, [c_void_p, ctypes.POINTER(c_int), c_void_p]),
    'rgp_overlay_workspace_bytes': (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    'rgp_overlay': (c_int, [ctypes.POINTER(OverlayArgs), c_void_p, c_size_t, c_void_p]),
    'rgp_overlay_status': (c_int, [c_void_p, ctypes.POINTER(c_int), c_void_p]),
    'rgp_dropout_apply': (c_int, [c_void_p, c_void_p, ctypes.c_longlong, ctypes.c_float, c_void_p]),
    'rgp_fcgru_set_dropout': (c_int, [c_void_p, ctypes.c_float, c_void_p]),
    'rgp_cascade_set_dropout': (c_int, [c_void_p, ctypes.c_float, c_void_p]),
    'rgp_c3d_wait_layer_grads': (c_int, [c_void_p, c_int, c_void_p]),
    'rgp_grcn_wait_grads': (c_int, [c_void_p, c_int, c_void_p]),
    'rgp_grcn_grads_top_early': (c_int, [c_void_p]),
    'rgp_grcn_persistent_workgroups': (c_int, [c_void_p]),
    'rgp_grcn_profile_enable': (c_int, [c_void_p, c_int]),
    'rgp_grcn_profile_read': (c_int, [c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_longlong)]),
    'rgp_c3d_profile_enable': (c_int, [c_void_p, c_int]),
    'rgp_c3d_profile_read': (c_int, [c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_longlong)]),
    'rgp_action_create': (c_int, [ctypes.POINTER(c_void_p), c_int, c_int, c_int, c_int, c_int]),
    'rgp_action_destroy': (c_int, [c_void_p]),
    'rgp_action_workspace_bytes': (c_size_t, [c_void_p]),
    'rgp_action_bind_workspace': (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    'rgp_action_set_weights': (c_int, [c_void_p, ctypes.POINTER(ActionWeights), c_void_p]),
    'rgp_action_get_weights': (c_int, [c_void_p, ctypes.POINTER(ActionWeights), c_void_p]),
    'rgp_action_bind_slots': (c_int, [c_void_p, ctypes.POINTER(ActionWeights), ctypes.POINTER(ActionWeights)]),
    'rgp_action_forward': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'rgp_action_forward_rows': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'rgp_action_loss': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    'rgp_action_train_step': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, ctypes.c_float, c_void_p, c_void_p]),
    'rgp_action_fc1_fwd': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    'rgp_action_tail': (c_int, [c_void_p, c_void_p, c_void_p]),
    'rgp_action_fc1_update': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, ctypes.c_float, c_void_p]),
    'rgp_action_read_buffer': (c_int, [c_void_p, c_char_p, c_void_p, c_void_p]),
    'rgp_action_buffer_elems': (c_size_t, [c_void_p, c_char_p]),
    'rgp_shallownet_set_dropout': (c_int, [c_void_p, ctypes.c_float, c_void_p]),
    'rgp_shallownet_read_buffer': (c_int, [c_void_p, c_char_p, c_void_p, c_void_p]),
    'rgp_shallownet_buffer_elems': (c_size_t, [c_void_p, c_char_p]),
    'rgp_salicon_workspace_bytes': (c_size_t, []),
    'rgp_salicon_batch': (c_int, [ctypes.POINTER(SaliconBatchArgs), c_void_p]),
    'rgp_salicon_status': (c_int, [c_void_p, ctypes.POINTER(c_int), c_void_p]),
    'rgp_euclid_loss_fwd_bwd': (c_int, [c_void_p, c_void_p, ctypes.c_longlong, ctypes.c_float, c_void_p, c_void_p, c_void_p,
                                        c_void_p]),
    'rgp_l2_reg': (c_int, [c_void_p, c_void_p, ctypes.c_longlong, ctypes.c_float, c_void_p, c_void_p, c_void_p]),
}
GRCN_STAGES = ('proj', 'xconv', 'convgru_seq', 'head', 'softmax')
C3D_STAGES = ('conv1a', 'conv2a', 'conv3a', 'conv3b', 'conv4a', 'conv4b', 'conv5a', 'conv5b', 'video_prep')

_lib = None


def load():
    """Load librgp_hip.so and bind every declared symbol.  Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RgpError('%s not found: the HIP extension is not built (run __graft_entry__.build()); '
                       'there is no CPU fallback' % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def kernel_source_hashes():
    """{file name: sha256[:16]} of the library's sources (csrc/ + include/rgp.h).  A PMC summary records them
    (scripts/pmc_summary.py) and bench.py compares: counters taken from another build of a kernel are reported as stale."""
    import glob
    import hashlib
    here = os.path.dirname(os.path.abspath(__file__))
    files = sorted(glob.glob(os.path.join(here, 'csrc', '*.hip')) + glob.glob(os.path.join(here, 'csrc', '*.h')))
    files.append(os.path.join(os.path.dirname(here), 'include', 'rgp.h'))
    out = {}
    for f in files:
        if os.path.exists(f):
            with open(f, 'rb') as fh:
                out[os.path.basename(f)] = hashlib.sha256(fh.read()).hexdigest()[:16]
    return out


# sources that define a kernel's code and launch geometry (prefix of the name rgp_c3d_layer_kernel_name returns)
KERNEL_SOURCES = {
    'conv_patch_bf16_kernel': ('conv_patch.hip.h', 'rgp_conv_patch.hip', 'rgp_c3d.hip', 'rgp_c3d_plan.h', 'rgp_host.h'),
    'conv_patch_slab_bf16_kernel': ('conv_patch_slab.hip.h', 'conv_patch.hip.h', 'rgp_conv_patch.hip', 'rgp_c3d.hip', 'rgp_c3d_plan.h',
                                    'rgp_host.h'),
    'conv_patch14_bf16_kernel': ('conv_patch14.hip.h', 'rgp_conv_patch.hip', 'rgp_c3d.hip', 'rgp_c3d_plan.h', 'rgp_host.h'),
}


def check(rc):
    if rc != 0:
        err = RgpError('librgp_hip error %d: %s' % (rc, load().rgp_last_error().decode()))
        err.code = int(rc)
        raise err
