"""ctypes binding of the C-ABI library ``libgeeco_hip.so`` (declared in include/geeco_hip.h).

The library is the product's only compute path.  There is deliberately no CPU/PyTorch
fallback: if the shared object is missing or a symbol does not resolve, importing the ops
raises ``GeecoNativeError`` (the build recipe is ``geeco_amd/csrc/build.sh``).
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_char_p, c_float, c_int, c_int32, c_int64, c_void_p, POINTER, Structure

_HERE = os.path.dirname(os.path.abspath(__file__))


def lib_path():
  """libgeeco_hip.so next to this file.  ``GEECO_DEV=1 GEECO_LIB=NAME`` loads another build from the same directory
  instead (the A/B and instrumentation builds of scripts/dev/build_variant.sh and build_stamps.sh); without GEECO_DEV=1
  GEECO_LIB is ignored.  No other environment variable changes what the package runs."""
  dev = os.environ.get('GEECO_DEV')
  name = os.environ.get('GEECO_LIB', 'libgeeco_hip.so') if dev and dev != '0' else 'libgeeco_hip.so'
  return os.path.join(_HERE, name)


LIB_PATH = lib_path()


GEECO_EINVAL, GEECO_ENOSUP = -1, -2      # include/geeco_hip.h
ABI_VERSION = 7       # GEECO_ABI_VERSION of include/geeco_hip.h this binding was written against


class GeecoNativeError(RuntimeError):
  pass


_P = c_void_p          # device (or host) pointer
_PP = POINTER(c_void_p)
_I, _L, _F = c_int, c_int64, c_float


class HeadsFinish(Structure):
  """geeco_heads_finish (include/geeco_hip.h): the pending batch sums of the heads' backward, opaque to the caller."""
  _fields_ = [('opaque', ctypes.c_ubyte * 1024)]


class LossShaping(Structure):
  """geeco_loss_shaping (include/geeco_hip.h): tf.losses' optional arguments for the shaped heads entry points."""
  _fields_ = [('sample_weight', c_void_p), ('sample_weight_stride', c_int64), ('class_weight', c_void_p),
              ('label_smoothing', c_float), ('huber_delta', c_float * 5)]


class SlabReduce(Structure):
  """geeco_slab_reduce (include/geeco_hip.h): one pending slab sum of a filter-gradient kernel."""
  _fields_ = [('part', c_void_p), ('dw', c_void_p), ('db', c_void_p), ('gs_dw', c_int64), ('gs_db', c_int64),
              ('KC', c_int64), ('S', c_int32), ('Cout', c_int32), ('groups', c_int32), ('reserved', c_int32)]


class AdamSegment(Structure):
  """geeco_adam_segment (include/geeco_hip.h): one piece of the arena with its own gradient source."""
  _fields_ = [('g', c_void_p), ('p_off', c_int64), ('count', c_int64)]


# The constants of include/geeco_hip.h the package mirrors live here and nowhere else (tests/test_abi_cpu.py compares each to its #define).
ADAM_SEGMENTS_MAX = 8
SLAB_REDUCE_MAX = 8

PREDICT_FEAT_MODES = {'plain': 0, 'constant': 1, 'residual': 2}     # GEECO_PREDICT_FEAT_* of include/geeco_hip.h

VARSTATS_CHUNK, VARSTATS_CLASSES = 4096, 40      # GEECO_VARSTATS_* of include/geeco_hip.h

REPLAY_MAXK, REPLAY_MAXHEADS = 64, 8      # the window lengths geeco_replay_states takes; GEECO_REPLAY_MAXHEADS of include/geeco_hip.h
REPLAY_SQUARED_ERROR, REPLAY_CLASS_HIT = 0, 1      # head kinds of geeco_replay_errors

LR_KINDS = ('constant', 'exponential', 'cosine', 'piecewise')      # GEECO_LR_* of include/geeco_hip.h, in order
LR_BOUNDARIES_MAX = 8


class LrSchedule(Structure):
  """geeco_lr_schedule (include/geeco_hip.h): a learning-rate schedule as the device holds it (float rates, int64 step counts)."""
  _fields_ = [('kind', c_int32), ('base_lr', c_float), ('warmup_steps', c_int64), ('decay_steps', c_int64), ('decay_rate', c_float),
              ('alpha', c_float), ('staircase', c_int32), ('n_boundaries', c_int32), ('boundaries', c_int64 * LR_BOUNDARIES_MAX),
              ('values', c_float * (LR_BOUNDARIES_MAX + 1))]

PERTURB_METHODS = ('occlusion', 'rise')      # GEECO_PERTURB_* of include/geeco_hip.h, in order


class PerturbDesc(Structure):
  """geeco_perturb_desc (include/geeco_hip.h): the occluder grid or the RISE masks of a perturbation pass."""
  _fields_ = [('method', c_int32), ('H', c_int32), ('W', c_int32), ('ph', c_int32), ('pw', c_int32), ('sy', c_int32), ('sx', c_int32),
              ('grid', c_int32), ('keep_threshold', ctypes.c_uint32), ('reserved', ctypes.c_uint32), ('key', ctypes.c_uint64)]


# symbol -> (restype, argtypes); mirrors include/geeco_hip.h one to one
SIGNATURES = {
    'geeco_abi_version': (_I, []),
    'geeco_last_error': (c_char_p, []),
    'geeco_has_dev_kernels': (_I, []),
    'geeco_debug_kernel_trace_begin': (None, []),
    'geeco_debug_kernel_trace_end': (c_char_p, []),
    'geeco_dynimg_alpha': (None, [_I, _P]),
    'geeco_dynimg_ws_bytes': (_L, [_I, _L]),
    'geeco_dynimg_fwd': (_I, [_P, _P, _L, _L, _P, _I, _I, _L, _I, _I, _P, _P, _P]),
    'geeco_goal_dynimgs_ws_bytes': (_L, [_I, _L]),
    'geeco_goal_dynimgs_fwd': (_I, [_P, _L, _L, _P, _P, _L, _L, _P, _P, _P, _I, _I, _L, _P, _P, _P, _P, _P]),
    'geeco_goal_dynimgs_u8_fwd': (_I, [_P, _P, _P, _L, _L, _P, _P, _P, _I, _I, _L, _P, _P, _P, _P, _P]),
    'geeco_goal_dynimgs_timeouts': (_I, [_P, _I, _P, _P]),
    'geeco_goal_dynimgs_set_wait_polls': (ctypes.c_uint, [ctypes.c_uint]),
    'geeco_dynimg_rgbd_fwd': (_I, [_P, _P, _L, _L, _P, _P, _L, _L, _P, _I, _I, _L, _P, _P, _P]),
    'geeco_pack_pixels': (_I, [_P, _L, _P, _L, _I, _L, _I, _I, _I, _P, _P]),
    'geeco_gather_windows': (_I, [_P, _I, _P, _I, _I, _L, _F, _P, _P]),
    'geeco_gather_windows_by_address': (_I, [_P, _P, _I, _I, _L, _P, _P]),
    'geeco_gather_windows_augmented': (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P]),
    'geeco_gather_windows_scene': (_I, [_P, _P, _P, _P, _P, _P, _P, _F, _I, _I, _I, _I, _I, _I, _P, _P]),      # additive within ABI 7
    'geeco_gather_windows_frames': (_I, [_P, _P, _P, _P, _P, _P, _P, _F, _I, _I, _I, _I, _I, _I, _P, _P]),     # additive within ABI 7
    'geeco_predict_range_check': (_I, [_P, _I, _L, _I, _F, _F, _P, _P]),
    'geeco_predict_push_dense': (_I, [_P, _I, _P, _P, _P, _I, _I, _L, _I, _I, _P, _P, _P, _P]),
    'geeco_predict_push_ring': (_I, [_P, _P, _P, _P, _I, _I, _L, _I, _P, _P, _P, _P, _P]),
    'geeco_predict_pack': (_I, [_P, _I, _I, _I, POINTER(_I), POINTER(_I), POINTER(_I), _P, _I, _P, _P, _P, _P, _L, _I, _P, _P]),
    'geeco_predict_pack_newest': (_I, [_P, _I, _I, _L, _I, _P, _P]),
    'geeco_predict_push_features': (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _L, _P]),
    'geeco_pack_frames_by_address': (_I, [_P, _I, _I, _L, _P, _P]),
    'geeco_window_states_fwd': (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _L, _P]),
    'geeco_window_states_bwd': (_I, [_P, _L, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    'geeco_conv3x3_fwd': (_I, [_P, _P, _P, _P, _I, _L, _L, _L, _L, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    'geeco_conv3x3_fwd_state': (_I, [_P, _P, _P, _P, _I, _L, _L, _L, _L, _I, _I, _I, _I, _I, _I, _P, _P, _I, _P, _L, _I, _I, _P, _L, _P]),
    'geeco_conv3x3_fwd_ws_bytes': (_L, [_I, _I, _I, _I, _I, _I, _I]),
    'geeco_conv3x3_dgrad': (_I, [_P, _P, _P, _P, _P, _I, _L, _L, _L, _L, _I, _I, _I, _I, _I, _I, _P, _P]),
    'geeco_conv3x3_dgrad_ws_bytes': (_L, [_I, _I, _I, _I, _I, _I, _I]),
    'geeco_conv3x3_dgrad_needs_wt': (_I, [_I, _I, _I, _I, _I]),
    'geeco_conv3x3_dgrad_relu_fields_supported': (_I, [_I, _I, _I, _I, _I]),
    'geeco_conv3x3_wgrad_ws_bytes': (_L, [_I, _I, _I, _I, _I, _I, _I]),
    'geeco_conv3x3_wgrad': (_I, [_P, _P, _P, _P, _I, _L, _L, _L, _L, _I, _I, _I, _I, _I, _I, _P, _P]),
    'geeco_conv2_dgrad_conv1_wgrad_ws_bytes': (_L, [_I]),
    'geeco_conv2_dgrad_conv1_wgrad': (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _L, _L, _L, _L, _L, _L, _I, _I, _I, _I, _P, _P]),
    'geeco_conv3x3_wgrad_partial': (_I, [_P, _P, _P, _P, _I, _L, _L, _L, _L, _I, _I, _I, _I, _I, _I, _P, _P,
                                         POINTER(SlabReduce), _I]),
    'geeco_conv2_dgrad_conv1_wgrad_partial': (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _L, _L, _L, _L, _L, _L, _I, _I, _I, _I,
                                                   _P, _P, POINTER(SlabReduce), _I]),
    'geeco_slab_reduce_batch': (_I, [POINTER(SlabReduce), _I, _P]),
    'geeco_slab_reduce_batch_prepare': (_I, [POINTER(SlabReduce), _I, _P, _F, _F, _F, _P, _P]),
    'geeco_conv_top_bwd': (_I, [_P, _P, _P, _P, _P, _L, _L, _L, _L, _I, _I, _I, _I, _I, _P,
                                _P, _P, _P, _P, _L, _L, _L, _L, _I, _I, _I, _I, _I, _P,
                                _P, _P, _P, _P, _L, _L, _L, _L, _I, _I, _I, _I, _I, _P, _I, _I, _P, POINTER(SlabReduce)]),
    'geeco_conv3x3_wgrad_pair': (_I, [_P, _P, _P, _P, _L, _L, _L, _L, _I, _I, _I, _I, _I, _P,
                                      _P, _P, _P, _P, _L, _L, _L, _L, _I, _I, _I, _I, _I, _P, _I, _I, _P, POINTER(SlabReduce)]),
    'geeco_relu_bits_pitch': (_L, [_I]),
    'geeco_conv3_fwd_relu_fields': (_I, [_P, _P, _P, _P, _P, _I, _L, _L, _L, _L, _L, _I, _I, _I, _P]),
    'geeco_conv3x3_dgrad_relu_fields': (_I, [_P, _P, _P, _P, _I, _L, _L, _L, _L, _I, _I, _I, _I, _I, _I, _P]),
    'geeco_relu_fields_elems': (_L, [_I, _I, _I]),
    'geeco_conv2_fwd_relu_fields': (_I, [_P, _P, _P, _P, _P, _I, _L, _L, _L, _L, _L, _I, _I, _I, _P]),
    'geeco_conv3_dgrad_relu_fields': (_I, [_P, _P, _P, _P, _I, _L, _L, _L, _L, _I, _I, _I, _P, _I]),
    'geeco_relu_bits_rows': (_L, [_I]),
    'geeco_conv1_fwd_relu_bits': (_I, [_P, _P, _P, _P, _P, _I, _L, _L, _L, _L, _L, _I, _I, _I, _P]),
    'geeco_conv1_fwd_relu_bits_rgb': (_I, [_P, _P, _P, _P, _P, _I, _L, _L, _L, _L, _L, _I, _I, _I, _P]),
    'geeco_conv2_dgrad_conv1_wgrad_bits': (_I, [_P, _P, _P, _P, _P, _P, _I, _L, _L, _L, _L, _L, _L, _I, _I, _I, _I, _P, _P,
                                                POINTER(SlabReduce), _I]),
    'geeco_transpose_hwio': (_I, [_P, _P, _I, _L, _L, _I, _I, _P]),
    'geeco_derive_conv_weights': (_I, [_I, _PP, _PP, POINTER(_I), POINTER(_I), POINTER(_L), _I, _L, _P, _P, _I, _I, _I, _L,
                                       _P]),
    'geeco_pad_mid': (_I, [_P, _P, _L, _I, _I, _I, _P]),
    'geeco_state_concat_fwd': (_I, [_PP, POINTER(_I), _I, _I, _P, _L, _I, _P, _I, _I, _P, _L, _P]),
    'geeco_state_concat_bwd': (_I, [_P, _L, _PP, _PP, POINTER(_I), _I, _I, _I, _I, _I, _I, _F, _P]),
    'geeco_gemm_ws_bytes': (_L, [_I, _I, _I]),
    'geeco_gemm_f32': (_I, [_P, _L, _I, _P, _L, _I, _P, _L, _I, _I, _I, _I, _P, _P]),
    'geeco_lstm_gates_fwd': (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _P]),
    'geeco_lstm_input_step_fwd': (_I, [_P, _L, _P, _L, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P]),
    'geeco_lstm_gates_bwd': (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _P]),
    'geeco_lstm_step_bwd_ws_bytes': (_L, [_I, _I, _I]),
    'geeco_lstm_step_bwd': (_I, [_P, _L, _P, _L, _P, _L, _P, _L, _P, _P, _L, _I, _I, _I, _PP, _PP, POINTER(_I), _I, _I, _I, _I, _P, _P, _P]),
    'geeco_colsum': (_I, [_P, _L, _I, _I, _P, _I, _P]),
    'geeco_heads_ws_bytes': (_L, [_I, _I, _I]),
    'geeco_heads_loss_fwd_bwd': (_I, [_P, _P, _P, _I, _PP, _PP, POINTER(_I), POINTER(_I), POINTER(_F), _PP,
                                      POINTER(_L), _F, _I, _I, _I, _P, _P, _I, _P, _P, _P, _PP, _PP, _P, _P]),
    'geeco_lstm_step_heads_fwd_bwd': (_I, [_P, _L, _P, _L, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _I, _PP, _PP, POINTER(_I),
                                           POINTER(_I), POINTER(_F), _PP, POINTER(_L), _F, _I, _P, _P, _I, _P, _P, _P, _PP, _PP,
                                           _P, _P, _P]),
    # additive within ABI 7: the two entry points above with a geeco_loss_shaping* behind Hfc
    'geeco_loss_shaping_sizeof': (_L, []),
    'geeco_heads_loss_shaped_fwd_bwd': (_I, [_P, _P, _P, _I, _PP, _PP, POINTER(_I), POINTER(_I), POINTER(_F), _PP,
                                             POINTER(_L), _F, _I, _I, _I, POINTER(LossShaping), _P, _P, _I, _P, _P, _P, _PP, _PP,
                                             _P, _P]),
    'geeco_lstm_step_heads_shaped_fwd_bwd': (_I, [_P, _L, _P, _L, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _I, _PP, _PP,
                                                  POINTER(_I), POINTER(_I), POINTER(_F), _PP, POINTER(_L), _F, _I,
                                                  POINTER(LossShaping), _P, _P, _I, _P, _P, _P, _PP, _PP, _P, _P, _P]),
    'geeco_lstm_seq_heads_fwd': (_I, [_P, _L, _P, _L, _P, _P, _P, _I, _PP, _PP, POINTER(_I), _I, _I, _I, _I, _P, _P, _P, _P]),
    'geeco_adam_prepare': (_I, [_P, _F, _F, _F, _P, _P]),
    'geeco_adam_tf': (_I, [_P, _P, _P, _P, _L, _P, _F, _F, _F, _F, _F, _P]),
    'geeco_adam_tf_segments': (_I, [_P, _P, _P, _P, _P, _I, _P, _F, _F, _F, _F, _F, _P]),
    'geeco_adam_tf_ema': (_I, [_P, _P, _P, _P, _P, _L, _P, _P, _F, _F, _F, _F, _F, _F, _P]),
    'geeco_adam_tf_segments_ema': (_I, [_P, _P, _P, _P, _P, _P, _I, _P, _P, _F, _F, _F, _F, _F, _F, _P]),
    'geeco_clip_ws_floats': (_L, [_L]),
    'geeco_grad_sumsq_segments': (_I, [_P, _P, _I, _L, _F, _F, _P, _P]),
    'geeco_clip_scale': (_I, [_P, _L, _F, _P, _P]),
    'geeco_adam_tf_segments_clip': (_I, [_P, _P, _P, _P, _P, _P, _I, _P, _P, _F, _P, _F, _F, _F, _F, _F, _P]),
    'geeco_guard_decide': (_I, [_P, _L, _F, _P, _P, _P]),
    'geeco_adam_tf_segments_guard': (_I, [_P, _P, _P, _P, _P, _P, _I, _P, _P, _F, _P, _P, _F, _F, _F, _F, _F, _P]),
    'geeco_adam_tf_segments_scaled': (_I, [_P, _P, _P, _P, _P, _P, POINTER(c_float), _I, _P, _P, _F, _P, _P, _F, _F, _F, _F, _F, _P]),
    'geeco_adam_prepare_schedule': (_I, [_P, POINTER(LrSchedule), _F, _F, _P, _P]),
    'geeco_slab_reduce_batch_prepare_schedule': (_I, [POINTER(SlabReduce), _I, _P, POINTER(LrSchedule), _F, _F, _P, _P]),
    'geeco_lr_schedule_eval': (_I, [POINTER(LrSchedule), _L, POINTER(ctypes.c_double)]),
    'geeco_variable_stats_ws_bytes': (_L, [_L]),      # additive within ABI 7
    'geeco_variable_stats': (_I, [_P, _P, _P, _P, _I, _L, _F, _F, POINTER(c_int64), POINTER(c_int64), _I, _P, _L, _P, _P, _P]),
    'geeco_grad_accumulate_segments': (_I, [_P, _P, _I, _L, _I, _P]),      # additive within ABI 7
    'geeco_sumsq': (_I, [_P, _L, _P, _P]),
    # additive within ABI 7: input gradients
    'geeco_conv1_dgrad': (_I, [_P, _P, _P, _I, _L, _L, _L, _I, _I, _I, _I, _I, _P]),
    'geeco_pack_pixels_bwd': (_I, [_P, _P, _L, _I, _P, _L, _I, _I, _L, _I, _I, _I, _P]),
    'geeco_dynimg_bwd_ws_bytes': (_L, [_I, _L, _I]),
    'geeco_dynimg_bwd': (_I, [_P, _P, _P, _L, _L, _P, _I, _I, _L, _I, _I, _P, _L, _L, _I, _P, _I, _P, _P]),
    # additive within ABI 7: episode replay
    'geeco_replay_states': (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _L, _P]),
    'geeco_replay_errors': (_I, [_P, _P, _I, _I, _I, POINTER(_I), POINTER(_I), POINTER(_I), _P, _P, _P]),
    # additive within ABI 7: episode replay for the dynamic-image controllers
    'geeco_replay_images_ws_bytes': (_L, [_I, _L]),
    'geeco_replay_images': (_I, [_P, _P, _I, _P, _P, _I, _I, _I, _I, _L, _P, _P, _P, _P, _P]),
    'geeco_replay_states_pair': (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _L, _P]),
    # additive within ABI 7: attributions
    'geeco_attr_path_point': (_I, [_P, _P, _P, _L, _F, _F, ctypes.c_uint64, ctypes.c_uint32, _L, _P]),
    'geeco_attr_accumulate': (_I, [_P, _P, _F, _L, _I, _P]),
    'geeco_attr_finish': (_I, [_P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _L, _I, _P]),
    # additive within ABI 7: perturbation attributions; the description is a host PerturbDesc, passed by address
    'geeco_perturb_desc_sizeof': (_L, []),
    'geeco_perturb_patch': (_I, [_P, _I, POINTER(c_int32)]),
    'geeco_perturb_apply': (_I, [_P, _P, _P, _L, _P, _I, _I, _I, _I, _I, _I, _P]),
    'geeco_perturb_score': (_I, [_P, _P, _P, _P, _I, _I, _P]),
    'geeco_perturb_accumulate': (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    'geeco_perturb_finish': (_I, [_P, _P, _P, _L, _P]),
}

_lib = None


def load():
  """Loads the shared library once and types every declared symbol. Raises if anything is missing."""
  global _lib
  if _lib is not None:
    return _lib
  if not os.path.exists(LIB_PATH):
    raise GeecoNativeError(
        "HIP library not built: %s is missing. Run geeco_amd/csrc/build.sh (hipcc, gfx950). "
        "geeco_amd has no CPU fallback." % LIB_PATH)
  try:
    lib = ctypes.CDLL(LIB_PATH)
  except OSError as e:
    raise GeecoNativeError("cannot load %s: %s" % (LIB_PATH, e))
  # the version first: a stale build (or another one picked through GEECO_LIB) must be named as such, not fail later on a
  # symbol or - worse - load with an entry point whose calling convention has changed
  try:
    lib.geeco_abi_version.restype = c_int
    have = int(lib.geeco_abi_version())
  except AttributeError:
    raise GeecoNativeError("%s is not a geeco_hip library (no geeco_abi_version)" % LIB_PATH)
  if have != ABI_VERSION:
    raise GeecoNativeError("ABI version mismatch: %s is version %d, this binding needs %d (rebuild: geeco_amd/csrc/build.sh)"
                           % (LIB_PATH, have, ABI_VERSION))
  for name, (res, args) in SIGNATURES.items():
    try:
      fn = getattr(lib, name)
    except AttributeError:
      raise GeecoNativeError("%s does not export %s (stale build?)" % (LIB_PATH, name))
    fn.restype = res
    fn.argtypes = args
  _lib = lib
  return lib


def check(rc: int, what: str):
  if rc != 0:
    msg = load().geeco_last_error()
    raise GeecoNativeError("%s failed (rc=%d): %s" % (what, rc, msg.decode() if msg else ''))
