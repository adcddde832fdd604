"""Thin tensor-level wrappers over the C-ABI (geeco_amd/_native.py), one submodule per kernel family.

PyTorch is plumbing only: tensors own device memory, ``torch.cuda.current_stream()`` provides the
HIP stream.  Every function enqueues HIP kernels from libgeeco_hip.so on that stream.

Callers write ``from geeco_amd import ops`` / ``ops.X(...)``: this namespace is what they read (and what a test or a recorder
patches).  The submodules import ``_marshal`` and ``_native`` only (``conv`` also ``optim``, for the schedule form of
``slab_reduce_batch``) and never this file; a call from one ops function to another does not pass through this namespace --
except ``VariableStatsPlan.run``, which the optimiser calls and whose ``variable_stats`` launch a recorder must see: the class
lives here.
"""
import torch

from .. import _native
from .._native import PREDICT_FEAT_MODES, REPLAY_CLASS_HIT, REPLAY_SQUARED_ERROR, check
from ._marshal import _lib, _p, _stream, _ws, same_out
from .input_stage import (check_input_stage, dynimg, dynimg_alpha, dynimg_bwd_into, dynimg_bwd_ws, dynimg_into, dynimg_rgbd_into,
                          dynimg_ws, goal_dynimgs_into, goal_dynimgs_timeouts, goal_dynimgs_u8_into, goal_dynimgs_ws,
                          pack_pixels_bwd_into, pack_pixels_into)
from .windows import (gather_windows_augmented_into, gather_windows_by_address_into, gather_windows_frames_into, gather_windows_into,
                      gather_windows_scene_into, pack_frames_by_address_into, window_states_bwd_into, window_states_fwd_into)
from .predict_io import (predict_pack_into, predict_pack_newest_into, predict_push_dense_into, predict_push_features_into,
                         predict_push_ring_into, predict_range_check_into)
from .replay_ops import (replay_errors_into, replay_images_into, replay_images_ws, replay_states_into, replay_states_pair_into)
from .attr_ops import attr_accumulate_into, attr_finish_into, attr_path_point_into
from .perturb_ops import (perturb_accumulate_into, perturb_apply_into, perturb_desc, perturb_finish_into, perturb_patch,
                          perturb_score_into, perturb_steps)
from .conv import (conv1_dgrad_into, conv1_fwd_relu_bits_into, conv1_fwd_relu_bits_rgb_into, conv2_dgrad_conv1_wgrad_bits_into,
                   conv2_dgrad_conv1_wgrad_into, conv2_dgrad_conv1_wgrad_ws_bytes, conv2_fwd_relu_fields_into,
                   conv3_dgrad_relu_fields_into, conv3_fwd_relu_fields_into, conv3x3, conv3x3_dgrad, conv3x3_dgrad_into,
                   conv3x3_dgrad_needs_wt, conv3x3_dgrad_relu_fields_into, conv3x3_dgrad_relu_fields_supported,
                   conv3x3_dgrad_ws_bytes, conv3x3_fwd_into, conv3x3_fwd_state_into, conv3x3_fwd_ws_bytes, conv3x3_wgrad,
                   conv3x3_wgrad_into, conv3x3_wgrad_pair_into, conv3x3_wgrad_ws_bytes, conv_top_bwd_into, derive_conv_weights,
                   kernel_trace, pad_mid_into, relu_bits_pitch, relu_bits_rows, relu_fields_elems, slab_reduce_batch,
                   transpose_hwio_into)
from .decoder_ops import (colsum_into, gemm, gemm_into, gemm_ws_bytes, heads_loss_into, heads_ws_bytes, loss_shaping,
                          lstm_gates_bwd_into, lstm_gates_fwd_into, lstm_input_step_fwd_into, lstm_seq_heads_into,
                          lstm_step_bwd_into, lstm_step_bwd_ws_bytes, lstm_step_heads_into, state_concat_bwd_into,
                          state_concat_fwd_into)
from .optim import (adam_prepare, adam_prepare_schedule, adam_tf, adam_tf_ema, adam_tf_segments, adam_tf_segments_clip,
                    adam_tf_segments_ema, adam_tf_segments_guard, adam_tf_segments_scaled, clip_scale, clip_ws_floats,
                    grad_accumulate_segments, grad_sumsq_segments, guard_decide, lr_schedule_eval, lr_schedule_struct, sumsq_into)
from .varstats_ops import VARSTATS_DTYPE, variable_stats, variable_stats_table, variable_stats_ws_bytes


class VariableStatsPlan:
  """What one model's statistics pass keeps on the device: the table of ``variables`` = [(offset, count)], the workspace and the
  records.  Allocated once; ``run`` enqueues the two launches and allocates nothing."""

  def __init__(self, variables, device):
    self.variables = [(int(o), int(c)) for o, c in variables]
    host = variable_stats_table(self.variables)
    self.nchunks = (host.size - 2 * len(self.variables)) // 2
    self.table = torch.from_numpy(host).to(device)
    self.ws = torch.zeros(variable_stats_ws_bytes(self.nchunks) // 4, dtype=torch.int32, device=device)
    self.out = torch.zeros(len(self.variables) * VARSTATS_DTYPE.itemsize, dtype=torch.uint8, device=device)

  def run(self, p, m, v, segments, n, grad_scale=1.0, eps=1e-8):
    variable_stats(self.out, self.ws, self.table, p, m, v, segments, n, self.variables, self.nchunks, grad_scale, eps)

  def records(self):
    """The records on the host (numpy, VARSTATS_DTYPE).  SYNCHRONISES: the copy waits for the stream."""
    return self.out.cpu().numpy().view(VARSTATS_DTYPE).copy()
