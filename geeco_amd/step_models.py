"""Inference-only step forms of the per-frame controllers, one frame per call with the encoder features of the older frames cached
on the device: ``E2EVMCStep``, ``GoalE2EVMCStep`` (batched_predictor.py, incremental=True)."""
from __future__ import annotations

import torch

from . import ops
from .decoder import LSTMDecoder
from .encoder import ConvEncoderStack, check_image_size
from .variables import _CELLS, VariableStore, model_variable_shapes


class _StepModelBase:
  """The per-frame controllers one frame at a time (batched_predictor.py, incremental=True).

  A window's state_t depends on frame t alone (conv_encoder sees one frame, graph.py:61-117) and the LSTM starts from the zero
  state on every call, so the features of the K - 1 older frames of a sliding window are the previous calls' features.  Per env
  a ring of the last K feature vectors [cells][ch] and joint states lives in HBM; ``step`` encodes only the N new frames
  (``ConvEncoderStack(Nf = N)``), pushes them, gathers every env's window oldest first into the decoder's states [K][N][D] and
  runs the decoder (T = K).  Same ``VariableStore`` layout as the full model: checkpoints restore unchanged.  There is no
  [N][K][H][W][C] window and no K * N-frame activation buffer."""

  def __init__(self, cfg, N, device, goal, scope, ch, mode, training=False, store=None, one_launch_decoder=False):
    if training:
      raise ValueError('%s is inference-only: training=True needs the full model (E2EVMC / GoalE2EVMC)' % type(self).__name__)
    self.cfg, self.N, self.goal, self.training = cfg, N, goal, False
    self.device = torch.device(device)
    self.K = cfg.window_size
    self.H, self.W, self.C = cfg.img_height, cfg.img_width, cfg.img_channels
    check_image_size(self.H, self.W)
    shapes = model_variable_shapes(cfg, goal)
    self.store = store or VariableStore(shapes, self.device, uniform_scopes=[scope + '/ConvEncoder'])
    self.ch, self.feat_mode = ch, mode
    N, K, jn = self.N, self.K, cfg.dim_jnt_state
    self.enc = ConvEncoderStack(self.store, [scope + '/ConvEncoder'], N, self.H, self.W, self.C, ch, False)
    D = _CELLS * (ch + jn + (ch if mode == 'constant' else 0))
    self.decoder = d = LSTMDecoder(self.store, scope + '/LSTMDecoder', cfg, N, K, D, False, one_launch=one_launch_decoder)
    f32 = dict(dtype=torch.float32, device=self.device)
    d.states.zero_()
    # the heads kernel of the step chain computes loss terms beside the predictions: zero labels nobody reads (the one-launch
    # decoder does not touch them)
    width = max(8, max(h[2] for h in d.heads))
    self._no_labels = torch.zeros(N, width, **f32)
    d.targets = [self._no_labels] * len(d.heads)
    d.target_strides = [width] * len(d.heads)
    self.feat_ring = torch.zeros(N, K, _CELLS, ch, **f32)
    self.jnt_ring = torch.zeros(N, K, jn, **f32)
    self.heads = torch.zeros(N, dtype=torch.int32, device=self.device)
    self.tgt_feat = torch.zeros(N, _CELLS, ch, **f32) if mode != 'plain' else None

  u8_window_keys = ()

  def step(self, frames, jnt, reset, ctl):
    """One control step of N envs, all on the device: frames [N][H][W][C] (float32, or uint8 RGB), jnt [N][J], reset [N] int32,
    ctl [N + 1] int32 (ctl[N] != 0: a frame failed the range check, no ring moves)."""
    N, K, HW, d = self.N, self.K, self.H * self.W, self.decoder
    ops.predict_pack_newest_into(self.enc.x_in[0], frames, N, HW, self.C)
    self.enc.forward()
    ops.predict_push_features_into(d.states, self.feat_ring, self.jnt_ring, self.heads, self.enc.features[0], jnt, reset, ctl,
                                   self.feat_mode, N, K, _CELLS, self.ch, self.cfg.dim_jnt_state, d.D, tgt_feat=self.tgt_feat)
    d.forward(False)

  def forward(self, backward_too=False):
    raise RuntimeError('%s has no window to run forward() on: call step(frames, jnt, reset, ctl)' % type(self).__name__)

  def predictions(self):
    return self.decoder.predictions()

  def check_device_errors(self):
    pass

  def endpoints(self):
    return {'conv8': self.enc.features}


class E2EVMCStep(_StepModelBase):
  """``e2e_vmc`` one frame per call: state_t = [feat_t | jnt_t] per cell (state_concatenation, graph.py:123-144)."""

  def __init__(self, cfg, N, device, training=False, store=None, one_launch_decoder=False):
    super().__init__(cfg, N, device, False, 'VMC', 256, 'plain', training, store, one_launch_decoder)


class GoalE2EVMCStep(_StepModelBase):
  """``goal_e2evmc`` with proc_obs 'sequence' one frame per call.  proc_tgt 'constant': [feat_t | jnt_t | tgt_feat]
  (representation_concatenation, graph.py:146-167); 'residual': [tgt_feat - feat_t | jnt_t] -- the ring holds feat_t and the
  subtraction happens in the gather, so a new goal changes every state of the window exactly.  The target's features are
  computed when the goal is set (``encode_targets``), not per call."""

  def __init__(self, cfg, N, device, training=False, store=None, one_launch_decoder=False):
    if cfg.proc_obs != 'sequence':
      raise ValueError("incremental mode caches per-frame encoder features: proc_obs='%s' has none (three encoder passes per call "
                       "whatever the window size)" % (cfg.proc_obs,))
    if cfg.proc_tgt not in ('constant', 'residual'):
      raise ValueError("incremental mode does not take proc_tgt='%s': the cached DynDiff features depend on the goal, a goal "
                       "change needs the K raw frames encoded again" % (cfg.proc_tgt,))
    super().__init__(cfg, N, device, True, 'GoalVMC', cfg.dim_s_obs, cfg.proc_tgt, training, store, one_launch_decoder)
    self.mode = 'seq_' + cfg.proc_tgt

  def encode_targets(self, tgt_frames, env_ids):
    """tgt_feat rows of the envs ``env_ids`` (index tensor on the device) <- the encoder's features of tgt_frames
    [len(env_ids)][H][W][C] (float32 on the device).  Runs eagerly, through the step's own encoder launches (Nf = N: the other
    rows encode whatever the input buffer holds); the input and activation buffers are scratch that every step rewrites."""
    n = len(env_ids)
    x = self.enc.x_in[0]
    packed = torch.empty(n, self.H, self.W, 4, dtype=torch.float32, device=self.device)
    ops.predict_pack_newest_into(packed, tgt_frames.contiguous(), n, self.H * self.W, self.C)
    x[env_ids] = packed
    self.enc.forward()
    self.tgt_feat[env_ids] = self.enc.features[0].view(self.N, _CELLS, self.ch)[env_ids]
