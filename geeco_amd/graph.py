"""Model graphs of the E2E-VMC controllers on the HIP kernels.

Counterpart of the reference's ``src/models/e2evmc/graph.py``: ``dynimg`` (:30-55), ``conv_encoder``
(:61-117), ``state_concatenation`` / ``representation_concatenation[_v2]`` (:123-192),
``lstm_decoder`` (:198-260), ``e2e_vmc`` (:268-319), ``goal_e2evmc`` (:321-416) and the loss
functions (:430-500).  The reference builds a TF graph once and runs it per batch; here a model
object owns static HBM buffers (inputs, activations, gradients) for a fixed batch size and
``forward()`` / ``backward()`` enqueue the same sequence of HIP kernels every step, so a whole
train step can be captured into a hipGraph (geeco_amd/estimator.py).

Data layout in HBM: NHWC fp32 activations; the G encoders of a model ("ConvEncoder",
"DynBuffEncoder", "DynDiffEncoder") are stacked along a leading group axis and each layer is ONE
launch over all groups; RGB inputs are channel-padded to 4 so conv1 gathers float4 pixels.

This file holds the two training / evaluation models (``_ModelBase``, ``GoalE2EVMC``, ``E2EVMC``): inputs, the step and where the
optimiser runs in it.  Their parts live next door and are re-imported here, so ``graph.X`` names the same object: variable creation
order in variables.py, ``ConvEncoderStack`` in encoder.py, ``head_table`` / ``LSTMDecoder`` in decoder.py, the optimiser step
(``OptimizerStep``, which ``_ModelBase`` inherits) in optimizer.py, the one-frame predictors' ``E2EVMCStep`` / ``GoalE2EVMCStep`` in
step_models.py.
"""
from __future__ import annotations

import contextlib

import torch

from . import ops
from .attribution import Attributions
from .perturbation import Perturbations
from .decoder import LSTMDecoder, head_table  # noqa: F401
from .encoder import ConvEncoderStack, check_image_size
from .optimizer import OptimizerStep
from .step_models import E2EVMCStep, GoalE2EVMCStep  # noqa: F401
from .train_options import TrainOptions
from .variables import _CELLS, VariableStore, model_variable_shapes


def build_store(cfg, goal, device, ema=False):
  """The variable store of a model: TF's creation order, the encoders' blocks at a common stride; ``ema``: with the shadow arena."""
  shapes = model_variable_shapes(cfg, goal)
  encoder_scopes = sorted({n.split('/conv')[0] for n in shapes if '/conv' in n}, key=lambda sc: list(shapes).index(sc + '/conv1/kernel'))
  return VariableStore(shapes, device, uniform_scopes=encoder_scopes, ema=ema)


class BesideBottom:
  """The hand-off in front of the fused encoder bottom, the last and longest launch of the backward, which leaves room on every CU for
  streaming work (finding 38; numbers: ``_ModelBase.backward_and_apply``).  Use: ``run_bottom(bottom)``, the side work under ``with
  side_work():`` (the model's optimiser stream), ``join()``.  ``run_bottom`` calls ``bottom(before_bottom)`` and records an event on
  the main stream when conv2's filter gradient has been launched: everything before it, conv3's input gradient too (the last reader
  of a variable of the optimiser's early piece, conv3's kernel), precedes the event; released any earlier the side work could not
  co-reside (conv2's filter gradient and conv3's input gradient fill the register file) but would start first and delay them.  With
  ``sums`` (a list) the pending slab sum of that filter gradient moves there, to run with the side work: only conv1's stays behind
  the bottom.  A bottom without such a launch marks behind its chain (nothing to hide behind).
  The side work is launched BEHIND the fused bottom (and waits for the event, recorded in front of it): the bottom's packet is the
  older one, its 256 persistent blocks take their CUs first, and the streaming blocks then fill what those leave, one per CU at a
  time.  Issued in front of it (hipGraph replays nodes in creation order) the streaming blocks take the wave slots first, the
  bottom's block cannot become resident on a CU until they have drained, and the bottom ends 35-45 us late (measured)."""

  def __init__(self, model, sums=None):
    self.side, self.main = model.optimizer_stream(), torch.cuda.current_stream()
    self.sums, self.event, self.marked = sums, torch.cuda.Event(), False

  def _mark(self, pending=None):
    self.event.record(self.main)
    if pending and self.sums is not None:
      self.sums.extend(pending)
      del pending[:]
    self.marked = True

  def run_bottom(self, bottom):
    bottom(self._mark)
    if not self.marked:
      self._mark()

  @contextlib.contextmanager
  def side_work(self):
    self.side.wait_event(self.event)
    with torch.cuda.stream(self.side):
      yield

  def join(self):
    self.main.wait_stream(self.side)


class _ModelBase(OptimizerStep, Attributions, Perturbations):
  """Static input buffers shared by both controllers (feed contract: geeco_gym.py:375-398).  ``attributions()`` (integrated gradients,
  SmoothGrad), the loop around ``input_gradients()``, is attribution.Attributions'; ``perturbation_attributions()``
  (occlusion sensitivity, RISE), the loop around the forward alone, is perturbation.Perturbations'."""

  labels_missing = None      # set by load_batch

  def __init__(self, cfg, N, device, goal, training, store=None, shared_frames=None, options=None, **raw):
    self.cfg, self.N, self.goal, self.training = cfg, N, goal, training
    # the options: ``raw``, checked here once (train_options.py), or ``options``, a record checked already (for THIS config and these
    # variables: it is taken as it is).  The attributes the step reads are set from the record in _setup_optimizer
    if options is not None and raw:
      raise TypeError('options= is a checked record; it does not go with %s' % ', '.join(sorted(raw)))
    if options is None:
      names = store.shapes if store is not None else model_variable_shapes(cfg, goal)
      options = TrainOptions.from_raw(raw, cfg, names, training=training)
    self.options = options if training else options._replace(lr_multipliers=None, variable_stats_mode=None, grad_accum=None)
    self.shared_frames = self._check_shared_frames(cfg, goal, shared_frames)
    self.device = torch.device(device)
    self.K = cfg.window_size
    self.H, self.W, self.C = cfg.img_height, cfg.img_width, cfg.img_channels
    check_image_size(self.H, self.W)
    self.store = store or build_store(cfg, goal, self.device, ema=self.options.ema_decay is not None)
    if training and (self.options.ema_decay is None) != (self.store.ema is None):
      # the store decides which optimiser entry point runs (apply_gradients / apply_gradients_of): one that keeps averaged weights needs the
      # decay, and a decay without the arena would silently average nothing
      raise ValueError('ema_decay=%r, but the VariableStore %s (VariableStore(ema=True) goes with a decay in (0, 1))'
                       % (raw.get('ema_decay', self.options.ema_decay), 'keeps no averaged weights' if self.store.ema is None else 'keeps averaged weights'))
    f32 = dict(dtype=torch.float32, device=self.device)
    N, K, H, W = self.N, self.K, self.H, self.W
    F = self.shared_frames
    if F is not None:
      # shared frames: a table of F resident frames + the windows' slot indices stand in for the dense windows
      images = {'frame_table': torch.zeros(F, dtype=torch.int64, device=self.device),
                'frame_index': torch.zeros(N, K, dtype=torch.int32, device=self.device)}
      if goal:
        images['target_index'] = torch.zeros(N, dtype=torch.int32, device=self.device)
      self.frames_u8 = True     # the kind of the table's frames (uint8 / 255 or float32): fixed before the step is captured
    else:
      images = {'rgb': torch.zeros(N, K, H, W, 3, **f32)}
    self.inputs = {
        **images,
        'jnt_state': torch.zeros(N, K, cfg.dim_jnt_state, **f32),
        'ee_state': torch.zeros(N, K, 7, **f32),
        'obj_state': torch.zeros(N, K, 7, **f32),
    }
    if cfg.control_mode == 'cartesian':        # labels consumed by the losses (estimator.py:206-216, 230-236)
      self.label_keys = ['cmd']
      self.inputs['cmd'] = torch.zeros(N, 4, **f32)
    elif cfg.control_mode == 'velocity':
      self.label_keys = ['vel_target', 'ee_target', 'grp_target']
      self.inputs['vel_target'] = torch.zeros(N, cfg.dim_jnt_state, **f32)
      self.inputs['ee_target'] = torch.zeros(N, 7, **f32)
      self.inputs['grp_target'] = torch.zeros(N, cfg.dim_grp_command, **f32)
    else:
      raise ValueError("Unknown control mode '%s'" % (cfg.control_mode,))
    if self.options.loss_shaping is not None and self.options.loss_shaping['sample_weights']:      # tf.losses' weights=, one per sample
      self.label_keys.append('sample_weight')
      self.inputs['sample_weight'] = torch.ones(N, **f32)
    if self.C == 4:
      self.inputs['depth'] = torch.zeros(N, K, H, W, 1, **f32)
    if goal and F is None:
      self.inputs['target_rgb'] = torch.zeros(N, H, W, 3, **f32)
      if self.C == 4:
        self.inputs['target_depth'] = torch.zeros(N, H, W, 1, **f32)
    self._setup_optimizer(training)      # the options' attributes, scal, lr_runs / backward_cut, the clip and guard buffers (optimizer.py)
    self._opt_stream = None     # optimizer_stream()
    # GoalE2EVMC's branch and the control block of its one-pass input stage; the gather mode of a model that takes shared_frames
    self.mode = self.dyn_ws2 = self.window_mode = None
    # RGB-D: rgb || depth (estimator.py:36,169,172).  The dynimg branch of the goal model forms the concat inside its
    # input kernels (no packed copy of all N * K frames: 1.07 GB read + 1.43 GB written per step at K = 32); the other
    # graphs pack once per step.
    self.last_from_dynimg = True   # current frame's padded copy out of the buffer-image kernel (bench.py reads it)
    self.split_rgbd = self.C == 4 and goal and cfg.proc_obs == 'dynimg' and (H * W) % 4 == 0
    if self.C == 4 and not self.split_rgbd:
      self.obs4 = torch.empty(N, K, H, W, 4, **f32)
      if goal:
        self.tgt4 = torch.empty(N, H, W, 4, **f32)

  @staticmethod
  def _check_shared_frames(cfg, goal, shared_frames):
    """``shared_frames=F``: the encoder runs once per DISTINCT frame of the batch, F slots.  Returns F or None."""
    if shared_frames is None:
      return None
    F = int(shared_frames)
    if F < 1:
      raise ValueError('shared_frames=%r: the frame table needs at least one slot' % (shared_frames,))
    if goal and cfg.proc_obs == 'dynimg':
      raise ValueError("shared_frames: proc_obs='dynimg' encodes one frame and two dynamic images per window, nothing is shared "
                       "between windows")
    if goal and cfg.proc_tgt == 'dyndiff':
      raise ValueError("shared_frames: proc_tgt='dyndiff' encodes a (frame, target) pair image per window position; it would "
                       "need a second table")
    if cfg.img_channels == 4:
      raise ValueError('shared_frames: img_channels=4 (RGB-D) is not supported, depth is a separate float32 stream')
    return F

  def _encode_shared(self):
    """Shared-frame forward up to the decoder's states: pack the table's frames, encode the F slots once, gather."""
    N, K, F, d, inp = self.N, self.K, self.shared_frames, self.decoder, self.inputs
    ops.pack_frames_by_address_into(self.enc.x_in[0], inp['frame_table'], F, self.H * self.W, self.frames_u8)
    self.enc.forward()
    ops.window_states_fwd_into(d.states, self.enc.features[0], inp['frame_index'], inp['jnt_state'], self.window_mode, F, N, K, _CELLS,
                               self.feat_ch[0], self.cfg.dim_jnt_state, d.D, tgt_idx=inp.get('target_index'))

  def _scatter_shared(self):
    """Its adjoint: d(states) -> the gradient of the F slots' features (ReluGrad of conv8 applied)."""
    N, K, F, d, inp = self.N, self.K, self.shared_frames, self.decoder, self.inputs
    ops.window_states_bwd_into(self.enc.dfeatures[0], d.dstates, d.D, inp['frame_index'], self.enc.features[0], self.window_mode, F, N, K,
                               _CELLS, self.feat_ch[0], self.cfg.dim_jnt_state, tgt_idx=inp.get('target_index'))

  # image inputs this model can read as uint8 frames behind window addresses (feed.WindowFeed.pointers()) instead of dense
  # float32 windows; () = none
  u8_window_keys = ()

  def load_batch(self, features, labels=None):
    """Copies one batch into the static input buffers (H2D or D2D; torch is plumbing here)."""
    self.labels_missing = []      # the label inputs this batch left as they were (perturbation_attributions(score='loss') asks)
    for k, buf in self.inputs.items():
      if hasattr(buf, 'pointers'):
        raise RuntimeError("load_batch: input '%s' is fed through window addresses (input_fn.WindowFeed.feed)" % k)
      src = labels.get(k) if (labels is not None and k in self.label_keys) else features.get(k)
      if src is None:
        if k in self.label_keys:
          self.labels_missing.append(k)
          continue
        raise KeyError("missing feature '%s'" % k)
      src = torch.as_tensor(src)
      if tuple(src.shape) != tuple(buf.shape):
        raise ValueError("feature '%s': expected shape %s, got %s" % (k, tuple(buf.shape), tuple(src.shape)))
      buf.copy_(src, non_blocking=True)

  def _frames(self):
    """obs_frames / tgt_frame of the model_fn (estimator.py:30-39, 161-175): rgb, or rgb||depth packed to 4 channels."""
    N, K, HW = self.N, self.K, self.H * self.W
    if self.C == 3:
      return self.inputs['rgb'], self.inputs.get('target_rgb')
    ops.pack_pixels_into(self.obs4, self.inputs['rgb'], HW * 3, N * K, HW, 3, 4, self.inputs['depth'], HW, 1)
    if self.goal:
      ops.pack_pixels_into(self.tgt4, self.inputs['target_rgb'], HW * 3, N, HW, 3, 4, self.inputs['target_depth'], HW, 1)
      return self.obs4, self.tgt4
    return self.obs4, None

  def _pack_time_major(self, xs, frames, then=None):
    """xs[t] <- frames[:, t] channel-padded to 4, one launch per step (``then(t)``: what else step t's slot needs, right behind)."""
    N, K, HW, C = self.N, self.K, self.H * self.W, self.C
    for t in range(K):
      ops.pack_pixels_into(xs[t], frames[:, t], K * HW * C, N, HW, C, 4)
      if then is not None:
        then(t)

  def _concat_states(self, feats_of, **kw):
    """states[t] <- [feats_of(t) | jnt_t] per cell, one launch per step (state_concatenation / representation_concatenation,
    graph.py:123-167)."""
    N, K, jn, d = self.N, self.K, self.cfg.dim_jnt_state, self.decoder
    for t in range(K):
      ops.state_concat_fwd_into(d.states[t], feats_of(t), self.feat_ch, 1, self.inputs['jnt_state'][:, t], K * jn, jn, N, _CELLS, d.D, **kw)

  def _scatter_states(self, launches_of):
    """The adjoint: per step t one launch per (dfeats, feats, keywords) of ``launches_of(t)``, d(states[t]) -> feature gradients."""
    N, jn, d = self.N, self.cfg.dim_jnt_state, self.decoder
    for t in range(self.K):
      for dfeats, feats, kw in launches_of(t):
        ops.state_concat_bwd_into(dfeats, d.dstates[t], d.D, feats, self.feat_ch, 1, jn, N, _CELLS, **kw)

  def forward(self, backward_too=False):
    """Inputs -> encoder(s) -> decoder states (``_encode``, or the shared-frame form) -> decoder, heads and losses."""
    if backward_too:
      # A training forward opens a new optimiser step: a ``_prepared`` left over from a step whose apply_gradients never came
      # (an exception between the parts, a one-graph capture that failed after recording part 2, a caller that ran the backward
      # alone to look at gradients) must not make THIS step's apply_gradients skip its adam_prepare.
      self._prepared = False
      del self._clip_calls[:]      # ... nor may the pieces it had handed to apply_gradients_of(last=False) join this step's
      del self._open_pieces[:]
    if self.shared_frames is not None:
      self._encode_shared()
    else:
      self._encode()
    self.decoder.forward(backward_too)
    if self.cfg.l2_regularizer > 0.0:    # loss_reg = l2 * sum(v^2)/2 over every variable (graph.py:13-15, estimator.py:66,202)
      ops.sumsq_into(self.scal[1:2], self.store.params, self.store.size)

  def backward(self, part=None, adam_prepare=False, defer_sums=None, before_bottom=None):
    """part None = whole backward; 'upper' / 'bottom' = the two halves the data-parallel runner captures
    separately (runtime.py): everything down to conv3, then the encoder bottom (conv2 / conv1).  ``adam_prepare``: see
    _prepare_args (the optimiser's scalars ride in the slab-sum launch of the part it is passed to -- once per step).
    ``defer_sums`` (a list, part 'upper'): the part's pending slab sums are handed to the caller instead of launched (no
    ``adam_prepare`` then); ``before_bottom`` (part 'bottom'): ConvEncoderStack.backward_bottom.  Both are BesideBottom's.
    Under ``lr_multipliers`` the backward stops at ``backward_cut``: 'no_bottom' runs no ``enc.backward_bottom`` (conv3's input
    gradient has no consumer either), 'decoder_only' no encoder launch at all.  The gradient arena of a variable below the cut is NOT
    written (it keeps what it held); any other frozen variable has its gradient computed and simply not applied."""
    pending = []      # the slab sums of every layer of this call: ONE launch at the end
    if part != 'bottom':
      if self.shared_frames is not None:
        self.decoder.backward()
        self._scatter_shared()
      else:
        self._decoder_backward()      # ... down to the encoders' feature gradients
      if self.backward_cut != 'decoder_only':
        self.enc.backward_upper(pending)
      if defer_sums is not None:
        if part == 'upper':
          defer_sums.extend(pending)
          return
        adam_prepare = False
    if part != 'upper' and self.backward_cut == 'full':
      self.enc.backward_bottom(pending, before_bottom if part == 'bottom' else None)
    prepare = self._prepare_args(adam_prepare)
    if pending or prepare is not None:
      ops.slab_reduce_batch(pending, prepare)

  # -- input gradients: d(loss)/d(frames), for saliency maps ---------------------------------------------

  def _refuse_sparse_inputs(self, who, slot_reason, address_reason):
    """ValueError unless the model reads dense float32 windows: what ``who`` (a pass that takes gradients with respect to the image
    inputs, or writes into them) cannot serve, with its own reason for each of the two."""
    if self.shared_frames is not None:
      raise ValueError('%s: shared_frames encodes frame slots, not windows: %s; use a model with dense windows' % (who, slot_reason))
    bound = [k for k, buf in self.inputs.items() if hasattr(buf, 'pointers')]
    if bound:
      raise ValueError("%s: input%s %s bound as uint8 window addresses: %s; feed dense float32 windows"
                       % (who, 's' if len(bound) > 1 else '', ', '.join("'%s'" % k for k in bound), address_reason))

  def check_input_gradients(self):
    """ValueError, with the reason, unless ``input_gradients`` serves this model."""
    if not self.training:
      raise ValueError('input_gradients: the model was built with training=False and has no backward; build it with training=True')
    self._refuse_sparse_inputs('input_gradients', "a slot's gradient is the sum over every window that holds the frame",
                               'the gradient is taken with respect to float32 frames')
    if self.backward_cut != 'full':
      raise ValueError("input_gradients: backward_cut=%r (lr_multipliers froze the encoder bottom) stops the backward above conv2; "
                       "the pass needs the full backward" % (self.backward_cut,))
    self.enc.check_input_gradient()

  def input_gradients(self, chunk_frames=96):
    """d(loss)/d(image inputs) after ``forward(backward_too=True)`` and ``backward()``: a dict of device tensors shaped like the
    inputs -- 'rgb' [N][K][H][W][3], 'target_rgb' (goal models), 'depth' / 'target_depth' (RGB-D; views, with the rgb ones, of one
    4-channel buffer).  Every contribution of a frame is summed: its encoder pass, and each dynamic image it is part of.  Eager
    launches only; the optimiser is never called and no training buffer is written."""
    self.check_input_gradients()
    N, K, H, W, C, HW = self.N, self.K, self.H, self.W, self.C, self.H * self.W
    dev, f32 = self.device, dict(dtype=torch.float32, device=self.device)
    dx = self.enc.input_gradient(chunk_frames)
    # the frames as the forward read them ([N][K][HW][C]); the one-pass RGB-D stage kept no packed copy: pack one now
    if C == 4 and self.split_rgbd and getattr(self, 'obs4', None) is None:
      self.obs4, self.tgt4 = torch.empty(N, K, H, W, 4, **f32), torch.empty(N, H, W, 4, **f32)
    if C == 4 and self.split_rgbd:
      ops.pack_pixels_into(self.obs4, self.inputs['rgb'], HW * 3, N * K, HW, 3, 4, self.inputs['depth'], HW, 1)
      ops.pack_pixels_into(self.tgt4, self.inputs['target_rgb'], HW * 3, N, HW, 3, 4, self.inputs['target_depth'], HW, 1)
      frames, tgt = self.obs4, self.tgt4
    else:
      frames, tgt = (self.inputs['rgb'], self.inputs.get('target_rgb')) if C == 3 else (self.obs4, getattr(self, 'tgt4', None))
    if getattr(self, 'd_frames', None) is None:
      self.d_frames = torch.zeros(N, K, H, W, C, **f32)
      self.d_tgt = torch.zeros(N, H, W, C, **f32) if self.goal else None
      self.dyn_bwd_ws = ops.dynimg_bwd_ws(N, HW, C, dev)
    df, dt, sK = self.d_frames, self.d_tgt, K * HW * C
    pack_bwd = lambda dst, g, stride, acc=False: ops.pack_pixels_bwd_into(dst, g, stride, N, HW, C, 4, accumulate=acc)
    pair_bwd = lambda g, t, acc_tgt: ops.dynimg_bwd_into(df[:, t], g, frames[:, t], 2, N, HW, C, 4, self.dyn_bwd_ws, sK, 0, sK, 0,
                                                         accumulate=True, frames2=tgt, d_frames2=dt, accumulate2=acc_tgt)
    if self.mode == 'dynimg':             # geeco-f: x_in = [current frame | buffer image | pair image]
      ops.dynimg_bwd_into(df, dx[1], frames, K, N, HW, C, 4, self.dyn_bwd_ws, sK, HW * C, sK, HW * C)      # overwrites all K frames
      pair_bwd(dx[2], K - 1, False)
      pack_bwd(df[:, K - 1], dx[0], sK, True)
    elif self.mode == 'seq_dyndiff':      # encoder 0: the frames; encoder 1: the (frame t, target) pair images
      dxs = dx.view(2, K, N, H, W, 4)
      for t in range(K):
        pack_bwd(df[:, t], dxs[0][t], sK)
        pair_bwd(dxs[1][t], t, t > 0)
    else:                                 # per-frame controllers, time-major slots; the goal models' slot K = the target
      dxs = dx[0].view(-1, N, H, W, 4)
      for t in range(K):
        pack_bwd(df[:, t], dxs[t], sK)
      if self.goal:
        pack_bwd(dt, dxs[K], HW * C)
    out = {'rgb': df[..., :3]}
    if self.goal:
      out['target_rgb'] = dt[..., :3]
    if C == 4:
      out['depth'] = df[..., 3:]
      if self.goal:
        out['target_depth'] = dt[..., 3:]
    return out

  def _bind_labels(self):
    K, inp = self.K, self.inputs
    ee_last, obj_last = inp['ee_state'][:, K - 1], inp['obj_state'][:, K - 1]   # features[...][:, -1, :3]
    if self.cfg.control_mode == 'cartesian':
      cmd = inp['cmd']
      tg = [(cmd, 4), (cmd[:, 3:], 4), (ee_last, K * 7), (obj_last, K * 7)]
    else:
      tg = [(inp['vel_target'], inp['vel_target'].shape[1]), (inp['ee_target'], 7),
            (inp['grp_target'], inp['grp_target'].shape[1]), (ee_last, K * 7), (obj_last, K * 7)]
    self.decoder.targets = [t for t, _ in tg]
    self.decoder.target_strides = [s for _, s in tg]
    self.decoder.sample_weight = inp.get('sample_weight')

  def redirect_late_gradients(self, staging, late_ranges):
    return self.enc.redirect_late_gradients(staging, late_ranges)

  # -- optimiser step: optimizer.OptimizerStep; what follows places it in the backward ---------
  def can_apply_beside_bottom(self):
    """backward_and_apply needs a training encoder on a CUDA device, and a backward that has a bottom to hide the optimiser beside
    (``backward_cut`` 'full')."""
    return bool(self.enc.training and self.store.params.is_cuda and self.backward_cut == 'full')

  def optimizer_stream(self):
    """The second stream of backward_and_apply: the first of the training encoder's two streams (a process gets 4 hardware queues
    by default; a stream more would share one with another stream -- RCCL's, perhaps)."""
    if self._opt_stream is None:
      self._opt_stream = self.enc.sides[0] if self.enc.sides else torch.cuda.Stream(device=self.store.params.device)
    return self._opt_stream

  def bottom_handoff(self, sums=None):
    return BesideBottom(self, sums)

  def backward_and_apply(self, early, late, form=None):
    """Backward + optimiser step of a single-GPU training step with the optimiser's HBM-streaming work hidden beside the fused
    encoder-bottom backward (round 6, profiles/HARDWARE_FINDINGS.md 38).  ``early`` / ``late`` = runtime.gradient_buckets(store):
    late = conv1 / conv2 of the encoders, whose gradients the last launch of the backward produces; early = everything else
    (99.4 % of the arena), complete once conv3's filter gradient exists.

      main:  ... conv3 wgrad | conv3 dgrad | conv2 wgrad | * | conv2 dgrad + conv1 wgrad (454 us, MFMA-bound) | conv1's slab sum | join | Adam(late)
      side:                                                * -> slab sums of conv2..conv8 (+ lr_t) -> Adam(early)

    The fused bottom holds two 209-VGPR waves per SIMD and 151 KB of LDS: 80 registers per lane and 9 KB of LDS stay free on every
    CU, room for one block of the slab sums (55 VGPRs, 4 KB) or of Adam (51 VGPRs) at a time, and the bottom moves 1.1 TB/s of the
    8 the HBM has.  Beside it the 35 + 33 us of streaming work take 190 + 155 us and end long before its 455 us are over, which
    stay 455.  Where `*` sits and that the side launches are issued behind the bottom's: BesideBottom.  Element by element the
    arithmetic of backward(adam_prepare=True) + apply_gradients(): bitwise the same parameters, slots and gradients
    (tests/test_model_gpu.py).
    ``form`` (``grad_accum_steps``, DESIGN 5.23: 'first' / 'middle' / 'last'; None = the model without the option): the accumulate launch
    over each half takes Adam's place, and in the last form Adam follows it there, reading the accumulator; the step counter and lr_t
    are prepared in the last form alone."""
    g, sums = self.store.grads, []
    apply = form in (None, 'last')
    src = g if form is None else self.store.accum      # what the optimiser step reads

    def half(ranges, last):
      if form is not None:
        self.accumulate_gradients_of([(g[off:off + n], off, n) for off, n in ranges], overwrite=form == 'first')
      if apply:
        self.apply_gradients_of([(src[off:off + n], off, n) for off, n in ranges], last=last)

    h = self.bottom_handoff(sums)
    self.backward(part='upper', defer_sums=sums)
    prepare = self._prepare_args(apply)
    h.run_bottom(lambda mark: self.backward(part='bottom', before_bottom=mark))
    with h.side_work():
      ops.slab_reduce_batch(sums, prepare)
      half(early, False)
    h.join()
    half(late, True)

  def backward_accumulate_apply(self, form):
    """The plain order of a micro-step (``grad_accum_steps``), where there is no bottom to hide streaming work beside (shared frames, a
    cut backward): the backward, ONE accumulate launch, and in the last form the optimiser step on the accumulator."""
    self.backward(adam_prepare=form == 'last')
    self.accumulate_gradients_of([(self.store.grads, 0, self.store.size)], overwrite=form == 'first')
    if form == 'last':
      self.apply_gradients()

  def micro_step(self, buckets=None):
    """One eager micro-step of a model with ``grad_accum_steps`` on the batch in ``inputs``, in the form the store's count asks for;
    ``buckets`` = (early, late) of runtime.gradient_buckets: the beside-bottom layout, None: the plain one.  Returns True when it
    applied the optimiser step."""
    form = self.micro_step_form()
    self.forward(backward_too=True)
    if buckets is not None:
      self.backward_and_apply(buckets[0], buckets[1], form=form)
    else:
      self.backward_accumulate_apply(form)
    self._accumulate_losses(form)
    return self.micro_step_done(form)

  def _refresh_after_update(self):
    s = self.store
    # weights changed: re-derive the padded / transposed copies now (the version stamp is unchanged, so
    # the next forward, eager or replayed, launches no pad / transpose kernels).  A model that shares the store
    # with the primary training stack (the one built for a ragged final batch) must refresh THAT stack's copies
    # too: the primary relies on its own post-Adam refresh and would otherwise run one step on stale copies.
    self.enc.refresh_derived()
    if s.primary_stack is not None and s.primary_stack is not self.enc:
      s.primary_stack.refresh_derived()

  def predictions(self):
    """estimator.py:48-61 / 183-197."""
    return self.decoder.predictions()

  def check_device_errors(self):
    """Raises if a kernel of this model reported an error on the device (today: a block of the one-pass input stage that gave up
    waiting, csrc/dynimg_goal.hip).  SYNCHRONISES the stream: called where the host reads results anyway (Estimator's loss
    read-outs and epoch ends, bench.py's loss check, ``endpoints``), never inside the step."""
    if self.dyn_ws2 is not None and self.mode == 'dynimg':
      ops.check_input_stage(self.dyn_ws2, self.N)

  @property
  def loss(self):
    """Device scalar: total loss of the last forward (local batch mean + L2 term, estimator.py:101,239)."""
    l = self.decoder.losses[0]
    if self.cfg.l2_regularizer > 0.0:
      l = l + (0.5 * float(self.cfg.l2_regularizer)) * self.scal[1]
    return l

  def loss_parts(self):
    """The loss terms of the last forward; under ``grad_accum_steps`` their mean over the micro-batches of the last optimiser step
    (zeros before the first one; the regulariser is that of the weights the last micro-batch ran on, the group's)."""
    l = self.decoder.losses
    out = {'loss': self.loss}
    if self.grad_accum is not None:
      l = self.store.accum_loss_mean
      out['loss'] = l[0] + (0.5 * float(self.cfg.l2_regularizer)) * self.scal[1] if self.cfg.l2_regularizer > 0.0 else l[0]
    for i, (_, key, _, _, _) in enumerate(self.decoder.heads):
      out['loss_' + key.replace('logits_', '')] = l[1 + i]
    if self.cfg.l2_regularizer > 0.0:
      out['loss_reg'] = (0.5 * float(self.cfg.l2_regularizer)) * self.scal[1]
    return out

  def train_step(self):
    if self.grad_accum is not None:
      return self.micro_step()
    self.forward(backward_too=True)
    self.backward(adam_prepare=True)
    self.apply_gradients()


class GoalE2EVMC(_ModelBase):
  """``goal_e2evmc`` (graph.py:321-416), every proc_obs x proc_tgt branch (scope 'GoalVMC')."""

  def __init__(self, cfg, N, device, training=True, store=None, one_launch_decoder=False, shared_frames=None, **options):
    """``shared_frames=F`` ('sequence' x 'constant' / 'residual' only) and ``**options``: see E2EVMC."""
    super().__init__(cfg, N, device, goal=True, training=training, store=store, shared_frames=shared_frames, **options)
    if cfg.proc_tgt not in ('constant', 'residual', 'dyndiff'):
      raise ValueError("Unknown processing mode for target image: %s!" % (cfg.proc_tgt,))
    if cfg.proc_obs not in ('sequence', 'dynimg'):
      raise ValueError("Unknown processing mode for frame buffer: %s!" % (cfg.proc_obs,))
    root = 'GoalVMC'
    N, K, H, W, C = self.N, self.K, self.H, self.W, self.C
    jn = cfg.dim_jnt_state
    self.mode = cfg.proc_obs if cfg.proc_obs == 'dynimg' else 'seq_' + cfg.proc_tgt
    self.window_mode = cfg.proc_tgt
    if self.mode == 'dynimg':             # geeco-f (:386-407); proc_tgt is ignored by this branch
      scopes, Nf, T = [root + '/ConvEncoder', root + '/DynBuffEncoder', root + '/DynDiffEncoder'], N, 1
      self.feat_ch = [cfg.dim_s_obs, cfg.dim_s_dyn, cfg.dim_s_diff]
      dims = self.feat_ch
    elif self.mode in ('seq_constant', 'seq_residual'):   # target goes through the SAME ConvEncoder (:354, 364)
      scopes, Nf, T = [root + '/ConvEncoder'], self.shared_frames or (K + 1) * N, K
      self.feat_ch = [cfg.dim_s_obs, cfg.dim_s_obs] if self.mode == 'seq_constant' else [cfg.dim_s_obs]
      dims = [cfg.dim_s_obs]
    else:                                  # seq_dyndiff (:371-381)
      scopes, Nf, T = [root + '/ConvEncoder', root + '/DynDiffEncoder'], K * N, K
      self.feat_ch = [cfg.dim_s_obs, cfg.dim_s_diff]
      dims = self.feat_ch
    self.enc = ConvEncoderStack(self.store, scopes, Nf, H, W, C, dims, training)
    D = _CELLS * (sum(self.feat_ch) + jn)
    self.decoder = LSTMDecoder(self.store, root + '/LSTMDecoder', cfg, N, T, D, training, one_launch=one_launch_decoder, loss_shaping=self.loss_shaping)
    self._bind_labels()
    self._keep_accumulator()
    if self.shared_frames is None:      # (the shared-frame step forms no dynamic image)
      self.dyn_ws = ops.dynimg_ws(N, H * W * 4, self.device)
      self.dyn_ws2 = ops.goal_dynimgs_ws(N, H * W, self.device)      # control block of the one-pass input stage (zero-filled once)
    # geeco-f reads its K-frame window ONCE, in the input kernel: that kernel can take the episodes' resident uint8 frames
    # directly (RGB, or RGB of RGB-D with depth dense), see ops.goal_dynimgs_u8_into
    if self.mode == 'dynimg' and (H * W) % 4 == 0 and (C == 3 or self.split_rgbd):
      self.u8_window_keys = ('rgb', 'target_rgb')

  def _encode_dynimg_state(self):
    """The three encoders and representation_concatenation_v2: [obs | dyn | jnt | tgt] (graph.py:169-192) of the current
    step's joint state, jnt_state_list[-1] (:388); the concat rides in conv8's split-K epilogue where that exists."""
    N, K, jn, d = self.N, self.K, self.cfg.dim_jnt_state, self.decoder
    jnt = self.inputs['jnt_state'][:, K - 1]
    ch = self.feat_ch
    Ctot = sum(ch) + jn
    state = dict(state=d.states[0], state_stride=d.D, feat_off=[0, ch[0], ch[0] + ch[1] + jn], Ctot=Ctot, jnt=jnt,
                 jnt_stride=K * jn, jnt_off=ch[0] + ch[1], J=jn)
    if not self.enc.forward(state if len(set(ch)) == 1 else None):
      feats = self.enc.features                               # [3][N][2][2][256]
      ops.state_concat_fwd_into(d.states[0], [feats[0], feats[1], feats[2]], ch, 2, jnt, K * jn, jn, N, _CELLS, d.D)

  def _encode(self):
    N, K, H, W, C = self.N, self.K, self.H, self.W, self.C
    HW, x_in, inp = H * W, self.enc.x_in, self.inputs
    u8 = hasattr(inp['rgb'], 'pointers')          # estimator: the Estimator bound window addresses (uint8 frames)
    if u8 and not hasattr(inp['target_rgb'], 'pointers'):
      raise RuntimeError('GoalE2EVMC: rgb comes as window addresses but target_rgb as a dense tensor')
    if self.mode == 'dynimg' and (u8 or HW % 4 == 0):
      # g0: current frame, rgb_frame_list[-1] (graph.py:387);  g1: dynimg(buffer) (:392);  g2: dynimg([cur, tgt]) (:397-400)
      # ONE launch: the pass over the window has the current frame in registers (its channel-padded copy and the pair image come
      # from there) and keeps both images in registers across their per-sample min / max; RGB-D forms rgb || depth in there too
      kw = dict(depth=inp['depth'], tgt_depth=inp['target_depth'], dsample_stride=K * HW, dframe_stride=HW) if self.split_rgbd else {}
      if u8:
        ops.goal_dynimgs_u8_into(x_in[0], x_in[1], x_in[2], inp['rgb'].table, inp['target_rgb'].table, K, N, HW, self.dyn_ws2, **kw)
      else:
        ops.goal_dynimgs_into(x_in[0], x_in[1], x_in[2], inp['rgb'], inp['target_rgb'], K, N, HW, self.dyn_ws2, K * HW * 3, HW * 3, **kw)
      self._encode_dynimg_state()
      return
    frames, tgt = self._frames()
    if self.mode == 'dynimg':             # (HW % 4 != 0: three launches)
      cur = frames[:, K - 1]
      ops.pack_pixels_into(x_in[0], cur, K * HW * C, N, HW, C, 4)
      ops.dynimg_into(x_in[1], frames, K, N, HW, C, 4, self.dyn_ws, K * HW * C, HW * C)
      ops.dynimg_into(x_in[2], cur, 2, N, HW, C, 4, self.dyn_ws, K * HW * C, 0, frames2=tgt)
      self._encode_dynimg_state()
    elif self.mode in ('seq_constant', 'seq_residual'):
      xs = x_in[0].view(K + 1, N, H, W, 4)                    # time-major; slot K = target frame
      self._pack_time_major(xs, frames)
      ops.pack_pixels_into(xs[K], tgt, HW * C, N, HW, C, 4)
      self.enc.forward()
      feats = self.enc.features[0].view(K + 1, N, _CELLS, self.feat_ch[0])
      if self.mode == 'seq_constant':     # representation_concatenation: [obs | jnt | tgt] (:146-167, 367)
        self._concat_states(lambda t: [feats[t], feats[K]])
      else:                               # state_concatenation(tgt_feat - feat, jnt) (:369-370)
        self._concat_states(lambda t: [feats[t]], sub_from=feats[K])
    else:                                 # seq_dyndiff
      xs = x_in.view(2, K, N, H, W, 4)
      self._pack_time_major(xs[0], frames, then=lambda t: ops.dynimg_into(xs[1][t], frames[:, t], 2, N, HW, C, 4, self.dyn_ws,
                                                                          K * HW * C, 0, frames2=tgt))      # :373-376
      self.enc.forward()
      f = [self.enc.features[g].view(K, N, _CELLS, self.feat_ch[g]) for g in range(2)]
      self._concat_states(lambda t: [f[0][t], f[1][t]])       # representation_concatenation(feat, tgt_feat, jnt) (:381)

  def _decoder_backward(self):
    N, K, jn, d = self.N, self.K, self.cfg.dim_jnt_state, self.decoder
    if self.mode == 'dynimg':
      feats, dfe = self.enc.features, self.enc.dfeatures
      cc = dict(feats=[feats[0], feats[1], feats[2]], dfeats=[dfe[0], dfe[1], dfe[2]], feat_ch=self.feat_ch, jnt_pos=2, J=jn,
                cells=_CELLS)
      if not d.backward(concat=cc):
        ops.state_concat_bwd_into(cc['dfeats'], d.dstates[0], d.D, cc['feats'], self.feat_ch, 2, jn, N, _CELLS)
      return
    d.backward()
    if self.mode in ('seq_constant', 'seq_residual'):
      ch = self.feat_ch[0]
      feats = self.enc.features[0].view(K + 1, N, _CELLS, ch)
      dfe = self.enc.dfeatures[0].view(K + 1, N, _CELLS, ch)
      if self.mode == 'seq_constant':
        self._scatter_states(lambda t: [([dfe[t], None], [feats[t], feats[K]], {}),
                                        ([None, dfe[K]], [feats[t], feats[K]], dict(accumulate=t > 0))])
      else:   # d(tgt - feat): -1 into feat_t, +1 (summed over the window) into the target features
        self._scatter_states(lambda t: [([dfe[t]], [feats[t]], dict(scale=-1.0)),
                                        ([dfe[K]], [feats[K]], dict(accumulate=t > 0, scale=1.0))])
    else:
      f = [self.enc.features[g].view(K, N, _CELLS, self.feat_ch[g]) for g in range(2)]
      df = [self.enc.dfeatures[g].view(K, N, _CELLS, self.feat_ch[g]) for g in range(2)]
      self._scatter_states(lambda t: [([df[0][t], df[1][t]], [f[0][t], f[1][t]], {})])

  def endpoints(self):
    """dynbuff / dyndiff debug endpoints (graph.py:377,393,401): the LAST computed images."""
    C, K, N = self.C, self.K, self.N
    self.check_device_errors()
    ep = {'conv8': self.enc.features}
    if self.mode == 'dynimg':
      ep['dynbuff'] = self.enc.x_in[1][..., :C]
      ep['dyndiff'] = self.enc.x_in[2][..., :C]
    elif self.mode == 'seq_dyndiff':
      ep['dyndiff'] = self.enc.x_in.view(2, K, N, self.H, self.W, 4)[1][K - 1][..., :C]
    return ep


class E2EVMC(_ModelBase):
  """``e2e_vmc`` (graph.py:268-319): per-frame encoder, K LSTM steps (scope 'VMC')."""

  def __init__(self, cfg, N, device, training=True, store=None, one_launch_decoder=False, shared_frames=None, **options):
    """``**options``: the training options by their public names (``train_options.TrainOptions`` documents them and
    ``train_options.EXCLUSIONS`` what they do not go with), or ``options=`` a record checked already.
    ``shared_frames=F``: the inputs are 'frame_table' [F] (int64 addresses of resident RGB frames, 0 = unused slot) and
    'frame_index' [N][K] (int32, window position -> slot) in place of 'rgb' (device_windows.DeviceWindows.frame_table); the encoder
    runs on the F slots once, forward and backward, instead of on all K * N window positions.  Same variables, same loss and
    gradients up to summation order."""
    super().__init__(cfg, N, device, goal=False, training=training, store=store, shared_frames=shared_frames, **options)
    N, K, H, W, C = self.N, self.K, self.H, self.W, self.C
    self.window_mode, self.feat_ch = 'plain', [256]
    # frames are processed time-major ([K][N]) so that step t's features are one dense block
    self.enc = ConvEncoderStack(self.store, ['VMC/ConvEncoder'], self.shared_frames or K * N, H, W, C, 256, training)
    D = _CELLS * (256 + cfg.dim_jnt_state)
    self.decoder = LSTMDecoder(self.store, 'VMC/LSTMDecoder', cfg, N, K, D, training, one_launch=one_launch_decoder, loss_shaping=self.loss_shaping)
    self._bind_labels()
    self._keep_accumulator()

  def _encode(self):
    N, K, H, W = self.N, self.K, self.H, self.W
    frames, _ = self._frames()
    self._pack_time_major(self.enc.x_in[0].view(K, N, H, W, 4), frames)
    self.enc.forward()
    feats = self.enc.features[0].view(K, N, _CELLS, 256)
    self._concat_states(lambda t: [feats[t]])     # state_concatenation (graph.py:123-144)

  def _decoder_backward(self):
    N, K = self.N, self.K
    self.decoder.backward()
    feats = self.enc.features[0].view(K, N, _CELLS, 256)
    dfe = self.enc.dfeatures[0].view(K, N, _CELLS, 256)
    self._scatter_states(lambda t: [([dfe[t]], [feats[t]], {})])

  def endpoints(self):
    return {'conv8': self.enc.features}
