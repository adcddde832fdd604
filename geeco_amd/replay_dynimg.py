"""Episode replay for the dynamic-image controllers: geeco-f (``proc_obs='dynimg'``) and ``proc_obs='sequence'`` x
``proc_tgt='dyndiff'`` over whole recorded episodes, with the contract of ``replay.EpisodeReplay`` (5.27).

Why these models can be replayed at all.  ``EpisodeReplay`` refuses them because "a dynamic image belongs to its window".  With the
goal fixed for the episode, as replay fixes it, that costs less than it sounds (graph.py:386-407 of the reference):
  geeco-f             per frame t three conv1 inputs -- the frame, the pair image dynimg([frame_t, goal]) and the buffer image of the
                      window ending at t -- and ONE LSTM step: nothing is encoded K times, and the episode is encoded in a few
                      launches at many frames instead of T batch-1 calls;
  'sequence' x 'dyndiff'   the pair image dynimg([frame_j, goal]) depends on frame j alone, so the ConvEncoder feature and the
                      DynDiffEncoder feature of a frame are shared by the K windows that hold it, exactly like 5.27's table.
The window at frame t is what the reference predictor holds after a reset at frame 0 and t pushes (``replay.window_frames``).

The pass is ``replay.ReplayPass``, shared with ``EpisodeReplay``; what this class adds.  Per chunk of at most ``chunk_frames``
frames ``ops.replay_images_into`` (csrc/replay_dynimg.hip) writes the conv1 inputs straight from the resident frames into the inputs of one inference ``ConvEncoderStack`` per encoder scope (geeco-f: ConvEncoder,
DynBuffEncoder, DynDiffEncoder; 'sequence': ConvEncoder, DynDiffEncoder), whose features go into tables [frames][cells][ch].  Per
``chunk_windows`` windows the decoder's states are built -- geeco-f: ``ops.state_concat_fwd_into`` over the three tables, one row
per frame, [obs | dyn | jnt | diff]; 'sequence': ``ops.replay_states_pair_into``, [obs | jnt | diff] for K steps -- and the decoder
runs: the one-launch K-step decoder for 'sequence'; for geeco-f, whose decoder has ONE step, the one-step path every T = 1
``LSTMDecoder`` takes (the gate GEMM and one per-sample launch), which is also what the geeco-f predictor runs.

Frame 0 of a ``proc_obs='dynimg'`` model.  After a reset the buffer holds K copies of frame 0 and the coefficients sum to zero, so
the raw buffer image is float32 rounding residue (exactly 0 at K <= 3) and the normalised image is that residue divided by its own
range: the reference's own behaviour, reproduced bit for bit from the same arithmetic as the predictors', but not something a
float64 model of the network predicts (DESIGN 5.29 has the measured ranges).  Row 0 is what a stepped predictor returns after
``reset()``; treat it as such.
"""
from __future__ import annotations

from . import ops
from .params import create_e2evmc_config
from .replay import ACTIVATION_BUDGET, EpisodeReplay, ReplayPass, activation_bytes_per_frame, checkpoint_is_goal
from .utils import load_model_config
from .variables import _CELLS


def check_dynimg_replay_config(cfg, goal):
  """(kind, encoder scopes, conv8 widths) of a model ``DynamicImageReplay`` serves: kind 'dynimg' (geeco-f: goal models with
  proc_obs='dynimg', whatever proc_tgt -- that branch of the dense model ignores it) or 'seq_dyndiff' (goal models with
  proc_obs='sequence' and proc_tgt='dyndiff').  ValueError for the others, before any allocation."""
  if cfg.img_channels != 3:
    raise ValueError('episode replay: img_channels=%d: replay reads resident RGB frames (img_channels=3); depth is a separate float32 '
                     'stream' % (cfg.img_channels,))
  if not goal:
    raise ValueError('episode replay: e2e_vmc has no goal and forms no dynamic image: EpisodeReplay serves it')
  if cfg.proc_tgt not in ('constant', 'residual', 'dyndiff'):
    raise ValueError("Unknown processing mode for target image: %s!" % (cfg.proc_tgt,))
  root = 'GoalVMC'
  if cfg.proc_obs == 'dynimg':
    return ('dynimg', [root + '/ConvEncoder', root + '/DynBuffEncoder', root + '/DynDiffEncoder'],
            [int(cfg.dim_s_obs), int(cfg.dim_s_dyn), int(cfg.dim_s_diff)])
  if cfg.proc_obs == 'sequence' and cfg.proc_tgt == 'dyndiff':
    return 'seq_dyndiff', [root + '/ConvEncoder', root + '/DynDiffEncoder'], [int(cfg.dim_s_obs), int(cfg.dim_s_diff)]
  if cfg.proc_obs == 'sequence':
    raise ValueError("episode replay: proc_obs='sequence', proc_tgt='%s' is a per-frame controller: EpisodeReplay serves it (one encoder "
                     "pass per frame, no dynamic image)" % (cfg.proc_tgt,))
  raise ValueError("Unknown processing mode for frame buffer: %s!" % (cfg.proc_obs,))


def serves_dynamic_images(cfg, goal):
  """Whether ``DynamicImageReplay`` (True) or ``EpisodeReplay`` (False) is the class for this config; a config neither serves goes to
  ``EpisodeReplay``, whose refusal says why."""
  return bool(goal) and cfg.img_channels == 3 and (cfg.proc_obs == 'dynimg' or (cfg.proc_obs == 'sequence' and cfg.proc_tgt == 'dyndiff'))


def default_chunk_frames(cfg, dims, max_frames, budget=ACTIVATION_BUDGET):
  """The frames one chunk takes by default: every encoder scope has a stack of its own at ``chunk_frames`` frames, so the budget is
  divided by the number of stacks; at most ``max_frames``, at least 1."""
  per_stack = budget // len(dims)
  return int(max(1, min(max_frames, min(per_stack // activation_bytes_per_frame(cfg, ch) for ch in dims))))


def open_replay(model_dir, checkpoint_name=None, goal=None, cfg=None, **kw):
  """The replay class that serves ``model_dir``'s config -- ``DynamicImageReplay`` for geeco-f and 'sequence' x 'dyndiff',
  ``EpisodeReplay`` for the per-frame controllers (and for the configs neither serves: its refusal says why) -- built with ``kw``
  (use_ema, device, max_frames, chunk_frames, chunk_windows)."""
  if cfg is None:
    cfg = create_e2evmc_config(load_model_config(model_dir, 'e2evmc_config'))
  if goal is None:
    goal = checkpoint_is_goal(model_dir, checkpoint_name)
  cls = DynamicImageReplay if serves_dynamic_images(cfg, goal) else EpisodeReplay
  return cls(model_dir, checkpoint_name, goal=goal, cfg=cfg, **kw)


class DynamicImageReplay(ReplayPass):
  """geeco-f and goal_e2evmc 'sequence' x 'dyndiff' (RGB) over whole recorded episodes: one encoder stack per encoder scope, their
  conv1 inputs written by the image stage (these models are all goal models)."""

  pad_tables = True      # the geeco-f state rows are always built chunk_windows at a time

  def _check_config(self):
    self.kind, scopes, dims = check_dynimg_replay_config(self.cfg, self.goal)
    return scopes, dims

  def _default_chunk_frames(self, dims):
    return default_chunk_frames(self.cfg, dims, self.max_frames)

  def _check_image(self):
    if self.HW % 4:
      raise ValueError('episode replay: %d x %d pixels: the image stage reads four pixels at a time (H * W %% 4 == 0)'
                       % (self.cfg.img_height, self.cfg.img_width))

  def _decoder_shape(self):
    # geeco-f's decoder has ONE step: the one-step path every T = 1 LSTMDecoder takes, which is also what its predictor runs
    self.K_dec = 1 if self.kind == 'dynimg' else self.K
    return self.K_dec, _CELLS * (sum(self.dims) + self.J)

  def _allocate(self):
    import torch
    self.ws = ops.replay_images_ws(self.chunk_frames, self.HW, self.device)
    self._h_addr = torch.zeros(self.max_frames, dtype=torch.int64, pin_memory=True)
    self._d_addr = torch.zeros(self.max_frames, dtype=torch.int64, device=self.device)

  def _check_inputs(self, frames, u8, goal_dev):
    import torch
    if frames.data_ptr() % (4 if u8 else 16):
      raise ValueError('episode replay: frames at an address that is no multiple of %d' % (4 if u8 else 16))
    if (goal_dev.dtype == torch.uint8) != u8:
      raise ValueError('episode replay: the goal frame is %s but the frames are %s: the pair image reads both as one kind'
                       % (goal_dev.dtype, frames.dtype))

  def replay(self, episode, goal_frame=None, labels=True, return_images=False):
    """The controller's commands over one episode: arguments, result keys, 'errors' and 'episode_errors' as ``EpisodeReplay.replay``.
    ``return_images``: also the dynamic images the model saw at every frame, under the keys of the predictors' ``debug_images``:
    'dyndiff' [T][H][W][3] (the pair image of frame t and the goal) and, for geeco-f, 'dynbuff' [T][H][W][3] (the buffer image of the
    window ending at t); they are gathered in device buffers allocated by that call.  Everything is queued on the current stream; the
    host reads once, at the end."""
    return self._pass(episode, goal_frame, labels, return_images)

  def _encode(self, addr, T, u8, goal_dev, return_images):
    import torch
    F, HW = self.chunk_frames, self.HW
    self._h_addr[:T].copy_(torch.from_numpy(addr))
    self._d_addr.copy_(self._h_addr, non_blocking=True)
    # the conv1 inputs of every frame, then every encoder once per chunk; x[-1] is the pair image, x[1] geeco-f's buffer image
    x = [e.x_in[0].view(F, HW, 4) for e in self.encs]
    shown = {'dyndiff': x[-1], 'dynbuff': x[1]} if self.kind == 'dynimg' else {'dyndiff': x[-1]}
    images = {k: torch.empty(T, HW, 3, dtype=torch.float32, device=self.device) for k in shown} if return_images else {}
    for c0 in range(0, T, F):
      c1 = min(c0 + F, T)
      ops.replay_images_into(x[0], shown.get('dynbuff'), x[-1], self._d_addr, goal_dev, T, c0, c1, self.K, HW, self.ws)
      for e, table, ch in zip(self.encs, self.tables, self.dims):
        e.forward()
        table[c0:c1].copy_(e.features[0].view(F, _CELLS, ch)[:c1 - c0])
      for k, v in images.items():
        v[c0:c1].copy_(shown[k][:c1 - c0, :, :3])
    return images

  def _build_states(self, w0, w1, T):
    d, W, J, jnt = self.decoder, self.chunk_windows, self.J, self._du['jnt']
    if self.kind == 'dynimg':      # one state row per frame: [obs | dyn | jnt | diff] (graph.py: _encode_dynimg_state)
      ops.state_concat_fwd_into(d.states[0], [t[w0:w0 + W] for t in self.tables], self.dims, 2, jnt[w0:w0 + W], J, J, W, _CELLS, d.D)
    else:
      ops.replay_states_pair_into(d.states, self.tables[0], self.tables[1], jnt, T, w0, w1, self.K, _CELLS, self.dims[0], self.dims[1], J)
