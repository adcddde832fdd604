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

The pass.  Per chunk of at most ``chunk_frames`` frames ``ops.replay_images_into`` (csrc/replay_dynimg.hip) writes the conv1 inputs
straight from the resident frames into the inputs of one inference ``ConvEncoderStack`` per encoder scope (geeco-f: ConvEncoder,
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

import numpy as np

from . import ops
from .params import create_e2evmc_config
from .replay import ACTIVATION_BUDGET, EpisodeReplay, activation_bytes_per_frame, checkpoint_is_goal, error_heads, recorded_labels
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


class DynamicImageReplay:
  """geeco-f and goal_e2evmc 'sequence' x 'dyndiff' (RGB) over whole recorded episodes."""

  def __init__(self, model_dir, checkpoint_name=None, use_ema=False, device=None, max_frames=512, chunk_frames=None,
               chunk_windows=None, goal=None, cfg=None):
    """Restores ``model_dir``'s checkpoint, builds one inference encoder stack per encoder scope at ``chunk_frames`` frames (default:
    ``default_chunk_frames``) and ONE decoder at ``chunk_windows`` windows per launch (default min(max_frames, 256)), and allocates
    every buffer once.  ``goal`` / ``cfg`` as ``EpisodeReplay`` takes them (these models are all goal models)."""
    import torch
    from . import estimator as est
    from .batched_predictor import _Layout
    from .decoder import LSTMDecoder
    from .encoder import ConvEncoderStack, check_image_size
    from .variables import VariableStore, model_variable_shapes
    if cfg is None:
      cfg = create_e2evmc_config(load_model_config(model_dir, 'e2evmc_config'))
    if goal is None:
      goal = checkpoint_is_goal(model_dir, checkpoint_name)
    self.cfg, self.goal = cfg, bool(goal)
    self.kind, scopes, dims = check_dynimg_replay_config(cfg, self.goal)
    self.max_frames = int(max_frames)
    if self.max_frames < 1:
      raise ValueError('max_frames must be >= 1, got %r' % (max_frames,))
    F = default_chunk_frames(cfg, dims, self.max_frames) if chunk_frames is None else int(chunk_frames)
    W = min(self.max_frames, 256) if chunk_windows is None else int(chunk_windows)
    if not 1 <= F <= 65535 or W < 1:
      raise ValueError('chunk_frames=%r must lie in 1..65535 and chunk_windows=%r be >= 1' % (chunk_frames, chunk_windows))
    check_image_size(cfg.img_height, cfg.img_width)
    self.K, self.J, self.HW = cfg.window_size, cfg.dim_jnt_state, cfg.img_height * cfg.img_width
    if self.HW % 4:
      raise ValueError('episode replay: %d x %d pixels: the image stage reads four pixels at a time (H * W %% 4 == 0)' % (cfg.img_height, cfg.img_width))
    if not torch.cuda.is_available():
      raise RuntimeError('geeco_amd episode replay needs an MI355X (no CPU fallback)')
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    if dev.index is None:
      dev = torch.device('cuda', torch.cuda.current_device())
    self.device, self.chunk_frames, self.chunk_windows, self.dims = dev, F, W, dims
    K, J, M, H, Wd = self.K, self.J, self.max_frames, cfg.img_height, cfg.img_width
    # every table holds whole decoder launches: the geeco-f state rows are always built chunk_windows at a time
    Mp = -(-M // W) * W
    f32 = dict(dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
      self.store = VariableStore(model_variable_shapes(cfg, True), dev)
      est.restore_for_inference(self.store, model_dir, checkpoint_name, use_ema=use_ema)
      self.encs = [ConvEncoderStack(self.store, [sc], F, H, Wd, 3, ch, False) for sc, ch in zip(scopes, dims)]
      self.K_dec = 1 if self.kind == 'dynimg' else K
      D = _CELLS * (sum(dims) + J)
      self.decoder = d = LSTMDecoder(self.store, 'GoalVMC/LSTMDecoder', cfg, W, self.K_dec, D, False, one_launch=True)
      d.states.zero_()
      # one step: the decoder's one-step chain computes loss terms beside the predictions; zero labels nobody reads (replay.py)
      width = max(8, max(h[2] for h in d.heads))
      no_labels = torch.zeros(W, width, **f32)
      d.targets, d.target_strides = [no_labels] * len(d.heads), [width] * len(d.heads)
      self.heads = [(key, off, size) for (_, key, size, _, _), (off, _, _) in zip(d.heads, error_heads(cfg))]
      self._err_heads = error_heads(cfg)
      P, nh = d.OT, len(d.heads)
      self.tables = [torch.zeros(Mp, _CELLS, ch, **f32) for ch in dims]
      self.ws = ops.replay_images_ws(F, self.HW, dev)
      self._h_addr = torch.zeros(M, dtype=torch.int64, pin_memory=True)
      self._d_addr = torch.zeros(M, dtype=torch.int64, device=dev)
      self._goal_in = {np.dtype(np.uint8): torch.zeros(1, self.HW, 3, dtype=torch.uint8, device=dev),
                       np.dtype(np.float32): torch.zeros(1, self.HW, 3, **f32)}
      up, down = _Layout(), _Layout()
      up.add('jnt', (Mp, J), np.float32)
      up.add('labels', (M, P), np.float32)
      down.add('preds', (M, P), np.float32)
      down.add('errors', (M, nh), np.float32)
      down.add('episode', (nh,), np.float32)
      self._h_up, self._h_down = (torch.zeros(l.size, dtype=torch.uint8, pin_memory=True) for l in (up, down))
      self._d_up, self._d_down = (torch.zeros(l.size, dtype=torch.uint8, device=dev) for l in (up, down))
      self._hu, self._du, self._hd, self._dd = up.host(self._h_up), up.device(self._d_up), down.host(self._h_down), down.device(self._d_down)
      self._dense = {}      # frames of dense host episodes, per dtype (EpisodeReplay._frames_on_device)
      torch.cuda.synchronize(dev)

  # the episode's frames and the goal frame come in exactly as EpisodeReplay takes them
  _frames_on_device = EpisodeReplay._frames_on_device
  _goal_on_device = EpisodeReplay._goal_on_device

  def replay(self, episode, goal_frame=None, labels=True, return_images=False):
    """The controller's commands over one episode: arguments, result keys, 'errors' and 'episode_errors' as ``EpisodeReplay.replay``.
    ``return_images``: also the dynamic images the model saw at every frame, under the keys of the predictors' ``debug_images``:
    'dyndiff' [T][H][W][3] (the pair image of frame t and the goal) and, for geeco-f, 'dynbuff' [T][H][W][3] (the buffer image of the
    window ending at t); they are gathered in device buffers allocated by that call.  Everything is queued on the current stream; the
    host reads once, at the end."""
    import torch
    if isinstance(episode, (tuple, list)):
      episode = {'rgb': episode[0], 'jnt_state': episode[1]}
    F, W, K, J, HW = self.chunk_frames, self.chunk_windows, self.K, self.J, self.HW
    H, Wd = self.cfg.img_height, self.cfg.img_width
    geeco_f = self.kind == 'dynimg'
    with torch.cuda.device(self.device):
      frames, T, u8 = self._frames_on_device(episode['rgb'])
      if T < 1:
        raise ValueError('episode replay: an episode needs at least one frame')
      if T > self.max_frames:
        raise ValueError('episode replay: the episode holds %d frames, this replay was built for max_frames=%d' % (T, self.max_frames))
      if frames.data_ptr() % (4 if u8 else 16):
        raise ValueError('episode replay: frames at an address that is no multiple of %d' % (4 if u8 else 16))
      jnt = np.asarray(episode['jnt_state'], dtype=np.float32)
      if jnt.shape != (T, J):
        raise ValueError('episode replay: jnt_state must be [%d, %d], got %s' % (T, J, jnt.shape))
      if goal_frame is None:
        goal_frame = episode.get('target_rgb')
      if goal_frame is None:
        raise ValueError("episode replay: a goal model needs goal_frame= (or the episode's 'target_rgb')")
      goal_dev = self._goal_on_device(goal_frame)
      if (goal_dev.dtype == torch.uint8) != u8:
        raise ValueError('episode replay: the goal frame is %s but the frames are %s: the pair image reads both as one kind'
                         % (goal_dev.dtype, frames.dtype))
      lab = None
      if labels is not False and labels is not None:
        lab = recorded_labels(self.cfg, episode if labels is True else labels, T)
      # one upload: the frames' addresses; joint states and recorded values
      self._h_addr[:T].copy_(torch.from_numpy(frames.data_ptr() + np.arange(T, dtype=np.int64) * (HW * 3 * (1 if u8 else 4))))
      self._d_addr.copy_(self._h_addr, non_blocking=True)
      self._hu['jnt'][:T] = jnt
      if lab is not None:
        self._hu['labels'][:T] = lab
      self._d_up.copy_(self._h_up, non_blocking=True)
      images = {}
      if return_images:
        images['dyndiff'] = torch.empty(T, HW, 3, dtype=torch.float32, device=self.device)
        if geeco_f:
          images['dynbuff'] = torch.empty(T, HW, 3, dtype=torch.float32, device=self.device)
      # the conv1 inputs of every frame, then every encoder once per chunk
      x = [e.x_in[0].view(F, HW, 4) for e in self.encs]
      for c0 in range(0, T, F):
        c1 = min(c0 + F, T)
        ops.replay_images_into(x[0], x[1] if geeco_f else None, x[-1], self._d_addr, goal_dev, T, c0, c1, K, HW, self.ws)
        for e, table, ch in zip(self.encs, self.tables, self.dims):
          e.forward()
          table[c0:c1].copy_(e.features[0].view(F, _CELLS, ch)[:c1 - c0])
        if return_images:
          images['dyndiff'][c0:c1].copy_(x[-1][:c1 - c0, :, :3])
          if geeco_f:
            images['dynbuff'][c0:c1].copy_(x[1][:c1 - c0, :, :3])
      # the windows, chunk_windows per decoder launch (always the full launch: rows past the last window keep what they held)
      d, preds, jnt_dev = self.decoder, self._dd['preds'], self._du['jnt']
      for w0 in range(0, T, W):
        w1 = min(w0 + W, T)
        if geeco_f:      # one state row per frame: [obs | dyn | jnt | diff] (graph.py: _encode_dynimg_state)
          ops.state_concat_fwd_into(d.states[0], [t[w0:w0 + W] for t in self.tables], self.dims, 2, jnt_dev[w0:w0 + W], J, J, W, _CELLS, d.D)
        else:
          ops.replay_states_pair_into(d.states, self.tables[0], self.tables[1], jnt_dev, T, w0, w1, K, _CELLS, self.dims[0], self.dims[1], J)
        d.forward(False)
        preds[w0:w1].copy_(d.preds[:w1 - w0])
      if lab is not None:
        ops.replay_errors_into(self._dd['errors'], self._dd['episode'], preds, self._du['labels'], T, self._err_heads)
      self._h_down.copy_(self._d_down, non_blocking=True)      # the one read
      torch.cuda.current_stream().synchronize()
      images = {k: v.cpu().numpy().reshape(T, H, Wd, 3) for k, v in images.items()}
    out = {key: self._hd['preds'][:T, off:off + size].copy() for key, off, size in self.heads}
    if lab is not None:
      out['errors'] = self._hd['errors'][:T].copy()
      out['episode_errors'] = {key: float(self._hd['episode'][i]) for i, (key, _, _) in enumerate(self.heads)}
    out.update(images)
    return out
