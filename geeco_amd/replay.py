"""Episode replay: what a trained per-frame controller would have commanded at EVERY frame of a recorded episode, and how far
that is from what was recorded.

Semantics.  The window at frame ``t`` of a T-frame episode is what the reference predictor holds after a reset at frame 0 followed
by ``t`` pushes (src/models/e2evmc/predictor.py:192-200, :144-146): slot ``k`` (oldest first) shows frame ``max(0, t - K + 1 + k)``
and the joint-state rows follow the same index (``window_frames``).  A goal model's target frame is constant over the episode and
comes from the caller, as ``set_goal`` takes it.  So ``replay`` returns, row for row, what a batch-1 predictor stepped through the
episode after ``reset()`` returns -- without the per-frame graph replay and round trip, and with every frame encoded ONCE.
``ReplayPass`` is that pass, shared with the dynamic-image controllers (replay_dynimg.py): validate, one upload, the
frames into feature tables, per ``chunk_windows`` windows the decoder's states and the decoder, the errors, one read.  What
``EpisodeReplay`` adds: the T frames go through ``ops.pack_frames_by_address_into`` and one ``ConvEncoderStack`` in chunks of at most ``chunk_frames`` frames, their
features wait in a table [T][cells][ch], ``ops.replay_states_into`` builds the decoder's states of up to ``chunk_windows`` windows per
launch from it (csrc/replay.hip) and the one-launch K-step decoder (``LSTMDecoder(one_launch=True)``) runs on them.

Recorded values.  The recorded value of frame ``t`` is the label ``pickplace_input_fn`` pairs with the window ENDING at ``t``:
``episode_windows`` (input_fn.py) takes ``labels[key][start + K - 1]`` of the per-frame arrays ``_finish_episode`` leaves, i.e.
``cmd[t]`` / ``ctrl[t]`` as recorded at frame t and the NEXT frame's states as targets, ``vel_target[t] = vel_state[t + 1]``,
``ee_target[t] = ee_state[t + 1]``, ``grp_target[t] = grp_state[t + 1]`` (the episode's last recorded frame is dropped, so every
kept frame has a successor).  The heads read them as the model's ``_bind_labels`` does (estimator.py:206-216, 230-236 of the
reference): cartesian ``cmd_ee = cmd[t][:3]``, gripper class ``rint(cmd[t][3]) + 1``; velocity ``cmd_vel = vel_target[t]``,
``cmd_ee = ee_target[t][:3]``, ``cmd_grp = grp_target[t]``; both ``pos_ee = ee_state[t][:3]``, ``pos_obj = obj_state[t][:3]`` (the
window's last frame, ``features[...][:, -1, :3]``).  The frames ``t < K - 1``, whose window is padded, have no training window; they
take the same rule.  Heads and their column layout come from ``decoder.head_table``.

Errors (``ops.replay_errors_into``): per frame and regression head the mean over the head's columns of the squared difference; for
the gripper logits 1.0 where the argmax (first maximum) is the recorded class, else 0.0; per head the mean over the frames.

Refused: the dynamic-image variants (``proc_obs='dynimg'``, ``proc_tgt='dyndiff'``) -- a dynamic image belongs to its window, so
nothing is shared between windows; ``Estimator.predict`` on dense windows serves them -- and RGB-D models.
"""
from __future__ import annotations

import os

import numpy as np

from . import ops
from .decoder import head_table
from .params import create_e2evmc_config
from .utils import load_model_config
from .variables import _CELLS, ENC_FILTERS, ENC_STRIDES

TOL_FRAME_RANGE = 1e-6      # the predictors' tolerance on fed float frames (predictor.py:18)
ACTIVATION_BUDGET = 2 << 30      # bytes of encoder activations the default chunk may take


def window_frames(T, K):
  """int64 [T][K]: the frame slot k (oldest first) of the window at frame t shows, ``max(0, t - K + 1 + k)``."""
  t, k = np.arange(T, dtype=np.int64)[:, None], np.arange(K, dtype=np.int64)[None, :]
  return np.maximum(t - K + 1 + k, 0)


def check_replay_config(cfg, goal):
  """(variable scope, feature channels, state mode) of a model replay serves; ValueError for the others, before any allocation."""
  if cfg.img_channels != 3:
    raise ValueError('episode replay: img_channels=%d: replay reads resident RGB frames (img_channels=3); depth is a separate float32 '
                     'stream' % (cfg.img_channels,))
  if not goal:
    return 'VMC', 256, 'plain'
  if cfg.proc_obs != 'sequence' or cfg.proc_tgt not in ('constant', 'residual'):
    raise ValueError("episode replay: proc_obs='%s', proc_tgt='%s': replay encodes every frame once and shares its features between "
                     "the windows that hold it, but a dynamic image (proc_obs='dynimg', proc_tgt='dyndiff') belongs to its window, so "
                     "nothing is shared between windows; Estimator.predict on dense windows serves these models"
                     % (cfg.proc_obs, cfg.proc_tgt))
  return 'GoalVMC', int(cfg.dim_s_obs), cfg.proc_tgt


def activation_bytes_per_frame(cfg, ch):
  """Bytes of one frame in an inference ``ConvEncoderStack``: the channel-padded input and the eight layers' outputs."""
  h, w = cfg.img_height, cfg.img_width
  total = h * w * 4
  for cout, s in zip(list(ENC_FILTERS) + [ch], ENC_STRIDES):
    h, w = ops.same_out(h, s), ops.same_out(w, s)
    total += h * w * cout
  return 4 * total


def default_chunk_frames(cfg, ch, max_frames, budget=ACTIVATION_BUDGET):
  """The frames one encoder pass takes by default: what ``budget`` bytes of activations hold, at most ``max_frames`` (+ 1 slot: a
  goal model's target frame rides in the first chunk) and at least 1."""
  return int(max(1, min(max_frames + 1, budget // activation_bytes_per_frame(cfg, ch))))


def recorded_labels(cfg, episode, T):
  """float32 [T][P]: the recorded values of the T frames in the heads' columns (module docstring), the gripper class as an index in
  the first column of its head.  ``episode``: per-frame arrays as ``load_episode`` returns them."""
  def col(key, n):
    if key not in episode:
      raise ValueError("episode replay: labels need the per-frame array '%s' of the episode (or pass labels=False)" % key)
    a = np.asarray(episode[key], dtype=np.float32)
    if a.ndim != 2 or a.shape[0] < T or a.shape[1] < n:
      raise ValueError("episode replay: '%s' of shape %s for %d frames of >= %d values" % (key, a.shape, T, n))
    return a[:T, :n]
  heads = head_table(cfg)
  out = np.zeros((T, sum(h[2] for h in heads)), np.float32)
  if cfg.control_mode == 'cartesian':
    cmd = col('cmd', 4)
    src = {'cmd_ee': cmd[:, :3], 'logits_cmd_grp': np.rint(cmd[:, 3:4]) + 1.0}      # tf.math.rint: round half to even, as np.rint
  else:
    src = {'cmd_vel': col('vel_target', cfg.dim_jnt_state), 'cmd_ee': col('ee_target', 3), 'cmd_grp': col('grp_target', cfg.dim_grp_command)}
  src['pos_ee'], src['pos_obj'] = col('ee_state', 3), col('obj_state', 3)
  off = 0
  for _, key, size, _, _ in heads:
    out[:, off:off + src[key].shape[1]] = src[key]
    off += size
  return out


def error_heads(cfg):
  """(first column, columns, kind) per head for ``ops.replay_errors_into``."""
  out, off = [], 0
  for _, _, size, kind, _ in head_table(cfg):
    out.append((off, size, ops.REPLAY_CLASS_HIT if kind == 1 else ops.REPLAY_SQUARED_ERROR))
    off += size
  return out


def checkpoint_is_goal(model_dir, checkpoint_name=None):
  """Whether the checkpoint holds goal_e2evmc's variables ('GoalVMC/...') or e2e_vmc's ('VMC/...')."""
  import torch
  from . import estimator as est
  ckpt = os.path.join(model_dir, checkpoint_name) if checkpoint_name else est.latest_checkpoint(model_dir)
  if ckpt is None:
    raise FileNotFoundError('no checkpoint in %s' % model_dir)
  if os.path.exists(ckpt + '.pt'):
    names = list(torch.load(ckpt + '.pt', map_location='cpu')['names'])
  else:
    from . import tf_checkpoint
    names = list(tf_checkpoint.read_checkpoint(ckpt))
  return any(n.startswith('GoalVMC/') for n in names)


def _resident_frames(x, what):
  """A DeviceWindows of one episode, a device tensor or a host array -> the frames as they are (tensor or array)."""
  from .device_windows import DeviceWindows
  if isinstance(x, DeviceWindows):
    if len(x.segments) != 1 or x.augment is not None:
      raise ValueError("episode replay: '%s' must be the windows of ONE resident episode as recorded (got %d segments%s)"
                       % (what, len(x.segments), ', augmented' if x.augment is not None else ''))
    frames, _, divisor = x.segments[0]
    if frames is None:
      raise RuntimeError("episode replay: the '%s' stream was not uploaded (device_keys excluded it)" % what)
    import torch
    if (frames.dtype, divisor) not in ((torch.uint8, 255.0), (torch.float32, 1.0)):
      raise ValueError("episode replay: '%s' frames of type %s with divisor %g are neither the uint8 (255) nor the float32 (1) form"
                       % (what, frames.dtype, divisor))
    return frames
  return x


class ReplayPass:
  """What every replay class shares: the restored store, one inference encoder stack per encoder scope with its feature table
  [frames][cells][ch], ONE decoder, every buffer allocated once, and the pass itself (``_pass``).  A subclass supplies the models it
  serves (``_check_config``), the decoder's shape (``_decoder_shape``), its own buffers (``_allocate``), the frames' way into the
  tables (``_encode``) and the decoder's states of a range of windows (``_build_states``)."""

  pad_tables = False      # tables and joint states padded to whole decoder launches of chunk_windows rows

  def __init__(self, model_dir, checkpoint_name=None, use_ema=False, device=None, max_frames=512, chunk_frames=None,
               chunk_windows=None, goal=None, cfg=None):
    """Restores ``model_dir``'s checkpoint (``restore_for_inference``), builds one inference encoder stack per encoder scope at
    ``chunk_frames`` frames (default: the class's ``default_chunk_frames``, from the activation footprint) and ONE decoder at
    ``chunk_windows`` windows per launch (default min(max_frames, 256)), and allocates every buffer once.  ``goal``: goal_e2evmc
    (True) or e2e_vmc (False); None reads it off the checkpoint's variable names.  ``cfg``: the model's config instead of
    ``model_dir``/e2evmc_config.json."""
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
    scopes, dims = self._check_config()
    self.max_frames = int(max_frames)
    if self.max_frames < 1:
      raise ValueError('max_frames must be >= 1, got %r' % (max_frames,))
    F = self._default_chunk_frames(dims) if chunk_frames is None else int(chunk_frames)
    W = min(self.max_frames, 256) if chunk_windows is None else int(chunk_windows)
    if not 1 <= F <= 65535 or W < 1:
      raise ValueError('chunk_frames=%r must lie in 1..65535 and chunk_windows=%r be >= 1' % (chunk_frames, chunk_windows))
    H, Wd = cfg.img_height, cfg.img_width
    check_image_size(H, Wd)
    self.K, self.J, self.HW = cfg.window_size, cfg.dim_jnt_state, H * Wd
    self._check_image()
    if not torch.cuda.is_available():
      raise RuntimeError('geeco_amd episode replay needs an MI355X (no CPU fallback)')
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    if dev.index is None:
      dev = torch.device('cuda', torch.cuda.current_device())
    self.device, self.chunk_frames, self.chunk_windows, self.dims = dev, F, W, dims
    J, M = self.J, self.max_frames
    rows = -(-M // W) * W if self.pad_tables else M
    f32 = dict(dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
      self.store = VariableStore(model_variable_shapes(cfg, self.goal), dev)
      est.restore_for_inference(self.store, model_dir, checkpoint_name, use_ema=use_ema)
      self.encs = [ConvEncoderStack(self.store, [sc], F, H, Wd, 3, ch, False) for sc, ch in zip(scopes, dims)]
      steps, D = self._decoder_shape()
      self.decoder = d = LSTMDecoder(self.store, ('GoalVMC' if self.goal else 'VMC') + '/LSTMDecoder', cfg, W, steps, D, False, one_launch=True)
      d.states.zero_()
      # one step: the decoder's one-step chain computes loss terms beside the predictions; zero labels nobody reads (step_models.py)
      width = max(8, max(h[2] for h in d.heads))
      no_labels = torch.zeros(W, width, **f32)
      d.targets, d.target_strides = [no_labels] * len(d.heads), [width] * len(d.heads)
      self.heads = [(key, off, size) for (_, key, size, _, _), (off, _, _) in zip(d.heads, error_heads(cfg))]
      self._err_heads = error_heads(cfg)
      P, nh = d.OT, len(d.heads)
      self.tables = [torch.zeros(rows, _CELLS, ch, **f32) for ch in dims]
      self._goal_in = {np.dtype(np.uint8): torch.zeros(1, self.HW, 3, dtype=torch.uint8, device=dev),
                       np.dtype(np.float32): torch.zeros(1, self.HW, 3, **f32)} if self.goal else {}
      self._allocate()
      # what one replay uploads beside the frames (joint states, recorded values) and downloads (predictions, errors)
      up, down = _Layout(), _Layout()
      up.add('jnt', (rows, J), np.float32)
      up.add('labels', (M, P), np.float32)
      down.add('preds', (M, P), np.float32)
      down.add('errors', (M, nh), np.float32)
      down.add('episode', (nh,), np.float32)
      self._h_up, self._h_down = (torch.zeros(l.size, dtype=torch.uint8, pin_memory=True) for l in (up, down))
      self._d_up, self._d_down = (torch.zeros(l.size, dtype=torch.uint8, device=dev) for l in (up, down))
      self._hu, self._du, self._hd, self._dd = up.host(self._h_up), up.device(self._d_up), down.host(self._h_down), down.device(self._d_down)
      self._dense = {}      # frames of dense host episodes, per dtype: [max_frames][HW * 3], allocated on the first such episode
      torch.cuda.synchronize(dev)

  # -- what a subclass supplies (the first two before any allocation; the rest with self.device current) -------------------------
  def _check_config(self):
    """(encoder scopes, their conv8 widths) of ``self.cfg`` / ``self.goal``, or the ValueError that says what is not served."""
    raise NotImplementedError

  def _default_chunk_frames(self, dims):
    raise NotImplementedError

  def _check_image(self):
    """Further conditions on the image size."""

  def _decoder_shape(self):
    """(steps, input width) of the decoder."""
    raise NotImplementedError

  def _allocate(self):
    """The class's own buffers."""

  def _check_inputs(self, frames, u8, goal_dev):
    """Further conditions on the resident frames and the goal frame of one episode."""

  def _encode(self, addr, T, u8, goal_dev, return_images):
    """Every frame once: ``addr`` (int64 [T], the frames' device addresses) -> rows [0, T) of ``self.tables``.  Returns the device
    tensors [T][HW][3] to hand back as images, by key."""
    raise NotImplementedError

  def _build_states(self, w0, w1, T):
    """The decoder's states of the windows [w0, w1) -> rows [0, w1 - w0) of ``self.decoder.states``."""
    raise NotImplementedError

  # -- inputs ------------------------------------------------------------------------------------------------------------------
  def _frames_on_device(self, rgb):
    """``rgb`` -> (device tensor of T contiguous [HW * 3] frames, T, uint8?).  Host arrays are copied into a buffer kept per dtype."""
    import torch
    H, W = self.cfg.img_height, self.cfg.img_width
    rgb = _resident_frames(rgb, 'rgb')
    if isinstance(rgb, torch.Tensor):
      if rgb.dtype not in (torch.uint8, torch.float32):
        raise ValueError('episode replay: frames must be uint8 or float32, got %s' % (rgb.dtype,))
      if rgb.dim() < 2 or rgb[0].numel() != self.HW * 3 or not rgb.is_contiguous():
        raise ValueError('episode replay: frames of shape %s, expected contiguous [T, %d, %d, 3]' % (tuple(rgb.shape), H, W))
      T = int(rgb.shape[0])
      if rgb.device != self.device:
        if rgb.is_cuda:
          raise RuntimeError('episode replay: episode frames live on %s but are read on %s' % (rgb.device, self.device))
        return self._frames_on_device(rgb.numpy())
      if rgb.dtype == torch.float32 and rgb.data_ptr() % 4:
        raise ValueError('episode replay: float32 frames at an address that is no multiple of 4')
      return rgb, T, rgb.dtype == torch.uint8
    a = np.asarray(rgb)
    if a.dtype not in (np.dtype(np.uint8), np.dtype(np.float32)):
      raise ValueError('episode replay: frames must be uint8 or float32, got %s' % (a.dtype,))
    if a.ndim != 4 or a.shape[1:] != (H, W, 3):
      raise ValueError('episode replay: frames of shape %s, expected [T, %d, %d, 3]' % (a.shape, H, W))
    T = int(a.shape[0])
    if T > self.max_frames:
      raise ValueError('episode replay: the episode holds %d frames, this replay was built for max_frames=%d' % (T, self.max_frames))
    if a.dtype == np.float32 and T:
      lo, hi = float(np.amin(a)), float(np.amax(a))
      if not (-TOL_FRAME_RANGE <= lo and hi <= 1 + TOL_FRAME_RANGE):      # (a NaN fails too)
        raise ValueError('episode replay: frames exceed range! Expected %s, got %s!' % ((0 - TOL_FRAME_RANGE, 1 + TOL_FRAME_RANGE), (lo, hi)))
    if a.dtype not in self._dense:
      self._dense[a.dtype] = torch.zeros(self.max_frames, self.HW * 3, dtype=torch.uint8 if a.dtype == np.uint8 else torch.float32,
                                         device=self.device)
    buf = self._dense[a.dtype]
    if T:
      buf[:T].copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(T, -1)))
    return buf, T, a.dtype == np.uint8

  def _goal_on_device(self, goal_frame):
    """The target frame ([H, W, >=3]; uint8, or floats in [0, 1]) as a device tensor [1][HW][3] of its own dtype."""
    import torch
    H, W = self.cfg.img_height, self.cfg.img_width
    g = _resident_frames(goal_frame, 'target_rgb')
    if isinstance(g, torch.Tensor):
      if g.numel() != self.HW * 3 or g.dtype not in (torch.uint8, torch.float32):
        raise ValueError('episode replay: the goal frame must be one uint8 or float32 [%d, %d, 3] frame, got %s %s' % (H, W, g.dtype, tuple(g.shape)))
      buf = self._goal_in[np.dtype(np.uint8 if g.dtype == torch.uint8 else np.float32)]
      buf.copy_(g.reshape(1, self.HW, 3))
      return buf
    g = np.asarray(g)
    if g.ndim != 3 or g.shape[:2] != (H, W) or g.shape[2] < 3:
      raise ValueError('episode replay: the goal frame must be [%d, %d, >=3], got %s' % (H, W, g.shape))
    g = np.ascontiguousarray(g[..., :3])      # extra channels are cut off (predictor.py:206-209)
    if g.dtype != np.uint8:
      if not np.issubdtype(g.dtype, np.floating):
        raise ValueError('episode replay: the goal frame must be uint8 or floating point, got %s' % (g.dtype,))
      g = g.astype(np.float32)
    buf = self._goal_in[g.dtype]
    buf.copy_(torch.from_numpy(g.reshape(1, self.HW, 3)))
    return buf

  # -- the pass ----------------------------------------------------------------------------------------------------------------
  def replay(self, episode, goal_frame=None, labels=True):
    """The controller's commands over one episode.

    ``episode``: a mapping with 'rgb' -- the resident frames of ONE episode: a ``DeviceWindows`` of it (``episode_windows(dev=...)``;
    its frames are read as recorded, uint8 / 255 or float32), a device tensor [T][H][W][3], or a dense host array [T][H][W][3]
    (uint8, or float32 in [0, 1]) -- and 'jnt_state' [T][J]; or the pair ``(rgb, jnt_state)``.  ``goal_frame`` (goal models): the
    target frame [H][W][>=3] as ``set_goal`` takes it (default: the episode's 'target_rgb').  ``labels``: True reads the recorded
    values off the episode's per-frame arrays (``recorded_labels``), a mapping is read instead of the episode, False computes no
    errors.

    Returns numpy arrays: one per head under the keys ``Estimator.predict`` yields ('cmd_ee', 'logits_cmd_grp', ...), each [T][size],
    row t = the prediction on the window at frame t; with labels 'errors' [T][heads] (the heads in ``decoder.head_table`` order) and
    'episode_errors' {head: float}.  Everything is queued on the current stream; the host reads once, at the end."""
    return self._pass(episode, goal_frame, labels, False)

  def _pass(self, episode, goal_frame, labels, return_images):
    import torch
    if isinstance(episode, (tuple, list)):
      episode = {'rgb': episode[0], 'jnt_state': episode[1]}
    W, J = self.chunk_windows, self.J
    with torch.cuda.device(self.device):
      frames, T, u8 = self._frames_on_device(episode['rgb'])
      if T < 1:
        raise ValueError('episode replay: an episode needs at least one frame')
      if T > self.max_frames:
        raise ValueError('episode replay: the episode holds %d frames, this replay was built for max_frames=%d' % (T, self.max_frames))
      jnt = np.asarray(episode['jnt_state'], dtype=np.float32)
      if jnt.shape != (T, J):
        raise ValueError('episode replay: jnt_state must be [%d, %d], got %s' % (T, J, jnt.shape))
      goal_dev = None
      if self.goal:
        if goal_frame is None:
          goal_frame = episode.get('target_rgb')
        if goal_frame is None:
          raise ValueError("episode replay: a goal model needs goal_frame= (or the episode's 'target_rgb')")
        goal_dev = self._goal_on_device(goal_frame)
      self._check_inputs(frames, u8, goal_dev)
      lab = None
      if labels is not False and labels is not None:
        lab = recorded_labels(self.cfg, episode if labels is True else labels, T)
      # one upload: joint states and recorded values (and, in _encode, the frames' addresses)
      self._hu['jnt'][:T] = jnt
      if lab is not None:
        self._hu['labels'][:T] = lab
      self._d_up.copy_(self._h_up, non_blocking=True)
      # every frame once
      addr = frames.data_ptr() + np.arange(T, dtype=np.int64) * (self.HW * 3 * (1 if u8 else 4))
      images = self._encode(addr, T, u8, goal_dev, return_images)
      # the windows, chunk_windows per decoder launch (always the full launch: rows past the last window keep what they held)
      d, preds = self.decoder, self._dd['preds']
      for w0 in range(0, T, W):
        w1 = min(w0 + W, T)
        self._build_states(w0, w1, T)
        d.forward(False)
        preds[w0:w1].copy_(d.preds[:w1 - w0])
      if lab is not None:
        ops.replay_errors_into(self._dd['errors'], self._dd['episode'], preds, self._du['labels'], T, self._err_heads)
      self._h_down.copy_(self._d_down, non_blocking=True)      # the one read
      torch.cuda.current_stream().synchronize()
      images = {k: v.cpu().numpy().reshape(T, self.cfg.img_height, self.cfg.img_width, 3) for k, v in images.items()}
    out = {key: self._hd['preds'][:T, off:off + size].copy() for key, off, size in self.heads}
    if lab is not None:
      out['errors'] = self._hd['errors'][:T].copy()
      out['episode_errors'] = {key: float(self._hd['episode'][i]) for i, (key, _, _) in enumerate(self.heads)}
    out.update(images)
    return out


class EpisodeReplay(ReplayPass):
  """The per-frame controllers (e2e_vmc; goal_e2evmc 'sequence' x 'constant' / 'residual', RGB) over whole recorded episodes: ONE
  encoder stack, the frames packed by address, the goal frame riding in slot 0 of the first chunk."""

  def _check_config(self):
    scope, self.ch, self.mode = check_replay_config(self.cfg, self.goal)
    return [scope + '/ConvEncoder'], [self.ch]

  def _default_chunk_frames(self, dims):
    return default_chunk_frames(self.cfg, dims[0], self.max_frames)

  def _decoder_shape(self):
    return self.K, _CELLS * (self.ch + self.J + (self.ch if self.mode == 'constant' else 0))

  def _allocate(self):
    import torch
    F = self.chunk_frames
    self.enc, self.feat = self.encs[0], self.tables[0]
    self.tgt_feat = torch.zeros(_CELLS, self.ch, dtype=torch.float32, device=self.device) if self.mode != 'plain' else None
    # chunk c of an episode encodes the frames [c F - g, (c + 1) F - g) (g = 1 for a goal model: its target frame rides in slot 0 of
    # the first chunk); one table row per chunk, uploaded in one copy
    self.n_chunks = -(-(self.max_frames + 1) // F)
    self._h_table = torch.zeros(self.n_chunks, F, dtype=torch.int64, pin_memory=True)
    self._d_table = torch.zeros(self.n_chunks, F, dtype=torch.int64, device=self.device)

  def _encode(self, addr, T, u8, goal_dev, return_images):
    import torch
    F, HW = self.chunk_frames, self.HW
    g = 1 if self.goal else 0
    nc = -(-(T + g) // F)
    table = np.zeros(nc * F, np.int64)
    table[g:g + T] = addr
    self._h_table[:nc].copy_(torch.from_numpy(table.reshape(nc, F)))
    self._d_table[:nc].copy_(self._h_table[:nc], non_blocking=True)
    x0 = self.enc.x_in[0]
    for c in range(nc):
      lo, hi = max(c * F - g, 0), min((c + 1) * F - g, T)
      ops.pack_frames_by_address_into(x0, self._d_table[c], F, HW, u8)
      if g and c == 0:
        ops.predict_pack_newest_into(x0[0:1], goal_dev, 1, HW, 3)      # slot 0 (address 0: zeros) <- the target frame
      self.enc.forward()
      feats = self.enc.features[0].view(F, _CELLS, self.ch)
      first = g if c == 0 else 0
      if hi > lo:
        self.feat[lo:hi].copy_(feats[first:first + hi - lo])
      if g and c == 0:
        self.tgt_feat.copy_(feats[0])
    return {}

  def _build_states(self, w0, w1, T):
    ops.replay_states_into(self.decoder.states, self.feat, self._du['jnt'], self.mode, T, w0, w1, self.K, _CELLS, self.ch, self.J,
                           tgt_feat=self.tgt_feat)


def dataset_episodes(dataset_dir, split_name, mode, device, fetch_target=False):
  """The episodes of a dataset split, each uploaded once (``episode_to_device``) and yielded as the mapping ``EpisodeReplay.replay``
  takes: the per-frame arrays of ``load_episode``, 'rgb' (and 'target_rgb') as resident device tensors, 'name' = the record's file."""
  from . import input_fn
  from .device_windows import episode_to_device
  meta = input_fn.get_meta_v4(dataset_dir)
  H, W = meta.img_height, meta.img_width
  for path in input_fn.collect_tfrecords(dataset_dir, split_name, mode):
    ex = input_fn.load_episode(path, meta, fetch_target, raw_rgb=True, image_keys=('rgb',))
    states, dev = episode_to_device(ex, device, image_keys=('rgb',))
    ep = {k: v for k, v in states.items() if k != '_hw'}
    ep['rgb'] = dev['rgb'].view(-1, H, W, 3)
    if 'target_rgb' in dev:
      ep['target_rgb'] = dev['target_rgb'].view(H, W, 3)
    ep['name'] = os.path.basename(path)
    yield ep
