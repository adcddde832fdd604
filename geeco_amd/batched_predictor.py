"""Batched predictor API: B control loops (simulator envs) stepped by ONE call.

``BatchedGoalE2EVMCPredictor`` / ``BatchedE2EVMCPredictor`` are the batched counterparts of the reference's
``GoalE2EVMCPredictor`` / ``E2EVMCPredictor`` (``src/models/e2evmc/predictor.py``) and the one predictor engine of this package:
the batch-1 classes of ``predictor`` are views of it with ``num_envs=1``.  Per env the semantics are the reference's
(:127-209): a window of the last ``window_size`` frames, padded with the first frame after a reset; frames [H, W, C] with
channels 0..2 in [0 - 1e-6, 1 + 1e-6]; the gripper logits re-mapped to argmax - 1 in cartesian mode; the reference's five
outputs in velocity mode; ``dynbuff`` / ``dyndiff`` when the model computes them (and ``debug_images=True``).  Every output gets
a leading [B] axis.

One ``predict`` = one H2D of a pinned staging block (frames, joint states, pending resets), one replayed hipGraph (range check,
window push, the model's forward at N = B, output pack: csrc/predict_io.hip) and one D2H of the packed outputs.  The K-frame
windows live in HBM: dense fp32 windows shifted in place, or -- uint8 frames on a model whose input kernel reads uint8 windows
(geeco-f RGB) -- a mirrored uint8 ring per env whose window start the graph itself advances.

``incremental=True`` (the per-frame controllers: e2e_vmc, goal_e2evmc 'sequence' x 'constant' / 'residual') keeps no frame window
at all: per env a ring of the last K encoder FEATURE vectors and joint states (step_models.E2EVMCStep / GoalE2EVMCStep).  A call
encodes only the B new frames; the graph is range check, newest-frame pack, encoder at N = B, feature push + state gather,
decoder, output pack.  Same methods, errors and returned dict.
"""
from __future__ import annotations

import numpy as np
import torch

from . import estimator as est
from . import graph, ops
from .params import create_e2evmc_config
from .runtime import _CAPTURE_MODE, CAPTURE_LOCK
from .utils import load_model_config

TOL_FRAME_RANGE = 1e-6  # tolerance for value range of fed frames (predictor.py:18)
_ALIGN = 256
_TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.uint8): torch.uint8, np.dtype(np.int32): torch.int32}


def range_bounds():
  """The float32 interval [lo, hi] holding exactly the float32 values v with -TOL <= v <= 1 + TOL in double precision (the
  batch-1 check compares np.amin / np.amax of a float32 frame against these Python floats, predictor.py:135-138)."""
  lo = np.float32(-TOL_FRAME_RANGE)
  if float(lo) < -TOL_FRAME_RANGE:
    lo = np.nextafter(lo, np.float32(np.inf))
  hi = np.float32(1 + TOL_FRAME_RANGE)
  if float(hi) > 1 + TOL_FRAME_RANGE:
    hi = np.nextafter(hi, np.float32(-np.inf))
  return float(lo), float(hi)


class _Layout:
  """Named, 256-byte aligned regions of one byte block (the staging block, the output block)."""

  def __init__(self):
    self.parts, self.size = [], 0

  def add(self, name, shape, dtype):
    dtype = np.dtype(dtype)
    n = int(np.prod(shape)) * dtype.itemsize
    self.parts.append((name, self.size, n, tuple(shape), dtype))
    self.size += -(-n // _ALIGN) * _ALIGN

  def device(self, buf):
    return {name: buf[off:off + n].view(_TORCH[dt]).view(shape) for name, off, n, shape, dt in self.parts}

  def host(self, buf):
    a = buf.numpy()
    return {name: a[off:off + n].view(dt).reshape(shape) for name, off, n, shape, dt in self.parts}


class _AddressTable:
  """What ``feed.WindowFeed.pointers()`` hands a model: ``pointers`` marks the input as window addresses and ``table`` is the
  int64 device table of per-env addresses its input kernel reads when it runs (graph.GoalE2EVMC._encode)."""

  def __init__(self, table, shape):
    self.table, self.shape = table, tuple(shape)

  def pointers(self):
    return self


class _BatchedPredictorBase:
  _goal = False

  def __init__(self, model_dir, num_envs, checkpoint_name=None, memcap=0.8, device=None, frame_dtype='float32',
               debug_images=False, incremental=False, use_ema=False):
    """``use_ema``: run the checkpoint's averaged weights (a training run with params['ema_decay']); KeyError if it holds none."""
    B = int(num_envs)
    if B < 1:
      raise ValueError('num_envs must be >= 1, got %d' % B)
    fd = np.dtype(frame_dtype)
    if fd not in (np.dtype(np.float32), np.dtype(np.uint8)):
      raise ValueError("frame_dtype must be 'float32' or 'uint8', got %s" % (frame_dtype,))
    cfg = load_model_config(model_dir, 'e2evmc_config')
    cfg['batch_size'] = B
    self._cfg = cfg = create_e2evmc_config(cfg)
    self._u8 = fd == np.dtype(np.uint8)
    self._incremental = bool(incremental)
    if self._incremental:
      if not self._goal:
        ctor = graph.E2EVMCStep
      elif cfg.proc_obs == 'sequence' and cfg.proc_tgt in ('constant', 'residual'):
        ctor = graph.GoalE2EVMCStep
      elif cfg.proc_obs == 'sequence':
        raise ValueError("incremental=True does not take proc_obs='sequence' with proc_tgt='%s': the cached DynDiff features depend "
                         "on the goal, a goal change needs the K raw frames encoded again" % (cfg.proc_tgt,))
      else:
        raise ValueError("incremental=True caches per-frame encoder features: proc_obs='%s' has none (three encoder passes per "
                         "call whatever the window size)" % (cfg.proc_obs,))
    else:
      ctor = graph.GoalE2EVMC if self._goal else graph.E2EVMC
    if self._u8 and cfg.img_channels != 3:
      raise ValueError('uint8 frames are for RGB models (img_channels == 3); an RGB-D model takes float32 frames [H, W, 4]')
    if not torch.cuda.is_available():
      raise RuntimeError('geeco_amd predictor needs an MI355X (no CPU fallback)')
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    if dev.index is None:
      dev = torch.device('cuda', torch.cuda.current_device())
    self._dev = dev
    if memcap and 0.0 < memcap < 1.0:
      torch.cuda.set_per_process_memory_fraction(float(memcap), dev)
    self.num_envs, self._fdtype = B, fd
    H, W, C, K, J = cfg.img_height, cfg.img_width, cfg.img_channels, cfg.window_size, cfg.dim_jnt_state
    self._dims = (B, H, W, C, K, J)
    with torch.cuda.device(dev):
      # the per-frame controllers' K-step decoder as one launch (geeco-f runs T = 1: its decoder ignores the argument)
      m = self._model = ctor(cfg, B, dev, training=False, one_launch_decoder=True)
      est.restore_for_inference(m.store, model_dir, checkpoint_name, use_ema=use_ema)
      # uint8 frames on a model whose input kernel reads uint8 windows: the mirrored ring (no fp32 window is ever written)
      self._ring = self._u8 and not self._incremental and 'rgb' in m.u8_window_keys
      self._make_staging_block()
      self._ctl = torch.zeros(B + 1, dtype=torch.int32, device=dev)      # per env "frame out of range", then "any env"
      self._make_output_block(debug_images)
      if self._ring:
        self._ring_buf = torch.zeros(B, 2 * K, H * W * 3, dtype=torch.uint8, device=dev)
        self._heads = torch.zeros(B, dtype=torch.int32, device=dev)
        self._tgt_u8 = torch.zeros(B, H * W * 3, dtype=torch.uint8, device=dev)
        stride = 2 * K * H * W * 3
        self._win_table = torch.tensor([self._ring_buf.data_ptr() + b * stride for b in range(B)], dtype=torch.int64, device=dev)
        self._tgt_table = torch.tensor([self._tgt_u8.data_ptr() + b * H * W * 3 for b in range(B)], dtype=torch.int64,
                                       device=dev)
        m.inputs['rgb'] = _AddressTable(self._win_table, (B, K, H, W, 3))        # the dense fp32 window is never allocated again
        m.inputs['target_rgb'] = _AddressTable(self._tgt_table, (B, H, W, 3))
      self._lo, self._hi = range_bounds()
      self._pending = np.ones(B, dtype=bool)         # every env starts with its window padded by its first frame
      self._goal_set = np.zeros(B, dtype=bool)
      # one eager run (the kernels' one-time set-up, as EvalStepRunner's warm-up) with the "any bad" word set: no window moves
      self._ctl[B] = 1
      self._call_body()
      torch.cuda.synchronize(dev)
      self._graph = torch.cuda.CUDAGraph()
      with CAPTURE_LOCK:
        with torch.cuda.graph(self._graph, capture_error_mode=_CAPTURE_MODE):
          self._call_body()
      torch.cuda.synchronize(dev)

  def _make_staging_block(self):
    """What one call uploads: frames, joint states and pending resets in one pinned block and its device twin."""
    B, H, W, C, K, J = self._dims
    dev, fd = self._dev, self._fdtype
    stage = _Layout()
    stage.add('frames', (B, H, W, C), fd)
    stage.add('jnt', (B, J), np.float32)
    stage.add('reset', (B,), np.int32)
    self._h_stage = torch.empty(stage.size, dtype=torch.uint8, pin_memory=True)
    self._d_stage = torch.zeros(stage.size, dtype=torch.uint8, device=dev)
    self._h = stage.host(self._h_stage)
    self._d = stage.device(self._d_stage)

  def _make_output_block(self, debug_images):
    """What one call downloads: the packed outputs, the range-check words and the debug images, in one block."""
    B, H, W, C, K, J = self._dims
    dev, cfg, m = self._dev, self._cfg, self._model
    # outputs in the order the API returns them: (name, source column, width, argmax - 1)
    off, cols = 0, {}
    for _, key, size, _, _ in m.decoder.heads:
      cols[key] = (off, size)
      off += size
    if cfg.control_mode == 'cartesian':
      self._segs = [('cmd_ee',) + cols['cmd_ee'] + (False,), ('cmd_grp',) + cols['logits_cmd_grp'] + (True,),
                    ('pos_ee',) + cols['pos_ee'] + (False,), ('pos_obj',) + cols['pos_obj'] + (False,)]
    else:
      self._segs = [(k,) + cols[k] + (False,) for k in ('cmd_vel', 'cmd_ee', 'cmd_grp', 'pos_ee', 'pos_obj')]
    F = sum(1 if a else n for _, _, n, a in self._segs)
    self._imgs = self._debug_sources() if debug_images and not self._incremental else []   # step models compute no images
    out = _Layout()
    out.add('out', (B, F), np.float32)
    out.add('ctl', (B + 1,), np.int32)
    if self._imgs:
      out.add('images', (len(self._imgs), B, H, W, C), np.float32)
    self._h_outblk = torch.empty(out.size, dtype=torch.uint8, pin_memory=True)
    self._d_outblk = torch.zeros(out.size, dtype=torch.uint8, device=dev)
    self._ho = out.host(self._h_outblk)
    self._do = out.device(self._d_outblk)

  def _debug_sources(self):
    return []

  @property
  def cfg(self):
    return self._cfg

  @property
  def window_form(self):
    """'ring': the mirrored uint8 ring the model's input kernel reads through its address table (uint8 frames on a model with
    uint8 window inputs, geeco-f RGB); 'dense': the model's fp32 windows, shifted in place; 'features': no frame window, per env
    a ring of the last K encoder feature vectors (incremental=True)."""
    if self._incremental:
      return 'features'
    return 'ring' if self._ring else 'dense'

  def frame_buffer(self):
    """The pinned staging array [B, H, W, C] the next ``predict`` uploads from: frames rendered straight into it (and passed to
    ``predict`` as they are) skip the host copy."""
    return self._h['frames']

  def _call_body(self):
    """What the graph holds, in stream order: range check, window push, forward at N = B, output pack."""
    B, H, W, C, K, J = self._dims
    HW, m, d, ctl = H * W, self._model, self._d, self._ctl
    if not self._u8:
      ops.predict_range_check_into(ctl, d['frames'], B, HW, C, self._lo, self._hi)
    if self._incremental:
      m.step(d['frames'], d['jnt'], d['reset'], ctl)      # newest-frame pack, encoder at N = B, feature push + gather, decoder
      ops.predict_pack_into(self._do['out'], self._do['ctl'], m.decoder.preds, ctl, B, [s[1:] for s in self._segs])
      return
    inp = m.inputs
    if self._ring:
      ops.predict_push_ring_into(self._ring_buf, self._heads, self._win_table, inp['jnt_state'], d['frames'], d['jnt'],
                                 d['reset'], ctl, B, K, HW, J)
    else:
      ops.predict_push_dense_into(inp['rgb'], inp.get('depth'), inp['jnt_state'], d['frames'], d['jnt'], d['reset'], ctl, B, K,
                                  HW, C, J)
    m.forward(backward_too=False)
    ops.predict_pack_into(self._do['out'], self._do['ctl'], m.decoder.preds, ctl, B, [s[1:] for s in self._segs],
                          self._imgs, HW, C, self._do.get('images'))

  def _env_ids(self, env_ids):
    B = self.num_envs
    if env_ids is None:
      return np.arange(B)
    ids = np.asarray(env_ids, dtype=np.int64).reshape(-1)
    if ids.size and (ids.min() < 0 or ids.max() >= B):
      raise ValueError('env_ids %s outside 0..%d' % (ids.tolist(), B - 1))
    return ids

  def reset(self, env_ids=None):
    """The next frame fed to these envs (None = all) pads their whole window (predictor.py:192-200)."""
    self._pending[self._env_ids(env_ids)] = True

  def predict(self, frames, jnt_state):
    """Feeds one frame per env ([B, H, W, C], float32 in [0, 1] or uint8) and the joint states [B, dim_jnt_state]; returns the
    predictions of all B envs, each with a leading [B] axis."""
    B, H, W, C, K, J = self._dims
    if self._goal and not self._goal_set.all():
      raise RuntimeError('set_goal(tgt_frame) must be called before predict(): envs %s have no goal'
                         % np.flatnonzero(~self._goal_set).tolist())
    if not isinstance(frames, np.ndarray) or frames.dtype != self._fdtype:
      raise ValueError('frames must be a numpy array of %s in this predictor (frame_dtype), got %s'
                       % (self._fdtype, getattr(frames, 'dtype', type(frames))))
    if tuple(frames.shape) != (B, H, W, C):
      raise ValueError('Fed frames have wrong dimensions! Expected %s, got %s!' % ((B, H, W, C), tuple(frames.shape)))
    jnt = np.asarray(jnt_state, dtype=np.float32)
    if jnt.shape != (B, J):
      raise ValueError('jnt_state must be [%d, %d], got %s' % (B, J, tuple(jnt.shape)))
    h = self._h
    if frames.__array_interface__['data'][0] != h['frames'].__array_interface__['data'][0]:
      np.copyto(h['frames'], frames)
    h['jnt'][...] = jnt
    h['reset'][...] = self._pending
    with torch.cuda.device(self._dev):
      self._d_stage.copy_(self._h_stage, non_blocking=True)        # the one H2D
      self._graph.replay()
      self._h_outblk.copy_(self._d_outblk, non_blocking=True)      # the one D2H
      torch.cuda.current_stream().synchronize()
      self._model.check_device_errors()
    ctl = self._ho['ctl']
    if ctl[B]:
      bad = np.flatnonzero(ctl[:B])
      rng = [(float(np.amin(h['frames'][b, ..., :3])), float(np.amax(h['frames'][b, ..., :3]))) for b in bad]
      raise AssertionError('; '.join('env %d: Fed frame exceeds range! Expected %s, got %s!'
                                     % (b, (0 - TOL_FRAME_RANGE, 1 + TOL_FRAME_RANGE), r) for b, r in zip(bad, rng)))
    self._pending[:] = False
    o, res, col = self._ho['out'], {}, 0
    for name, _, n, argmax in self._segs:
      w = 1 if argmax else n
      res[name] = o[:, col:col + w].copy()
      col += w
    for i, name in enumerate(self._img_names):
      res[name] = self._ho['images'][i].copy()
    return res

  _img_names = ()


class BatchedGoalE2EVMCPredictor(_BatchedPredictorBase):
  """Goal-conditioned E2EVMC for B envs per call (the batched GoalE2EVMCPredictor, predictor.py:43-209)."""
  _goal = True

  def _debug_sources(self):
    m, cfg, K = self._model, self._cfg, self._cfg.window_size
    src, names = [], []
    if cfg.proc_obs == 'dynimg':
      src.append(m.enc.x_in[1])
      names.append('dynbuff')
    if cfg.proc_tgt == 'dyndiff':
      src.append(m.enc.x_in[2] if m.mode == 'dynimg' else m.enc.x_in.view(2, K, self.num_envs, cfg.img_height, cfg.img_width, 4)[1][K - 1])
      names.append('dyndiff')
    self._img_names = tuple(names)
    return src

  def set_goal(self, tgt_frames, env_ids=None):
    """Sets the target frame of every env ([B, H, W, >=C]) or, with env_ids, of those envs (one frame [H, W, >=C] for all of
    them, or one per env).  Extra channels are cut off (predictor.py:206-209).  Frames come in the predictor's frame_dtype."""
    B, H, W, C, K, J = self._dims
    ids = self._env_ids(env_ids)
    t = np.asarray(tgt_frames)
    if (t.dtype != np.uint8) if self._u8 else not np.issubdtype(t.dtype, np.floating):
      raise ValueError('goal frames must be %s in this predictor (frame_dtype), got %s' % (self._fdtype, t.dtype))
    if t.ndim == 3:
      t = np.broadcast_to(t, (len(ids),) + t.shape)
    if t.ndim != 4 or t.shape[0] != len(ids) or t.shape[1:3] != (H, W) or t.shape[3] < C:
      raise ValueError('goal frames must be [%d, %d, %d, >=%d], got %s' % (len(ids), H, W, C, tuple(t.shape)))
    t = np.ascontiguousarray(t[..., :C])
    idx = torch.as_tensor(ids, device=self._dev)
    with torch.cuda.device(self._dev):
      if self._incremental:      # the goals' features, once per goal: the per-call graph only reads them
        tf = t.astype(np.float32) / np.float32(255.0) if self._u8 else t.astype(np.float32)   # the device's u8 division
        if len(ids):
          self._model.encode_targets(torch.from_numpy(tf).to(self._dev), idx)
        self._goal_set[ids] = True
        return
      inp = self._model.inputs
      if self._ring:
        self._tgt_u8[idx] = torch.from_numpy(t.reshape(len(ids), -1)).to(self._dev)
      else:
        tf = t.astype(np.float32) / np.float32(255.0) if self._u8 else t.astype(np.float32)   # the device's u8 division
        inp['target_rgb'][idx] = torch.from_numpy(np.ascontiguousarray(tf[..., :3])).to(self._dev)
        if C == 4:
          inp['target_depth'][idx] = torch.from_numpy(np.ascontiguousarray(tf[..., 3:4])).to(self._dev)
    self._goal_set[ids] = True


class BatchedE2EVMCPredictor(_BatchedPredictorBase):
  """E2E VMC for B envs per call (the batched E2EVMCPredictor, predictor.py:212-379)."""
  _goal = False
