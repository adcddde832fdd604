"""High-level predictor API (batch-1 inference) on the HIP kernels.

Counterpart of the reference's ``src/models/e2evmc/predictor.py``: ``GoalE2EVMCPredictor`` (:43-209)
and ``E2EVMCPredictor`` (:212-379) with the same constructor and methods (``predict``, ``reset``,
``set_goal``, ``cfg``).  Semantics kept: the frame buffer holds the last ``window_size`` frames and is
padded with the first frame after a reset (:192-200); frames must be [H, W, C] in [0, 1] (:127-138);
the gripper logits are re-mapped to {-1, 0, 1} (:183-189); ``dynbuff`` / ``dyndiff`` debug images are
returned when the model computes them (:167-170).

Both classes are one-env views of the batched predictor (``batched_predictor``, ``num_envs=1``, float32 frames, debug images
on): that engine owns the model, the checkpoint restore, the window in HBM and the replayed hipGraph.  What lives here is the
batch-1 contract: the host-side frame assertions with the reference's messages, un-batched arguments and an un-batched dict.
``incremental=True`` (per-frame models: e2e_vmc, goal_e2evmc 'sequence' x 'constant' / 'residual') is passed through: a call
encodes the new frame only, the features of the window's older frames wait in a ring on the device.
"""
from __future__ import annotations

import numpy as np

from .batched_predictor import TOL_FRAME_RANGE, BatchedE2EVMCPredictor, BatchedGoalE2EVMCPredictor


class _PredictorBase:
  _core_cls = None

  def __init__(self, model_dir, checkpoint_name=None, memcap=0.8, device=None, incremental=False, use_ema=False):
    # one prediction at a time (predictor.py:56): cfg.batch_size == 1
    self._core = self._core_cls(model_dir, 1, checkpoint_name=checkpoint_name, memcap=memcap, device=device,
                                frame_dtype='float32', debug_images=True, incremental=incremental, use_ema=use_ema)
    self._model = self._core._model

  @property
  def cfg(self):
    return self._core.cfg

  def _check_frame(self, frame):
    cfg = self.cfg
    expected = (cfg.img_height, cfg.img_width, cfg.img_channels)
    assert tuple(frame.shape) == expected, \
        "Fed frame has wrong dimensions! Expected %s, got %s!" % (expected, tuple(frame.shape))
    lo, hi = float(np.amin(frame[..., :3])), float(np.amax(frame[..., :3]))
    assert -TOL_FRAME_RANGE <= lo and hi <= 1 + TOL_FRAME_RANGE, \
        "Fed frame exceeds range! Expected %s, got %s!" % ((0 - TOL_FRAME_RANGE, 1 + TOL_FRAME_RANGE), (lo, hi))

  def predict(self, rgb_frame, jnt_state):
    """Feeds the frame (padding the buffer after a reset) and returns the predictions."""
    if self._core._goal and not self._core._goal_set[0]:
      raise RuntimeError('set_goal(tgt_frame) must be called before predict()')
    self._check_frame(rgb_frame)
    out = self._core.predict(np.ascontiguousarray(rgb_frame, dtype=np.float32)[None],
                             np.asarray(jnt_state, dtype=np.float32).reshape(1, -1))
    return {k: v[0] for k, v in out.items()}

  def reset(self):
    self._core.reset()


class GoalE2EVMCPredictor(_PredictorBase):
  """High-level API to run goal-conditioned E2EVMC (predictor.py:43-209)."""
  _core_cls = BatchedGoalE2EVMCPredictor

  def set_goal(self, tgt_frame):
    """Sets the target frame (predictor.py:206-209)."""
    self._core.set_goal(np.asarray(tgt_frame, dtype=np.float32)[None])      # the core cuts off extra channels


class E2EVMCPredictor(_PredictorBase):
  """High-level API to run E2E VMC (predictor.py:212-379)."""
  _core_cls = BatchedE2EVMCPredictor
