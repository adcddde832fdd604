"""Restatement of the opt-in skipping of optimiser steps whose gradient is not finite, written from its semantics and not
from the kernels (tests/test_skip_nonfinite_cpu.py checks it, tests/test_skip_nonfinite_gpu.py holds the device to it).

  G_i  = g_i * grad_scale + l2 * p_i           the total gradient, as the Adam kernels form it
  norm = sqrt(sum_i G_i^2) in FLOAT32          (the verdict is a float32 property: squares that overflow float32 count as non-finite)
  applied iff norm is finite;  guard = [verdict, skipped steps in all, skipped steps in a row]

``norm_f32`` adds the partials in the one order the header documents for geeco_clip_scale / geeco_guard_decide (256 strided serial sums,
the 6-level butterfly of each 64-lane wave, the four wave sums left to right), in numpy float32: every addition is one IEEE
operation, so the device's norm is this one bit for bit.  ``decide`` is the rest of geeco_guard_decide.  The float64 side
(``total_grad_is_finite``, ``oracle_gradient``) says what the verdict SHOULD be from the inputs alone.
"""
import numpy as np

import _clip_ref as C

H = 136                 # the shapes of tests/test_clip_gpu.py
K3 = 3
MODELS = {'e2e_vmc': (False, {}), 'goal residual': (True, dict(proc_obs='sequence', proc_tgt='residual'))}
_CASES = {}


def norm_f32(partials):
  """sqrt of the float32 sum of ``partials`` in the documented order."""
  x = np.asarray(partials, np.float32)
  with np.errstate(over='ignore', invalid='ignore'):
    acc = np.zeros(256, np.float32)
    for i in range(0, x.size, 256):          # thread t: partials t, t + 256, ... ascending
      row = x[i:i + 256]
      acc[:row.size] = acc[:row.size] + row
    lane = np.arange(256)
    for o in (32, 16, 8, 4, 2, 1):           # v += shfl_xor(v, o) inside each wave of 64
      acc = acc + acc[lane ^ o]
    w = acc[::64]
    total = np.float32(np.float32(np.float32(w[0] + w[1]) + w[2]) + w[3])
    return np.sqrt(total, dtype=np.float32)


def decide(partials, clip, guard):
  """(out2 as float32[2], guard as int list) after one geeco_guard_decide on ``guard`` = [verdict, total, consecutive]."""
  norm = norm_f32(partials)
  _, total, row = (int(x) for x in guard)
  if np.isfinite(norm):
    c = np.float32(clip)
    s = np.float32(1.0) if c == 0 else np.float32(c / (c if norm <= c else norm))
    return np.array([s, norm], np.float32), [1, total, 0]
  return np.array([0.0, norm], np.float32), [0, total + 1, row + 1]


def total_grad_is_finite(p, g, grad_scale=1.0, l2=0.0):
  """float64: every element of G finite AND the sum of squares inside float32's range."""
  G = C.total_grad(p, g, grad_scale, l2)
  with np.errstate(over='ignore', invalid='ignore'):
    return bool(np.isfinite(G).all() and np.sum(G * G) <= float(np.finfo(np.float32).max))


def case(name):
  """(ocfg, cfg, goal, P, feats, labels) of tests/test_clip_gpu.py's two models, once per model and left unchanged."""
  if name not in _CASES:
    from geeco_amd.params import create_e2evmc_config
    from oracle import geeco_oracle as O
    goal, extra = MODELS[name]
    ocfg = O.make_config(window_size=K3, img_height=H, img_width=H, batch_size=4, lr=1e-3, **extra)
    P = O.init_params(O.model_param_shapes(ocfg, goal), seed=1)
    feats, labels = O.synthetic_batch(ocfg, goal, 4, seed=3, H=H, W=H)
    _CASES[name] = (ocfg, create_e2evmc_config(ocfg._asdict()), goal, P, feats, labels)
  return _CASES[name]


def poisoned(labels, row=0):
  """The batch's labels with ONE value replaced: cmd[row, 0] = NaN (a regression target; never the gripper column, which a kernel
  turns into a class index)."""
  out = {k: v.copy() for k, v in labels.items()}
  out['cmd'][row, 0] = np.nan
  return out


def oracle_gradient(name, labels=None):
  """The float64 oracle's gradient of the case's batch (``labels``: another set of labels for it), every variable in one vector."""
  import torch
  from oracle import geeco_oracle as O
  ocfg, _, goal, P, feats, own = case(name)
  _, _, grads, _, _ = O.OracleTrainer(ocfg, goal, P, dtype=torch.float64).loss_and_grads(feats, own if labels is None else labels)
  return np.concatenate([g.numpy().ravel() for g in grads.values()])
