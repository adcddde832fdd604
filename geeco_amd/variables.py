"""Flat parameter arenas with TF-named views.

The reference keeps 60 ``tf.Variable``s (+ Adam slots) created by ``tf.layers`` under the scopes
listed in SURVEY.md 8b.  Here all trainable variables live in ONE contiguous fp32 buffer in HBM
(creation order = TF's), with three same-shaped siblings (gradient, Adam m, Adam v), so the
optimiser is a single fused pass and data-parallel training all-reduces a single bucket.  A fourth
sibling is opt-in: ``ema``, the exponential moving average of the parameters the same pass keeps.
Each variable starts on a 16-byte boundary (float4 loads in the conv kernels); the few pad floats
are zero and stay zero under Adam (g = 0).

The training options are checked in train_options.py; its names are re-imported here, where they used to live.  What an option needs
of the arena stays here: ``lr_multiplier_runs``, ``backward_cut``, ``variable_stats_scalars``, ``ema_decay_at``.
"""
from __future__ import annotations

import collections
import math
import re

import numpy as np
import torch

from .train_options import (LOSS_SHAPING_KEYS, LR_BOUNDARIES_MAX, LR_KINDS, SKIP_NONFINITE_DEFAULT_LIMIT, _LR_FIELDS,  # noqa: F401
                            check_clip_norm, check_ema_decay, check_grad_accum_steps, check_loss_shaping, check_lr_multipliers,
                            check_lr_schedule, check_skip_nonfinite, check_variable_stats, regression_prediction_keys)

ENC_FILTERS = (32, 48, 64, 128, 192, 256, 256)      # conv1..conv7 (graph.py:76-110); conv8 = dim_out
ENC_STRIDES = (1, 2, 2, 2, 2, 2, 2, 2)
_CELLS = 4   # the reference hard-codes the 2x2 tiling of the joint state (graph.py:139,163,188)


def encoder_shapes(scope, cin, dim_out):
  """<scope>/conv{i}/{kernel [3,3,Cin,Cout], bias [Cout]} (graph.py:76-115)."""
  shapes = collections.OrderedDict()
  c = cin
  for i, f in enumerate(list(ENC_FILTERS) + [dim_out]):
    shapes['%s/conv%d/kernel' % (scope, i + 1)] = (3, 3, c, f)
    shapes['%s/conv%d/bias' % (scope, i + 1)] = (f,)
    c = f
  return shapes


def decoder_shapes(scope, dim_in, cfg):
  """LSTMCell kernel/bias, fc1, heads (graph.py:217-259)."""
  H = cfg.dim_h_lstm
  s = collections.OrderedDict()
  s[scope + '/lstm_cell/kernel'] = (dim_in + H, 4 * H)
  s[scope + '/lstm_cell/bias'] = (4 * H,)
  s[scope + '/fc1/kernel'] = (H, cfg.dim_h_fc)
  s[scope + '/fc1/bias'] = (cfg.dim_h_fc,)
  if cfg.control_mode == 'cartesian':
    heads = [('pred_cmd_ee', 3), ('logits_cmd_grp', cfg.num_grp_states)]
  elif cfg.control_mode == 'velocity':
    heads = [('pred_cmd_vel', cfg.dim_jnt_state), ('pred_cmd_ee', 3), ('pred_cmd_grp', cfg.dim_grp_command)]
  else:
    raise ValueError("Unknown control mode '%s'" % (cfg.control_mode,))
  heads += [('pred_aux_ee', 3), ('pred_aux_obj', 3)]
  for name, n in heads:
    s['%s/%s/kernel' % (scope, name)] = (cfg.dim_h_fc, n)
    s['%s/%s/bias' % (scope, name)] = (n,)
  return s


def model_variable_shapes(cfg, goal: bool):
  """Variable creation order of ``e2e_vmc`` (graph.py:268-319) / ``goal_e2evmc`` (graph.py:321-416)."""
  C, jn = cfg.img_channels, cfg.dim_jnt_state
  if C not in (3, 4):
    raise ValueError("Unsupported number of channels for input frame: %d!" % C)
  s = collections.OrderedDict()
  if not goal:
    s.update(encoder_shapes('VMC/ConvEncoder', C, 256))
    s.update(decoder_shapes('VMC/LSTMDecoder', _CELLS * (256 + jn), cfg))
    return s
  root = 'GoalVMC'
  if cfg.proc_tgt not in ('constant', 'residual', 'dyndiff'):
    raise ValueError("Unknown processing mode for target image: %s!" % (cfg.proc_tgt,))
  if cfg.proc_obs == 'sequence':
    s.update(encoder_shapes(root + '/ConvEncoder', C, cfg.dim_s_obs))
    if cfg.proc_tgt == 'constant':
      din = _CELLS * (cfg.dim_s_obs + jn + cfg.dim_s_obs)
    elif cfg.proc_tgt == 'residual':
      din = _CELLS * (cfg.dim_s_obs + jn)
    else:
      s.update(encoder_shapes(root + '/DynDiffEncoder', C, cfg.dim_s_diff))
      din = _CELLS * (cfg.dim_s_obs + jn + cfg.dim_s_diff)
  elif cfg.proc_obs == 'dynimg':
    s.update(encoder_shapes(root + '/ConvEncoder', C, cfg.dim_s_obs))
    s.update(encoder_shapes(root + '/DynBuffEncoder', C, cfg.dim_s_dyn))
    s.update(encoder_shapes(root + '/DynDiffEncoder', C, cfg.dim_s_diff))
    din = _CELLS * (cfg.dim_s_obs + cfg.dim_s_dyn + jn + cfg.dim_s_diff)
  else:
    raise ValueError("Unknown processing mode for frame buffer: %s!" % (cfg.proc_obs,))
  s.update(decoder_shapes(root + '/LSTMDecoder', din, cfg))
  return s


def variable_stats_scalars(rec, count, lr_t, multiplier=1.0, applied=True, histograms=False):
  """One variable's record of ``geeco_variable_stats`` (a numpy scalar of ``ops.VARSTATS_DTYPE``, or any mapping with its fields) of ``count`` elements as the
  dictionary ``model.variable_stats()`` reports.  Square roots and ratios are formed here, in float64, from the device's sums.
  ``update_norm`` = lr_t * multiplier * sqrt(sum of u^2): the length of the step Adam just took in this variable; 0 for a frozen variable
  (``multiplier`` 0) and for a step that was skipped (``applied`` false).  A frozen variable -- one whose gradient no piece of the
  step covered -- reports every ``grad_*`` as None.  ``update_ratio`` is None where the weights' norm is 0."""
  def tensor(t, covered):
    finite = int(covered) - int(t['nonfinite'])
    lo, hi = float(t['min']), float(t['max'])
    return dict(norm=math.sqrt(float(t['sumsq'])), max_abs=max(abs(lo), abs(hi)) if finite > 0 else 0.0,
                mean=float(t['sum']) / finite if finite > 0 else 0.0, zero_fraction=int(t['zeros']) / float(covered) if covered else 0.0,
                nonfinite=int(t['nonfinite']), finite=finite)
  count = int(count)
  covered = int(rec['grad_covered'])
  out = {}
  if covered and float(multiplier) != 0.0:
    g = tensor(rec['grad'], covered)
    out.update(grad_norm=g['norm'], grad_max_abs=g['max_abs'], grad_mean=g['mean'], grad_zero_fraction=g['zero_fraction'], grad_nonfinite=g['nonfinite'])
  else:
    out.update(grad_norm=None, grad_max_abs=None, grad_mean=None, grad_zero_fraction=None, grad_nonfinite=None)
  w = tensor(rec['param'], count)
  out.update(weight_norm=w['norm'], weight_max_abs=w['max_abs'], weight_nonfinite=w['nonfinite'])
  moved = applied and float(multiplier) != 0.0
  out['update_norm'] = float(lr_t) * float(multiplier) * math.sqrt(float(rec['update_sumsq'])) if moved else 0.0
  out['update_ratio'] = out['update_norm'] / out['weight_norm'] if out['weight_norm'] > 0.0 else None
  if histograms:
    out['histograms'] = {}
    for name, key, n in (('gradients', 'grad', covered if out['grad_norm'] is not None else 0), ('weights', 'param', count)):
      if n:
        t = rec[key]
        out['histograms'][name] = dict(neg=[int(x) for x in t['neg']], pos=[int(x) for x in t['pos']], zeros=int(t['zeros']),
                                       min=float(t['min']), max=float(t['max']), sum=float(t['sum']), sum_squares=float(t['sumsq']),
                                       num=n - int(t['nonfinite']))
  return out


def lr_multiplier_runs(offsets, size, multipliers):
  """The arena as maximal contiguous runs [(offset, count, multiplier)] of one multiplier each.  ``offsets``: {name: offset} in arena
  order (``VariableStore.offsets``), ``size``: the arena's length.  A variable's span runs up to the next variable's offset, so the
  alignment pads and the pads of the uniform stride join the variable in front of them; frozen runs (multiplier 0) are dropped.
  Offsets and counts are multiples of 4 floats."""
  names = list(offsets)
  runs = []
  for i, n in enumerate(names):
    lo, hi = offsets[n], offsets[names[i + 1]] if i + 1 < len(names) else size
    mul = float(multipliers[n])
    if runs and runs[-1][2] == mul and runs[-1][1] == lo:
      runs[-1][1] = hi
    else:
      runs.append([lo, hi, mul])
  return [(lo, hi - lo, mul) for lo, hi, mul in runs if mul != 0.0 and hi > lo]


BACKWARD_CUTS = ('full', 'no_bottom', 'decoder_only')
_ENC_BOTTOM = re.compile(r'/conv[12]/(kernel|bias)$')
_ENC_ANY = re.compile(r'/conv\d+/(kernel|bias)$')


def backward_cut(multipliers):
  """Where the backward of a model with these per-variable multipliers (None: no option) stops: 'full' (anything trainable in conv1 /
  conv2 of any encoder), 'no_bottom' (conv1 and conv2, kernel and bias, frozen in every encoder), 'decoder_only' (every encoder
  variable frozen)."""
  if multipliers is None:
    return 'full'
  if all(mul == 0.0 for n, mul in multipliers.items() if _ENC_ANY.search(n)):
    return 'decoder_only'
  if all(mul == 0.0 for n, mul in multipliers.items() if _ENC_BOTTOM.search(n)):
    return 'no_bottom'
  return 'full'


def ema_decay_at(decay, t):
  """d_t = min(decay, (1 + t) / (10 + t)) in float32, as the Adam kernels compute it from the device's step counter."""
  t = np.float32(t)
  return min(np.float32(decay), (np.float32(1) + t) / (np.float32(10) + t))


class VariableStore:
  """Named views into flat param / grad / Adam arenas."""

  ALIGN = 4   # floats

  def __init__(self, shapes, device, uniform_scopes=None, ema=False):
    """``ema``: also hold the shadow arena ``ema`` (same size, alignment and device), the exponential moving average of the
    parameters that the optimiser's EMA entry points keep; it starts equal to the parameters.  ``uniform_scopes``: scope prefixes (the encoders of one model) whose variable blocks must start at a COMMON
    stride, so that one grouped launch can address encoder g at base + g * stride.  Blocks of equal size (the default
    dim_s_obs == dim_s_dyn == dim_s_diff) already do; a shorter block (smaller conv8) is followed by zero pad floats."""
    self.shapes = collections.OrderedDict(shapes)
    self.device = torch.device(device)
    self.offsets = collections.OrderedDict()
    al = lambda v: -(-v // self.ALIGN) * self.ALIGN
    stride, first = 0, {}
    if uniform_scopes and len(uniform_scopes) > 1:
      for g, sc in enumerate(uniform_scopes):
        names = [n for n in self.shapes if n.startswith(sc + '/')]
        first[names[0]] = g
        stride = max(stride, sum(al(int(np.prod(self.shapes[n]))) for n in names))
    off, start0 = 0, None
    for name, shp in self.shapes.items():
      off = al(off)
      if name in first:
        if first[name] == 0:
          start0 = off
        else:
          off = max(off, start0 + first[name] * stride)
      self.offsets[name] = off
      off += int(np.prod(shp))
    self.size = -(-off // self.ALIGN) * self.ALIGN
    self.params = torch.zeros(self.size, dtype=torch.float32, device=self.device)
    self.grads = torch.zeros(self.size, dtype=torch.float32, device=self.device)
    self.adam_m = torch.zeros(self.size, dtype=torch.float32, device=self.device)
    self.adam_v = torch.zeros(self.size, dtype=torch.float32, device=self.device)
    self.ema = torch.zeros(self.size, dtype=torch.float32, device=self.device) if ema else None
    self._shadow = None           # shadow_view()
    self.base = self              # ... and, on such a view, the store it was taken from
    self.global_step = torch.zeros(1, dtype=torch.int64, device=self.device)
    self.version = 0      # bumped whenever the parameters are (re)written from the host side
    self.primary_stack = None     # the first training ConvEncoderStack built on this store (encoder.py: lazy_refresh)
    self.late_staging = None      # data parallel: the conv1 / conv2 gradients on their way to the exchange (runtime.TrainStepRunner)
    # grad_accum_steps (keep_accumulator()): the accumulator arena, the micro-batches it holds so far (a HOST count) and
    # the losses' sum over them / mean over the last complete group.  None / 0 for a store without the option.  On the store because
    # the model built for a ragged final batch shares them; NOT checkpointed: a restart drops a partly filled group.
    self.accum = self.accum_loss_sum = self.accum_loss_mean = None
    self.accum_count = 0

  def keep_accumulator(self, losses):
    """The option's state, created once by the first training model with ``grad_accum_steps``: ``accum`` (float32, the arena's size
    and alignment, zeros) and the two loss buffers of ``losses`` floats."""
    if self.accum is None:
      f32 = dict(dtype=torch.float32, device=self.device)
      self.accum = torch.zeros(self.size, **f32)
      self.accum_loss_sum, self.accum_loss_mean = torch.zeros(losses, **f32), torch.zeros(losses, **f32)
      self.accum_count = 0

  # -- views ------------------------------------------------------------------------------
  def _view(self, arena, name):
    shp = self.shapes[name]
    o = self.offsets[name]
    return arena[o:o + int(np.prod(shp))].view(*shp)

  def var(self, name):
    return self._view(self.params, name)

  def grad(self, name):
    return self._view(self.grads, name)

  def ema_var(self, name):
    return self._view(self.ema, name)

  def shadow_view(self):
    """This store with the shadow arena in the parameters' place: what an evaluation / prediction model is built on to run on the
    averaged weights.  Shares every arena (nothing is copied; the view follows training) and has no shadow arena of its own.  For
    inference models only -- they re-derive their weight copies on every forward, so the view carries no version of its own."""
    if self.ema is None:
      raise ValueError('this VariableStore keeps no averaged weights (VariableStore(ema=True))')
    if self._shadow is None:
      view = object.__new__(VariableStore)
      view.__dict__.update(self.__dict__)
      view.params, view.ema, view._shadow, view.primary_stack, view.base = self.ema, None, None, None, self
      self._shadow = view
    return self._shadow

  def _params_rewritten(self):
    """The parameters were (re)written from the host side: the shadow arena restarts from them."""
    if self.ema is not None:
      self.ema.copy_(self.params)
    self.version += 1

  def count_parameters(self) -> int:
    """models/e2evmc/utils.py:10-14."""
    return int(sum(int(np.prod(s)) for s in self.shapes.values()))

  # -- initialisation / (de)serialisation -----------------------------------------------------
  def initialize(self, seed=0):
    """glorot-uniform kernels, zero biases (tf.layers / LSTMCell defaults [TF1.15])."""
    rng = np.random.default_rng(seed)
    for name, shp in self.shapes.items():
      if name.endswith('/bias'):
        val = np.zeros(shp, np.float32)
      else:
        if len(shp) == 4:
          fan_in, fan_out = shp[0] * shp[1] * shp[2], shp[0] * shp[1] * shp[3]
        else:
          fan_in, fan_out = shp
        lim = math.sqrt(6.0 / (fan_in + fan_out))
        val = rng.uniform(-lim, lim, size=shp).astype(np.float32)
      self.var(name).copy_(torch.from_numpy(val))
    self._params_rewritten()

  def load_numpy(self, values: dict, ema_values=None):
    """``ema_values`` ({name: array}, a store with the shadow arena): the shadow tensors; None = they restart from the parameters."""
    for name in self.shapes:
      self.var(name).copy_(torch.from_numpy(np.ascontiguousarray(values[name], dtype=np.float32)))
    self._params_rewritten()
    if ema_values is not None and self.ema is not None:
      for name in self.shapes:
        self.ema_var(name).copy_(torch.from_numpy(np.ascontiguousarray(ema_values[name], dtype=np.float32)))

  def to_numpy(self, which='params'):
    arena = {'params': self.params, 'grads': self.grads, 'adam_m': self.adam_m, 'adam_v': self.adam_v, 'ema': self.ema}[which]
    if arena is None:
      raise ValueError('this VariableStore keeps no averaged weights (VariableStore(ema=True))')
    host = arena.detach().cpu().numpy()
    out = collections.OrderedDict()
    for name, shp in self.shapes.items():
      o = self.offsets[name]
      out[name] = host[o:o + int(np.prod(shp))].reshape(shp).copy()
    return out

  def state_dict(self):
    sd = {'params': self.params.detach().cpu(), 'adam_m': self.adam_m.detach().cpu(),
          'adam_v': self.adam_v.detach().cpu(), 'global_step': self.global_step.detach().cpu(),
          'names': list(self.shapes.keys()), 'shapes': [tuple(s) for s in self.shapes.values()],
          'offsets': list(self.offsets.values())}
    if self.ema is not None:
      sd['ema'] = self.ema.detach().cpu()
    return sd

  def load_state_dict(self, sd):
    if list(sd['names']) != list(self.shapes.keys()) or [tuple(s) for s in sd['shapes']] != \
        [tuple(s) for s in self.shapes.values()]:
      raise ValueError('checkpoint variables do not match the model graph')
    self.params.copy_(sd['params'])
    self.adam_m.copy_(sd['adam_m'])
    self.adam_v.copy_(sd['adam_v'])
    self.global_step.copy_(sd['global_step'])
    self._params_rewritten()       # (a checkpoint without shadow weights: they restart from its parameters)
    if self.ema is not None and sd.get('ema') is not None:
      self.ema.copy_(sd['ema'])
