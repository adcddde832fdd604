"""Flat parameter arenas with TF-named views.

The reference keeps 60 ``tf.Variable``s (+ Adam slots) created by ``tf.layers`` under the scopes
listed in SURVEY.md 8b.  Here all trainable variables live in ONE contiguous fp32 buffer in HBM
(creation order = TF's), with three same-shaped siblings (gradient, Adam m, Adam v), so the
optimiser is a single fused pass and data-parallel training all-reduces a single bucket.  A fourth
sibling is opt-in: ``ema``, the exponential moving average of the parameters the same pass keeps.
Each variable starts on a 16-byte boundary (float4 loads in the conv kernels); the few pad floats
are zero and stay zero under Adam (g = 0).
"""
from __future__ import annotations

import collections
import collections.abc
import math
import numbers
import re

import numpy as np
import torch

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


def check_ema_decay(value, key='ema_decay'):
  """The decay of the shadow weights: None or 0 = off (returns None), else a float in (0, 1); anything else raises ValueError
  naming ``key``."""
  if value is None or (isinstance(value, numbers.Real) and value == 0):
    return None
  if isinstance(value, bool) or not isinstance(value, numbers.Real) or not 0.0 < float(value) < 1.0:
    raise ValueError('%s=%r: the decay of the averaged weights must lie in (0, 1) (None or 0 = off)' % (key, value))
  return float(value)


def check_clip_norm(value, key='clip_norm'):
  """The global norm the gradient is clipped to: None or 0 = off (returns None), else a finite number > 0 that float32 holds;
  anything else raises ValueError naming ``key``."""
  if value is None or (isinstance(value, numbers.Real) and not isinstance(value, bool) and value == 0):
    return None
  f32 = np.finfo(np.float32)
  if isinstance(value, bool) or not isinstance(value, numbers.Real) or not float(f32.tiny) <= float(value) <= float(f32.max):
    raise ValueError('%s=%r: the norm to clip the gradient to must be a finite number > 0, a normal float32 (None or 0 = off)' % (key, value))
  return float(value)


SKIP_NONFINITE_DEFAULT_LIMIT = 100


def check_skip_nonfinite(value, key='skip_nonfinite'):
  """Skipping of optimiser steps whose gradient is not finite: None or False = off (returns None); True = on with the
  default limit of 100 consecutive skipped steps; an integer L >= 1 = on with limit L.  Returns the limit; anything else raises
  ValueError naming ``key``."""
  if value is None or value is False:
    return None
  if value is True:
    return SKIP_NONFINITE_DEFAULT_LIMIT
  if isinstance(value, numbers.Integral) and value >= 1:
    return int(value)
  raise ValueError('%s=%r: True, or the number of consecutive skipped steps after which training stops, an integer >= 1 '
                   '(None or False = off)' % (key, value))


def check_variable_stats(value, key='variable_stats'):
  """Per-variable statistics on logging steps: None or False = off (returns None); True = the scalars (returns
  'scalars'); 'histograms' = the scalars and the magnitude histograms (returns 'histograms').  Anything else raises ValueError naming
  ``key``."""
  if value is None or value is False:
    return None
  if value is True:
    return 'scalars'
  if isinstance(value, str) and value == 'histograms':
    return 'histograms'
  raise ValueError("%s=%r: True (scalars per variable) or 'histograms' (scalars and histograms); None or False = off" % (key, value))


def check_grad_accum_steps(value, key='grad_accum_steps'):
  """Gradient accumulation over micro-batches: None or 1 = off (returns None); an integer A >= 2 = one optimiser step
  per A micro-batches (returns A).  Anything else raises ValueError naming ``key``."""
  if value is None:
    return None
  if isinstance(value, (bool, np.bool_)) or not isinstance(value, numbers.Integral) or value < 1:
    raise ValueError('%s=%r: the number of micro-batches per optimiser step must be an integer >= 1 (None or 1 = off)' % (key, value))
  return None if int(value) == 1 else int(value)


LOSS_SHAPING_KEYS = ('sample_weights', 'grp_class_weights', 'label_smoothing', 'huber_delta')


def regression_prediction_keys(cfg):
  """Prediction keys of the regression heads (decoder.head_table's, in its order): the heads ``huber_delta`` may name."""
  if cfg.control_mode == 'cartesian':
    return ('cmd_ee', 'pos_ee', 'pos_obj')
  if cfg.control_mode == 'velocity':
    return ('cmd_vel', 'cmd_ee', 'cmd_grp', 'pos_ee', 'pos_obj')
  raise ValueError("Unknown control mode '%s'" % (cfg.control_mode,))


def check_loss_shaping(value, cfg, key='loss_shaping'):
  """Loss shaping (tf.losses' ``weights=``, ``label_smoothing=`` and ``tf.losses.huber_loss(delta=)``): None = off, or a dict
  with any of ``sample_weights`` (bool: the loss reads a weight per sample, labels['sample_weight']), ``grp_class_weights`` (one finite
  weight >= 0 per gripper class, ``cfg.num_grp_states`` of them; cartesian mode only), ``label_smoothing`` (a float in [0, 1); cartesian
  mode only) and ``huber_delta`` (a finite float > 0 for every regression head, or {prediction key: delta}).  Returns None when every entry
  is neutral, else dict(sample_weights=bool, grp_class_weights=tuple or None, label_smoothing=float, huber_delta={prediction key: delta});
  anything else raises ValueError naming ``key``."""
  if value is None:
    return None
  if not isinstance(value, collections.abc.Mapping):
    raise ValueError('%s=%r: None or a dict with the keys %s' % (key, value, ', '.join(LOSS_SHAPING_KEYS)))
  unknown = sorted(set(value) - set(LOSS_SHAPING_KEYS), key=str)
  if unknown:
    raise ValueError('%s: unknown key(s) %s (known: %s)' % (key, ', '.join(repr(k) for k in unknown), ', '.join(LOSS_SHAPING_KEYS)))
  real = lambda v: isinstance(v, numbers.Real) and not isinstance(v, bool) and math.isfinite(float(v))
  f32max = float(np.finfo(np.float32).max)
  cartesian = cfg.control_mode == 'cartesian'
  sw = value.get('sample_weights')
  if sw is not None and not isinstance(sw, bool):
    raise ValueError("%s['sample_weights']=%r: True or False" % (key, sw))
  cw = value.get('grp_class_weights')
  if cw is not None:
    if not cartesian:
      raise ValueError("%s['grp_class_weights']: control_mode=%r has no gripper classes (cartesian mode only)" % (key, cfg.control_mode))
    if isinstance(cw, (str, bytes)) or not isinstance(cw, (collections.abc.Sequence, np.ndarray)) or len(cw) != cfg.num_grp_states or \
        not all(real(v) and 0.0 <= float(v) <= f32max for v in cw):
      raise ValueError("%s['grp_class_weights']=%r: %d finite weights >= 0, one per gripper class" % (key, cw, cfg.num_grp_states))
    cw = tuple(float(v) for v in cw)
    if all(v == 1.0 for v in cw):
      cw = None
  eps = value.get('label_smoothing')
  if eps is None:
    eps = 0.0
  if not real(eps) or not 0.0 <= float(eps) < 1.0:
    raise ValueError("%s['label_smoothing']=%r: a float in [0, 1)" % (key, eps))
  if float(eps) != 0.0 and not cartesian:
    raise ValueError("%s['label_smoothing']: control_mode=%r has no cross-entropy head (cartesian mode only)" % (key, cfg.control_mode))
  heads = regression_prediction_keys(cfg)
  hd = value.get('huber_delta')
  ok = lambda v: real(v) and 0.0 < float(v) <= f32max
  if hd is None:
    hd = {}
  elif isinstance(hd, collections.abc.Mapping):
    bad = sorted(set(hd) - set(heads), key=str)
    if bad:
      raise ValueError("%s['huber_delta']: %s is no regression head of control_mode=%r (heads: %s)"
                       % (key, ', '.join(repr(k) for k in bad), cfg.control_mode, ', '.join(heads)))
    for k, v in hd.items():
      if not ok(v):
        raise ValueError("%s['huber_delta'][%r]=%r: a finite float > 0" % (key, k, v))
    hd = {k: float(hd[k]) for k in heads if k in hd}
  elif ok(hd):
    hd = {k: float(hd) for k in heads}
  else:
    raise ValueError("%s['huber_delta']=%r: a finite float > 0, or {prediction key: delta}" % (key, hd))
  if not sw and cw is None and float(eps) == 0.0 and not hd:
    return None
  return dict(sample_weights=bool(sw), grp_class_weights=cw, label_smoothing=float(eps), huber_delta=hd)


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


def check_lr_multipliers(value, names, key='lr_multipliers'):
  """Per-variable learning-rate multipliers.  ``value``: None or an empty mapping = off (returns None); else an ordered
  mapping {regular expression: multiplier}.  A variable of ``names`` takes the multiplier of the FIRST expression that ``re.search``
  finds in its name, 1 if none does; a multiplier is a finite number >= 0 that float32 holds, 0 = the variable is frozen.  Returns
  {name: float} in the order of ``names``, or None when every variable ends up at exactly 1 (that model is the model without the
  option).  An expression that matches no variable, or anything else, raises ValueError naming ``key``."""
  if value is None or (isinstance(value, collections.abc.Mapping) and not value):
    return None
  if not isinstance(value, collections.abc.Mapping):
    raise ValueError('%s=%r: must be None or a mapping {regular expression: multiplier}' % (key, value))
  names = list(names)
  patterns = []
  for pat, mul in value.items():
    if not isinstance(pat, str):
      raise ValueError('%s: the pattern %r is not a string' % (key, pat))
    try:
      rx = re.compile(pat)
    except re.error as e:
      raise ValueError('%s: the pattern %r is not a regular expression: %s' % (key, pat, e))
    if isinstance(mul, (bool, np.bool_)) or not isinstance(mul, numbers.Real) or not 0.0 <= float(mul) <= float(np.finfo(np.float32).max):
      raise ValueError('%s: %r: the multiplier %r must be a finite number >= 0 that float32 holds (0 = frozen)' % (key, pat, mul))
    if not any(rx.search(n) for n in names):
      raise ValueError('%s: the pattern %r matches no variable of the model' % (key, pat))
    patterns.append((rx, float(np.float32(mul))))
  out = collections.OrderedDict()
  for n in names:
    out[n] = next((mul for rx, mul in patterns if rx.search(n)), 1.0)
  return None if all(mul == 1.0 for mul in out.values()) else out


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


LR_KINDS = ('constant', 'exponential', 'cosine', 'piecewise')
LR_BOUNDARIES_MAX = 8      # GEECO_LR_BOUNDARIES_MAX of include/geeco_hip.h
_LR_FIELDS = ('kind', 'warmup_steps', 'decay_steps', 'decay_rate', 'alpha', 'staircase', 'boundaries', 'values')


def check_lr_schedule(value, base_lr, key='lr_schedule'):
  """The learning-rate schedule the device evaluates from its step counter.  ``value``: None, or a mapping with 'kind'
  ('constant', 'exponential', 'cosine', 'piecewise') and of 'warmup_steps', 'decay_steps', 'decay_rate', 'staircase', 'alpha',
  'boundaries', 'values' those the kind uses; ``base_lr``: the constant rate it starts from (cfg.lr).  None, or 'constant' without
  warm-up, is off and returns None; else the normalised schedule, a dictionary with every field (``ops.lr_schedule_struct`` takes
  it).  Anything else raises ValueError naming ``key`` and the offending field."""
  if value is None:
    return None

  def bad(field, why):
    return ValueError('%s: %s=%r: %s' % (key, field, value.get(field) if isinstance(value, collections.abc.Mapping) else value, why))

  def whole(field, least, default=None):
    x = value.get(field, default)
    if isinstance(x, bool) or not isinstance(x, numbers.Integral) or not least <= int(x) < 2 ** 62:
      raise bad(field, 'must be a whole number >= %d' % least)
    return int(x)

  def rate(field, x, above_zero=False, most=float(np.finfo(np.float32).max)):
    ok = not isinstance(x, bool) and isinstance(x, numbers.Real) and 0.0 <= float(x) <= most and not (above_zero and float(np.float32(x)) <= 0.0)
    if not ok:
      raise bad(field, 'must be a finite number %s that float32 holds' % ('> 0' if above_zero else ('in [0, 1]' if most == 1.0 else '>= 0')))
    return float(x)

  if not isinstance(value, collections.abc.Mapping):
    raise bad('value', "must be None or a mapping with 'kind' and the fields the kind uses")
  for field in value:
    if field not in _LR_FIELDS:
      raise ValueError('%s: unknown field %r (known: %s)' % (key, field, ', '.join(_LR_FIELDS)))
  kind = value.get('kind')
  if not isinstance(kind, str) or kind not in LR_KINDS:
    raise bad('kind', 'must be one of %s' % ', '.join(LR_KINDS))
  out = dict(kind=kind, base_lr=0.0, warmup_steps=whole('warmup_steps', 0, 0), decay_steps=1, decay_rate=1.0, alpha=0.0, staircase=False,
             boundaries=(), values=())
  if kind == 'piecewise':      # base_lr is ignored
    boundaries, values = value.get('boundaries', ()), value.get('values')
    if isinstance(boundaries, (str, bytes)) or not isinstance(boundaries, collections.abc.Sequence) or len(boundaries) > LR_BOUNDARIES_MAX:
      raise bad('boundaries', 'must be a sequence of at most %d step counts' % LR_BOUNDARIES_MAX)
    for i, b in enumerate(boundaries):
      if isinstance(b, bool) or not isinstance(b, numbers.Integral) or abs(int(b)) >= 2 ** 62 or (i and int(b) <= int(boundaries[i - 1])):
        raise bad('boundaries', 'must be whole numbers, strictly increasing (entry %d)' % i)
    if isinstance(values, (str, bytes)) or not isinstance(values, collections.abc.Sequence) or len(values) != len(boundaries) + 1:
      raise bad('values', 'must be a sequence of %d rates, one more than boundaries' % (len(boundaries) + 1))
    out['boundaries'] = tuple(int(b) for b in boundaries)
    out['values'] = tuple(rate('values', v) for v in values)
    return out
  if isinstance(base_lr, bool) or not isinstance(base_lr, numbers.Real) or not 0.0 <= float(base_lr) <= float(np.finfo(np.float32).max):
    raise ValueError('%s: base_lr=%r (the configured lr) must be a finite number >= 0 that float32 holds' % (key, base_lr))
  out['base_lr'] = float(base_lr)
  if kind == 'constant':
    return out if out['warmup_steps'] else None
  out['decay_steps'] = whole('decay_steps', 1)
  if kind == 'exponential':
    out['decay_rate'] = rate('decay_rate', value.get('decay_rate'), above_zero=True)
    staircase = value.get('staircase', False)
    if not isinstance(staircase, (bool, np.bool_)):
      raise bad('staircase', 'must be True or False')
    out['staircase'] = bool(staircase)
  else:
    out['alpha'] = rate('alpha', value.get('alpha', 0.0), most=1.0)
  return out


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
