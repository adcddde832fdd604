"""The opt-ins of the training step: their checks, the record they travel in, and the table of what excludes what.

An option enters as a raw value under its public name -- a keyword of ``graph.E2EVMC`` / ``graph.GoalE2EVMC``, or an entry of the
Estimator's ``params`` -- is checked ONCE, by ``TrainOptions.from_raw``, and is handed on as one field of that record.  Which option
refuses which other option, data parallelism or ``shared_frames`` is ``EXCLUSIONS``, read by ``check_exclusions``.  The ``check_*``
functions are the options' value checks: each returns the normalised value (None = the option is off) or raises ValueError naming
``key``.  Adding an option: DESIGN.md 5.24.
"""
from __future__ import annotations

import collections
import collections.abc
import math
import numbers
import re

import numpy as np

from ._native import LR_BOUNDARIES_MAX, LR_KINDS      # GEECO_LR_* of include/geeco_hip.h (importing _native loads no library)


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



# public name of an option (constructor keyword, key of ``params``) -> the field of TrainOptions that holds its normalised value
FIELDS = collections.OrderedDict([
    ('ema_decay', 'ema_decay'), ('clip_norm', 'clip_norm'), ('lr_schedule', 'lr_schedule'), ('skip_nonfinite', 'skip_limit'),
    ('lr_multipliers', 'lr_multipliers'), ('variable_stats', 'variable_stats_mode'), ('loss_shaping', 'loss_shaping'),
    ('grad_accum_steps', 'grad_accum')])
# how messages word an option's name: a constructor's keyword, or the entry of the Estimator's params
KEYWORD, PARAMS = '%s', "params['%s']"


class TrainOptions(collections.namedtuple('TrainOptions', list(FIELDS.values()), defaults=(None,) * len(FIELDS))):
  """The normalised options of one model, immutable; None in every field is the model without options.  By public name:

  ``ema_decay`` (a float in (0, 1); None / 0 = off): the optimiser step also keeps an exponential moving average of the
  parameters in ``store.ema`` (tf.train.ExponentialMovingAverage with num_updates = global_step); a store passed in
  must have been built with the arena (``build_store(..., ema=True)``).
  ``clip_norm`` (a finite number > 0; None / 0 = off): the optimiser step clips the total gradient g / world + l2 * p by its global norm
  first (tf.clip_by_global_norm), on the device; ``clip_out`` then holds [scale, norm before clipping] of the last step.
  ``lr_schedule`` (``check_lr_schedule``; None, or 'constant' without warm-up = off): the learning rate of every step is the
  schedule's value at the device's step counter, with ``cfg.lr`` as its base rate, evaluated by the thread that forms Adam's lr_t
  (DESIGN 5.18): a captured step follows it and a restored counter continues it; ``scal[2]`` then holds the rate of the last step.
  ``skip_nonfinite`` (True, or the tolerated number of consecutive skipped steps, an integer >= 1; None / False = off; field
  ``skip_limit``): an optimiser step whose gradient has a non-finite global norm leaves p, m, v and the shadow arena as they are --
  the step counter still advances; ``guard`` then holds [last verdict, skipped steps in all, in a row] and ``clip_out``
  [scale, norm].
  ``lr_multipliers`` (``check_lr_multipliers``: an ordered mapping {regular expression: multiplier}, first match wins, 0 =
  frozen; None, empty or all ones = off): every variable is updated with lr * its multiplier inside the one Adam pass, a frozen
  variable's p, m, v and averaged weight keep every bit, and the backward stops at the lowest layer with anything to train
  (``backward_cut``).
  ``variable_stats`` (True, or 'histograms'; None / False = off; field ``variable_stats_mode``): ``variable_stats()`` reports, per
  variable, the norms and counts of the last step's gradient, weights and update from one statistics pass on the device (DESIGN
  5.21).  The step itself is unchanged.
  ``loss_shaping`` (``check_loss_shaping``; None or all-neutral = off): the losses take tf.losses' optional arguments (DESIGN
  5.22) -- ``sample_weights``: a weight per sample, the input 'sample_weight' [N] (a label; ones until fed); ``grp_class_weights``: a weight
  per gripper class; ``label_smoothing``; ``huber_delta``: Huber in place of MSE on the named regression heads.  Means run over the samples
  whose weight is not zero; ``loss_parts()`` reports the shaped terms.  Same launches as without it.
  ``grad_accum_steps`` (an integer A >= 2; None / 1 = off; field ``grad_accum``): one optimiser step per A micro-batches
  -- each micro-step's gradient is stored into / added to ``store.accum`` by one launch, and the A-th runs the optimiser step, every
  option with it, on the accumulator with grad_scale 1 / A: the mean of the micro-batch gradients.  ``micro_step()`` /
  ``runtime.TrainStepRunner`` choose the form from ``store.accum_count``; ``loss_parts()`` reports the mean over the micro-batches of
  the last optimiser step.  The accumulator is not checkpointed.

  What is single-GPU and what does not go with ``shared_frames``: ``EXCLUSIONS``."""
  __slots__ = ()

  @classmethod
  def from_raw(cls, raw, cfg, names, key=KEYWORD, training=True):
    """The record of the raw values ``raw`` ({public name: value}; a name that is no option raises TypeError, as an unexpected keyword
    does), each checked once by its ``check_*``, in the order the models' constructors always checked them.  ``cfg``: the model config
    (``lr``, the base rate of the schedule, and what ``loss_shaping`` may name); ``names``: the model's variable names, for
    ``lr_multipliers``; ``key``: KEYWORD or PARAMS.  ``training`` false (a model that is not training): ``lr_multipliers``,
    ``variable_stats`` and ``grad_accum_steps`` are neither checked nor kept.  The Estimator checks its params before it knows the
    model: without ``cfg`` the schedule is checked against lr 0.0 and ``loss_shaping`` not at all, without ``names``
    ``lr_multipliers`` must be a mapping and no more; what was not checked stays None."""
    for name in raw:
      if name not in FIELDS:
        raise TypeError('got an unexpected keyword argument %r (the options: %s)' % (name, ', '.join(FIELDS)))
    get = lambda name: (raw.get(name), key % name)
    mults = raw.get('lr_multipliers')
    if names is None and mults is not None and not isinstance(mults, collections.abc.Mapping):
      raise ValueError('%s=%r: must be None or a mapping {regular expression: multiplier}' % (key % 'lr_multipliers', mults))
    return cls(loss_shaping=None if cfg is None else check_loss_shaping(raw.get('loss_shaping'), cfg, key % 'loss_shaping'),
               variable_stats_mode=check_variable_stats(*get('variable_stats')) if training else None,
               ema_decay=check_ema_decay(*get('ema_decay')), clip_norm=check_clip_norm(*get('clip_norm')),
               skip_limit=check_skip_nonfinite(*get('skip_nonfinite')),
               lr_schedule=check_lr_schedule(raw.get('lr_schedule'), getattr(cfg, 'lr', 0.0), key % 'lr_schedule'),
               grad_accum=check_grad_accum_steps(*get('grad_accum_steps')) if training else None,
               lr_multipliers=check_lr_multipliers(mults, names, key % 'lr_multipliers') if training and names is not None else None)

  @classmethod
  def from_params(cls, params, cfg, names):
    """``from_raw`` of the options among the Estimator's ``params``, worded as params['...']."""
    return cls.from_raw({name: params[name] for name in FIELDS if name in params}, cfg, names, PARAMS)

  def for_mode(self, mode):
    """What the model of an Estimator mode (``estimator.ModeKeys``' values) takes: 'train' everything; 'eval' ``loss_shaping`` alone (the
    reference builds the same loss in TRAIN and EVAL); 'infer' nothing (PREDICT forms no loss)."""
    return self if mode == 'train' else TrainOptions(loss_shaping=self.loss_shaping if mode == 'eval' else None)


# What excludes what.  Each row: (public name, the entries of the option the rule is about (None: the option as a whole), what it does
# not go with, the reason -- the one sentence behind "<key> is single-GPU: [with W ranks ]" / "<key> with <shared_frames>: ").  What:
# 'ranks' = more than one rank; 'dp' = the three-part data-parallel step, so also one rank with ``TrainStepRunner(dp=True)``;
# 'shared_frames'.  The last row is ``shared_frames`` itself, which is no field of the record.
EXCLUSIONS = (
    ('lr_multipliers', None, 'dp', "the buckets of the gradient exchange would have to shrink with the backward's cut point, which has not "
                                   "been decided"),
    ('lr_multipliers', None, 'shared_frames', 'the shared-frame backward has no cut points; drop one of the two options'),
    ('variable_stats', None, 'ranks', "where the late bucket's gradient lives after the exchange has not been decided"),
    ('loss_shaping', ('sample_weights', 'grp_class_weights'), 'ranks',
     'the global count of non-zero weights is not the sum the loss_scale arithmetic assumes, and the exchange has not been decided'),
    ('grad_accum_steps', None, 'dp', 'the micro-steps that apply nothing should skip the gradient exchange altogether, which has not been built'),
    ('shared_frames', None, 'ranks', 'the gradient exchange of the shared-frame step has not been decided'),
)


def check_exclusions(options, world=1, dp=False, shared_frames=False, key=KEYWORD):
  """Raises ValueError for the first row of ``EXCLUSIONS`` that ``options`` (a TrainOptions) runs into.  ``world``: the ranks of the
  process group; ``dp``: the data-parallel step is forced (``TrainStepRunner(dp=True)``); ``shared_frames``: whether the model has it."""
  for name, entries, what, reason in EXCLUSIONS:
    value = bool(shared_frames) if name == 'shared_frames' else getattr(options, FIELDS[name])
    if entries is not None and value is not None:
      entries = [e for e in entries if value[e]]
      value = entries or None
    if value is None or value is False:
      continue
    who = key % name + ('[%s]' % '], ['.join(repr(e) for e in entries) if entries else '')
    if what == 'shared_frames':
      if shared_frames:
        raise ValueError('%s with %s: %s' % (who, key % 'shared_frames', reason))
    elif world > 1 or (dp and what == 'dp'):
      raise ValueError('%s is single-GPU: %s%s' % (who, 'with %d ranks ' % world if world > 1 else '', reason))
