"""Float64 restatement of the learning-rate schedules, written from the table of semantics and not from the C function.

s = the number of completed updates (t - 1 for the t of Adam's bias correction), w = warmup_steps, u = s - w:
  s <  w   lr(s) = L0 (s + 1) / w, L0 = base_lr, or values[0] for 'piecewise'
  s >= w   constant     base_lr
           exponential  base_lr decay_rate^(u / decay_steps); staircase: the exponent is floor(u / decay_steps)
           cosine       base_lr ((1 - alpha) 0.5 (1 + cos(pi min(u, decay_steps) / decay_steps)) + alpha)
           piecewise    values[i] for the first i with u <= boundaries[i], else values[n]
Rates and values enter after rounding to float32, as the device holds them; step counts are integers of any size.
"""
import math

import numpy as np


def f32(x):
  """The float32 nearest to x, as a Python float (exact in float64)."""
  return float(np.float32(x))


def schedule(kind, base_lr=0.0, warmup_steps=0, decay_steps=1, decay_rate=1.0, alpha=0.0, staircase=False, boundaries=(), values=()):
  """A schedule with every field, as ``geeco_amd.variables.check_lr_schedule`` normalises one (``ops.lr_schedule_struct`` takes it)."""
  return dict(kind=kind, base_lr=base_lr, warmup_steps=warmup_steps, decay_steps=decay_steps, decay_rate=decay_rate, alpha=alpha,
              staircase=staircase, boundaries=tuple(boundaries), values=tuple(values))


def lr_at(sch, s):
  """lr(s) in float64."""
  s, w = int(s), int(sch['warmup_steps'])
  base = f32(sch['base_lr'])
  if s < w:
    first = f32(sch['values'][0]) if sch['kind'] == 'piecewise' else base
    return first * (float(s + 1) / float(w))      # (the fraction first: the last warm-up step is L0 exactly)
  u = s - w
  if sch['kind'] == 'constant':
    return base
  if sch['kind'] == 'exponential':
    ds = int(sch['decay_steps'])
    exponent = float(u // ds) if sch['staircase'] else float(u) / float(ds)
    return base * math.pow(f32(sch['decay_rate']), exponent)
  if sch['kind'] == 'cosine':
    ds, a = int(sch['decay_steps']), f32(sch['alpha'])
    return base * ((1.0 - a) * 0.5 * (1.0 + math.cos(math.pi * float(min(u, ds)) / float(ds))) + a)
  if sch['kind'] == 'piecewise':
    for b, v in zip(sch['boundaries'], sch['values']):
      if u <= int(b):
        return f32(v)
    return f32(sch['values'][len(sch['boundaries'])])
  raise ValueError(sch['kind'])


def lr_t_at(sch, s, beta1=0.9, beta2=0.999):
  """Adam's lr_t of the step that follows s completed updates (t = s + 1): lr(s) sqrt(1 - beta2^t) / (1 - beta1^t), float64."""
  t = float(int(s) + 1)
  return lr_at(sch, s) * math.sqrt(1.0 - math.pow(f32(beta2), t)) / (1.0 - math.pow(f32(beta1), t))
