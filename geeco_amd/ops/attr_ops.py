"""Attributions (csrc/attribution.hip; geeco_amd/attribution.py)."""
from __future__ import annotations

import torch

from .._native import check
from ._marshal import _lib, _p, _stream


def _attr_flat(who, **tensors):
  """ValueError unless every given tensor is a contiguous float32 device tensor; returns their element counts."""
  for name, t in tensors.items():
    if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
      raise ValueError('%s: %s must be a contiguous float32 device tensor' % (who, name))
  return {name: (None if t is None else t.numel()) for name, t in tensors.items()}


def _attr_period(who, baseline, n):
  if baseline is None:
    return 0
  period = baseline.numel()
  if period < 1 or n % period:
    raise ValueError('%s: a baseline of %d floats does not divide the %d of the input' % (who, period, n))
  return period


def attr_path_point_into(dst, x, baseline, alpha, sigma=0.0, key=0, step=0):
  """dst <- b + alpha * (x - b) + sigma * z(key, step, i), b = baseline[i % baseline.numel()] (None: zeros); each operation rounded
  to float32 on its own, no clamp (include/geeco_hip.h: geeco_attr_path_point, with the counter layout of z).  dst and x of one
  size, not overlapping.  Bad arguments raise ValueError before anything is queued."""
  n = _attr_flat('attr_path_point', dst=dst, x=x, baseline=baseline)
  if n['dst'] != n['x'] or n['x'] < 1:
    raise ValueError('attr_path_point: dst of %d floats for x of %d' % (n['dst'], n['x']))
  if not (float(sigma) >= 0.0 and float(alpha) == float(alpha)):
    raise ValueError('attr_path_point: alpha=%r, sigma=%r (sigma >= 0, no NaN)' % (alpha, sigma))
  if not (0 <= int(key) < 1 << 64 and 0 <= int(step) < 1 << 32):
    raise ValueError('attr_path_point: key=%r outside 64 bits or step=%r outside 32' % (key, step))
  period = _attr_period('attr_path_point', baseline, n['x'])
  check(_lib().geeco_attr_path_point(_p(dst), _p(x), _p(baseline), period, float(alpha), float(sigma), int(key), int(step), n['x'],
                                     _stream()), 'geeco_attr_path_point')


def attr_accumulate_into(acc, g, weight, overwrite):
  """acc <- (0 if overwrite else acc) + weight * g, product and sum rounded to float32 on their own."""
  n = _attr_flat('attr_accumulate', acc=acc, g=g)
  if n['acc'] != n['g'] or n['g'] < 1:
    raise ValueError('attr_accumulate: acc of %d floats for g of %d' % (n['acc'], n['g']))
  check(_lib().geeco_attr_accumulate(_p(acc), _p(g), float(weight), n['g'], 1 if overwrite else 0, _stream()), 'geeco_attr_accumulate')


def attr_finish_into(attr, saliency, sample_sum, acc, x, baseline, multiply_by_input, N, frames, HW, C):
  """acc / x / attr [N][frames][HW][C] -> attr = (x - b) * acc (``multiply_by_input``) or acc; saliency [N][frames][HW] = max_c |attr|;
  sample_sum [N] in the fixed order of include/geeco_hip.h: geeco_attr_finish.  attr may be acc."""
  n = _attr_flat('attr_finish', attr=attr, saliency=saliency, sample_sum=sample_sum, acc=acc, x=x, baseline=baseline)
  if not 1 <= int(C) <= 4:
    raise ValueError('attr_finish: C=%d outside 1..4' % C)
  if min(N, frames, HW) < 1:
    raise ValueError('attr_finish: N=%d frames=%d HW=%d' % (N, frames, HW))
  pixels = N * frames * HW
  if n['attr'] != pixels * C or n['acc'] != pixels * C or n['saliency'] != pixels or n['sample_sum'] != N or \
     (multiply_by_input and n['x'] != pixels * C):
    raise ValueError('attr_finish: attr / acc / x / saliency / sample_sum of %s / %s / %s / %s / %s floats for N=%d frames=%d HW=%d C=%d'
                     % (n['attr'], n['acc'], n['x'], n['saliency'], n['sample_sum'], N, frames, HW, C))
  period = _attr_period('attr_finish', baseline, pixels * C) if multiply_by_input else 0
  check(_lib().geeco_attr_finish(_p(attr), _p(saliency), _p(sample_sum), _p(acc), _p(x), _p(baseline), period,
                                 1 if multiply_by_input else 0, N, frames, HW, C, _stream()), 'geeco_attr_finish')
