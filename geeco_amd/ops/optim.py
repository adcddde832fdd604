"""The optimiser: Adam, learning-rate schedules, clipping, the non-finite guard, accumulation (csrc/adam.hip, lr_schedule.hip,
clip.hip, guard.hip, grad_accum.hip)."""
from __future__ import annotations

import ctypes

import torch

from .. import _native
from .._native import check
from ._marshal import _adam_segments, _lib, _p, _stream


def adam_prepare(global_step, lr, scal, beta1=0.9, beta2=0.999):
  check(_lib().geeco_adam_prepare(_p(global_step), lr, beta1, beta2, _p(scal), _stream()), 'geeco_adam_prepare')


def lr_schedule_struct(schedule):
  """``geeco_lr_schedule`` of a normalised schedule (the dictionary ``train_options.check_lr_schedule`` returns); a struct is passed
  through.  Rates and values are rounded to float32 here: the struct is what the device evaluates."""
  if isinstance(schedule, _native.LrSchedule):
    return schedule
  st = _native.LrSchedule()
  st.kind = _native.LR_KINDS.index(schedule['kind'])
  st.base_lr, st.decay_rate, st.alpha = schedule['base_lr'], schedule['decay_rate'], schedule['alpha']
  st.warmup_steps, st.decay_steps, st.staircase = schedule['warmup_steps'], schedule['decay_steps'], int(bool(schedule['staircase']))
  boundaries, values = schedule['boundaries'], schedule['values']
  if len(boundaries) > _native.LR_BOUNDARIES_MAX or (schedule['kind'] == 'piecewise' and len(values) != len(boundaries) + 1):
    raise ValueError('lr_schedule_struct: %d boundaries (at most %d) need one value more, got %d'
                     % (len(boundaries), _native.LR_BOUNDARIES_MAX, len(values)))
  st.n_boundaries = len(boundaries)
  for i, b in enumerate(boundaries):
    st.boundaries[i] = b
  for i, v in enumerate(values[:_native.LR_BOUNDARIES_MAX + 1]):
    st.values[i] = v
  return st


def lr_schedule_eval(schedule, step):
  """``geeco_lr_schedule_eval``: lr(step) of the schedule in float64, on the host, by the function the device evaluates."""
  out = ctypes.c_double()
  check(_lib().geeco_lr_schedule_eval(ctypes.byref(lr_schedule_struct(schedule)), int(step), ctypes.byref(out)), 'geeco_lr_schedule_eval')
  return out.value


def _scal_holds_lr(scal):
  if scal.numel() < 3:
    raise ValueError('a learning-rate schedule stores lr in scal[2]: scal holds %d floats' % scal.numel())


def adam_prepare_schedule(global_step, schedule, scal, beta1=0.9, beta2=0.999):
  """``geeco_adam_prepare_schedule``: adam_prepare with lr(s) of ``schedule`` at the step the counter is advanced to; scal[2] = lr(s)."""
  _scal_holds_lr(scal)
  check(_lib().geeco_adam_prepare_schedule(_p(global_step), ctypes.byref(lr_schedule_struct(schedule)), beta1, beta2, _p(scal), _stream()),
        'geeco_adam_prepare_schedule')


def adam_tf(p, g, m, v, n, scal, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0, l2=0.0):
  check(_lib().geeco_adam_tf(_p(p), _p(g), _p(m), _p(v), n, _p(scal), beta1, beta2, eps, grad_scale, l2, _stream()),
        'geeco_adam_tf')


def adam_tf_ema(p, g, m, v, ema, n, scal, global_step, decay, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0, l2=0.0):
  """``geeco_adam_tf_ema``: adam_tf, and the shadow arena ``ema`` follows the new parameters in the same pass."""
  check(_lib().geeco_adam_tf_ema(_p(p), _p(g), _p(m), _p(v), _p(ema), n, _p(scal), _p(global_step), decay, beta1, beta2, eps, grad_scale,
                                 l2, _stream()), 'geeco_adam_tf_ema')


def adam_tf_segments(p, m, v, segments, scal, g_out=None, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0, l2=0.0):
  """``geeco_adam_tf_segments``: the Adam update of up to 8 pieces of the arena, ``segments`` = [(gradient tensor of the piece, offset
  in the arena, count)], offsets / counts in floats and multiples of 4; ``g_out``: the gradient arena that also receives the pieces'
  gradients (a piece whose source IS its place in that arena needs none)."""
  arr = _adam_segments(segments)
  check(_lib().geeco_adam_tf_segments(_p(p), _p(g_out), _p(m), _p(v), arr, len(segments), _p(scal), beta1, beta2, eps, grad_scale, l2,
                                      _stream()), 'geeco_adam_tf_segments')


def adam_tf_segments_ema(p, m, v, ema, segments, scal, global_step, decay, g_out=None, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0,
                         l2=0.0):
  """``geeco_adam_tf_segments_ema``: adam_tf_segments, and the pieces' part of the shadow arena ``ema`` (indexed like ``p``) follows."""
  arr = _adam_segments(segments)
  check(_lib().geeco_adam_tf_segments_ema(_p(p), _p(g_out), _p(m), _p(v), _p(ema), arr, len(segments), _p(scal), _p(global_step), decay,
                                          beta1, beta2, eps, grad_scale, l2, _stream()), 'geeco_adam_tf_segments_ema')


def clip_ws_floats(n):
  """Partial sums ``grad_sumsq_segments`` writes for an arena of ``n`` floats (one per fixed chunk)."""
  return int(_lib().geeco_clip_ws_floats(int(n)))


def grad_sumsq_segments(partials, p, segments, n, grad_scale=1.0, l2=0.0):
  """``geeco_grad_sumsq_segments``: partials[k] = sum of (g * grad_scale + l2 * p)^2 over chunk k of the arena [0, n); the gradient of an
  element comes from the piece of ``segments`` (as ``adam_tf_segments`` takes them, but any offset and count) that covers it, an
  element no piece covers adds 0.  Any partition of the same elements gives bitwise the same partials.  ``p`` may be None when l2 == 0."""
  if partials.numel() < clip_ws_floats(n):
    raise ValueError('grad_sumsq_segments: %d partials for an arena of %d floats, %d needed' % (partials.numel(), n, clip_ws_floats(n)))
  arr = _adam_segments(segments)
  check(_lib().geeco_grad_sumsq_segments(_p(p), arr, len(segments), int(n), grad_scale, l2, _p(partials), _stream()),
        'geeco_grad_sumsq_segments')


def clip_scale(out2, partials, nchunks, clip):
  """``geeco_clip_scale``: out2[0] = clip / max(norm, clip), out2[1] = norm = sqrt(sum of the first ``nchunks`` partials)."""
  if out2.numel() < 2 or partials.numel() < nchunks:
    raise ValueError('clip_scale: out2 holds 2 floats, partials at least nchunks = %d' % nchunks)
  check(_lib().geeco_clip_scale(_p(partials), int(nchunks), clip, _p(out2), _stream()), 'geeco_clip_scale')


def adam_tf_segments_clip(p, m, v, segments, scal, clip_dev, ema=None, global_step=None, decay=0.0, g_out=None, beta1=0.9, beta2=0.999,
                          eps=1e-8, grad_scale=1.0, l2=0.0):
  """``geeco_adam_tf_segments_clip``: adam_tf_segments (``ema`` None) or adam_tf_segments_ema on the total gradient times
  ``clip_dev[0]`` (clip_scale's out2).  Offsets are multiples of 4 floats, counts any number >= 1: the whole arena is one piece."""
  arr = _adam_segments(segments)
  check(_lib().geeco_adam_tf_segments_clip(_p(p), _p(g_out), _p(m), _p(v), _p(ema), arr, len(segments), _p(scal), _p(global_step), decay,
                                           _p(clip_dev), beta1, beta2, eps, grad_scale, l2, _stream()), 'geeco_adam_tf_segments_clip')


def guard_decide(out2, guard, partials, nchunks, clip=0.0):
  """``geeco_guard_decide``: norm = sqrt(sum of the first ``nchunks`` partials) as ``clip_scale`` forms it.  Finite: out2 = [clip_scale's s
  (``clip`` > 0) or 1.0 (``clip`` == 0), norm], guard = [1, total, 0]; not finite: out2 = [0, norm], guard = [0, total + 1, consecutive + 1].
  ``guard``: three int64 on the device."""
  if out2.numel() < 2 or partials.numel() < nchunks or guard.numel() < 3 or guard.dtype != torch.int64:
    raise ValueError('guard_decide: out2 holds 2 floats, guard 3 int64, partials at least nchunks = %d' % nchunks)
  check(_lib().geeco_guard_decide(_p(partials), int(nchunks), clip, _p(out2), _p(guard), _stream()), 'geeco_guard_decide')


def adam_tf_segments_guard(p, m, v, segments, scal, clip_dev, guard, ema=None, global_step=None, decay=0.0, g_out=None, beta1=0.9, beta2=0.999,
                           eps=1e-8, grad_scale=1.0, l2=0.0):
  """``geeco_adam_tf_segments_guard``: ``adam_tf_segments_clip`` when ``guard[0]`` (guard_decide's verdict) is 1; when it is 0 only ``g_out``
  is written and p, m, v and ``ema`` keep every bit."""
  arr = _adam_segments(segments)
  check(_lib().geeco_adam_tf_segments_guard(_p(p), _p(g_out), _p(m), _p(v), _p(ema), arr, len(segments), _p(scal), _p(global_step), decay,
                                            _p(clip_dev), _p(guard), beta1, beta2, eps, grad_scale, l2, _stream()), 'geeco_adam_tf_segments_guard')


def adam_tf_segments_scaled(p, m, v, segments, lr_mul, scal, clip_dev=None, guard=None, ema=None, global_step=None, decay=0.0, g_out=None,
                            beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0, l2=0.0):
  """``geeco_adam_tf_segments_scaled``: the update of ``adam_tf_segments_guard`` with piece k at ``scal[0] * lr_mul[k]`` (``lr_mul``: one
  finite number > 0 per piece; a frozen piece is one that is left out).  ``clip_dev`` None: the gradient is not scaled; ``guard`` None:
  the step is always applied.  Every multiplier 1.0 gives bitwise the entry point without multipliers."""
  arr = _adam_segments(segments)
  if len(lr_mul) != len(segments):
    raise ValueError('adam_tf_segments_scaled: %d pieces with %d multipliers' % (len(segments), len(lr_mul)))
  mul = (ctypes.c_float * len(segments))(*[float(x) for x in lr_mul])
  check(_lib().geeco_adam_tf_segments_scaled(_p(p), _p(g_out), _p(m), _p(v), _p(ema), arr, mul, len(segments), _p(scal), _p(global_step), decay,
                                             _p(clip_dev), _p(guard), beta1, beta2, eps, grad_scale, l2, _stream()),
        'geeco_adam_tf_segments_scaled')


def grad_accumulate_segments(acc, segments, n, overwrite):
  """``geeco_grad_accumulate_segments``: the pieces of ``segments`` (as ``adam_tf_segments_clip`` takes them) stored into
  (``overwrite``: the accumulator is not read) or added to the accumulator arena ``acc`` of ``n`` floats; what no piece covers keeps
  every bit."""
  if acc.numel() < n:
    raise ValueError('grad_accumulate_segments: an accumulator of %d floats for an arena of %d' % (acc.numel(), n))
  arr = _adam_segments(segments)
  check(_lib().geeco_grad_accumulate_segments(_p(acc), arr, len(segments), int(n), int(bool(overwrite)), _stream()),
        'geeco_grad_accumulate_segments')


def sumsq_into(out, p, n):
  check(_lib().geeco_sumsq(_p(p), n, _p(out), _stream()), 'geeco_sumsq')
