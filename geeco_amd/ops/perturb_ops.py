"""Perturbation attributions (csrc/perturbation.hip; geeco_amd/perturbation.py)."""
from __future__ import annotations

import ctypes

from .. import _native
from .._native import check
from ._marshal import _lib, _p, _stream
from .attr_ops import _attr_flat, _attr_period


def perturb_desc(method, H, W, patch=None, stride=None, grid=None, keep_prob=None, key=0):
  """The geeco_perturb_desc of an occlusion grid (``patch`` = (ph, pw), ``stride`` = (sy, sx)) or of RISE masks (``grid`` = g in
  2..31, ``keep_prob`` in (0, 1), ``key``: the generator's 64-bit key) on H x W images.  ValueError for what no kernel serves.  The
  keep probability becomes the integer threshold a 32-bit word is compared with: round(keep_prob * 2^32) within 1 .. 2^32 - 1."""
  if method not in _native.PERTURB_METHODS:
    raise ValueError('perturb_desc: method=%r must be one of %s' % (method, ', '.join(repr(m) for m in _native.PERTURB_METHODS)))
  if min(int(H), int(W)) < 1 or int(H) * int(W) > 1 << 28:
    raise ValueError('perturb_desc: H=%r, W=%r' % (H, W))
  d = _native.PerturbDesc(method=_native.PERTURB_METHODS.index(method), H=int(H), W=int(W), ph=1, pw=1, sy=1, sx=1, grid=2, keep_threshold=1)
  if method == 'occlusion':
    try:
      (ph, pw), (sy, sx) = patch, stride
      ok = all(int(v) == v and 1 <= int(v) < 1 << 30 for v in (ph, pw, sy, sx))
    except (TypeError, ValueError):
      ok = False
    if not ok:
      raise ValueError('perturb_desc: patch=%r and stride=%r must be pairs of integers >= 1' % (patch, stride))
    d.ph, d.pw, d.sy, d.sx = int(ph), int(pw), int(sy), int(sx)
  else:
    if grid is None or int(grid) != grid or not 2 <= int(grid) <= 31:
      raise ValueError('perturb_desc: grid=%r must be an integer in 2..31' % (grid,))
    if keep_prob is None or not 0.0 < float(keep_prob) < 1.0:
      raise ValueError('perturb_desc: keep_prob=%r must lie in (0, 1)' % (keep_prob,))
    if not 0 <= int(key) < 1 << 64:
      raise ValueError('perturb_desc: key=%r outside 64 bits' % (key,))
    d.grid, d.key = int(grid), int(key)
    d.keep_threshold = min(max(int(round(float(keep_prob) * 2.0 ** 32)), 1), (1 << 32) - 1)
  return d


def perturb_patch(desc, step=0):
  """(Gy, Gx, (y0, y1, x0, x1)): the grid of an occlusion description and the patch of ``step`` (host only; RISE: 0, 0 and an empty
  patch)."""
  if int(step) != step or not 0 <= int(step) < 1 << 31:
    raise ValueError('perturb_patch: step=%r' % (step,))
  out = (ctypes.c_int32 * 6)()
  check(_lib().geeco_perturb_patch(ctypes.addressof(desc), int(step), out), 'geeco_perturb_patch')
  return out[0], out[1], tuple(out[2:6])


def perturb_steps(desc):
  """Gy * Gx of an occlusion description."""
  Gy, Gx, _ = perturb_patch(desc)
  return Gy * Gx


def _check_step(who, desc, step, sample0):
  if not isinstance(desc, _native.PerturbDesc):
    raise ValueError('%s: desc must come from perturb_desc' % who)
  if int(step) != step or not 0 <= int(step) < 1 << 31 or int(sample0) != sample0 or not 0 <= int(sample0) < 1 << 31:
    raise ValueError('%s: step=%r, sample0=%r must be integers >= 0' % (who, step, sample0))
  if desc.method == 0 and int(step) >= perturb_steps(desc):
    raise ValueError('%s: step=%d outside the grid of %d positions' % (who, step, perturb_steps(desc)))


def perturb_apply_into(dst, x, fill, desc, step, prev_step=-1, sample0=0):
  """dst <- x occluded by step ``step`` of ``desc`` (include/geeco_hip.h: geeco_perturb_apply): x where o == 0, fill where o == 1,
  x + o * (fill - x) otherwise, fill = ``fill``[i % fill.numel()] (None: zeros).  dst / x: [N][frames][H][W][C] (or [N][H][W][C]).
  ``prev_step`` >= 0 (occlusion): dst holds that step's result; only the two patches are written.  ``sample0``: the number of the
  first sample in the random draws.  Bad arguments raise ValueError before anything is queued."""
  n = _attr_flat('perturb_apply', dst=dst, x=x, fill=fill)
  _check_step('perturb_apply', desc, step, sample0)
  if x.dim() not in (4, 5) or tuple(dst.shape) != tuple(x.shape) or n['x'] < 1:
    raise ValueError('perturb_apply: dst %s for x %s ([N][frames][H][W][C] or [N][H][W][C])' % (tuple(dst.shape), tuple(x.shape)))
  N, frames = int(x.shape[0]), (int(x.shape[1]) if x.dim() == 5 else 1)
  H, W, C = (int(v) for v in x.shape[-3:])
  if (H, W) != (desc.H, desc.W) or not 1 <= C <= 4 or N > 65535:
    raise ValueError('perturb_apply: x %s for a description of %d x %d images (C in 1..4, N <= 65535)' % (tuple(x.shape), desc.H, desc.W))
  if int(prev_step) != prev_step or int(prev_step) < -1 or (desc.method == 0 and int(prev_step) >= perturb_steps(desc)):
    raise ValueError('perturb_apply: prev_step=%r (-1, or a step of the grid)' % (prev_step,))
  period = _attr_period('perturb_apply', fill, n['x'])
  check(_lib().geeco_perturb_apply(_p(dst), _p(x), _p(fill), period, ctypes.addressof(desc), int(step), int(prev_step), int(sample0), N,
                                   frames, C, _stream()), 'geeco_perturb_apply')


def perturb_score_into(d, preds, preds0, w):
  """d[n] <- sum_j w[j] * (preds[n][j] - preds0[n][j])^2, j ascending, every operation rounded to float32."""
  n = _attr_flat('perturb_score', d=d, preds=preds, preds0=preds0, w=w)
  if preds.dim() != 2 or tuple(preds.shape) != tuple(preds0.shape) or n['preds'] < 1 or n['d'] != preds.shape[0] or n['w'] != preds.shape[1]:
    raise ValueError('perturb_score: d of %d, w of %d floats for preds %s and preds0 %s' % (n['d'], n['w'], tuple(preds.shape), tuple(preds0.shape)))
  check(_lib().geeco_perturb_score(_p(d), _p(preds), _p(preds0), _p(w), int(preds.shape[0]), int(preds.shape[1]), _stream()), 'geeco_perturb_score')


def perturb_accumulate_into(num, den, d, desc, step, overwrite, sample0=0):
  """num / den [N][H][W] <- (0 if overwrite else num / den) + d[n] * o / o where step ``step`` of ``desc`` hid the pixel (o != 0)."""
  n = _attr_flat('perturb_accumulate', num=num, den=den, d=d)
  _check_step('perturb_accumulate', desc, step, sample0)
  if num.dim() != 3 or tuple(num.shape) != tuple(den.shape) or tuple(num.shape[1:]) != (desc.H, desc.W) or n['d'] != num.shape[0] or \
     not 1 <= num.shape[0] <= 65535:
    raise ValueError('perturb_accumulate: num %s, den %s, d of %d floats for a description of %d x %d images'
                     % (tuple(num.shape), tuple(den.shape), n['d'], desc.H, desc.W))
  check(_lib().geeco_perturb_accumulate(_p(num), _p(den), _p(d), ctypes.addressof(desc), int(step), int(sample0), int(num.shape[0]),
                                        1 if overwrite else 0, _stream()), 'geeco_perturb_accumulate')


def perturb_finish_into(saliency, num, den):
  """saliency <- num / den where den > 0, +0 elsewhere."""
  n = _attr_flat('perturb_finish', saliency=saliency, num=num, den=den)
  if not n['saliency'] == n['num'] == n['den'] or n['num'] < 1:
    raise ValueError('perturb_finish: saliency / num / den of %d / %d / %d floats' % (n['saliency'], n['num'], n['den']))
  check(_lib().geeco_perturb_finish(_p(saliency), _p(num), _p(den), n['num'], _stream()), 'geeco_perturb_finish')
