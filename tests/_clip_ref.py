"""float64 restatement of the opt-in global-norm gradient clipping, written from tf.clip_by_global_norm and
tf.train.AdamOptimizer, not from the kernels (tests/test_clip_cpu.py checks it by hand, tests/test_clip_gpu.py holds the device to it).

  G_i  = g_i * grad_scale + l2 * p_i           the total gradient, as the Adam kernels form it (float32 constants)
  norm = sqrt(sum_i G_i^2),   s = c / max(norm, c)
  Adam consumes G_i * s = g_i * (grad_scale * s) + (l2 * s) * p_i: ``_primitive_refs.adam_ref`` with both constants scaled by s.

Bounds of the clipped step = ``_primitive_refs.adam_bounds`` at the scaled constants, widened for the ONE rounding the step has on
top of the unclipped one: the kernel forms G (two products and a sum: |dG| <= 2 U (|g gs| + |l2 p|), adam_bounds' own budget)
and then rounds the product G * s once more, |d(G s)| <= U |G s| <= U Gs, Gs = |g gs s| + |l2 s p|.  (The restatement itself adds
none: it is handed float32(grad_scale), float32(l2) and the float32 s and multiplies them in float64.)  That extra U Gs goes through
adam_bounds' own formulas:
    m' = b1 m + (1 - b1) G s                        -> + U (1 - b1) Gs
    v' = b2 v + (1 - b2) (G s)^2,  d(x^2) = 2 |x| dx  -> + U (1 - b2) 2 |G s| Gs
    p' = p - lr_t m' / (sqrt(v') + eps)             -> the two through the quotient, as adam_bounds propagates its own.
"""
import numpy as np

import _primitive_refs as R

U = R.U


def _f32(x):
  return float(np.float32(x))


def total_grad(p, g, grad_scale=1.0, l2=0.0):
  """G in float64 from the float32 arrays and the float32 values of the two constants."""
  return R._f64(g) * _f32(grad_scale) + _f32(l2) * R._f64(p)


def global_norm(p, g, grad_scale=1.0, l2=0.0):
  G = total_grad(p, g, grad_scale, l2)
  return float(np.sqrt(np.sum(G * G)))


def clip_scale(norm, c):
  """s = c / max(norm, c): 1 whenever norm <= c."""
  c = _f32(c)
  return c / max(float(norm), c)


def clipped_adam_ref(p, g, m, v, lr_t, s, b1=0.9, b2=0.999, eps=1e-8, grad_scale=1.0, l2=0.0):
  """One clipped update in float64: p', m', v'.  ``s``: the scale (the float32 value the device holds, or clip_scale's).  The constants
  are the float32 values a kernel carries (1 - b1 and 1 - b2 are exact in float32, so float64 arithmetic on them gives the same)."""
  b1, b2, eps = _f32(b1), _f32(b2), _f32(eps)
  return R.adam_ref(p, g, m, v, lr_t, b1, b2, eps, _f32(grad_scale) * float(s), _f32(l2) * float(s), const=np.float64)


def clipped_adam_bounds(p, g, m, v, lr_t, s, b1=0.9, b2=0.999, eps=1e-8, grad_scale=1.0, l2=0.0):
  """adam_bounds at the scaled constants, widened by the rounding of G * s (module docstring)."""
  gs, l2s = _f32(grad_scale) * float(s), _f32(l2) * float(s)
  bp, bm, bv = R.adam_bounds(p, g, m, v, lr_t, b1, b2, eps, gs, l2s)
  b1, b2, eps = _f32(b1), _f32(b2), _f32(eps)
  p64, g64 = R._f64(p), R._f64(g)
  Gs = np.abs(g64 * gs) + np.abs(l2s * p64)
  gg = g64 * gs + l2s * p64
  xm = U * (1.0 - b1) * Gs
  xv = U * (1.0 - b2) * 2.0 * np.abs(gg) * Gs
  _, m2, v2 = clipped_adam_ref(p, g, m, v, lr_t, s, b1, b2, eps, grad_scale, l2)
  root = np.sqrt(v2)
  den = root + eps
  step = float(lr_t) * m2 / den
  xp = float(lr_t) * xm / den + np.abs(step) * xv / (2 * np.maximum(root, 1e-300) * den)
  return bp + xp, bm + xm, bv + xv
