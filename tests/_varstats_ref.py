"""Restatement of the per-variable statistics record (include/geeco_hip.h: geeco_variable_stats) in numpy float64 and
integers, written from its semantics and not from the kernels (tests/test_variable_stats_cpu.py checks it against values worked by
hand, tests/test_variable_stats_gpu.py holds the device to it).

  G_i = g_i * grad_scale            ONE float32 product; its float32 bit pattern decides what G_i is
  non-finite: exponent field 255;  zero: +-0;  otherwise class = clamp(((bits >> 23) & 0xff) - 127, -32, 7) + 32, by sign
  sums, extrema: over the finite elements, in float64 here
  u_i = m_i / (sqrt(v_i) + eps)     in float64 from the float32 inputs (eps as the float32 the device is handed)
"""
import numpy as np

CLASSES = 40
F32_MAX = float(np.finfo(np.float32).max)


def classes(x):
  """(class or -1, is negative, is non-finite, is zero) per element of the float32 array ``x``."""
  bits = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.int64)
  ex = (bits >> 23) & 0xff
  nonfinite = ex == 255
  zero = (bits & 0x7fffffff) == 0
  cls = np.clip(ex - 127, -32, 7) + 32
  cls = np.where(nonfinite | zero, -1, cls)
  return cls, (bits >> 31) == 1, nonfinite, zero


def tensor(x):
  """The record of one tensor from its float32 values ``x`` (those that exist: uncovered elements are left out by the caller)."""
  x = np.ascontiguousarray(x, dtype=np.float32)
  cls, negative, nonfinite, zero = classes(x)
  fin = x[~nonfinite].astype(np.float64)
  neg = np.bincount(cls[(cls >= 0) & negative], minlength=CLASSES).astype(np.int64)
  pos = np.bincount(cls[(cls >= 0) & ~negative], minlength=CLASSES).astype(np.int64)
  return dict(nonfinite=int(nonfinite.sum()), zeros=int(zero.sum()), sum=float(fin.sum()), sumsq=float((fin * fin).sum()),
              abs_sum=float(np.abs(fin).sum()), min=float(fin.min()) if fin.size else float('inf'),
              max=float(fin.max()) if fin.size else float('-inf'), neg=neg, pos=pos)


def update(m, v, eps):
  """sum of u^2 and max |u| over the finite u, the count of the others."""
  m64, v64 = np.asarray(m, np.float32).astype(np.float64), np.asarray(v, np.float32).astype(np.float64)
  with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
    u = m64 / (np.sqrt(v64) + float(np.float32(eps)))
  ok = np.isfinite(u) & (np.abs(u) <= F32_MAX)
  uf = u[ok]
  return dict(sumsq=float((uf * uf).sum()), max_abs=float(np.abs(uf).max()) if uf.size else 0.0, nonfinite=int((~ok).sum()))


def record(g, covered, p, m, v, grad_scale=1.0, eps=1e-8):
  """One variable: ``g``, ``p``, ``m``, ``v`` its float32 elements, ``covered`` a boolean mask of the elements that have a gradient."""
  with np.errstate(invalid='ignore', over='ignore', under='ignore'):
    G = np.asarray(g, np.float32) * np.float32(grad_scale)
  covered = np.asarray(covered, bool)
  return dict(grad_covered=int(covered.sum()), grad=tensor(G[covered]), param=tensor(p), update=update(m, v, eps))
