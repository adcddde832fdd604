"""What every kernel family needs to hand Python values to the C-ABI (geeco_amd/_native.py): the loaded library, the current
stream, tensors and lists as ctypes arguments, the shared argument checks and the two return conventions."""
from __future__ import annotations

import ctypes

import torch

from .. import _native
from .._native import check


def _lib():
  return _native.load()


def _stream():
  return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
  if t is None:
    return None
  assert t.is_cuda and t.dtype in (torch.float32, torch.int64, torch.int32, torch.int16, torch.uint8), (t.device, t.dtype)
  return ctypes.c_void_p(t.data_ptr())


def _parr(ts):
  arr = (ctypes.c_void_p * len(ts))()
  for i, t in enumerate(ts):
    arr[i] = t.data_ptr() if t is not None else None
  return arr


def _iarr(vals):
  arr = (ctypes.c_int * len(vals))()
  for i, v in enumerate(vals):
    arr[i] = int(v)
  return arr


def _check_tables(tables, device, message, exact=False):
  """ValueError(message) unless every (tensor, dtype, n) of ``tables`` is a contiguous table of that dtype with at least (``exact``:
  exactly) n entries on ``device``."""
  for t, dt, n in tables:
    if not (t.is_cuda and t.dtype == dt and t.is_contiguous() and (t.numel() == n if exact else t.numel() >= n) and t.device == device):
      raise ValueError(message)


def same_out(size: int, stride: int) -> int:
  return -(-size // stride)


def _ws(nbytes, device):
  return torch.empty(nbytes // 4 + 4, dtype=torch.float32, device=device) if nbytes > 0 else None


_ALPHA_CACHE = {}


def _alpha_buf(K):
  if K not in _ALPHA_CACHE:
    buf = (ctypes.c_float * K)()
    _lib().geeco_dynimg_alpha(K, ctypes.cast(buf, ctypes.c_void_p))
    _ALPHA_CACHE[K] = buf
  return _ALPHA_CACHE[K]


def _adam_segments(segments):
  if not 1 <= len(segments) <= _native.ADAM_SEGMENTS_MAX:
    raise ValueError('adam_tf_segments: 1..%d pieces, got %d' % (_native.ADAM_SEGMENTS_MAX, len(segments)))
  arr = (_native.AdamSegment * len(segments))()
  for a, (g, off, n) in zip(arr, segments):
    if g.numel() < n:
      raise ValueError('adam_tf_segments: a piece of %d floats with %d gradients' % (n, g.numel()))
    a.g, a.p_off, a.count = _p(g), int(off), int(n)
  return arr


def _accepted(rc, what):
  """The return of a wrapper whose entry point may decline: False for GEECO_ENOSUP (nothing launched), else ``check`` and True."""
  if rc == _native.GEECO_ENOSUP:
    return False
  check(rc, what)
  return True


def _slab_item(pending, reserved_cus, summing_entry=True):
  """The item of a filter-gradient wrapper that launches one deferred slab sum: None when ``pending`` is None (the caller runs the
  entry point that sums itself, and ``reserved_cus`` is refused when there is such an entry: ``summing_entry``), else a fresh
  geeco_slab_reduce for the entry point to fill; ``_defer_slab_sum`` files it behind the launch."""
  if pending is None:
    if summing_entry and reserved_cus:
      raise ValueError('reserved_cus is an argument of the deferred-slab-sum form: pass pending=[...]')
    return None
  return _native.SlabReduce()


def _defer_slab_sum(pending, item):
  """Appends the item the launch filled to ``pending`` when the kernel left slabs to sum."""
  if item is not None and item.S > 0:
    pending.append(item)
