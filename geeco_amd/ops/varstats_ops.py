"""Per-variable statistics (csrc/varstats.hip)."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from .. import _native
from .._native import check
from ._marshal import _adam_segments, _lib, _p, _stream

_VS_TENSOR = [('nonfinite', '<i8'), ('zeros', '<i8'), ('sum', '<f4'), ('sumsq', '<f4'), ('min', '<f4'), ('max', '<f4'),
              ('neg', '<i8', (_native.VARSTATS_CLASSES,)), ('pos', '<i8', (_native.VARSTATS_CLASSES,))]
# geeco_varstats_record of include/geeco_hip.h, field for field
VARSTATS_DTYPE = np.dtype([('grad_covered', '<i8'), ('grad', _VS_TENSOR), ('param', _VS_TENSOR), ('update_nonfinite', '<i8'),
                           ('update_sumsq', '<f4'), ('update_max_abs', '<f4')])
assert VARSTATS_DTYPE.itemsize == 1368


def variable_stats_ws_bytes(nchunks):
  return int(_lib().geeco_variable_stats_ws_bytes(int(nchunks)))


def variable_stats_table(variables, chunk=_native.VARSTATS_CHUNK):
  """The table ``geeco_variable_stats`` reads on the device, on the host (int64, flat): per variable of ``variables`` = [(offset, count)]
  its first chunk and its number of chunks, then per chunk its arena offset and element count.  A variable is cut from its own first
  element into chunks of ``chunk`` elements, the last one shorter: no chunk straddles two variables or holds a pad float.  Needs no GPU."""
  head, chunks = [], []
  for off, cnt in variables:
    off, cnt = int(off), int(cnt)
    if off < 0 or off % 4 or cnt < 1:
      raise ValueError('variable_stats_table: a variable at offset %d with %d elements (offsets are multiples of 4, counts >= 1)' % (off, cnt))
    nc = -(-cnt // chunk)
    head += [len(chunks), nc]
    chunks += [(off + k * chunk, min(chunk, cnt - k * chunk)) for k in range(nc)]
  return np.array(head + [x for c in chunks for x in c], dtype=np.int64)


def variable_stats(out, ws, table, p, m, v, segments, n, variables, nchunks, grad_scale=1.0, eps=1e-8):
  """``geeco_variable_stats``: one record per variable of ``variables`` = [(offset, count)] into ``out`` (uint8, VARSTATS_DTYPE.itemsize
  bytes per variable); ``table``: ``variable_stats_table(variables)`` on the device, ``ws``: ``variable_stats_ws_bytes(nchunks)`` bytes;
  ``segments``: the gradient's pieces as ``grad_sumsq_segments`` takes them."""
  nvar = len(variables)
  if out is not None and out.numel() * out.element_size() < nvar * VARSTATS_DTYPE.itemsize:
    raise ValueError('variable_stats: %d bytes of records for %d variables' % (out.numel() * out.element_size(), nvar))
  if ws is not None and ws.numel() * ws.element_size() < variable_stats_ws_bytes(nchunks):
    raise ValueError('variable_stats: a workspace of %d bytes, %d needed' % (ws.numel() * ws.element_size(), variable_stats_ws_bytes(nchunks)))
  if table is not None and (table.dtype != torch.int64 or table.numel() < 2 * nvar + 2 * max(int(nchunks), 0)):
    raise ValueError('variable_stats: the table holds 2 int64 per variable and 2 per chunk')
  arr = _adam_segments(segments)
  offs = (ctypes.c_int64 * max(nvar, 1))(*[int(o) for o, _ in variables])
  cnts = (ctypes.c_int64 * max(nvar, 1))(*[int(c) for _, c in variables])
  check(_lib().geeco_variable_stats(_p(p), _p(m), _p(v), arr, len(segments), int(n), grad_scale, eps, offs, cnts, nvar, _p(table), int(nchunks),
                                    _p(ws), _p(out), _stream()), 'geeco_variable_stats')

