"""The conv encoder: forward, input and filter gradients, sign bits and fields, the fused bottom, the deferred slab sums, the
derived weights (csrc/conv_*.hip, misc.hip) and the kernel trace."""
from __future__ import annotations

import ctypes

import torch

from .. import _native
from .._native import check
from ._marshal import _accepted, _defer_slab_sum, _iarr, _lib, _p, _parr, _slab_item, _stream, _ws, same_out
from .optim import _scal_holds_lr, lr_schedule_struct


def conv3x3_fwd_into(y, x, w, b, G, gs_x, gs_w, gs_b, gs_y, N, H, W, Cin, Cout, stride, relu=True, ws=None):
  check(_lib().geeco_conv3x3_fwd(_p(x), _p(w), _p(b), _p(y), G, gs_x, gs_w, gs_b, gs_y, N, H, W, Cin, Cout,
                                 stride, 1 if relu else 0, _p(ws), _stream()), 'geeco_conv3x3_fwd')


def conv3x3_fwd_state_into(y, x, w, b, G, gs_x, gs_w, gs_b, gs_y, N, H, W, Cin, Cout, stride, ws, state, state_stride, feat_off,
                           Ctot, jnt, jnt_stride, jnt_off, J):
  """The top layer's forward with the one-step decoder's state concat in the split-K epilogue (``geeco_conv3x3_fwd_state``).
  Returns False (nothing launched) when the shape has no such epilogue: run conv3x3_fwd_into + state_concat_fwd_into."""
  rc = _lib().geeco_conv3x3_fwd_state(_p(x), _p(w), _p(b), _p(y), G, gs_x, gs_w, gs_b, gs_y, N, H, W, Cin, Cout, stride, _p(ws),
                                      _iarr(feat_off), Ctot, _p(jnt), jnt_stride, jnt_off, J, _p(state), state_stride, _stream())
  return _accepted(rc, 'geeco_conv3x3_fwd_state')


def conv3x3_fwd_ws_bytes(G, N, H, W, Cin, Cout, stride):
  return int(_lib().geeco_conv3x3_fwd_ws_bytes(G, N, H, W, Cin, Cout, stride))


def conv3x3_dgrad_into(dx, dz, wt, ymask, G, gs_dz, gs_wt, gs_dx, N, H, W, Cin, Cout, stride, ws=None, w=None, gs_w=0):
  check(_lib().geeco_conv3x3_dgrad(_p(dz), _p(w), _p(wt), _p(ymask), _p(dx), G, gs_dz, gs_w, gs_wt, gs_dx, N, H, W,
                                   Cin, Cout, stride, _p(ws), _stream()), 'geeco_conv3x3_dgrad')


def conv1_dgrad_into(dx, dz1, w1, G, gs_dz, gs_w, gs_dx, F, H, W, Cin, Cout=32):
  """conv1's input gradient: dx [G][F][H][W][4] <- dz1 [G][F][H][W][32], w1 the [3][3][Cin][32] variable (geeco_conv1_dgrad).  Returns
  False, nothing launched, for a layer the kernel was not built for."""
  rc = _lib().geeco_conv1_dgrad(_p(dz1), _p(w1), _p(dx), G, gs_dz, gs_w, gs_dx, F, H, W, Cin, Cout, _stream())
  return _accepted(rc, 'geeco_conv1_dgrad')


def conv3x3_dgrad_ws_bytes(G, N, H, W, Cin, Cout, stride):
  return int(_lib().geeco_conv3x3_dgrad_ws_bytes(G, N, H, W, Cin, Cout, stride))


def conv3x3_dgrad_needs_wt(H, W, Cin, Cout, stride):
  return bool(_lib().geeco_conv3x3_dgrad_needs_wt(H, W, Cin, Cout, stride))


def conv3x3_dgrad_relu_fields_supported(H, W, Cin, Cout, stride):
  return bool(_lib().geeco_conv3x3_dgrad_relu_fields_supported(H, W, Cin, Cout, stride))


def conv3x3_wgrad_ws_bytes(G, N, H, W, Cin, Cout, stride):
  return int(_lib().geeco_conv3x3_wgrad_ws_bytes(G, N, H, W, Cin, Cout, stride))


def conv3x3_wgrad_into(dw, db, x, dz, G, gs_x, gs_dz, gs_dw, gs_db, N, H, W, Cin, Cout, stride, ws, pending=None,
                       reserved_cus=0):
  """``pending`` (a list): the kernel's final slab sum is not launched but appended to it (``slab_reduce_batch``
  finishes all of them in one launch; ``ws`` must stay untouched until then).  ``reserved_cus`` (data parallel; needs
  ``pending``): CUs conv2's persistent filter-gradient kernel leaves to a collective running beside it."""
  item = _slab_item(pending, reserved_cus)
  if item is None:
    check(_lib().geeco_conv3x3_wgrad(_p(x), _p(dz), _p(dw), _p(db), G, gs_x, gs_dz, gs_dw, gs_db, N, H, W, Cin,
                                     Cout, stride, _p(ws), _stream()), 'geeco_conv3x3_wgrad')
    return
  check(_lib().geeco_conv3x3_wgrad_partial(_p(x), _p(dz), _p(dw), _p(db), G, gs_x, gs_dz, gs_dw, gs_db, N, H, W, Cin,
                                           Cout, stride, _p(ws), _stream(), ctypes.byref(item), int(reserved_cus)),
        'geeco_conv3x3_wgrad_partial')
  _defer_slab_sum(pending, item)


def _take_pending(items, pending):
  """Appends copies of the slab sums a paired launch recorded in the ctypes array ``items`` (S > 0) to ``pending``."""
  for it in items if items is not None else ():
    if it.S > 0:
      c = _native.SlabReduce()
      ctypes.memmove(ctypes.byref(c), ctypes.byref(it), ctypes.sizeof(c))
      pending.append(c)


def conv3x3_wgrad_pair_into(a, b, G, stride, pending=None):
  """Two independent filter gradients in ONE launch (``geeco_conv3x3_wgrad_pair``).  ``a`` / ``b``: dicts with the arguments of
  ``conv3x3_wgrad_into`` (dw, db, x, dz, gs_x, gs_dz, gs_dw, gs_db, N, H, W, Cin, Cout, ws); ``a`` = the longer problem.
  Returns False (nothing launched) when the shapes are outside the paired kernel: the caller launches them one by one."""
  lib = _lib()
  items = (_native.SlabReduce * 2)() if pending is not None else None
  rc = lib.geeco_conv3x3_wgrad_pair(
      _p(a['x']), _p(a['dz']), _p(a['dw']), _p(a['db']), a['gs_x'], a['gs_dz'], a['gs_dw'], a['gs_db'], a['N'], a['H'], a['W'],
      a['Cin'], a['Cout'], _p(a['ws']),
      _p(b['x']), _p(b['dz']), _p(b['dw']), _p(b['db']), b['gs_x'], b['gs_dz'], b['gs_dw'], b['gs_db'], b['N'], b['H'], b['W'],
      b['Cin'], b['Cout'], _p(b['ws']), G, stride, _stream(), items)
  if not _accepted(rc, 'geeco_conv3x3_wgrad_pair'):
    return False
  _take_pending(items, pending)
  return True


def conv_top_bwd_into(d, a, b, G, stride, pending=None):
  """conv7's input gradient + conv7's / conv8's filter gradients as ONE heterogeneous grid (``geeco_conv_top_bwd``).  ``d``: dict
  with the arguments of ``conv3x3_dgrad_into`` (dx, dz, wt, ymask, w, gs_dz, gs_w, gs_wt, gs_dx, N, H, W, Cin, Cout, ws);
  ``a`` / ``b`` as for ``conv3x3_wgrad_pair_into``.  Returns False (nothing launched) outside the combined kernels."""
  lib = _lib()
  items = (_native.SlabReduce * 2)() if pending is not None else None
  none = (None, None, None, None, 0, 0, 0, 0, 0, 0, 0, 0, 0, None)      # b is None: ONE filter gradient beside the input gradient
  wa = lambda q: none if q is None else (_p(q['x']), _p(q['dz']), _p(q['dw']), _p(q['db']), q['gs_x'], q['gs_dz'], q['gs_dw'],
                                         q['gs_db'], q['N'], q['H'], q['W'], q['Cin'], q['Cout'], _p(q['ws']))
  rc = lib.geeco_conv_top_bwd(_p(d['dz']), _p(d['w']), _p(d['wt']), _p(d['ymask']), _p(d['dx']), d['gs_dz'], d['gs_w'], d['gs_wt'],
                              d['gs_dx'], d['N'], d['H'], d['W'], d['Cin'], d['Cout'], _p(d['ws']), *wa(a), *wa(b), G, stride,
                              _stream(), items)
  if not _accepted(rc, 'geeco_conv_top_bwd'):
    return False
  _take_pending(items, pending)
  return True


def slab_reduce_batch(pending, prepare=None, beta1=0.9, beta2=0.999):
  """Finishes the deferred slab sums of ``pending`` (<= 8 per launch) and empties the list.  ``prepare`` = (global_step, lr,
  scal): the last launch also does adam_prepare's work (one block more instead of a dependent launch); a learning-rate schedule
  (``lr_schedule_struct``) in place of the float ``lr``: adam_prepare_schedule's."""
  MAX = _native.SLAB_REDUCE_MAX
  chunks = [pending[i:i + MAX] for i in range(0, len(pending), MAX)] or ([[]] if prepare is not None else [])
  for j, chunk in enumerate(chunks):
    arr = (_native.SlabReduce * max(len(chunk), 1))(*chunk)
    if prepare is not None and j == len(chunks) - 1:
      step, lr, scal = prepare
      if isinstance(lr, (dict, _native.LrSchedule)):
        _scal_holds_lr(scal)
        check(_lib().geeco_slab_reduce_batch_prepare_schedule(arr, len(chunk), _p(step), ctypes.byref(lr_schedule_struct(lr)), beta1, beta2,
                                                              _p(scal), _stream()), 'geeco_slab_reduce_batch_prepare_schedule')
      else:
        check(_lib().geeco_slab_reduce_batch_prepare(arr, len(chunk), _p(step), float(lr), beta1, beta2, _p(scal), _stream()),
              'geeco_slab_reduce_batch_prepare')
    else:
      check(_lib().geeco_slab_reduce_batch(arr, len(chunk), _stream()), 'geeco_slab_reduce_batch')
  del pending[:]


def conv2_dgrad_conv1_wgrad_ws_bytes(G):
  return int(_lib().geeco_conv2_dgrad_conv1_wgrad_ws_bytes(G))


def conv2_dgrad_conv1_wgrad_into(dw1, db1, dz2, w2, y1, x, G, gs_dz2, gs_w2, gs_y1, gs_x, gs_dw1, gs_db1, N, H, W, ws,
                                 dz1=None, real_channels=3, pending=None, reserved_cus=0):
  """Fused encoder bottom backward: conv2's input gradient + conv1's filter/bias gradient (dz1 stays on chip).
  dw1 [G][3][3][real_channels][32]; ``pending`` / ``reserved_cus`` as for ``conv3x3_wgrad_into``."""
  item = _slab_item(pending, reserved_cus)
  if item is None:
    check(_lib().geeco_conv2_dgrad_conv1_wgrad(_p(dz2), _p(w2), _p(y1), _p(x), _p(dw1), _p(db1), _p(dz1), G, gs_dz2,
                                               gs_w2, gs_y1, gs_x, gs_dw1, gs_db1, N, H, W, real_channels, _p(ws),
                                               _stream()), 'geeco_conv2_dgrad_conv1_wgrad')
    return
  check(_lib().geeco_conv2_dgrad_conv1_wgrad_partial(_p(dz2), _p(w2), _p(y1), _p(x), _p(dw1), _p(db1), _p(dz1), G,
                                                     gs_dz2, gs_w2, gs_y1, gs_x, gs_dw1, gs_db1, N, H, W, real_channels,
                                                     _p(ws), _stream(), ctypes.byref(item), int(reserved_cus)),
        'geeco_conv2_dgrad_conv1_wgrad_partial')
  _defer_slab_sum(pending, item)


def relu_bits_pitch(W):
  return int(_lib().geeco_relu_bits_pitch(W))


def relu_bits_rows(H):
  return int(_lib().geeco_relu_bits_rows(H))


def conv1_fwd_relu_bits_into(y, bits, x, w, b, G, gs_x, gs_w, gs_b, gs_y, gs_bits, N, H, W):
  """conv1 forward (4 -> 32, stride 1, bias, ReLU) that also writes y's sign bits (int32 [G][N][Hp][Wp], zero-filled once by the caller)."""
  check(_lib().geeco_conv1_fwd_relu_bits(_p(x), _p(w), _p(b), _p(y), _p(bits), G, gs_x, gs_w, gs_b, gs_y, gs_bits, N, H,
                                         W, _stream()), 'geeco_conv1_fwd_relu_bits')


def conv1_fwd_relu_bits_rgb_into(y, bits, x, w3, b, G, gs_x, gs_w, gs_b, gs_y, gs_bits, N, H, W):
  """conv1_fwd_relu_bits_into reading the RGB kernel variable [G][3][3][3][32] itself (no channel-padded copy)."""
  check(_lib().geeco_conv1_fwd_relu_bits_rgb(_p(x), _p(w3), _p(b), _p(y), _p(bits), G, gs_x, gs_w, gs_b, gs_y, gs_bits, N, H,
                                             W, _stream()), 'geeco_conv1_fwd_relu_bits_rgb')


def conv2_dgrad_conv1_wgrad_bits_into(dw1, db1, dz2, w2, y1_bits, x, G, gs_dz2, gs_w2, gs_bits, gs_x, gs_dw1, gs_db1, N, H,
                                      W, ws, real_channels=3, pending=None, reserved_cus=0):
  """Fused encoder bottom backward with the ReluGrad mask given as conv1's sign bits."""
  item = _slab_item(pending, reserved_cus, summing_entry=False)
  check(_lib().geeco_conv2_dgrad_conv1_wgrad_bits(_p(dz2), _p(w2), _p(y1_bits), _p(x), _p(dw1), _p(db1), G, gs_dz2, gs_w2,
                                                  gs_bits, gs_x, gs_dw1, gs_db1, N, H, W, real_channels, _p(ws), _stream(),
                                                  ctypes.byref(item) if item is not None else None, int(reserved_cus)),
        'geeco_conv2_dgrad_conv1_wgrad_bits')
  _defer_slab_sum(pending, item)


def relu_fields_elems(N, H, W):
  return int(_lib().geeco_relu_fields_elems(N, H, W))


def conv2_fwd_relu_fields_into(y, fields, x, w, b, G, gs_x, gs_w, gs_b, gs_y, gs_fields, N, H, W):
  """conv2 forward (32 -> 48, stride 2, bias, ReLU) that also writes y's sign fields (int16, relu_fields_elems per encoder)."""
  check(_lib().geeco_conv2_fwd_relu_fields(_p(x), _p(w), _p(b), _p(y), _p(fields), G, gs_x, gs_w, gs_b, gs_y, gs_fields, N,
                                           H, W, _stream()), 'geeco_conv2_fwd_relu_fields')


def conv3_dgrad_relu_fields_into(dx, dz, w, fields, G, gs_dz, gs_w, gs_fields, gs_dx, N, H, W, reserved_cus=0):
  """conv3 input gradient (48 -> 64, stride 2) masked by the sign fields of conv2's output; H, W = dims of dx.
  ``reserved_cus`` (data parallel): CUs this persistent kernel leaves to a collective running beside it."""
  check(_lib().geeco_conv3_dgrad_relu_fields(_p(dz), _p(w), _p(fields), _p(dx), G, gs_dz, gs_w, gs_fields, gs_dx, N, H, W,
                                             _stream(), int(reserved_cus)), 'geeco_conv3_dgrad_relu_fields')


def conv3_fwd_relu_fields_into(y, fields, x, w, b, G, gs_x, gs_w, gs_b, gs_y, gs_fields, N, H, W):
  """conv3 forward (48 -> 64, stride 2, bias, ReLU) that also writes y's byte sign fields (uint8 [G][N][H/2][W/2][8])."""
  check(_lib().geeco_conv3_fwd_relu_fields(_p(x), _p(w), _p(b), _p(y), _p(fields), G, gs_x, gs_w, gs_b, gs_y, gs_fields, N,
                                           H, W, _stream()), 'geeco_conv3_fwd_relu_fields')


def conv3x3_dgrad_relu_fields_into(dx, dz, w, fields, G, gs_dz, gs_w, gs_fields, gs_dx, N, H, W, Cin, Cout, stride):
  """LDS-staged input gradient masked by the byte sign fields of the layer below ([G][N][H][W][Cin / 8])."""
  check(_lib().geeco_conv3x3_dgrad_relu_fields(_p(dz), _p(w), _p(fields), _p(dx), G, gs_dz, gs_w, gs_fields, gs_dx, N, H, W,
                                               Cin, Cout, stride, _stream()), 'geeco_conv3x3_dgrad_relu_fields')


def transpose_hwio_into(wt, w, G, gs_w, gs_wt, Cin, Cout):
  check(_lib().geeco_transpose_hwio(_p(w), _p(wt), G, gs_w, gs_wt, Cin, Cout, _stream()), 'geeco_transpose_hwio')


def derive_conv_weights(ws, wts, cins, couts, G, gs_w, pad_src=None, pad_dst=None, pad_cin=0, pad_cin_padded=0,
                        pad_cout=0):
  """One launch: wts[i] = per-tap transpose of ws[i] (G encoders at stride gs_w) and the zero-padded conv1 kernel."""
  n = len(ws)
  larr = (ctypes.c_int64 * max(n, 1))(*[int(t[0].numel()) for t in wts])
  check(_lib().geeco_derive_conv_weights(
      n, _parr(ws) if n else None, _parr(wts) if n else None, _iarr(cins) if n else None, _iarr(couts) if n else None,
      larr, G, gs_w, _p(pad_src), _p(pad_dst), pad_cin, pad_cin_padded, pad_cout,
      int(pad_dst[0].numel()) if pad_dst is not None else 0, _stream()), 'geeco_derive_conv_weights')


def pad_mid_into(dst, src, A, B, Bd, C):
  check(_lib().geeco_pad_mid(_p(src), _p(dst), A, B, Bd, C, _stream()), 'geeco_pad_mid')


# convenience (allocating) forms used by the parity tests -------------------------------------
def conv3x3(x, w, b, stride, relu=True):
  """x [N,H,W,Cin] (Cin % 4 == 0), w [3,3,Cin,Cout], b [Cout] -> y [N,Ho,Wo,Cout]."""
  N, H, W, Cin = x.shape
  Cout = w.shape[3]
  y = torch.empty(N, same_out(H, stride), same_out(W, stride), Cout, dtype=torch.float32, device=x.device)
  ws = _ws(conv3x3_fwd_ws_bytes(1, N, H, W, Cin, Cout, stride), x.device)
  conv3x3_fwd_into(y, x.contiguous(), w.contiguous(), b.contiguous(), 1, 0, 0, 0, 0, N, H, W, Cin, Cout, stride, relu,
                   ws)
  return y


def conv3x3_dgrad(dz, w, ymask, in_hw, stride):
  """dz [N,Ho,Wo,Cout], w [3,3,Cin,Cout], ymask [N,H,W,Cin] or None -> dx [N,H,W,Cin]."""
  N, Ho, Wo, Cout = dz.shape
  Cin = w.shape[2]
  H, W = in_hw
  wt = torch.empty(3, 3, Cout, Cin, dtype=torch.float32, device=dz.device)
  transpose_hwio_into(wt, w.contiguous(), 1, 0, 0, Cin, Cout)
  dx = torch.empty(N, H, W, Cin, dtype=torch.float32, device=dz.device)
  ws = _ws(conv3x3_dgrad_ws_bytes(1, N, H, W, Cin, Cout, stride), dz.device)
  conv3x3_dgrad_into(dx, dz.contiguous(), wt, ymask, 1, 0, 0, 0, N, H, W, Cin, Cout, stride, ws, w=w.contiguous())
  return dx


def conv3x3_wgrad(x, dz, stride):
  """x [N,H,W,Cin], dz [N,Ho,Wo,Cout] -> dw [3,3,Cin,Cout], db [Cout]."""
  N, H, W, Cin = x.shape
  Cout = dz.shape[3]
  dw = torch.empty(3, 3, Cin, Cout, dtype=torch.float32, device=x.device)
  db = torch.empty(Cout, dtype=torch.float32, device=x.device)
  ws = _ws(conv3x3_wgrad_ws_bytes(1, N, H, W, Cin, Cout, stride), x.device)
  conv3x3_wgrad_into(dw, db, x.contiguous(), dz.contiguous(), 1, 0, 0, 0, 0, N, H, W, Cin, Cout, stride, ws)
  return dw, db


# diagnostics ---------------------------------------------------------------------------------
def kernel_trace(fn):
  """Runs ``fn()`` and returns the names of the conv kernels its calls dispatched (in launch order)."""
  lib = _lib()
  lib.geeco_debug_kernel_trace_begin()
  try:
    fn()
  finally:
    names = lib.geeco_debug_kernel_trace_end()
  return [n for n in (names.decode() if names else '').split(';') if n]
