"""Decoder pieces: state concat, GEMM, LSTM, heads and losses (csrc/decoder_*.hip)."""
from __future__ import annotations

import ctypes

import torch

from .. import _native
from .._native import check
from ._marshal import _accepted, _iarr, _lib, _p, _parr, _stream, _ws


def state_concat_fwd_into(state, feats, feat_ch, jnt_pos, jnt, jnt_stride, J, N, cells, state_stride, sub_from=None):
  check(_lib().geeco_state_concat_fwd(_parr(feats), _iarr(feat_ch), len(feats), jnt_pos, _p(jnt), jnt_stride, J,
                                      _p(sub_from), N, cells, _p(state), state_stride, _stream()),
        'geeco_state_concat_fwd')


def state_concat_bwd_into(dfeats, dstate, dstate_stride, feats_fwd, feat_ch, jnt_pos, J, N, cells, accumulate=False,
                          scale=1.0):
  check(_lib().geeco_state_concat_bwd(_p(dstate), dstate_stride, _parr(feats_fwd), _parr(dfeats), _iarr(feat_ch),
                                      len(feats_fwd), jnt_pos, J, N, cells, 1 if accumulate else 0, float(scale),
                                      _stream()), 'geeco_state_concat_bwd')


def gemm_ws_bytes(M, N, K):
  return int(_lib().geeco_gemm_ws_bytes(M, N, K))


def gemm_into(C, A, B, M, N, K, lda, ldb, ldc, ta=False, tb=False, accumulate=False, ws=None):
  check(_lib().geeco_gemm_f32(_p(A), lda, 1 if ta else 0, _p(B), ldb, 1 if tb else 0, _p(C), ldc, M, N, K,
                              1 if accumulate else 0, _p(ws), _stream()), 'geeco_gemm_f32')


def gemm(A, B, ta=False, tb=False):
  """Allocating form for tests: op(A) @ op(B) with row-major 2-D tensors."""
  M, K = (A.shape[1], A.shape[0]) if ta else A.shape
  N = B.shape[0] if tb else B.shape[1]
  C = torch.empty(M, N, dtype=torch.float32, device=A.device)
  ws = _ws(gemm_ws_bytes(M, N, K), A.device)
  gemm_into(C, A.contiguous(), B.contiguous(), M, N, K, A.shape[1], B.shape[1], N, ta, tb, False, ws)
  return C


def lstm_gates_fwd_into(c, h, gates, z, bias, c_prev, N, H):
  check(_lib().geeco_lstm_gates_fwd(_p(z), _p(bias), _p(c_prev), _p(c), _p(h), _p(gates), N, H, _stream()),
        'geeco_lstm_gates_fwd')


def lstm_input_step_fwd_into(z, c, h, gates, x, wx, bias, N, H, D, ldx, ldw, ws):
  """The cell's first step (zero state): gate GEMM + gate math, the split-K slab sum inside the gate kernel (two launches)."""
  check(_lib().geeco_lstm_input_step_fwd(_p(x), ldx, _p(wx), ldw, _p(bias), _p(z), _p(c), _p(h), _p(gates), N, H, D, _p(ws),
                                         _stream()), 'geeco_lstm_input_step_fwd')


def lstm_gates_bwd_into(dz, dc_prev, gates, c_prev, c, dh, dc, N, H):
  check(_lib().geeco_lstm_gates_bwd(_p(gates), _p(c_prev), _p(c), _p(dh), _p(dc), _p(dz), _p(dc_prev), N, H,
                                    _stream()), 'geeco_lstm_gates_bwd')


def lstm_step_bwd_ws_bytes(N, D, H4):
  return int(_lib().geeco_lstm_step_bwd_ws_bytes(N, D, H4))


def lstm_step_bwd_into(dwx, db, dx, x, dz, wx, N, D, H4, ldw, ws, feats_fwd=None, dfeats=None, feat_ch=None, jnt_pos=0, J=0,
                       cells=0, pending=None):
  """Two launches: dwx = x^T dz, db = colsum(dz), split-K partials of dx = dz wx^T side by side; then dx's slab sum with
  the state-concat backward (``dfeats``) in its epilogue -- and, if ``pending`` (what lstm_step_heads_into left behind), the
  heads' batch sums as extra blocks of the first grid."""
  nf = len(feats_fwd) if feats_fwd else 0
  check(_lib().geeco_lstm_step_bwd(_p(x), D, _p(dz), H4, _p(wx), ldw, _p(dwx), ldw, _p(db), _p(dx), D, N, D, H4,
                                   _parr(feats_fwd) if nf else None, _parr(dfeats) if nf else None,
                                   _iarr(feat_ch) if nf else None, nf, jnt_pos, J, cells, _p(ws),
                                   ctypes.byref(pending) if pending is not None else None, _stream()),
        'geeco_lstm_step_bwd')


def colsum_into(out, a, lda, M, N, accumulate=False):
  check(_lib().geeco_colsum(_p(a), lda, M, N, _p(out), 1 if accumulate else 0, _stream()), 'geeco_colsum')


def heads_ws_bytes(N, H, Hfc):
  return int(_lib().geeco_heads_ws_bytes(N, H, Hfc))


def _head_arrays(heads_w, heads_b, head_size, head_kind, head_weight, targets, target_stride):
  """The heads' parallel arrays as both heads entry points take them, in argument order: nheads, weights, biases, sizes, kinds,
  loss weights, targets, target strides."""
  nh = len(heads_w)
  return (nh, _parr(heads_w), _parr(heads_b), _iarr(head_size), _iarr(head_kind), (ctypes.c_float * nh)(*[float(v) for v in head_weight]),
          _parr(targets), (ctypes.c_int64 * nh)(*[int(v) for v in target_stride]))


def loss_shaping(sample_weight=None, class_weight=None, label_smoothing=0.0, huber_delta=None):
  """A geeco_loss_shaping for ``heads_loss_into`` / ``lstm_step_heads_into`` (``shaping=``): tf.losses' ``weights=`` as a device
  vector ``sample_weight`` [N] (a strided view is fine) and / or a device table ``class_weight`` [size of the cross-entropy head],
  ``label_smoothing``, and ``huber_delta`` = one delta per head (read for the heads of kind 2).  The tensors are read by the
  kernels when they run: the struct holds a reference to each, and whoever replays a captured call keeps them alive beyond it."""
  s = _native.LossShaping()
  s.tensors = (sample_weight, class_weight)
  for t in (sample_weight, class_weight):
    assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.dim() == 1), (t.device, t.dtype, t.shape)
  if sample_weight is not None:
    s.sample_weight, s.sample_weight_stride = sample_weight.data_ptr(), int(sample_weight.stride(0))
  if class_weight is not None:
    assert class_weight.is_contiguous()
    s.class_weight = class_weight.data_ptr()
  s.label_smoothing = float(label_smoothing)
  for i, d in enumerate(huber_delta or ()):
    s.huber_delta[i] = float(d)
  return s


def heads_loss_into(preds, losses, h, fc1_w, fc1_b, heads_w, heads_b, head_size, head_kind, head_weight, targets,
                    target_stride, loss_scale, N, H, Hfc, ws, dh=None, d_fc1_w=None, d_fc1_b=None, d_heads_w=None,
                    d_heads_b=None, shaping=None):
  """fc1 + heads + losses (+ their gradients when ``dh`` is given); see include/geeco_hip.h.  ``shaping`` (a ``loss_shaping``):
  the shaped entry point, which also takes heads of kind 2 (Huber)."""
  backward = dh is not None
  heads = _head_arrays(heads_w, heads_b, head_size, head_kind, head_weight, targets, target_stride)
  tail = (_p(preds), _p(losses), 1 if backward else 0, _p(dh), _p(d_fc1_w), _p(d_fc1_b), _parr(d_heads_w) if backward else None,
          _parr(d_heads_b) if backward else None, _p(ws), _stream())
  if shaping is None:
    check(_lib().geeco_heads_loss_fwd_bwd(_p(h), _p(fc1_w), _p(fc1_b), *heads, loss_scale, N, H, Hfc, *tail),
          'geeco_heads_loss_fwd_bwd')
  else:
    check(_lib().geeco_heads_loss_shaped_fwd_bwd(_p(h), _p(fc1_w), _p(fc1_b), *heads, loss_scale, N, H, Hfc,
                                                 ctypes.byref(shaping), *tail), 'geeco_heads_loss_shaped_fwd_bwd')


def lstm_step_heads_into(z, c, h, gates, x, wx, bias, N, H, D, ldx, ldw, gemm_ws, preds, losses, fc1_w, fc1_b, heads_w, heads_b,
                         head_size, head_kind, head_weight, targets, target_stride, loss_scale, Hfc, heads_ws, dz=None,
                         d_fc1_w=None, d_fc1_b=None, d_heads_w=None, d_heads_b=None, pending=None, shaping=None):
  """One-step decoder from a zero state: the gate GEMM + ONE per-sample launch (slab sum, gate math, fc1, heads, loss terms and,
  when ``dz`` is given, everything back to the gate gradients).  ``pending`` (an _native.HeadsFinish): the batch sums are left for
  lstm_step_bwd_into(pending=...); None: they run here.  ``shaping`` (a ``loss_shaping``): the shaped entry point.  Returns False
  (nothing launched) for shapes the per-sample kernel does not serve: the caller then runs lstm_input_step_fwd_into +
  heads_loss_into (+ lstm_gates_bwd_into)."""
  backward = dz is not None
  head = (_p(x), ldx, _p(wx), ldw, _p(bias), _p(z), _p(c), _p(h), _p(gates), N, H, D, _p(gemm_ws), _p(fc1_w), _p(fc1_b),
          *_head_arrays(heads_w, heads_b, head_size, head_kind, head_weight, targets, target_stride), loss_scale, Hfc)
  tail = (_p(preds), _p(losses), 1 if backward else 0, _p(dz), _p(d_fc1_w), _p(d_fc1_b), _parr(d_heads_w) if backward else None,
          _parr(d_heads_b) if backward else None, _p(heads_ws), ctypes.byref(pending) if pending is not None else None, _stream())
  if shaping is None:
    rc, what = _lib().geeco_lstm_step_heads_fwd_bwd(*head, *tail), 'geeco_lstm_step_heads_fwd_bwd'
  else:
    rc, what = (_lib().geeco_lstm_step_heads_shaped_fwd_bwd(*head, ctypes.byref(shaping), *tail),
                'geeco_lstm_step_heads_shaped_fwd_bwd')
  return _accepted(rc, what)


def lstm_seq_heads_into(preds, zx, wh, bias, fc1_w, fc1_b, heads_w, heads_b, head_size, N, T, H, Hfc, ldz, ldw, h_last=None,
                        c_last=None):
  """Inference decoder after the hoisted input projection in ONE launch: T LSTM steps from the zero state over ``zx`` [T][N][4H]
  (row stride ``ldz``; X Wx without bias), fc1 and the heads on the last output -> ``preds`` [N][sum sizes]; ``h_last`` / ``c_last``
  [N][H] optionally receive the final state.  Returns False (nothing launched) for shapes the kernel does not serve: the caller
  then runs the step chain (gemm_into + lstm_gates_fwd_into per step, heads_loss_into)."""
  nh = len(heads_w)
  rc = _lib().geeco_lstm_seq_heads_fwd(_p(zx), ldz, _p(wh), ldw, _p(bias), _p(fc1_w), _p(fc1_b), nh, _parr(heads_w), _parr(heads_b),
                                       _iarr(head_size), N, T, H, Hfc, _p(preds), _p(h_last), _p(c_last), _stream())
  return _accepted(rc, 'geeco_lstm_seq_heads_fwd')
