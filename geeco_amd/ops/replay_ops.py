"""Episode replay (csrc/replay.hip, replay_dynimg.hip; geeco_amd/replay.py, replay_dynimg.py)."""
from __future__ import annotations

import ctypes

import torch

from .. import _native
from .._native import PREDICT_FEAT_MODES, REPLAY_CLASS_HIT, REPLAY_SQUARED_ERROR, check
from ._marshal import _alpha_buf, _iarr, _lib, _p, _stream


def _replay_windows(who, T, t0, t1, K):
  """ValueError unless K is a window length the predictors take and the windows [t0, t1) lie inside the T frames."""
  if not 1 <= int(K) <= _native.REPLAY_MAXK:
    raise ValueError('%s: K=%d outside 1..%d' % (who, K, _native.REPLAY_MAXK))
  if not (T >= 1 and 0 <= t0 < t1 <= T):
    raise ValueError('%s: windows [%d, %d) outside the %d frames' % (who, t0, t1, T))


def _replay_states_shape(who, states, K, n, width):
  """ValueError unless ``states`` is a contiguous [K][N][stride] with N >= n windows and stride >= width columns."""
  if states.dim() != 3 or not states.is_contiguous() or states.shape[0] != K or states.shape[1] < n or states.shape[2] < width:
    raise ValueError('%s: states of shape %s for K=%d steps of >= %d windows of %d columns (contiguous [K][N][stride])'
                     % (who, tuple(states.shape), K, n, width))


def replay_states_into(states, feat, jnt, mode, T, t0, t1, K, cells, ch, J, tgt_feat=None):
  """feat [T][cells][ch] / jnt [T][J] of one episode -> states [K][N][state_stride] (a contiguous 3-D tensor, N >= t1 - t0): row
  t - t0 of step k <- frame max(0, t - K + 1 + k) for the windows t0 <= t < t1, in the columns of predict_push_features_into for
  ``mode`` ('plain', 'constant', 'residual'; tgt_feat [cells][ch] for the last two).  Rows t1 - t0 .. N - 1 are not touched.  Bad
  arguments raise ValueError before anything is queued."""
  if mode not in PREDICT_FEAT_MODES:
    raise ValueError("replay_states: mode=%r must be 'plain', 'constant' or 'residual'" % (mode,))
  _replay_windows('replay_states', T, t0, t1, K)
  if (mode == 'plain') != (tgt_feat is None):
    raise ValueError("replay_states: tgt_feat goes with the modes 'constant' and 'residual' (mode=%r)" % (mode,))
  if min(cells, ch, J) < 1:
    raise ValueError('replay_states: cells=%d ch=%d J=%d' % (cells, ch, J))
  _replay_states_shape('replay_states', states, K, t1 - t0, cells * (ch + J + (ch if mode == 'constant' else 0)))
  if feat.numel() < T * cells * ch or jnt.numel() < T * J or (tgt_feat is not None and tgt_feat.numel() < cells * ch):
    raise ValueError('replay_states: feat / jnt / tgt_feat of %d / %d / %s floats for T=%d cells=%d ch=%d J=%d'
                     % (feat.numel(), jnt.numel(), None if tgt_feat is None else tgt_feat.numel(), T, cells, ch, J))
  check(_lib().geeco_replay_states(_p(feat), _p(jnt), _p(tgt_feat), PREDICT_FEAT_MODES[mode], T, t0, t1, states.shape[1], K, cells, ch,
                                   J, _p(states), states.shape[2], _stream()), 'geeco_replay_states')


def replay_errors_into(out_frame, out_episode, preds, labels, T, heads):
  """preds / labels [>= T][P] -> out_frame [T][len(heads)] and out_episode [len(heads)] (the mean over the frames, one fixed order):
  heads = (first column, columns, kind) per head; kind REPLAY_SQUARED_ERROR: the mean over the head's columns of the squared
  difference; REPLAY_CLASS_HIT: 1 where the argmax of the logits (first maximum) is the class index labels[t][first column], else
  0.  NaN predictions give NaN.  Bad arguments raise ValueError before anything is queued."""
  heads = [tuple(int(v) for v in h) for h in heads]
  if not 1 <= len(heads) <= _native.REPLAY_MAXHEADS:
    raise ValueError('replay_errors: %d heads outside 1..%d' % (len(heads), _native.REPLAY_MAXHEADS))
  if preds.dim() != 2 or labels.dim() != 2 or preds.shape[1] != labels.shape[1] or not (preds.is_contiguous() and labels.is_contiguous()):
    raise ValueError('replay_errors: preds %s and labels %s must be contiguous [T][P] tensors of one width' % (tuple(preds.shape), tuple(labels.shape)))
  P = int(preds.shape[1])
  if not 1 <= T <= min(preds.shape[0], labels.shape[0]):
    raise ValueError('replay_errors: T=%d outside 1..%d rows' % (T, min(preds.shape[0], labels.shape[0])))
  for i, (off, size, kind) in enumerate(heads):
    if not (1 <= size <= 64 and off >= 0 and off + size <= P):
      raise ValueError('replay_errors: head %d [%d, +%d) outside the %d prediction columns (1..64 columns per head)' % (i, off, size, P))
    if kind not in (REPLAY_SQUARED_ERROR, REPLAY_CLASS_HIT):
      raise ValueError('replay_errors: head %d kind=%d must be 0 (squared error) or 1 (class hit)' % (i, kind))
  if out_frame.numel() < T * len(heads) or out_episode.numel() < len(heads) or not (out_frame.is_contiguous() and out_episode.is_contiguous()):
    raise ValueError('replay_errors: outputs of %d / %d floats for T=%d and %d heads' % (out_frame.numel(), out_episode.numel(), T, len(heads)))
  check(_lib().geeco_replay_errors(_p(preds), _p(labels), T, P, len(heads), _iarr([h[0] for h in heads]), _iarr([h[1] for h in heads]),
                                   _iarr([h[2] for h in heads]), _p(out_frame), _p(out_episode), _stream()), 'geeco_replay_errors')


# -- episode replay for the dynamic-image controllers (csrc/replay_dynimg.hip, the state kernel of replay.hip; replay_dynimg.py) --
def replay_images_ws(windows, HW, device):
  """The workspace of replay_images_into for up to ``windows`` windows per call (per-block min / max; no zero-fill contract)."""
  return torch.empty(max(int(_lib().geeco_replay_images_ws_bytes(int(windows), int(HW))) // 4, 4), dtype=torch.float32, device=device)


def replay_images_into(cur_out, buf_out, diff_out, frame_addr, goal, T, t0, t1, K, HW, ws):
  """The conv1 inputs of the windows t0 <= t < t1 of one episode, read from its resident frames: frame_addr [>= T] int64 DEVICE
  addresses of the frames ([HW][3], uint8 or float32 as ``goal`` is), goal one frame of the same kind -> row t - t0 of cur_out
  (frame t as R, G, B, 0), diff_out (the normalised pair image of frame t and the goal) and buf_out (the normalised dynamic image
  of the frames max(0, t - K + 1 + k); None skips it), each a contiguous float32 [>= t1 - t0][HW][4].  Bitwise the images of
  goal_dynimgs_into / goal_dynimgs_u8_into on the explicitly built windows (include/geeco_hip.h: geeco_replay_images).  Bad arguments
  raise ValueError before anything is queued."""
  if HW < 4 or HW % 4:
    raise ValueError('replay_images: HW=%d must be a multiple of 4' % (HW,))
  _replay_windows('replay_images', T, t0, t1, K)
  if cur_out is None or diff_out is None:
    raise ValueError('replay_images: cur_out and diff_out are always written (only buf_out may be None)')
  n = t1 - t0
  for name, o in (('cur_out', cur_out), ('buf_out', buf_out), ('diff_out', diff_out)):
    if o is not None and (o.dtype != torch.float32 or not o.is_contiguous() or o.numel() < n * HW * 4):
      raise ValueError('replay_images: %s must be a contiguous float32 tensor of >= %d x %d x 4 values, got %s %s'
                       % (name, n, HW, o.dtype, tuple(o.shape)))
    if o is not None and o.data_ptr() % 16:
      raise ValueError('replay_images: %s is misaligned (16 bytes)' % name)
  if goal.dtype not in (torch.uint8, torch.float32) or goal.numel() != HW * 3 or not goal.is_contiguous():
    raise ValueError('replay_images: the goal must be one contiguous uint8 or float32 [%d][3] frame, got %s %s' % (HW, goal.dtype, tuple(goal.shape)))
  u8 = goal.dtype == torch.uint8
  if goal.data_ptr() % (4 if u8 else 16):
    raise ValueError('replay_images: the goal frame is misaligned (%d bytes)' % (4 if u8 else 16))
  if frame_addr.dtype != torch.int64 or not frame_addr.is_contiguous() or frame_addr.numel() < T:
    raise ValueError('replay_images: frame_addr must be a contiguous int64 table of >= T=%d addresses' % (T,))
  need = n * -(-(HW // 4) // 256) * 4
  if ws.dtype != torch.float32 or ws.numel() < need or ws.data_ptr() % 16:
    raise ValueError('replay_images: ws of %d floats for %d windows of %d pixels (replay_images_ws), 16-byte aligned' % (ws.numel(), n, HW))
  check(_lib().geeco_replay_images(_p(frame_addr), _p(goal), 1 if u8 else 0, ctypes.cast(_alpha_buf(K), ctypes.c_void_p),
                                   ctypes.cast(_alpha_buf(2), ctypes.c_void_p), T, t0, t1, K, HW, _p(cur_out), _p(buf_out), _p(diff_out),
                                   _p(ws), _stream()), 'geeco_replay_images')


def replay_states_pair_into(states, feat, tgt_feat, jnt, T, t0, t1, K, cells, ch, ch_t, J):
  """replay_states_into with a per-frame second table: feat [T][cells][ch], tgt_feat [T][cells][ch_t], jnt [T][J] -> states
  [K][N][state_stride] (contiguous, N >= t1 - t0), per cell the columns [feat | jnt | tgt] of the dense 'sequence' x 'dyndiff' model
  (state_concat_fwd_into with jnt_pos = 1).  Rows t1 - t0 .. N - 1 are not touched.  Bad arguments raise ValueError before anything
  is queued."""
  _replay_windows('replay_states_pair', T, t0, t1, K)
  if min(cells, ch, ch_t, J) < 1:
    raise ValueError('replay_states_pair: cells=%d ch=%d ch_t=%d J=%d' % (cells, ch, ch_t, J))
  _replay_states_shape('replay_states_pair', states, K, t1 - t0, cells * (ch + J + ch_t))
  if feat.numel() < T * cells * ch or tgt_feat.numel() < T * cells * ch_t or jnt.numel() < T * J:
    raise ValueError('replay_states_pair: feat / tgt_feat / jnt of %d / %d / %d floats for T=%d cells=%d ch=%d ch_t=%d J=%d'
                     % (feat.numel(), tgt_feat.numel(), jnt.numel(), T, cells, ch, ch_t, J))
  check(_lib().geeco_replay_states_pair(_p(feat), _p(tgt_feat), _p(jnt), T, t0, t1, states.shape[1], K, cells, ch, ch_t, J, _p(states),
                                        states.shape[2], _stream()), 'geeco_replay_states_pair')
