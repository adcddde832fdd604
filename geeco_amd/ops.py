"""Thin tensor-level wrappers over the C-ABI (geeco_amd/_native.py).

PyTorch is plumbing only: tensors own device memory, ``torch.cuda.current_stream()`` provides the
HIP stream.  Every function enqueues HIP kernels from libgeeco_hip.so on that stream.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _native
from ._native import check


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


# --------------------------------------------------------------------------------------------
# dynamic image
# --------------------------------------------------------------------------------------------
_ALPHA_CACHE = {}


def _alpha_buf(K):
  if K not in _ALPHA_CACHE:
    buf = (ctypes.c_float * K)()
    _lib().geeco_dynimg_alpha(K, ctypes.cast(buf, ctypes.c_void_p))
    _ALPHA_CACHE[K] = buf
  return _ALPHA_CACHE[K]


def dynimg_alpha(K: int):
  return [float(v) for v in _alpha_buf(K)]


def dynimg_ws(N, hwc, device):
  nbytes = _lib().geeco_dynimg_ws_bytes(N, hwc)
  return torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device)


def dynimg_into(out, frames, K, N, HW, C, Cpad, ws, sample_stride, frame_stride, frames2=None):
  """out [N][HW][Cpad] <- normalised dynamic image of K frames (graph.py:30-55)."""
  check(_lib().geeco_dynimg_fwd(_p(frames), _p(frames2), sample_stride, frame_stride,
                                ctypes.cast(_alpha_buf(K), ctypes.c_void_p), N, K, HW, C, Cpad, _p(out), _p(ws),
                                _stream()), 'geeco_dynimg_fwd')


def dynimg_rgbd_into(out, rgb, depth, K, N, HW, ws, sample_stride, frame_stride, dsample_stride, dframe_stride, rgb2=None,
                     depth2=None):
  """out [N][HW][4] <- normalised dynamic image of K RGB-D frames whose rgb / depth live in separate tensors."""
  check(_lib().geeco_dynimg_rgbd_fwd(_p(rgb), _p(rgb2), sample_stride, frame_stride, _p(depth), _p(depth2), dsample_stride,
                                     dframe_stride, ctypes.cast(_alpha_buf(K), ctypes.c_void_p), N, K, HW, _p(out), _p(ws),
                                     _stream()), 'geeco_dynimg_rgbd_fwd')


def goal_dynimgs_ws(N, HW, device):
  """The workspace of goal_dynimgs_into / goal_dynimgs_u8_into (per-sample arrival counters + per-block min / max slots):
  zero-filled here ONCE; every call finds and leaves the counters zero."""
  return torch.zeros(max(int(_lib().geeco_goal_dynimgs_ws_bytes(N, HW)) // 4, 1), dtype=torch.int32, device=device)


def goal_dynimgs_into(cur_out, buf_out, diff_out, rgb, tgt_rgb, K, N, HW, ws, sample_stride, frame_stride, depth=None,
                      tgt_depth=None, dsample_stride=0, dframe_stride=0):
  """The goal model's three conv1 inputs (current frame padded, buffer image, diff image) in ONE launch and one pass over the
  window (both images normalised in registers before their only store).  ``ws`` = goal_dynimgs_ws(N, HW, device)."""
  check(_lib().geeco_goal_dynimgs_fwd(_p(rgb), sample_stride, frame_stride, _p(tgt_rgb), _p(depth), dsample_stride,
                                      dframe_stride, _p(tgt_depth), ctypes.cast(_alpha_buf(K), ctypes.c_void_p),
                                      ctypes.cast(_alpha_buf(2), ctypes.c_void_p), N, K, HW, _p(cur_out), _p(buf_out),
                                      _p(diff_out), _p(ws), _stream()), 'geeco_goal_dynimgs_fwd')


def goal_dynimgs_u8_into(cur_out, buf_out, diff_out, win_ptrs, tgt_ptrs, K, N, HW, ws, depth=None, tgt_depth=None,
                         dsample_stride=0, dframe_stride=0):
  """goal_dynimgs_into fed from resident uint8 frames: win_ptrs / tgt_ptrs are int64 DEVICE tensors of N addresses (window n =
  K consecutive [HW][3] uint8 frames; its target frame).  Bitwise the images of gather_windows_into(divisor 255) +
  goal_dynimgs_into, without the fp32 window tensor in between."""
  _check_tables(((win_ptrs, torch.int64, N), (tgt_ptrs, torch.int64, N)), buf_out.device, exact=True, message=(
      'goal_dynimgs_u8: address tables must be contiguous int64 tensors of N=%d entries on %s' % (N, buf_out.device)))
  check(_lib().geeco_goal_dynimgs_u8_fwd(ctypes.c_void_p(win_ptrs.data_ptr()), ctypes.c_void_p(tgt_ptrs.data_ptr()), _p(depth),
                                         dsample_stride, dframe_stride, _p(tgt_depth), ctypes.cast(_alpha_buf(K), ctypes.c_void_p),
                                         ctypes.cast(_alpha_buf(2), ctypes.c_void_p), N, K, HW, _p(cur_out), _p(buf_out),
                                         _p(diff_out), _p(ws), _stream()), 'geeco_goal_dynimgs_u8_fwd')


def goal_dynimgs_timeouts(ws, N) -> int:
  """Blocks of the one-pass input stage whose wait for their sample's blocks EVER expired on this workspace (their images are
  NaN).  Synchronises the current stream: for the places where the host reads the loss anyway."""
  n = ctypes.c_int64(-1)
  check(_lib().geeco_goal_dynimgs_timeouts(_p(ws), N, _stream(), ctypes.cast(ctypes.byref(n), ctypes.c_void_p)), 'geeco_goal_dynimgs_timeouts')
  return int(n.value)


def check_input_stage(ws, N):
  """Raises when the one-pass input stage reported a timeout on ``ws`` (include/geeco_hip.h: geeco_goal_dynimgs_timeouts)."""
  n = goal_dynimgs_timeouts(ws, N)
  if n:
    raise RuntimeError('geeco_amd: %d block(s) of the one-pass input stage gave up waiting for the other blocks of their sample '
                       '(the device did not start the blocks of a launch in index order: CU masking, a partitioned device, a '
                       'co-resident persistent kernel?).  The images of those samples were written as NaN (conv1\'s ReLU turns '
                       'them into zeros: the losses of those steps are finite and WRONG); zero-fill the workspace (ops.goal_dynimgs_ws) before using it again.' % n)


def dynimg(frames: torch.Tensor, Cpad=None) -> torch.Tensor:
  """frames [N,K,H,W,C] contiguous -> [N,H,W,Cpad]."""
  N, K, H, W, C = frames.shape
  Cpad = Cpad or C
  out = torch.empty(N, H, W, Cpad, dtype=torch.float32, device=frames.device)
  ws = dynimg_ws(N, H * W * C, frames.device)
  dynimg_into(out, frames.contiguous(), K, N, H * W, C, Cpad, ws, K * H * W * C, H * W * C)
  return out


def pack_pixels_into(dst, src, src_sample_stride, N, HW, C1, Cpad, src2=None, src2_sample_stride=0, C2=0):
  check(_lib().geeco_pack_pixels(_p(src), src_sample_stride, _p(src2), src2_sample_stride, N, HW, C1, C2, Cpad,
                                 _p(dst), _stream()), 'geeco_pack_pixels')


def pack_pixels_bwd_into(d_src, d_dst, src_sample_stride, N, HW, C1, Cpad, accumulate=False, d_src2=None, src2_sample_stride=0, C2=0,
                         accumulate2=False):
  """The adjoint of pack_pixels_into: d_src[n][p][:C1] (+)= d_dst[n][p][:C1]; d_src2 takes the next C2 channels."""
  check(_lib().geeco_pack_pixels_bwd(_p(d_dst), _p(d_src), src_sample_stride, 1 if accumulate else 0, _p(d_src2), src2_sample_stride,
                                     1 if accumulate2 else 0, N, HW, C1, C2, Cpad, _stream()), 'geeco_pack_pixels_bwd')


def dynimg_bwd_ws(N, HW, C, device):
  return torch.empty((int(_lib().geeco_dynimg_bwd_ws_bytes(N, HW, C)) + 3) // 4, dtype=torch.float32, device=device)


def dynimg_bwd_into(d_frames, g, frames, K, N, HW, C, Cpad, ws, sample_stride, frame_stride, d_sample_stride, d_frame_stride,
                    accumulate=False, frames2=None, d_frames2=None, accumulate2=False):
  """The adjoint of dynimg_into: g [N][HW][Cpad] (gradient of the normalised image) -> d_frames[n][t] (+)= alpha_t dD[n], and in the
  two-frame form d_frames2[n] (+)= alpha_1 dD[n] (include/geeco_hip.h: the tie rule, the summation order)."""
  check(_lib().geeco_dynimg_bwd(_p(g), _p(frames), _p(frames2), sample_stride, frame_stride, ctypes.cast(_alpha_buf(K), ctypes.c_void_p),
                                N, K, HW, C, Cpad, _p(d_frames), d_sample_stride, d_frame_stride, 1 if accumulate else 0, _p(d_frames2),
                                1 if accumulate2 else 0, _p(ws), _stream()), 'geeco_dynimg_bwd')


def gather_windows_into(out, src, starts_dev, N, K, frame_elems, divisor=1.0):
  """out[n][k] <- src[starts[n] + k] / divisor for an episode resident in HBM (uint8 or float32 frames)."""
  assert src.is_cuda and src.dtype in (torch.uint8, torch.float32) and starts_dev.dtype == torch.int32
  if not (src.device == out.device == starts_dev.device):
    raise RuntimeError('gather_windows: source %s, starts %s and output %s must be on one device' %
                       (src.device, starts_dev.device, out.device))
  check(_lib().geeco_gather_windows(ctypes.c_void_p(src.data_ptr()), 1 if src.dtype == torch.uint8 else 0,
                                    ctypes.c_void_p(starts_dev.data_ptr()), N, K, frame_elems, float(divisor), _p(out),
                                    _stream()), 'geeco_gather_windows')


def gather_windows_by_address_into(out, addr, kind, N, K, frame_elems):
  """out[n][k] <- frame k of the window at addr[n] (int64 device table; kind[n] int32: 0 = uint8 frames / 255, 1 = float32
  frames copied), ONE launch whatever the windows' order, episodes or kinds; bitwise gather_windows_into per window."""
  _check_tables(((addr, torch.int64, N), (kind, torch.int32, N)), out.device,
                'gather_windows_by_address: the tables must be contiguous int64 / int32 tensors of N=%d entries on %s' % (N, out.device))
  if out.numel() < N * K * frame_elems:
    raise ValueError('gather_windows_by_address: output of %d floats for %d x %d frames of %d' % (out.numel(), N, K, frame_elems))
  check(_lib().geeco_gather_windows_by_address(_p(addr), _p(kind), N, K, frame_elems, _p(out), _stream()),
        'geeco_gather_windows_by_address')


def _check_window_gather(who, out, tables, sigma, N, K, H, W, C, extras=True, per_frame=False):
  """The host-side checks of the three transforming gathers (csrc/window_gather.hip) under the entry's name ``who``: ``tables`` =
  (addr, kind, shift, colour, occ_rect, occ_colour, noise_key), the optional ones None; ``extras``: the entry takes the last
  three; ``per_frame``: addr is [N][K], shift is optional and C == 1 takes no extras."""
  addr, kind, shift, colour, occ_rect, occ_colour, noise_key = tables
  if (occ_rect is None) != (occ_colour is None):
    raise ValueError('%s: occ_rect and occ_colour come together' % who)
  if per_frame and C != 3 and (occ_rect is not None or float(sigma) != 0.0):
    raise ValueError('%s: C=%d takes the shift only (occluders and noise are built for RGB streams)' % (who, C))
  sized = ((addr, torch.int64, N * K if per_frame else N), (kind, torch.int32, N), (shift, torch.int32, 2 * N),
           (colour, torch.float32, 2 * C * N), (occ_rect, torch.int32, 16 * N), (occ_colour, torch.float32, 12 * N),
           (noise_key, torch.int32, 2))
  required = 2 if per_frame else 3
  _check_tables([t for i, t in enumerate(sized) if i < required or t[0] is not None], out.device,
                '%s: the tables must be contiguous int64 %s, int32 kinds [N], int32 shifts [N][2]%s float32 colour [N][%d]%s for N=%d%s on %s' % (
                    who, 'frame addresses [N][K]' if per_frame else 'addresses [N]', ',' if extras else ' and', 2 * C,
                    ', int32 rectangles [N][4][4], float32 rectangle colours [N][4][3] and an int32 key [2]' if extras else '', N,
                    ', K=%d' % K if per_frame else '', out.device))
  if out.numel() < N * K * H * W * C:
    raise ValueError('%s: output of %d floats for %d x %d frames of %d x %d x %d' % (who, out.numel(), N, K, H, W, C))


def gather_windows_augmented_into(out, addr, kind, shift, colour, N, K, H, W, C):
  """gather_windows_by_address_into with a per-window augmentation: out[n][k][y][x][c] <- pixel (y - dy, x - dx) of frame k of
  the window at addr[n], (dy, dx) = shift[n] (int32 [N][2] device table), times gain[c] plus bias[c] clamped to [0, 1] when
  ``colour`` (float32 [N][2 * C] = gain[C], bias[C]; None: values unchanged); exactly 0 where the source pixel is outside the
  frame.  ONE launch; any shift is safe (include/geeco_hip.h: geeco_gather_windows_augmented)."""
  _check_window_gather('gather_windows_augmented', out, (addr, kind, shift, colour, None, None, None), 0.0, N, K, H, W, C, extras=False)
  check(_lib().geeco_gather_windows_augmented(_p(addr), _p(kind), _p(shift), _p(colour), N, K, H, W, C, _p(out), _stream()),
        'geeco_gather_windows_augmented')


def gather_windows_scene_into(out, addr, kind, shift, colour, occ_rect, occ_colour, noise_key, sigma, tag, N, K, H, W, C):
  """gather_windows_augmented_into of an RGB stream (C == 3) with occluders and sensor noise behind the gather:
  ``occ_rect`` int32 [N][4][4] = (y0, x0, h, w) per slot and ``occ_colour`` float32 [N][4][3], both None for no occluders;
  ``noise_key`` int32 [2] (the two uint32 words of the Philox key, on the device; None only when ``sigma`` == 0); ``tag`` 0 for
  'rgb', 1 for 'target_rgb'.  ONE launch (include/geeco_hip.h: geeco_gather_windows_scene)."""
  _check_window_gather('gather_windows_scene', out, (addr, kind, shift, colour, occ_rect, occ_colour, noise_key), sigma, N, K, H, W, C)
  check(_lib().geeco_gather_windows_scene(_p(addr), _p(kind), _p(shift), _p(colour), _p(occ_rect), _p(occ_colour), _p(noise_key),
                                          float(sigma), int(tag), N, K, H, W, C, _p(out), _stream()), 'geeco_gather_windows_scene')


def gather_windows_frames_into(out, frame_addr, kind, shift, colour, occ_rect, occ_colour, noise_key, sigma, tag, N, K, H, W, C):
  """gather_windows_scene_into following ONE ADDRESS PER FRAME: out[n][k] is built from the frame at
  ``frame_addr[n][k]`` (int64 [N][K] device table, read when the kernel runs), so a slot may show any resident frame of its
  window's kind -- a dropped frame delivered again, a camera that lags.  ``shift`` may be None (no shift); C == 1 (depth) takes
  ``shift`` and ``colour`` only.  Everything else, and every value, as gather_windows_scene_into / _augmented_into /
  _by_address_into for the arguments that are set; the noise counter's k is the OUTPUT slot.  The caller has checked that every
  address holds a whole frame (DeviceWindows.frame_addresses).  ONE launch (include/geeco_hip.h: geeco_gather_windows_frames)."""
  _check_window_gather('gather_windows_frames', out, (frame_addr, kind, shift, colour, occ_rect, occ_colour, noise_key), sigma,
                       N, K, H, W, C, per_frame=True)
  check(_lib().geeco_gather_windows_frames(_p(frame_addr), _p(kind), _p(shift), _p(colour), _p(occ_rect), _p(occ_colour), _p(noise_key),
                                           float(sigma), int(tag), N, K, H, W, C, _p(out), _stream()), 'geeco_gather_windows_frames')


# -- batched predictor I/O (csrc/predict_io.hip; geeco_amd/batched_predictor.py) --------------------------------------------
def predict_range_check_into(ctl, frames, B, HW, C, lo, hi):
  """ctl[b] = ctl[B] = 1 when channels 0..2 of env b's float32 frame leave [lo, hi] (or hold a NaN); never clears them."""
  check(_lib().geeco_predict_range_check(_p(frames), B, HW, C, float(lo), float(hi), _p(ctl), _stream()),
        'geeco_predict_range_check')


def predict_push_dense_into(rgb, depth, jnt_state, frames, jnt, reset, ctl, B, K, HW, C, J):
  """Shifts the dense windows of B envs in place by one frame (all K slots = the frame where reset[b]); nothing moves while
  ctl[B] is set.  frames: [B][HW][C] float32, or uint8 (C == 3, divided by 255 as gather_windows_into does)."""
  u8 = frames.dtype == torch.uint8
  check(_lib().geeco_predict_push_dense(_p(frames), 1 if u8 else 0, _p(jnt), _p(reset), _p(ctl[B:B + 1]), B, K, HW, C, J,
                                        _p(rgb), _p(depth), _p(jnt_state), _stream()), 'geeco_predict_push_dense')


def predict_push_ring_into(ring, heads, win_table, jnt_state, frames_u8, jnt, reset, ctl, B, K, HW, J):
  """Writes B uint8 frames into the mirrored rings [B][2K][HW*3] and points win_table (int64, device) at each env's window."""
  check(_lib().geeco_predict_push_ring(_p(frames_u8), _p(jnt), _p(reset), _p(ctl[B:B + 1]), B, K, HW, J, _p(ring), _p(heads),
                                       _p(win_table), _p(jnt_state), _stream()), 'geeco_predict_push_ring')


def predict_pack_into(out, ctl_out, preds, ctl, B, segs, imgs=(), HW=0, C=0, img_out=None):
  """preds [B][P] -> out [B][F]: segs = (src column, length, argmax) per returned head; control words -> ctl_out (zeroed in
  ctl); imgs: up to two [B][HW][4] images -> img_out [len(imgs)][B][HW][C]."""
  imgs = list(imgs) + [None] * (2 - len(imgs))
  check(_lib().geeco_predict_pack(_p(preds), preds.shape[1], B, len(segs), _iarr([s[0] for s in segs]),
                                  _iarr([s[1] for s in segs]), _iarr([int(s[2]) for s in segs]), _p(out), out.shape[1],
                                  _p(ctl), _p(ctl_out), _p(imgs[0]), _p(imgs[1]), HW, C, _p(img_out), _stream()),
        'geeco_predict_pack')


PREDICT_FEAT_MODES = {'plain': 0, 'constant': 1, 'residual': 2}     # GEECO_PREDICT_FEAT_* of include/geeco_hip.h


def predict_pack_newest_into(x_in, frames, B, HW, C):
  """frames [B][HW][C] (float32, or uint8 with C == 3: divided by 255 as the dense push does) -> encoder input x_in [B][HW][4]."""
  check(_lib().geeco_predict_pack_newest(_p(frames), 1 if frames.dtype == torch.uint8 else 0, B, HW, C, _p(x_in), _stream()),
        'geeco_predict_pack_newest')


def predict_push_features_into(states, feat_ring, jnt_ring, heads, feat, jnt, reset, ctl, mode, B, K, cells, ch, J, state_stride,
                               tgt_feat=None):
  """Pushes the new features [B][cells][ch] / joint states [B][J] into the rings [B][K][..] (every slot where reset[b]), writes
  states [K][B][state_stride] oldest first in the columns of state_concat_fwd_into for ``mode`` ('plain', 'constant',
  'residual') and advances heads [B]; nothing moves while ctl[B] is set."""
  check(_lib().geeco_predict_push_features(_p(feat), _p(jnt), _p(reset), _p(ctl[B:B + 1]), _p(tgt_feat), PREDICT_FEAT_MODES[mode],
                                           B, K, cells, ch, J, _p(feat_ring), _p(jnt_ring), _p(heads), _p(states), state_stride,
                                           _stream()), 'geeco_predict_push_features')


# -- episode replay (csrc/replay.hip; geeco_amd/replay.py) ---------------------------------------------------------------------
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


REPLAY_SQUARED_ERROR, REPLAY_CLASS_HIT = 0, 1      # head kinds of geeco_replay_errors


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


# -- attributions (csrc/attribution.hip; geeco_amd/attribution.py) --------------------------------------------------------------
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


# -- shared-frame training (csrc/shared_frames.hip; graph.py: shared_frames=F) ------------------------------------------------
def pack_frames_by_address_into(x_in, table, F, HW, frames_u8):
  """table [F] int64 device addresses of resident RGB frames (uint8 or float32, one kind per call; 0 = unused slot) -> the
  encoder input x_in [F][HW][4] (uint8 divided by 255 as gather_windows_into does; zeros for an unused slot)."""
  assert table.dtype == torch.int64 and table.numel() >= F
  check(_lib().geeco_pack_frames_by_address(_p(table), F, 1 if frames_u8 else 0, HW, _p(x_in), _stream()),
        'geeco_pack_frames_by_address')


def window_states_fwd_into(states, feat, idx, jnt, mode, F, N, K, cells, ch, J, state_stride, tgt_idx=None):
  """feat [F][cells][ch] gathered through idx [N][K] (int32) into states [K][N][state_stride], ONE launch, in the columns of
  state_concat_fwd_into for ``mode`` ('plain', 'constant', 'residual'); tgt_idx [N]: slot of each window's target frame."""
  assert idx.dtype == torch.int32 and (tgt_idx is None or tgt_idx.dtype == torch.int32)
  check(_lib().geeco_window_states_fwd(_p(feat), _p(idx), _p(jnt), _p(tgt_idx), PREDICT_FEAT_MODES[mode], F, N, K, cells, ch, J,
                                       _p(states), state_stride, _stream()), 'geeco_window_states_fwd')


def window_states_bwd_into(dfeat, dstates, state_stride, idx, feat, mode, F, N, K, cells, ch, J, tgt_idx=None):
  """The adjoint of window_states_fwd_into: dfeat [F][cells][ch] <- per slot the sum, in one fixed order, of the feature (and
  target) columns of dstates [K][N][state_stride] over the window positions that use it, masked by ``feat`` > 0 (the forward's
  features: ReluGrad of the encoder's last layer, as state_concat_bwd_into).  Unreferenced slots get zeros."""
  assert idx.dtype == torch.int32 and (tgt_idx is None or tgt_idx.dtype == torch.int32)
  check(_lib().geeco_window_states_bwd(_p(dstates), state_stride, _p(feat), _p(idx), _p(tgt_idx), PREDICT_FEAT_MODES[mode], F, N, K,
                                       cells, ch, J, _p(dfeat), _stream()), 'geeco_window_states_bwd')


# --------------------------------------------------------------------------------------------
# conv encoder
# --------------------------------------------------------------------------------------------
def conv3x3_fwd_into(y, x, w, b, G, gs_x, gs_w, gs_b, gs_y, N, H, W, Cin, Cout, stride, relu=True, ws=None):
  check(_lib().geeco_conv3x3_fwd(_p(x), _p(w), _p(b), _p(y), G, gs_x, gs_w, gs_b, gs_y, N, H, W, Cin, Cout,
                                 stride, 1 if relu else 0, _p(ws), _stream()), 'geeco_conv3x3_fwd')


def conv3x3_fwd_state_into(y, x, w, b, G, gs_x, gs_w, gs_b, gs_y, N, H, W, Cin, Cout, stride, ws, state, state_stride, feat_off,
                           Ctot, jnt, jnt_stride, jnt_off, J):
  """The top layer's forward with the one-step decoder's state concat in the split-K epilogue (``geeco_conv3x3_fwd_state``).
  Returns False (nothing launched) when the shape has no such epilogue: run conv3x3_fwd_into + state_concat_fwd_into."""
  rc = _lib().geeco_conv3x3_fwd_state(_p(x), _p(w), _p(b), _p(y), G, gs_x, gs_w, gs_b, gs_y, N, H, W, Cin, Cout, stride, _p(ws),
                                      _iarr(feat_off), Ctot, _p(jnt), jnt_stride, jnt_off, J, _p(state), state_stride, _stream())
  if rc == _native.GEECO_ENOSUP:
    return False
  check(rc, 'geeco_conv3x3_fwd_state')
  return True


def conv3x3_fwd_ws_bytes(G, N, H, W, Cin, Cout, stride):
  return int(_lib().geeco_conv3x3_fwd_ws_bytes(G, N, H, W, Cin, Cout, stride))


def conv3x3_dgrad_into(dx, dz, wt, ymask, G, gs_dz, gs_wt, gs_dx, N, H, W, Cin, Cout, stride, ws=None, w=None, gs_w=0):
  check(_lib().geeco_conv3x3_dgrad(_p(dz), _p(w), _p(wt), _p(ymask), _p(dx), G, gs_dz, gs_w, gs_wt, gs_dx, N, H, W,
                                   Cin, Cout, stride, _p(ws), _stream()), 'geeco_conv3x3_dgrad')


def conv1_dgrad_into(dx, dz1, w1, G, gs_dz, gs_w, gs_dx, F, H, W, Cin, Cout=32):
  """conv1's input gradient: dx [G][F][H][W][4] <- dz1 [G][F][H][W][32], w1 the [3][3][Cin][32] variable (geeco_conv1_dgrad).  Returns
  False, nothing launched, for a layer the kernel was not built for."""
  rc = _lib().geeco_conv1_dgrad(_p(dz1), _p(w1), _p(dx), G, gs_dz, gs_w, gs_dx, F, H, W, Cin, Cout, _stream())
  if rc == _native.GEECO_ENOSUP:
    return False
  check(rc, 'geeco_conv1_dgrad')
  return True


def conv3x3_dgrad_ws_bytes(G, N, H, W, Cin, Cout, stride):
  return int(_lib().geeco_conv3x3_dgrad_ws_bytes(G, N, H, W, Cin, Cout, stride))


def _ws(nbytes, device):
  return torch.empty(nbytes // 4 + 4, dtype=torch.float32, device=device) if nbytes > 0 else None


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
  if pending is None:
    if reserved_cus:
      raise ValueError('reserved_cus is an argument of the deferred-slab-sum form: pass pending=[...]')
    check(_lib().geeco_conv3x3_wgrad(_p(x), _p(dz), _p(dw), _p(db), G, gs_x, gs_dz, gs_dw, gs_db, N, H, W, Cin,
                                     Cout, stride, _p(ws), _stream()), 'geeco_conv3x3_wgrad')
    return
  item = _native.SlabReduce()
  check(_lib().geeco_conv3x3_wgrad_partial(_p(x), _p(dz), _p(dw), _p(db), G, gs_x, gs_dz, gs_dw, gs_db, N, H, W, Cin,
                                           Cout, stride, _p(ws), _stream(), ctypes.byref(item), int(reserved_cus)),
        'geeco_conv3x3_wgrad_partial')
  if item.S > 0:
    pending.append(item)


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
  if rc == _native.GEECO_ENOSUP:
    return False
  check(rc, 'geeco_conv3x3_wgrad_pair')
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
  if rc == _native.GEECO_ENOSUP:
    return False
  check(rc, 'geeco_conv_top_bwd')
  _take_pending(items, pending)
  return True


def slab_reduce_batch(pending, prepare=None, beta1=0.9, beta2=0.999):
  """Finishes the deferred slab sums of ``pending`` (<= 8 per launch) and empties the list.  ``prepare`` = (global_step, lr,
  scal): the last launch also does adam_prepare's work (one block more instead of a dependent launch); a learning-rate schedule
  (``lr_schedule_struct``) in place of the float ``lr``: adam_prepare_schedule's."""
  MAX = 8
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
  if pending is None:
    if reserved_cus:
      raise ValueError('reserved_cus is an argument of the deferred-slab-sum form: pass pending=[...]')
    check(_lib().geeco_conv2_dgrad_conv1_wgrad(_p(dz2), _p(w2), _p(y1), _p(x), _p(dw1), _p(db1), _p(dz1), G, gs_dz2,
                                               gs_w2, gs_y1, gs_x, gs_dw1, gs_db1, N, H, W, real_channels, _p(ws),
                                               _stream()), 'geeco_conv2_dgrad_conv1_wgrad')
    return
  item = _native.SlabReduce()
  check(_lib().geeco_conv2_dgrad_conv1_wgrad_partial(_p(dz2), _p(w2), _p(y1), _p(x), _p(dw1), _p(db1), _p(dz1), G,
                                                     gs_dz2, gs_w2, gs_y1, gs_x, gs_dw1, gs_db1, N, H, W, real_channels,
                                                     _p(ws), _stream(), ctypes.byref(item), int(reserved_cus)),
        'geeco_conv2_dgrad_conv1_wgrad_partial')
  if item.S > 0:
    pending.append(item)


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
  item = _native.SlabReduce() if pending is not None else None
  check(_lib().geeco_conv2_dgrad_conv1_wgrad_bits(_p(dz2), _p(w2), _p(y1_bits), _p(x), _p(dw1), _p(db1), G, gs_dz2, gs_w2,
                                                  gs_bits, gs_x, gs_dw1, gs_db1, N, H, W, real_channels, _p(ws), _stream(),
                                                  ctypes.byref(item) if item is not None else None, int(reserved_cus)),
        'geeco_conv2_dgrad_conv1_wgrad_bits')
  if item is not None and item.S > 0:
    pending.append(item)


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
  ws = torch.empty(conv3x3_wgrad_ws_bytes(1, N, H, W, Cin, Cout, stride) // 4 + 4, dtype=torch.float32, device=x.device)
  conv3x3_wgrad_into(dw, db, x.contiguous(), dz.contiguous(), 1, 0, 0, 0, 0, N, H, W, Cin, Cout, stride, ws)
  return dw, db


# --------------------------------------------------------------------------------------------
# decoder pieces
# --------------------------------------------------------------------------------------------
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
  ws = torch.empty(gemm_ws_bytes(M, N, K) // 4 + 4, dtype=torch.float32, device=A.device)
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
  if rc == _native.GEECO_ENOSUP:
    return False
  check(rc, what)
  return True


def lstm_seq_heads_into(preds, zx, wh, bias, fc1_w, fc1_b, heads_w, heads_b, head_size, N, T, H, Hfc, ldz, ldw, h_last=None,
                        c_last=None):
  """Inference decoder after the hoisted input projection in ONE launch: T LSTM steps from the zero state over ``zx`` [T][N][4H]
  (row stride ``ldz``; X Wx without bias), fc1 and the heads on the last output -> ``preds`` [N][sum sizes]; ``h_last`` / ``c_last``
  [N][H] optionally receive the final state.  Returns False (nothing launched) for shapes the kernel does not serve: the caller
  then runs the step chain (gemm_into + lstm_gates_fwd_into per step, heads_loss_into)."""
  nh = len(heads_w)
  rc = _lib().geeco_lstm_seq_heads_fwd(_p(zx), ldz, _p(wh), ldw, _p(bias), _p(fc1_w), _p(fc1_b), nh, _parr(heads_w), _parr(heads_b),
                                       _iarr(head_size), N, T, H, Hfc, _p(preds), _p(h_last), _p(c_last), _stream())
  if rc == _native.GEECO_ENOSUP:
    return False
  check(rc, 'geeco_lstm_seq_heads_fwd')
  return True


# --------------------------------------------------------------------------------------------
# optimiser
# --------------------------------------------------------------------------------------------
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


def _adam_segments(segments):
  if not 1 <= len(segments) <= _native.ADAM_SEGMENTS_MAX:
    raise ValueError('adam_tf_segments: 1..%d pieces, got %d' % (_native.ADAM_SEGMENTS_MAX, len(segments)))
  arr = (_native.AdamSegment * len(segments))()
  for a, (g, off, n) in zip(arr, segments):
    if g.numel() < n:
      raise ValueError('adam_tf_segments: a piece of %d floats with %d gradients' % (n, g.numel()))
    a.g, a.p_off, a.count = _p(g), int(off), int(n)
  return arr


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


# --------------------------------------------------------------------------------------------
# per-variable statistics
# --------------------------------------------------------------------------------------------
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


class VariableStatsPlan:
  """What one model's statistics pass keeps on the device: the table of ``variables`` = [(offset, count)], the workspace and the
  records.  Allocated once; ``run`` enqueues the two launches and allocates nothing."""

  def __init__(self, variables, device):
    self.variables = [(int(o), int(c)) for o, c in variables]
    host = variable_stats_table(self.variables)
    self.nchunks = (host.size - 2 * len(self.variables)) // 2
    self.table = torch.from_numpy(host).to(device)
    self.ws = torch.zeros(variable_stats_ws_bytes(self.nchunks) // 4, dtype=torch.int32, device=device)
    self.out = torch.zeros(len(self.variables) * VARSTATS_DTYPE.itemsize, dtype=torch.uint8, device=device)

  def run(self, p, m, v, segments, n, grad_scale=1.0, eps=1e-8):
    variable_stats(self.out, self.ws, self.table, p, m, v, segments, n, self.variables, self.nchunks, grad_scale, eps)

  def records(self):
    """The records on the host (numpy, VARSTATS_DTYPE).  SYNCHRONISES: the copy waits for the stream."""
    return self.out.cpu().numpy().view(VARSTATS_DTYPE).copy()


# --------------------------------------------------------------------------------------------
# diagnostics
# --------------------------------------------------------------------------------------------
def kernel_trace(fn):
  """Runs ``fn()`` and returns the names of the conv kernels its calls dispatched (in launch order)."""
  lib = _lib()
  lib.geeco_debug_kernel_trace_begin()
  try:
    fn()
  finally:
    names = lib.geeco_debug_kernel_trace_end()
  return [n for n in (names.decode() if names else '').split(';') if n]
