"""Window gathers and shared-frame training (csrc/window_gather.hip, shared_frames.hip; graph.py: shared_frames=F)."""
from __future__ import annotations

import ctypes

import torch

from .._native import PREDICT_FEAT_MODES, check
from ._marshal import _check_tables, _lib, _p, _stream


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
