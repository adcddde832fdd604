"""The dynamic-image input stage and the pixel packing (csrc/dynimg*.hip, input_grad.hip, frame_pack.hip)."""
from __future__ import annotations

import ctypes

import torch

from .._native import check
from ._marshal import _alpha_buf, _check_tables, _lib, _p, _stream


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
