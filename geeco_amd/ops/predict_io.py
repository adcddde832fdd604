"""Batched predictor I/O (csrc/predict_io.hip; geeco_amd/batched_predictor.py)."""
from __future__ import annotations

import torch

from .._native import PREDICT_FEAT_MODES, check
from ._marshal import _iarr, _lib, _p, _stream


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
