"""numpy restatement of the time augmentation (include/geeco_hip.h: geeco_gather_windows_frames): (starts, frame_src)
become the frame each slot shows, and every slot then goes through the element functions the other augmentations are held to,
tests/_augment_ref.py and tests/_augment_scene_ref.py, unchanged -- the noise counter's k is therefore the OUTPUT slot."""
import numpy as np

from _augment_ref import augment_windows
from _augment_scene_ref import scene_windows


def compose(K, lag, drops):
  """The source row of one window from its definition, slot by slot: the lag first (slot k shows frame k - lag), then the drops on
  the lagged sequence (a dropped slot k >= 1 shows what slot k - 1 shows)."""
  row = [k - int(lag) for k in range(K)]
  for k in range(1, K):
    if k in drops:
      row[k] = row[k - 1]
  return row


def slot_frame_indices(starts, frame_src):
  """int64 [n][K]: the recorded frame of each slot, max(start + src, 0)."""
  return np.maximum(np.asarray(starts, np.int64)[:, None] + np.asarray(frame_src, np.int64), 0)


def time_values(episodes, picks, frame_src, frame_shape):
  """``episodes``: host arrays [T][fe] (uint8 or float32); ``picks`` [(episode, start)] per window.  -> (real numbers float64
  [n][K] + frame_shape, the same frames converted in float32 -- uint8 / 255 with numpy's IEEE division, float32 copied -- for the
  bitwise checks)."""
  idx = slot_frame_indices([st for _, st in picks], frame_src)
  v64 = np.empty(idx.shape + tuple(frame_shape), np.float64)
  v32 = np.empty(idx.shape + tuple(frame_shape), np.float32)
  for n, (e, _) in enumerate(picks):
    fr = np.asarray(episodes[e])[idx[n]]
    if fr.dtype == np.uint8:
      v64[n] = (fr.astype(np.float64) / 255.0).reshape(v64[n].shape)
      v32[n] = (fr.astype(np.float32) / np.float32(255.0)).reshape(v32[n].shape)
    else:
      v64[n] = fr.astype(np.float64).reshape(v64[n].shape)
      v32[n] = fr.reshape(v32[n].shape)
  return v64, v32


def time_windows(values, shift=None, colour=None, occ_rect=None, occ_colour=None, key=None, sigma=0.0, tag=0):
  """``values`` [n][K][H][W][C] from ``time_values`` -> float64 of the same shape: what the existing restatements give for windows
  whose k-th frame is that frame."""
  n = values.shape[0]
  shift = np.zeros((n, 2), np.int32) if shift is None else shift
  if values.shape[-1] == 3:
    return scene_windows(values, shift, colour, occ_rect, occ_colour, key, sigma, tag)
  assert occ_rect is None and not sigma
  return augment_windows(values, shift, colour)
