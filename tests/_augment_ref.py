"""numpy restatement of the window augmentation (include/geeco_hip.h: geeco_gather_windows_augmented), in float64.
Written from the definition -- out[y][x][c] = tint(v[y - dy][x - dx][c]) where that source pixel exists, else 0 -- with the
zero fill produced directly (slices of a zero array), never by masking a wrapped-around roll."""
import numpy as np


def moved(frames, dy, dx):
  """``frames`` [..., H, W, C] moved by (dy, dx) whole pixels, zeros moving in: out[..., y, x, :] = frames[..., y - dy, x - dx, :]
  where 0 <= y - dy < H and 0 <= x - dx < W.  Keeps the dtype (a pure move is exact)."""
  frames = np.asarray(frames)
  H, W = frames.shape[-3:-1]
  dy, dx = int(dy), int(dx)
  out = np.zeros_like(frames)
  if abs(dy) >= H or abs(dx) >= W:
    return out
  out[..., max(dy, 0):H + min(dy, 0), max(dx, 0):W + min(dx, 0), :] = \
      frames[..., max(-dy, 0):H + min(-dy, 0), max(-dx, 0):W + min(-dx, 0), :]
  return out


def in_view(H, W, dy, dx):
  """bool [H, W]: output pixels whose source pixel lies inside the frame."""
  y, x = np.mgrid[0:H, 0:W]
  return (y - int(dy) >= 0) & (y - int(dy) < H) & (x - int(dx) >= 0) & (x - int(dx) < W)


def augment_windows(values, shift, colour=None):
  """``values`` [n, ..., H, W, C]: the plain windows as real numbers (uint8 frames: u8 / 255), any leading window axes after n.
  ``shift`` [n][2] = (dy, dx); ``colour`` [n][2 * C] = gain[C], bias[C] or None.  float64 [n, ..., H, W, C]:
  clip(v * gain + bias, 0, 1) of the moved pixels (v itself without ``colour``), exactly 0 outside the view."""
  values = np.asarray(values, np.float64)
  n, (H, W, C) = values.shape[0], values.shape[-3:]
  out = np.zeros_like(values)
  for i in range(n):
    dy, dx = (int(s) for s in shift[i])
    v = values[i]
    if colour is not None:
      gain, bias = np.asarray(colour[i][:C], np.float64), np.asarray(colour[i][C:2 * C], np.float64)
      v = np.clip(v * gain + bias, 0.0, 1.0)          # the tint is per pixel: it commutes with the move
    out[i] = moved(v, dy, dx)                         # (zeros move in AFTER the tint: they are not tinted)
  return out
