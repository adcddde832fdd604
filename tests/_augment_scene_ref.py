"""numpy restatement of the scene augmentation (include/geeco_hip.h: geeco_gather_windows_scene), in float64 on
top of tests/_augment_ref.py: Philox4x32-10 from its definition (Salmon et al., SC'11; 64-bit products split into halves), the
Box-Muller normals of its four output words, the rectangles painted as slices, the noise added and clipped."""
import numpy as np

from _augment_ref import augment_windows

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
  """``counter`` [..., 4] and ``key`` [..., 2] (or [2]) of 32-bit words -> uint32 [..., 4]."""
  c = [np.asarray(counter, np.uint64)[..., i] & MASK for i in range(4)]
  k = [np.asarray(key, np.uint64)[..., i] & MASK for i in range(2)]
  for _ in range(10):
    p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]          # < 2^64: no wrap
    c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
    k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
  return np.stack(np.broadcast_arrays(*c), axis=-1).astype(np.uint32)


def normals_of_words(x):
  """uint32 [..., 4] -> float64 [..., 4]: (x0, x1) -> z0, z1 and (x2, x3) -> z2, z3 by Box-Muller, ua = ((xa >> 8) + 0.5) 2^-24 in
  (0, 1), ub = (xb >> 8) 2^-24: z = sqrt(-2 ln ua) (cos, sin)(2 pi ub)."""
  x = np.asarray(x, np.uint32)
  out = np.empty(x.shape, np.float64)
  for a in (0, 2):
    ua = ((x[..., a] >> 8).astype(np.float64) + 0.5) * 2.0 ** -24
    ub = (x[..., a + 1] >> 8).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(ua))
    out[..., a], out[..., a + 1] = r * np.cos(2.0 * np.pi * ub), r * np.sin(2.0 * np.pi * ub)
  return out


def noise_field(key, tag, n, K, fe):
  """float64 [n][K][fe]: z of element e of frame k of window i = normal e % 4 of the counter (e // 4, k, i, tag)."""
  groups = -(-fe // 4)
  ctr = np.zeros((n, K, groups, 4), np.uint64)
  ctr[..., 0] = np.arange(groups)[None, None, :]
  ctr[..., 1] = np.arange(K)[None, :, None]
  ctr[..., 2] = np.arange(n)[:, None, None]
  ctr[..., 3] = tag
  z = normals_of_words(philox4x32_10(ctr, np.asarray(key, np.uint64)))
  return z.reshape(n, K, groups * 4)[:, :, :fe]


def paint(v, occ_rect, occ_colour):
  """``v`` [n, ..., H, W, 3] with the rectangles of each window painted in slot order (a later slot covers an earlier one), the
  slices clipped to the frame in Python integers; h <= 0 or w <= 0: an empty slot.  Keeps the dtype; returns (painted, bool
  [n][H][W] of covered pixels)."""
  v = np.array(v)
  n, (H, W) = v.shape[0], v.shape[-3:-1]
  covered = np.zeros((n, H, W), bool)
  for i in range(n):
    for j in range(4):
      y0, x0, h, w = (int(t) for t in occ_rect[i][j])
      if h <= 0 or w <= 0:
        continue
      ys, xs = slice(max(y0, 0), max(min(y0 + h, H), 0)), slice(max(x0, 0), max(min(x0 + w, W), 0))
      v[i][..., ys, xs, :] = np.asarray(occ_colour[i][j]).astype(v.dtype)
      covered[i][ys, xs] = True
  return v, covered


def scene_windows(values, shift, colour=None, occ_rect=None, occ_colour=None, key=None, sigma=0.0, tag=0):
  """``values`` [n, K, H, W, 3] plain windows as real numbers -> float64 [n, K, H, W, 3]: shift / tint (augment_windows), the
  rectangles, then clip(v + sigma z, 0, 1) (sigma == 0: no noise step)."""
  v = augment_windows(values, shift, colour)
  if occ_rect is not None:
    v, _ = paint(v, occ_rect, occ_colour)
  if sigma:
    n, K = v.shape[:2]
    z = noise_field(key, tag, n, K, int(np.prod(v.shape[2:]))).reshape(v.shape)
    v = np.clip(v + np.float64(np.float32(sigma)) * z, 0.0, 1.0)
  return v
