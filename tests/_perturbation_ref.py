"""numpy restatement of the perturbation kernels (include/geeco_hip.h: geeco_perturb_apply, geeco_perturb_score,
geeco_perturb_accumulate, geeco_perturb_finish).  Float32 operation by float32 operation in the header's stated order, so every
result is the device's to the bit; the draws come from tests/_augment_scene_ref.py's Philox4x32-10."""
import numpy as np

from _augment_scene_ref import philox4x32_10

F = np.float32


def positions(size, patch, stride):
  """The start of every position of a patch along one axis: 1 if the patch covers it, else ceil((size - patch) / stride) + 1, the
  last clamped to size - patch."""
  patch = min(patch, size)
  G = 1 if patch >= size else -(-(size - patch) // stride) + 1
  return [min(j * stride, size - patch) for j in range(G)]


def occlusion_grid(H, W, patch, stride):
  """(Gy, Gx, [(y0, y1, x0, x1) of step m = j * Gx + i])."""
  ys, xs = positions(H, patch[0], stride[0]), positions(W, patch[1], stride[1])
  ph, pw = min(patch[0], H), min(patch[1], W)
  return len(ys), len(xs), [(y, y + ph, x, x + pw) for y in ys for x in xs]


def occlusion_field(H, W, patch, stride, step, N):
  """o [N][H][W] of step ``step``: 1 inside the patch, the same for every sample."""
  y0, y1, x0, x1 = occlusion_grid(H, W, patch, stride)[2][step]
  o = np.zeros((N, H, W), F)
  o[:, y0:y1, x0:x1] = 1
  return o


def keep_threshold(keep_prob):
  return min(max(int(round(float(keep_prob) * 2.0 ** 32)), 1), (1 << 32) - 1)


def rise_draws(H, W, g, keep_prob, key, step, sample):
  """(bits float32 [g + 1][g + 1], dy, dx): word i is output i % 4 of the counter (i / 4, sample, step, 1) under the key's two
  words; bit = word < threshold; the two words behind the bits, modulo the cell size, are the shift."""
  nb = (g + 1) ** 2
  q = np.arange(-(-(nb + 2) // 4), dtype=np.uint64)
  ctr = np.stack([q, np.full_like(q, sample), np.full_like(q, step), np.ones_like(q)], -1)
  words = philox4x32_10(ctr, np.array([key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF], np.uint64)).reshape(-1).astype(np.uint64)
  bits = (words[:nb] < np.uint64(keep_threshold(keep_prob))).astype(F).reshape(g + 1, g + 1)
  return bits, int(words[nb] % np.uint64(-(-H // g))), int(words[nb + 1] % np.uint64(-(-W // g)))


def rise_mask(H, W, g, bits, dy, dx):
  """o [H][W] = 1 - keep of one mask from its bits and shift: the bilinear interpolation in the header's order, every operation in
  float32."""
  ch, cw = -(-H // g), -(-W // g)
  inv_ch, inv_cw = F(1) / F(ch), F(1) / F(cw)
  yy, xx = np.arange(H) + dy, np.arange(W) + dx
  r, c = yy // ch, xx // cw
  fy, fx = ((yy - r * ch).astype(F) * inv_ch)[:, None], ((xx - c * cw).astype(F) * inv_cw)[None, :]
  r1, c1 = np.minimum(r + 1, g), np.minimum(c + 1, g)
  k00, k01, k10, k11 = bits[r][:, c], bits[r][:, c1], bits[r1][:, c], bits[r1][:, c1]
  top, bot = k00 + fx * (k01 - k00), k10 + fx * (k11 - k10)
  out = F(1) - (top + fy * (bot - top))
  assert out.dtype == F
  return out


def rise_field(H, W, g, keep_prob, key, step, N, sample0=0):
  """o [N][H][W]: ``rise_mask`` of each sample's draws."""
  return np.stack([rise_mask(H, W, g, *rise_draws(H, W, g, keep_prob, key, step, sample0 + n)) for n in range(N)])


def fill_of(fill, n):
  """The fill as a flat float32 [n]: None = zeros, else its elements repeated with its own length as the period."""
  if fill is None:
    return np.zeros(n, F)
  b = np.asarray(fill, F).reshape(-1)
  assert n % b.size == 0
  return np.tile(b, n // b.size)


def apply(x, fill, o):
  """x [N][frames][H][W][C] (or [N][H][W][C]) occluded by o [N][H][W]: x where o == 0, fill where o == 1, x + o * (fill - x) else."""
  x = np.asarray(x, F)
  b = fill_of(fill, x.size).reshape(x.shape)
  oo = (o[:, None] if x.ndim == 5 else o)[..., None]
  mixed = x + oo * (b - x)
  assert mixed.dtype == F
  return np.where(oo == 0, x, np.where(oo == 1, b, mixed))


def score(preds, preds0, w):
  """d [N] = sum_j w_j (p - p0)^2, j ascending from +0, each operation in float32."""
  preds, preds0, w = np.asarray(preds, F), np.asarray(preds0, F), np.asarray(w, F)
  d = np.zeros(preds.shape[0], F)
  for j in range(preds.shape[1]):
    t = preds[:, j] - preds0[:, j]
    d = d + w[j] * (t * t)
  assert d.dtype == F
  return d


def accumulate(num, den, d, o, overwrite):
  """(num, den) [N][H][W] after one step: where o != 0, (0 if overwrite else num) + d[n] * o and (0 if overwrite else den) + o."""
  num0, den0 = (np.zeros_like(o), np.zeros_like(o)) if overwrite else (np.asarray(num, F), np.asarray(den, F))
  with np.errstate(invalid='ignore'):
    n1, d1 = num0 + np.asarray(d, F)[:, None, None] * o, den0 + o
  assert n1.dtype == F and d1.dtype == F
  return np.where(o != 0, n1, num0), np.where(o != 0, d1, den0)


def finish(num, den):
  with np.errstate(invalid='ignore', divide='ignore'):
    out = np.where(den > 0, np.asarray(num, F) / np.where(den > 0, den, F(1)), F(0))
  assert out.dtype == F
  return out


def saliency(fields, scores):
  """The whole estimator from the per-step fields [M][N][H][W] and scores [M][N]."""
  num = den = None
  for m, (o, d) in enumerate(zip(fields, scores)):
    num, den = accumulate(num, den, d, o, m == 0)
  return finish(num, den), den
