"""numpy restatement of the attribution kernels (include/geeco_hip.h: geeco_attr_path_point, geeco_attr_accumulate,
geeco_attr_finish).  Float32 operation by float32 operation, so everything but the noise term is the device's result to the bit;
the noise comes from tests/_augment_scene_ref.py's Philox4x32-10 / Box-Muller in float64."""
import numpy as np

from _augment_scene_ref import normals_of_words, philox4x32_10

F = np.float32
SLOTS = 1024                       # slots of the sample sum
IMAGE_KEYS = ('rgb', 'target_rgb', 'depth', 'target_depth')


def counters(step, n):
  """uint64 [ceil(n / 4)][4]: the Philox counter of each group of four elements, (low word of i / 4, high word of i / 4, step, 0)."""
  g = np.arange(-(-n // 4), dtype=np.uint64)
  ctr = np.zeros((g.size, 4), np.uint64)
  ctr[:, 0], ctr[:, 1], ctr[:, 2] = g & np.uint64(0xFFFFFFFF), g >> np.uint64(32), step
  return ctr


def key_words(key):
  """The 64-bit key as Philox's two key words (low, high)."""
  return np.array([key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF], np.uint64)


def input_key(seed, name):
  """The key ``attributions(seed=)`` gives the path points of image input ``name``: 4 * seed + its index in IMAGE_KEYS."""
  return (4 * int(seed) + IMAGE_KEYS.index(name)) & ((1 << 64) - 1)


def noise(key, step, n):
  """float64 [n]: z(key, step, i) = normal i % 4 of the counter of group i // 4."""
  return normals_of_words(philox4x32_10(counters(step, n), key_words(key))).reshape(-1)[:n]


def baseline_of(baseline, n):
  """The baseline as a flat float32 [n]: None = zeros, else its elements repeated with its own length as the period."""
  if baseline is None:
    return np.zeros(n, F)
  b = np.asarray(baseline, F).reshape(-1)
  assert n % b.size == 0
  return np.tile(b, n // b.size)


def path_point(x, baseline, alpha, sigma=0.0, key=0, step=0):
  """b + alpha * (x - b) [+ sigma * z], each operation rounded to float32.  sigma == 0: bitwise the device's; sigma > 0: the
  noise term is float64's, rounded once (the device forms z in float32), so the result is the device's within the generator's
  tolerance."""
  x = np.asarray(x, F)
  xf = x.reshape(-1)
  b = baseline_of(baseline, xf.size)
  out = b + F(alpha) * (xf - b)
  assert out.dtype == F
  if sigma:
    out = (out.astype(np.float64) + np.float64(F(sigma)) * noise(key, step, xf.size)).astype(F)
  return out.reshape(x.shape)


def accumulate(acc, g, weight, overwrite):
  g = np.asarray(g, F)
  start = np.zeros_like(g) if overwrite else np.asarray(acc, F)
  out = start + F(weight) * g
  assert out.dtype == F
  return out


def sample_sum(attr_sample):
  """The fixed order: groups of four elements, group q in slot q % 1024, slots add their groups ascending and a group's elements
  ascending from +0, the slots folded by halves."""
  a = np.asarray(attr_sample, F).reshape(-1)
  pad = (-a.size) % (4 * SLOTS)
  rows = np.concatenate([a, np.zeros(pad, F)]).reshape(-1, SLOTS, 4)      # (the padding adds +0: no bit changes)
  s = np.zeros(SLOTS, F)
  for r in rows:
    for j in range(4):
      s = s + r[:, j]
  half = SLOTS // 2
  while half:
    s = s[:half] + s[half:2 * half]
    half //= 2
  assert s.dtype == F
  return s[0]


def finish(acc, x, baseline, multiply_by_input):
  """acc / x [N][frames][HW][C] -> (attr, saliency [N][frames][HW], sample_sum [N])."""
  acc = np.asarray(acc, F)
  if multiply_by_input:
    b = baseline_of(baseline, acc.size).reshape(acc.shape)
    attr = (np.asarray(x, F) - b) * acc
  else:
    attr = acc.copy()
  assert attr.dtype == F
  return attr, np.abs(attr).max(axis=-1), np.array([sample_sum(a) for a in attr], F)
