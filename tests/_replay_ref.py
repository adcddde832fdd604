"""Host models of episode replay, in numpy: the window index rule, a literal simulation of the reference predictor's
frame buffer, the three state layouts and the error reduction in float64.  Shared by test_replay_cpu.py and test_replay_gpu.py."""
import numpy as np


def window_index(T, K):
  """[T][K]: slot k (oldest first) of the window at frame t shows frame max(0, t - K + 1 + k)."""
  return np.asarray([[max(0, t - K + 1 + k) for k in range(K)] for t in range(T)], np.int64).reshape(T, K)


def deque_simulation(T, K):
  """What the reference predictor's buffer holds after reset() at frame 0 and a push per frame (predictor.py:192-200: the first
  frame after a reset fills the whole buffer, every later one drops the oldest entry and is appended), as frame numbers [T][K]."""
  out, buf, fresh = [], [], True
  for t in range(T):
    if fresh:
      buf, fresh = [t] * K, False
    else:
      buf = buf[1:] + [t]
    out.append(list(buf))
  return np.asarray(out, np.int64).reshape(T, K)


def state_width(mode, cells, ch, J):
  return cells * (ch + J + (ch if mode == 'constant' else 0))


def states_ref(feat, jnt, tgt, mode, K, t0, t1):
  """float32 [K][t1 - t0][cells * Ctot]: per cell PLAIN [feat | jnt], CONSTANT [feat | jnt | tgt], RESIDUAL [tgt - feat | jnt] (one
  float32 subtraction), for the windows t0 .. t1 - 1 of the episode feat [T][cells][ch], jnt [T][J], tgt [cells][ch]."""
  T, cells, ch = feat.shape
  J = jnt.shape[1]
  idx = window_index(T, K)[t0:t1]                       # [n][K]
  n = t1 - t0
  Ctot = state_width(mode, 1, ch, J)
  out = np.zeros((K, n, cells, Ctot), np.float32)
  for k in range(K):
    f = feat[idx[:, k]]                                 # [n][cells][ch]
    out[k, :, :, :ch] = (tgt[None] - f) if mode == 'residual' else f
    out[k, :, :, ch:ch + J] = jnt[idx[:, k]][:, None, :]
    if mode == 'constant':
      out[k, :, :, ch + J:] = tgt[None]
  return out.reshape(K, n, cells * Ctot)


def errors_ref(preds, labels, heads):
  """float64 (frame [T][heads], episode [heads]) of float32 preds / labels [T][P]; heads = (first column, columns, kind): kind 0 the
  mean over the columns of the squared difference, kind 1 the hit of np.argmax (first maximum) on the class labels[t][first column],
  NaN where a logit is NaN."""
  p, l = preds.astype(np.float64), labels.astype(np.float64)
  T = p.shape[0]
  frame = np.zeros((T, len(heads)), np.float64)
  for h, (off, size, kind) in enumerate(heads):
    if kind == 0:
      frame[:, h] = ((p[:, off:off + size] - l[:, off:off + size]) ** 2).sum(axis=1) / size
    else:
      logits = p[:, off:off + size]
      bad = np.isnan(logits).any(axis=1)
      hit = (np.argmax(np.where(np.isnan(logits), -np.inf, logits), axis=1) == l[:, off]).astype(np.float64)
      frame[:, h] = np.where(bad, np.nan, hit)
  return frame, frame.mean(axis=0)


def episode_sum_order(values, threads=256):
  """The documented order of geeco_replay_errors' episode mean, in float32: thread i adds the frames i, i + threads, .. ascending, the
  partial sums are folded by halves, the result is divided by T."""
  v = np.asarray(values, np.float32)
  part = np.zeros(threads, np.float32)
  for i in range(threads):
    s = np.float32(0)
    for x in v[i::threads]:
      s = np.float32(s + x)
    part[i] = s
  half = threads // 2
  while half:
    part[:half] = part[:half] + part[half:2 * half]
    half //= 2
  return np.float32(part[0] / np.float32(len(v)))
