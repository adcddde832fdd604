"""Host restatements for the dynamic-image replay, in numpy: the image stage (current frame, pair image, buffer image per
window, from the window index rule), the same stage from a literal simulation of the reference predictor's frame buffer, and the
[feat | jnt | tgt] window states.  Shared by test_replay_dynimg_cpu.py and test_replay_dynimg_gpu.py."""
import numpy as np

import _replay_ref as R


def alpha(K):
  """graph.py:17-28 of the reference: float32 harmonic numbers summed in ascending order (csrc/dynimg.hip: geeco_dynimg_alpha)."""
  def H(t):
    h = np.float32(0)
    for i in range(1, t + 1):
      h = np.float32(h + np.float32(1) / np.float32(i))
    return h
  HT = H(K)
  return np.asarray([np.float32(2 * (K - t + 1)) - np.float32(K + 1) * np.float32(HT - H(t - 1)) for t in range(1, K + 1)], np.float32)


def dynimg(stack, dtype=np.float32):
  """stack [K][HW][3] -> the normalised dynamic image [HW][3]: sum_k alpha_k X_k with k ascending, (D - min) / (max - min + 1e-6)."""
  a = alpha(stack.shape[0]).astype(dtype)
  d = np.zeros(stack.shape[1:], dtype)
  for k in range(stack.shape[0]):
    d = d + a[k] * stack[k].astype(dtype)
  mn, mx = d.min(), d.max()
  return (d - mn) / (mx - mn + dtype(1e-6))


def pad4(img):
  """[..][3] -> [..][4] with a zero fourth channel."""
  return np.concatenate([img, np.zeros(img.shape[:-1] + (1,), img.dtype)], axis=-1)


def images_ref(frames, goal, K, t0, t1, buf=True, dtype=np.float32):
  """The model of geeco_replay_images: frames [T][HW][3] in [0, 1], goal [HW][3] -> (cur, buf, diff), each [t1 - t0][HW][4]; buf is None
  with ``buf=False``.  Window t shows the frames max(0, t - K + 1 + k), k = 0 .. K - 1."""
  idx = R.window_index(frames.shape[0], K)
  cur = np.stack([pad4(frames[t].astype(dtype)) for t in range(t0, t1)])
  diff = np.stack([pad4(dynimg(np.stack([frames[t], goal]), dtype)) for t in range(t0, t1)])
  b = np.stack([pad4(dynimg(frames[idx[t]], dtype)) for t in range(t0, t1)]) if buf else None
  return cur, b, diff


def images_by_buffer_simulation(frames, goal, K, buf=True, dtype=np.float32):
  """The same images from a literal simulation of the reference predictor (predictor.py:192-200, :144-146): reset, then one push per
  frame -- the first frame after a reset fills the whole buffer, every later one drops the oldest entry and is appended -- and at every
  frame the model's inputs from the buffer as it stands: its last entry, dynimg([last entry, goal]) and dynimg(buffer)."""
  cur, bufs, diff, held, fresh = [], [], [], [], True
  for t in range(frames.shape[0]):
    if fresh:
      held, fresh = [frames[t]] * K, False
    else:
      held = held[1:] + [frames[t]]
    cur.append(pad4(held[-1].astype(dtype)))
    diff.append(pad4(dynimg(np.stack([held[-1], goal]), dtype)))
    if buf:
      bufs.append(pad4(dynimg(np.stack(held), dtype)))
  return np.stack(cur), (np.stack(bufs) if buf else None), np.stack(diff)


def states_pair_ref(feat, tgt, jnt, K, t0, t1):
  """float32 [K][t1 - t0][cells * (ch + J + ch_t)]: per cell [feat | jnt | tgt] of frame max(0, t - K + 1 + k), for feat [T][cells][ch],
  tgt [T][cells][ch_t], jnt [T][J]."""
  T, cells, ch = feat.shape
  ch_t, J = tgt.shape[2], jnt.shape[1]
  idx = R.window_index(T, K)[t0:t1]
  out = np.zeros((K, t1 - t0, cells, ch + J + ch_t), np.float32)
  for k in range(K):
    out[k, :, :, :ch] = feat[idx[:, k]]
    out[k, :, :, ch:ch + J] = jnt[idx[:, k]][:, None, :]
    out[k, :, :, ch + J:] = tgt[idx[:, k]]
  return out.reshape(K, t1 - t0, -1)
