"""float64 restatements of the input-gradient kernels (include/geeco_hip.h: geeco_conv1_dgrad, geeco_pack_pixels_bwd,
geeco_dynimg_bwd), shared by tests/test_input_grad_cpu.py and tests/test_input_grad_gpu.py."""
import numpy as np
import torch

from oracle import geeco_oracle as O


def conv1_dgrad_ref(dz1, w1):
  """dx[f][y][x][ci] = sum_{ky,kx,co} dz1[f][y+1-ky][x+1-kx][co] w1[ky][kx][ci][co]: dz1 [F][H][W][Co], w1 [3][3][Cin][Co] ->
  [F][H][W][Cin], float64 (explicit shifted sums; no autograd)."""
  dz1, w1 = np.asarray(dz1, np.float64), np.asarray(w1, np.float64)
  F, H, W, _ = dz1.shape
  pad = np.zeros((F, H + 2, W + 2, dz1.shape[3]))
  pad[:, 1:H + 1, 1:W + 1] = dz1
  dx = np.zeros((F, H, W, w1.shape[2]))
  for ky in range(3):
    for kx in range(3):
      # dz1[y + 1 - ky][x + 1 - kx] = pad[y + 2 - ky][x + 2 - kx]
      dx += np.einsum('fyxo,io->fyxi', pad[:, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W], w1[ky, kx])
  return dx


def pack_bwd_ref(d_dst, C1, d_src=None, C2=0, d_src2=None):
  """The adjoint of geeco_pack_pixels in the arrays' own dtype: d_dst [..., Cpad] -> (d_src [..., C1], d_src2 [..., C2] or None);
  ``d_src`` / ``d_src2`` given: added to (one addition per element)."""
  d_dst = np.asarray(d_dst)
  a = d_dst[..., :C1] if d_src is None else np.asarray(d_src) + d_dst[..., :C1]
  b = None
  if C2:
    b = d_dst[..., C1:C1 + C2] if d_src2 is None else np.asarray(d_src2) + d_dst[..., C1:C1 + C2]
  return a, b


def dynimg_bwd_ref(g, frames, alpha=None):
  """The adjoint of the normalised dynamic image, float64, TF 1.15's tie rule (reduce_min / reduce_max share their gradient evenly
  among equal extrema): g [N][...] (gradient of out), frames [N][K][...] -> d_frames [N][K][...].
    D = sum_t alpha_t X_t, r = max - min + 1e-6, out = (D - min) / r,
    dD_i = g_i / r + [D_i == min] (sum_j g_j (out_j - 1) / r) / n_min - [D_i == max] (sum_j g_j out_j / r) / n_max."""
  g, frames = np.asarray(g, np.float64), np.asarray(frames, np.float64)
  N, K = frames.shape[:2]
  alpha = np.asarray(O.dynimg_alpha(K) if alpha is None else alpha, np.float64)
  out = np.zeros_like(frames)
  for n in range(N):
    D = np.tensordot(alpha, frames[n], axes=(0, 0))
    mn, mx = D.min(), D.max()
    r = mx - mn + 1e-6
    o = (D - mn) / r
    is_min, is_max = D == mn, D == mx
    dD = g[n] / r + is_min * ((g[n] * (o - 1.0)).sum() / r) / is_min.sum() - is_max * ((g[n] * o).sum() / r) / is_max.sum()
    out[n] = alpha.reshape((K,) + (1,) * D.ndim) * dD
  return out


def dynimg_autograd(g, frames):
  """The same through autograd of the oracle's ``dynimg`` (float64): equal to ``dynimg_bwd_ref`` wherever no two elements tie for
  an extremum -- torch's ``min(dim)`` sends the whole term to ONE index."""
  x = torch.tensor(np.asarray(frames, np.float64), requires_grad=True)
  O.dynimg(x).backward(torch.tensor(np.asarray(g, np.float64)))
  return x.grad.numpy()


def plant_extrema(frames, seed=0, margin=0.25):
  """In place: per sample one pixel value raised in every frame with a positive coefficient (and lowered where it is negative), one
  the other way round, so that the sample's D has a unique maximum and minimum with a wide margin (inputs in [0, 1])."""
  N, K = frames.shape[:2]
  alpha = O.dynimg_alpha(K).astype(np.float64)
  r = np.random.default_rng(seed)
  flat = frames.reshape(N, K, -1)
  for n in range(N):
    i, j = r.choice(flat.shape[2], 2, replace=False)
    for t in range(K):
      up = alpha[t] > 0
      flat[n, t, i] = 1.0 + margin if up else -margin
      flat[n, t, j] = -margin if up else 1.0 + margin
  return frames


def extrema_margin(frames):
  """min over samples of (D_max - second largest, second smallest - D_min), float64."""
  frames = np.asarray(frames, np.float64)
  N, K = frames.shape[:2]
  alpha = O.dynimg_alpha(K).astype(np.float64)
  worst = np.inf
  for n in range(N):
    D = np.sort(np.tensordot(alpha, frames[n], axes=(0, 0)).reshape(-1))
    worst = min(worst, D[-1] - D[-2], D[1] - D[0])
  return float(worst)
