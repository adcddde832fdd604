"""fp64 references, rounding bounds and seeded inputs for the small kernels every decoder and optimiser step runs
(tests/test_primitives_gpu.py holds the device side, tests/test_primitive_refs_cpu.py shows that the bounds reject wrong kernels).

Everything here is written from the mathematics (TF 1.15's LSTMCell / AdamOptimizer, the reference's three concatenations), not
from the kernels: numpy / torch in float64 on the float32 values the device is given.  A bound is an array with one entry per
output element: ``c * U * (sum of the magnitudes of the terms of that element)`` plus the propagated bounds of its inputs, with
U = 2**-24 (one round-to-nearest fp32 operation moves a value by at most U times its magnitude) and the count ``c`` written next
to each formula.  Nothing in a bound is taken from what a kernel returns.
"""
import math

import numpy as np
import torch

from oracle import geeco_oracle as O

U = 2.0 ** -24
# Library functions, in units of U relative to the result: expf is documented at 1 ulp and tanhf at 2 ulp (1 ulp <= 2 U); allowed
# here are 2 ulp and 4 ulp.  A float division that is not correctly rounded stays under 2.5 ulp: 5 U.
EXP_U, TANH_U, DIV_U = 4.0, 8.0, 5.0


# --------------------------------------------------------------------------------------------------------------------------
# comparison
# --------------------------------------------------------------------------------------------------------------------------
def _f64(a):
  return a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)


def within(got, ref, bound):
  """True when every element of ``got`` is finite and within ``bound`` (an array, or a scalar) of ``ref``."""
  got, ref = _f64(got), _f64(ref)
  bound = np.broadcast_to(np.asarray(bound, np.float64), ref.shape)
  return got.shape == ref.shape and bool(np.all(np.abs(got - ref) <= bound))      # a NaN compares false


def assert_within(got, ref, bound, what=''):
  """_close of tests/test_kernels_gpu.py with a bound per element: reports the element that misses its bound by the largest factor."""
  got, ref = _f64(got), _f64(ref)
  assert got.shape == ref.shape, (what, got.shape, ref.shape)
  bound = np.broadcast_to(np.asarray(bound, np.float64), ref.shape)
  err = np.abs(got - ref)
  bad = ~(err <= bound)
  if bad.any():
    ratio = np.where(np.isnan(err), np.inf, err / np.maximum(bound, 1e-300))
    at = np.unravel_index(int(ratio.argmax()), ratio.shape) if ratio.ndim else ()
    raise AssertionError('%s: %d of %d elements out of bound; worst at %s: got %.9g, reference %.9g, err %.3e (bound %.3e)' % (
        what, int(bad.sum()), bad.size, at, got[at], ref[at], err[at], bound[at]))


def worst_ratio(got, ref, bound):
  """max err / bound: printed by the GPU tests before they assert, so a log shows how much of each bound is used."""
  got, ref = _f64(got), _f64(ref)
  bound = np.broadcast_to(np.asarray(bound, np.float64), ref.shape)
  return float(np.max(np.abs(got - ref) / np.maximum(bound, 1e-300))) if ref.size else 0.0


# --------------------------------------------------------------------------------------------------------------------------
# Adam (tf.train.AdamOptimizer [TF 1.15]: epsilon beside sqrt(v); the reference adds l2 * p to the gradient before the moments)
# --------------------------------------------------------------------------------------------------------------------------
def lr_t_ref(lr, b1, b2, t):
  """lr sqrt(1 - b2^t) / (1 - b1^t) in float64 on the float32 values of lr, b1, b2 an entry point with float arguments receives."""
  lr, b1, b2 = (float(np.float32(x)) for x in (lr, b1, b2))
  return lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)


def _adam_consts(b1, b2, eps, grad_scale, l2, const):
  c = lambda x: float(const(x))
  one = const(1)
  return c(b1), float(one - const(b1)), c(b2), float(one - const(b2)), c(eps), c(grad_scale), c(l2)


def adam_ref(p, g, m, v, lr_t, b1=0.9, b2=0.999, eps=1e-8, grad_scale=1.0, l2=0.0, const=np.float32):
  """One update in float64 on the given (float32) state: returns p', m', v' as float64 arrays.  ``const``: the precision the
  constants are carried in: float32 (what a float32 kernel carries: float32(b1), float32(1) - float32(b1), ...) or float64 (the
  mathematical constants, for the comparison with TF's own float64 numpy reference)."""
  b1, omb1, b2, omb2, eps, gs, l2 = _adam_consts(b1, b2, eps, grad_scale, l2, const)
  p, g, m, v = (_f64(x) for x in (p, g, m, v))
  gg = g * gs + l2 * p
  m2 = b1 * m + omb1 * gg
  v2 = b2 * v + omb2 * gg * gg
  p2 = p - float(lr_t) * m2 / (np.sqrt(v2) + eps)
  return p2, m2, v2


def adam_bounds(p, g, m, v, lr_t, b1=0.9, b2=0.999, eps=1e-8, grad_scale=1.0, l2=0.0):
  """Bounds of p', m', v' for one float32 update from the given state.
    G = |g gs| + |l2 p|: gg = g gs + l2 p is two products and a sum: |d gg| <= 2 U G with or without a fused multiply-add (with
         l2 != 0 the two terms can cancel: G is then much larger than |gg|);
    m' = b1 m + (1 - b1) gg: two products and a sum on top of gg's error            -> 4 U (|b1 m| + (1 - b1) G);
    v' = b2 v + (1 - b2) gg gg: the products and the sum, at most 3 and 4 roundings on the two (non-negative) terms, and
         d(gg^2) = 2 |gg| d gg                                                        -> U (3 b2 v + (1 - b2) (4 gg^2 + 4 G |gg|));
    step = lr_t m' / (sqrt(v') + eps): product, square root, sum, division (1 + 1 + 1 + 2.5 U)   -> 8 U |step|,
         m's bound through the same quotient, and v's through d step / d v' = -step / (2 sqrt(v') (sqrt(v') + eps));
    p' = p - step: one rounding                                                       -> U |p'|."""
  b1, omb1, b2, omb2, eps, gs, l2 = _adam_consts(b1, b2, eps, grad_scale, l2, np.float32)
  p, g, m, v = (_f64(x) for x in (p, g, m, v))
  p2, m2, v2 = adam_ref(p, g, m, v, lr_t, b1, b2, eps, gs, l2)
  gg = g * gs + l2 * p
  G = np.abs(g * gs) + np.abs(l2 * p)
  bm = 4 * U * (np.abs(b1 * m) + omb1 * G)
  bv = U * (3 * b2 * np.abs(v) + omb2 * (4 * gg * gg + 4 * G * np.abs(gg)))
  root = np.sqrt(v2)
  den = root + eps
  step = float(lr_t) * m2 / den
  bp = U * np.abs(p2) + 8 * U * np.abs(step) + float(lr_t) * bm / den + np.abs(step) * bv / (2 * np.maximum(root, 1e-300) * den)
  return bp, bm, bv


def adam_inputs(n, seed):
  """p, g, m0, v0 (float32) with what the update is sensitive to: gradients over six decades and both signs, m0 != 0, v0 >= 0 with
  a quarter of exact zeros and the rest over ten decades (where sqrt(v) + eps and sqrt(v + eps) differ by orders of magnitude)."""
  r = np.random.default_rng(seed)
  p = r.standard_normal(n).astype(np.float32)
  g = (np.sign(r.standard_normal(n)) * 10.0 ** r.uniform(-6, 0, n)).astype(np.float32)
  m = (0.01 * r.standard_normal(n)).astype(np.float32)
  m[m == 0] = 0.01
  v = np.where(r.uniform(size=n) < 0.25, 0.0, 10.0 ** r.uniform(-12, -2, n)).astype(np.float32)
  return p, g, m, v


# --------------------------------------------------------------------------------------------------------------------------
# LSTM gate math (tf.nn.rnn_cell.LSTMCell [TF 1.15]: gate order i, j, f, o; forget bias 1)
# --------------------------------------------------------------------------------------------------------------------------
def _sigmoid(x):
  return 1.0 / (1.0 + np.exp(-x))


def lstm_gates_ref(z, bias, c_prev=None, forget_bias=1.0):
  """z [N][4H] (pre-activations without bias), bias [4H], c_prev [N][H] or None (zero) -> c, h [N][H], gates [N][4H] =
  [sigmoid(i) | tanh(j) | sigmoid(f + 1) | sigmoid(o)], float64."""
  z, bias = _f64(z), _f64(bias)
  H = z.shape[1] // 4
  x = z + bias
  si, tj, sf, so = _sigmoid(x[:, :H]), np.tanh(x[:, H:2 * H]), _sigmoid(x[:, 2 * H:3 * H] + forget_bias), _sigmoid(x[:, 3 * H:])
  cp = np.zeros_like(si) if c_prev is None else _f64(c_prev)
  c = sf * cp + si * tj
  return c, so * np.tanh(c), np.concatenate([si, tj, sf, so], 1)


def lstm_gates_fwd_bounds(z, bias, c_prev=None):
  """Bounds of c, h, gates for a float32 evaluation.  With x = z + b rounded once (dx = U |x|; the forget gate adds 1 and rounds
  again):
    sigmoid(x) = 1 / (1 + expf(-x)): expf's allowance, the sum, the division, and dx through the slope s (1 - s)
                                                   -> s U (EXP_U + 1 + DIV_U) + s (1 - s) dx   (d ln s / d ln E = -(1 - s): |.| <= 1);
    tanhf(x)                                       -> TANH_U U |t| + (1 - t^2) dx;
    c = sf cp + si tj: two products and a sum      -> 2 U (|sf cp| + |si tj|) + the gates' bounds times their cofactors;
    h = so tanhf(c)                                -> U |h| + |tanh c| b_so + so (TANH_U U |tanh c| + (1 - tanh^2 c) b_c)."""
  z, bias = _f64(z), _f64(bias)
  H = z.shape[1] // 4
  x = z + bias
  dx = U * np.abs(x)
  dx[:, 2 * H:3 * H] += U * np.abs(x[:, 2 * H:3 * H] + 1.0)
  c, h, gates = lstm_gates_ref(z, bias, c_prev)
  si, tj, sf, so = (gates[:, k * H:(k + 1) * H] for k in range(4))
  sig_b = lambda s, d: s * U * (EXP_U + 1 + DIV_U) + s * (1 - s) * d
  bsi, bsf, bso = sig_b(si, dx[:, :H]), sig_b(sf, dx[:, 2 * H:3 * H]), sig_b(so, dx[:, 3 * H:])
  btj = TANH_U * U * np.abs(tj) + (1 - tj * tj) * dx[:, H:2 * H]
  cp = np.zeros_like(si) if c_prev is None else _f64(c_prev)
  bc = 2 * U * (np.abs(sf * cp) + np.abs(si * tj)) + np.abs(cp) * bsf + np.abs(tj) * bsi + si * btj
  tc = np.tanh(c)
  bh = U * np.abs(h) + np.abs(tc) * bso + so * (TANH_U * U * np.abs(tc) + (1 - tc * tc) * bc)
  return bc, bh, np.concatenate([bsi, btj, bsf, bso], 1)


def lstm_gates_bwd_ref(z, bias, c_prev=None, dh=None, dc=None, forget_bias=1.0):
  """Gradients of L = sum(h dh) + sum(c dc) by autograd through the oracle's lstm_cell in float64 (its [x | h] W is fed z through
  an identity kernel and an empty h): returns dz [N][4H] and dc_prev [N][H] (None without c_prev)."""
  zt = torch.tensor(_f64(z), dtype=torch.float64, requires_grad=True)
  N, H4 = zt.shape
  H = H4 // 4
  cp = torch.tensor(_f64(c_prev), dtype=torch.float64, requires_grad=True) if c_prev is not None else None
  c, h = O.lstm_cell(zt, cp if cp is not None else zt.new_zeros(N, H), zt.new_zeros(N, 0), torch.eye(H4, dtype=torch.float64),
                     torch.tensor(_f64(bias), dtype=torch.float64), forget_bias=forget_bias)
  L = zt.sum() * 0.0
  if dh is not None:
    L = L + (h * torch.tensor(_f64(dh), dtype=torch.float64)).sum()
  if dc is not None:
    L = L + (c * torch.tensor(_f64(dc), dtype=torch.float64)).sum()
  L.backward()
  return zt.grad.numpy(), (cp.grad.numpy() if cp is not None else None)


def lstm_gates_bwd_bounds(z, bias, c_prev=None, dh=None, dc=None):
  """Bounds of dz, dc_prev for a float32 backward that reads the float32 c and gates of a float32 forward (their bounds b_c,
  b_si, ... above) and the exact dh, dc.  tc = tanhf(c): b_tc = TANH_U U |tc| + (1 - tc^2) b_c;  1 - tc^2: 2 U + 2 |tc| b_tc;
    A = dh so (1 - tc^2): three roundings + the factors' bounds;  dct = dc + A: one more on |dc| + |A|;
    every dz block is a product of four factors (<= 4 roundings: 4 U |dz|) + each factor's bound times its cofactor, where
    1 - s carries b_s + U;  dc_prev = dct sf."""
  z = _f64(z)
  N, H = z.shape[0], z.shape[1] // 4
  c, h, gates = lstm_gates_ref(z, bias, c_prev)
  bc, _, bg = lstm_gates_fwd_bounds(z, bias, c_prev)
  si, tj, sf, so = (gates[:, k * H:(k + 1) * H] for k in range(4))
  bsi, btj, bsf, bso = (bg[:, k * H:(k + 1) * H] for k in range(4))
  cp = np.zeros((N, H)) if c_prev is None else _f64(c_prev)
  dhv = np.zeros((N, H)) if dh is None else _f64(dh)
  dcv = np.zeros((N, H)) if dc is None else _f64(dc)
  tc = np.tanh(c)
  btc = TANH_U * U * np.abs(tc) + (1 - tc * tc) * bc
  omt, bomt = 1 - tc * tc, 2 * U + 2 * np.abs(tc) * btc
  A = dhv * so * omt
  bA = np.abs(dhv) * (so * bomt + omt * bso) + 3 * U * np.abs(A)
  dct = dcv + A
  bdct = bA + U * (np.abs(dcv) + np.abs(A))
  a = np.abs
  dzi, dzj, dzf, dzo = dct * tj * si * (1 - si), dct * si * (1 - tj * tj), dct * cp * sf * (1 - sf), dhv * tc * so * (1 - so)
  bi = a(tj * si * (1 - si)) * bdct + a(dct * si * (1 - si)) * btj + a(dct * tj) * ((1 - si) * bsi + si * (bsi + U)) + 4 * U * a(dzi)
  bj = a(si * (1 - tj * tj)) * bdct + a(dct * (1 - tj * tj)) * bsi + a(dct * si) * (2 * a(tj) * btj + 2 * U) + 4 * U * a(dzj)
  bf = a(cp * sf * (1 - sf)) * bdct + a(dct * cp) * ((1 - sf) * bsf + sf * (bsf + U)) + 4 * U * a(dzf)
  bo = a(dhv) * (a(so * (1 - so)) * btc + a(tc) * ((1 - so) * bso + so * (bso + U))) + 4 * U * a(dzo)
  bdcp = sf * bdct + a(dct) * bsf + U * a(dct * sf)
  return np.concatenate([bi, bj, bf, bo], 1), bdcp


def gates_inputs(N, H, seed):
  """z, bias, c_prev, dh, dc (float32): a third of the pre-activations are scaled into saturation (|z| up to about 20)."""
  r = np.random.default_rng(seed)
  z = r.standard_normal((N, 4 * H)) * np.where(r.uniform(size=(N, 4 * H)) < 0.33, 7.0, 1.0)
  f32 = lambda x: x.astype(np.float32)
  return (f32(np.clip(z, -20, 20)), f32(0.5 * r.standard_normal(4 * H)), f32(r.standard_normal((N, H))),
          f32(r.standard_normal((N, H))), f32(r.standard_normal((N, H))))


# The three-step chain (gemm + gates forward, gates backward + gemm, as LSTMDecoder._forward_chain / backward) against autograd
# through three oracle cells.  Its bound is a stability argument, not a per-element count: with |x| <= 1, Wx in +-0.25 (D = 5),
# Wh in +-0.125 (H = 8: absolute row sums <= 1), |dh_T| <= 1, every value stays O(1) and one step of the forward or backward
# recurrence adds a local error of at most 32 U (the per-element bounds above at these magnitudes) while multiplying the incoming
# (dh, dc) error by at most 2 (|dz / dh_prev| <= sum |Wh| <= 1 through slopes <= 1, plus the c path's factor sf <= 1).  Three
# forward steps: 32 U (1 + 2 + 4); the backward reads all of them and accumulates over three steps again: 32 * 7 * 7 U < 2048 U.
LSTM_CHAIN_ATOL = 2048 * U


def lstm_chain_ref(x, Wx, Wh, bias, dh_last):
  """x [T][N][D], zero initial state, L = sum(h_T dh_last): float64 autograd through T oracle cells.  Returns dict with c, h
  (lists per step), dz (list: the gradient of every step's pre-activation), dh0 = dL/dh_0 and dc0 = the part of dL/dc_0 that
  arrives along the cell path (what the decoder's ``dh`` / ``dc`` buffers hold when its backward loop reaches step 0)."""
  T, N, D = x.shape
  H = Wh.shape[0]
  t64 = lambda a: torch.tensor(_f64(a), dtype=torch.float64)
  kernel = torch.cat([t64(Wx), t64(Wh)], 0)
  xs = t64(x)
  c, h = xs.new_zeros(N, H), xs.new_zeros(N, H)
  biases, cs, hs, c0_pass = [], [], [], None
  for t in range(T):
    b = t64(bias).expand(N, 4 * H).clone().requires_grad_()      # a per-sample bias: its gradient is dz_t
    biases.append(b)
    c, h = O.lstm_cell(xs[t], c, h, kernel, b)
    cs.append(c.detach().numpy()); hs.append(h.detach().numpy())
    if t == 0:
      h.retain_grad()
      h0 = h
      c = c * 1.0                                                  # the copy only step 1 reads: its gradient excludes h_0's path
      c.retain_grad()
      c0_pass = c
  (h * t64(dh_last)).sum().backward()
  return dict(c=cs, h=hs, dz=[b.grad.numpy() for b in biases], dh0=h0.grad.numpy() if T > 1 else None,
              dc0=c0_pass.grad.numpy() if T > 1 else None)


# --------------------------------------------------------------------------------------------------------------------------
# state concat (the reference's state_concatenation / representation_concatenation(_v2): [features... | joints] per 2 x 2 cell)
# --------------------------------------------------------------------------------------------------------------------------
def state_concat_ref(feats, jnt, jnt_pos, sub_from=None):
  """feats: list of [N][2][2][C_f] tensors, jnt [N][J] inserted before feature ``jnt_pos`` (== len(feats): last), feature 0
  replaced by sub_from - feats[0] when given -> [N][4 * Ctot], built with torch.cat as the oracle builds its three layouts."""
  N = feats[0].shape[0]
  parts = [sub_from - feats[0] if sub_from is not None else feats[0]] + list(feats[1:])
  J = jnt.shape[-1]
  st = jnt.reshape(N, 1, 1, J).expand(N, 2, 2, J)
  parts.insert(jnt_pos, st)
  return torch.cat(parts, dim=-1).reshape(N, -1)


def state_concat_bwd_ref(pre, jnt, jnt_pos, dstate, scale=1.0, base=None):
  """Feature gradients through relu: feats = relu(pre) (pre: list of float64 [N][2][2][C_f] with zeros and negatives), state =
  state_concat_ref(feats, jnt, jnt_pos), L = sum(state dstate).  Returns per feature base_f + scale dL/dpre_f (base None: zero).
  The joint columns of dstate reach no feature."""
  leaves = [p.clone().double().requires_grad_() for p in pre]
  state = state_concat_ref([torch.relu(p) for p in leaves], jnt.double(), jnt_pos)
  (state * dstate.double()).sum().backward()
  return [(0.0 if base is None else base[f].double()) + scale * leaves[f].grad for f in range(len(pre))]


# --------------------------------------------------------------------------------------------------------------------------
# reductions and plumbing
# --------------------------------------------------------------------------------------------------------------------------
def colsum_ref(a, M, N, base=None):
  """a [rows >= M][lda >= N] -> sum over the first M rows of the first N columns (+ base), float64."""
  s = _f64(a)[:M, :N].sum(0)
  return s if base is None else s + _f64(base)[:N]


def colsum_bound(a, M, N, base=None):
  """A running float32 sum of M terms (+ the accumulate): at most M roundings, each within U of the running magnitude."""
  s = np.abs(_f64(a)[:M, :N]).sum(0)
  return (M + 1) * U * (s if base is None else s + np.abs(_f64(base)[:N]))


def sumsq_ref(p):
  p = _f64(p)
  return float((p * p).sum())


def sumsq_blocks(n):
  return min(1024, -(-n // 2048))


def sumsq_rel_bound(n):
  """Per thread ceil(n / (blocks 256)) squares in a running sum, 6 + 2 levels of the tree inside a block, then ``blocks`` atomic
  additions in any order; all terms >= 0, so the bound is relative."""
  blocks = sumsq_blocks(n)
  return (-(-n // (blocks * 256)) + 8 + blocks) * U


def gemm_ref(A, B, ta, tb, M, N, K, base=None):
  """op(A) op(B) in float64 from the leading M x K / K x N parts of padded row-major operands (+ base[:M, :N])."""
  A, B = _f64(A), _f64(B)
  a = A[:K, :M].T if ta else A[:M, :K]
  b = B[:N, :K].T if tb else B[:K, :N]
  c = a @ b
  return c if base is None else c + _f64(base)[:M, :N]


def gemm_bound(ref, K):
  """The bound of tests/test_kernels_gpu.py::test_gemm (standard-normal operands)."""
  return 1e-5 * np.abs(ref) + 2e-5 * math.sqrt(K)


def pad_mid_ref(src, Bd):
  A, B, C = src.shape
  out = np.zeros((A, Bd, C), src.dtype)
  out[:, :B] = src
  return out


def transpose_taps_ref(w):
  """[G][3][3][Cin][Cout] -> [G][3][3][Cout][Cin]."""
  return np.ascontiguousarray(np.swapaxes(w, -1, -2))


def pack_pixels_ref(src, src2, Cpad):
  """src [N][HW][C1] (+ src2 [N][HW][C2]) -> [N][HW][Cpad], zero-padded."""
  N, HW, C1 = src.shape
  out = np.zeros((N, HW, Cpad), np.float32)
  out[..., :C1] = src
  if src2 is not None:
    out[..., C1:C1 + src2.shape[2]] = src2
  return out


def gather_windows_ref(src, starts, K, divisor):
  """src [frames][E] (uint8 or float32) -> [N][K][E] float32: float32(src) / float32(divisor) (a copy at divisor 1)."""
  idx = np.asarray(starts)[:, None] + np.arange(K)[None, :]
  w = src[idx].astype(np.float32)
  return w / np.float32(divisor) if divisor != 1 else w
