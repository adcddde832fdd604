"""Cases, inputs, float64 reference and comparison for the decoder tail: fc1, the heads, the losses and their gradients
(heads_loss_kernel<SHAPED>, heads_sample_kernel<FUSE, G, SHAPED>, the finish roles of heads_finish_kernel / lstm_step_bwd_heads_kernel).
tests/test_decoder_tail_variants_gpu.py launches every case; tests/test_tail_refs_cpu.py shows without a GPU that the inputs have the
properties claimed here and that ``tail_compare`` rejects wrong kernels.  No GPU code; nothing is imported from geeco_amd.

Lattice inputs (every case whose ``h`` is an input): h = k / 1024, fc1/kernel = j / 8 (|j| <= 2), fc1/bias an odd multiple of 2**-14 =
half the step of the products, so every pre-activation is an odd multiple of 2**-14: never 0, and at least LATTICE_MARGIN from it.
The head kernels are j / 8 (three quarters of them 0) and the head biases odd multiples of 2**-18.  Every partial sum of fc1 and of
the heads is a multiple of the lattice step below 2**24 steps: float32 in ANY order gives the float64 value, so the predictions are
compared by equality, the ReLU mask is the same in both precisions, and a product path of reduced precision shows (h takes up to
eleven bits: bfloat16 holds eight).
Regression targets are multiples of 1 / 8 placed at the prediction's own lattice point plus {0, 1, 1 / 8, -1}: |pred - target| is
below 1 / 4 or above 7 / 8, the Huber delta 0.3 is off the lattice and far from both, so both branches occur and are decided alike.

Fused cases (the one-step decoder): h is the cell's output, |h| < 1.  fc1/kernel = j / 64 and every fc1 bias is
+-(FUSED_MARGIN + sum |column of fc1/kernel|): the sign of a pre-activation is that of its bias, by FUSED_MARGIN at least.  The
reference chain is linked at what the device returns: z against x Wx, (c, h, gates) against the gate math of the device's z, the
tail against the tail of the device's h, dz against the gate backward of the device's z and the reference's d(h).

Bound of one output element (``tail_math``): the standard forward bound of a float32 sum of k terms in any order,
gamma_k * sum |terms| with gamma_k = k U / (1 - k U), U = 2**-24 and k = the number of terms (a product and its addition: a
k-term dot product plus a bias is k + 1), plus the bounds of its operands times the magnitudes of their cofactors.  expf, logf and
the division take the allowances _primitive_refs gives the gate math (logf, documented at 1 ulp like expf, takes expf's).  On top,
no element is allowed more than tests/test_kernels_gpu.py::test_heads_loss allows it (``legacy_cap``).
"""
import math
from collections import namedtuple

import numpy as np

import _primitive_refs as P

U = P.U
EXP_U, DIV_U = P.EXP_U, P.DIV_U
LOG_U = P.EXP_U
MSE, XENT, HUBER = 0, 1, 2
DELTA = 0.3                       # Huber delta: off the lattice (the kernels hold float32(0.3))
SMOOTH = 0.1
CLASS_W = [1.0, 0.25, 2.0]
LATTICE_MARGIN = 2.0 ** -14
FUSED_MARGIN = 2.0 ** -6
HF_NC = 32                        # samples per chunk of the finish roles (decoder_step_bwd.hip)


def gamma(k):
  return k * U / (1.0 - k * U)


def gemm_plan(M, N, K):
  """split-K plan of the gate product as decoder_gemm.hip's gemm_plan states it -> S."""
  cdiv = lambda a, b: -(-a // b)
  s = max(1, 512 // (cdiv(M, 64) * cdiv(N, 64)))
  s = min(s, max(1, K // 64))
  k = cdiv(cdiv(K, s), 16) * 16
  return cdiv(K, k)


# ------------------------------------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------------------------------------
CART = [(3, MSE, 1.0), (3, XENT, 1.0), (3, MSE, 0.5), (3, MSE, 0.5)]                       # graph.py:233-239
VEL = [(7, MSE, 1.0), (3, MSE, 1.0), (2, MSE, 1.0), (3, MSE, 1.0), (3, MSE, 1.0)]          # graph.py:240-249
CART_S = [(3, HUBER, 1.0), (3, XENT, 1.0), (3, MSE, 0.5), (3, HUBER, 0.5)]
VEL_S = [(7, HUBER, 1.0), (3, MSE, 1.0), (2, HUBER, 1.0), (3, MSE, 1.0), (3, MSE, 1.0)]
WIDE = [(16, MSE, 1.0), (3, XENT, 1.0), (7, MSE, 0.5), (3, MSE, 0.5), (3, MSE, 0.5)]       # OT = 32, a head of 16
WIDE_S = [(16, HUBER, 1.0), (3, XENT, 1.0), (7, MSE, 0.5), (3, HUBER, 0.5), (3, MSE, 0.5)]
ONE = [(1, MSE, 1.0)]                                                                      # OT = 1
THIRD = [(3, MSE, 1.0), (2, MSE, 1.0), (3, XENT, 1.0), (3, MSE, 0.5)]                      # the kind-1 head is the third
TWO_CLS = [(3, XENT, 1.0), (3, MSE, 1.0), (3, XENT, 0.5)]                                  # two kind-1 heads, no class table

FULL = dict(sw=True, cw=True, smooth=SMOOTH)          # sample weights (some zero), class table, label smoothing
SW = dict(sw=True, cw=False, smooth=0.0)
SW_SMOOTH = dict(sw=True, cw=False, smooth=SMOOTH)

Case = namedtuple('Case', 'index id entry N H F heads shaping backward deferred D S layout sw_stride names marks')


def per_sample(H, F, heads):
  return 1 <= H <= 128 and F in (64, 128) and sum(sz for sz, _, _ in heads) <= 32


def _names(entry, H, F, heads, shaped, backward, deferred):
  tag = ', shaped>' if shaped else '>'
  if entry == 'step_heads':
    return (['gemm_f32_kernel', 'heads_sample_kernel<true' + tag] + ([] if deferred else ['heads_finish_kernel'])
            + (['lstm_step_bwd_heads_kernel'] if deferred else []))
  if per_sample(H, F, heads):
    return ['heads_sample_kernel<false' + tag, 'heads_finish_kernel']
  return ['heads_loss_kernel<shaped>' if shaped else 'heads_loss_kernel']


def _build():
  cases = []

  def add(entry, N, H, F, heads, shaping=None, backward=1, deferred=False, D=0, layout='dense', sw_stride=1, marks=()):
    S = gemm_plan(N, 4 * H, D) if entry == 'step_heads' else 0
    text = '%s-N%d-H%d-F%d-OT%d%s-%s%s%s%s%s' % (
        entry, N, H, F, sum(sz for sz, _, _ in heads), 'k' + ''.join(str(k) for _, k, _ in heads),
        'shaped' if shaping else 'plain', '' if backward else '-fwd', '-deferred' if deferred else '', '-D%d' % D if D else '',
        ('-model' if layout == 'model' else '') + ('-sw%d' % sw_stride if sw_stride != 1 else ''))
    cases.append(Case(len(cases), text, entry, N, H, F, heads, shaping, backward, deferred, D, S, layout, sw_stride,
                      _names(entry, H, F, heads, shaping is not None, backward, deferred), tuple(marks)))

  # ---- per-sample kernel + heads_finish_kernel: Hfc x H, unshaped and shaped, both tables, N over the chunk edges ----
  Ns = [1, 31, 32, 33, 65]
  k = 0
  for F in (64, 128):
    for H in (1, 100, 127, 128):
      for shaped in (False, True):
        cart = (k // 2) % 2 == 0
        heads = (CART_S if cart else VEL_S) if shaped else (CART if cart else VEL)
        add('heads', Ns[k % 5], H, F, heads, (FULL if cart else SW) if shaped else None, layout='model' if k % 3 == 0 else 'dense',
            sw_stride=3 if (shaped and k % 4 == 1) else 1,
            marks=(('drop_last_sample',) if k == 1 else ()) + (('mean_over_n',) if k == 3 else ())
            + (('dense_stride',) if k == 6 else ()) + (('swap_offsets', 'mask_da1', 'bf16') if k == 2 else ()))
        k += 1
  add('heads', 33, 100, 64, CART, backward=0)
  add('heads', 31, 128, 128, VEL_S, SW, backward=0, sw_stride=3)
  add('heads', 65, 127, 128, VEL, backward=0, layout='model')
  add('heads', 1, 1, 64, CART_S, FULL, backward=0, layout='model')
  add('heads', 65, 100, 128, CART_S, FULL, layout='model', sw_stride=3, marks=('drop_chunk_row', 'dense_stride'))
  # ---- a second trip of every N loop: 1025 and 4096 workgroups of the per-sample kernel, long chains of 32-sample chunks ----
  add('heads', 1025, 8, 64, CART_S, FULL)
  add('heads', 4096, 8, 64, CART_S, FULL, layout='model', sw_stride=3)
  # ---- width edges on the per-sample kernel ----
  add('heads', 33, 100, 64, WIDE)
  add('heads', 7, 128, 128, WIDE_S, FULL, layout='model')
  add('heads', 33, 100, 128, ONE)
  add('heads', 5, 128, 64, ONE, SW)
  add('heads', 33, 100, 64, THIRD, layout='model')
  add('heads', 7, 128, 128, THIRD, FULL)
  add('heads', 33, 128, 64, TWO_CLS)
  add('heads', 9, 100, 128, TWO_CLS, SW_SMOOTH, sw_stride=3)
  # ---- single-workgroup kernel: H = 129 (the smallest the per-sample kernel declines), Hfc = 96, N past 1024 ----
  add('heads', 7, 129, 128, CART, layout='model')
  add('heads', 33, 129, 128, CART_S, FULL, sw_stride=3, marks=('mean_over_n',))
  add('heads', 9, 64, 96, VEL)
  add('heads', 6, 64, 96, CART_S, FULL, layout='model')
  add('heads', 5, 64, 96, CART, backward=0)
  add('heads', 17, 40, 96, WIDE_S, FULL)
  add('heads', 3, 40, 96, ONE)
  add('heads', 1025, 16, 32, CART)
  add('heads', 1025, 16, 32, CART_S, FULL, sw_stride=3)
  add('heads', 4096, 8, 32, CART_S, FULL, layout='model')
  # ---- fused one-step decoder: <true, G, SHAPED> x H in {128, 100} x deferred; D for S = 1, 1 < S < 16, S > 16 with a remainder ----
  add('step_heads', 33, 128, 128, CART, deferred=True, D=1152, marks=('drop_slab', 'bf16'))
  add('step_heads', 5, 100, 128, CART_S, FULL, D=320, layout='model', marks=('drop_slab',))
  add('step_heads', 7, 100, 64, VEL, deferred=True, D=40)
  add('step_heads', 32, 128, 64, VEL_S, SW, deferred=True, D=1152, sw_stride=3)
  add('step_heads', 5, 128, 64, CART, backward=0, D=320)
  add('step_heads', 9, 100, 128, CART_S, FULL, backward=0, D=40)
  add('step_heads', 33, 100, 64, CART_S, FULL, D=1152, layout='model')
  add('step_heads', 1, 128, 128, CART, D=40)
  add('step_heads', 65, 100, 64, WIDE, deferred=True, D=320)
  return cases


CASES = _build()


# ------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------
def _cell(x, wx, bias):
  """The zero-state LSTM step in float64 -> z, h."""
  z = np.asarray(x, np.float64) @ np.asarray(wx, np.float64)
  _, h, _ = P.lstm_gates_ref(z, bias)
  return z, h


def tail_inputs(c):
  """-> dict of float32 arrays: h (heads) or x, wx, bias (step_heads); w1, b1, hw[], hb[], tg[] ([N][size], kind 1: [N][1]);
  sw [N] / cw [3] or None."""
  r = np.random.default_rng(7000 + c.index)
  f32 = lambda a: np.ascontiguousarray(a, np.float32)
  N, H, F = c.N, c.H, c.F
  inp = {}
  if c.entry == 'step_heads':
    inp['x'] = f32(r.standard_normal((N, c.D)))
    inp['wx'] = f32(r.standard_normal((c.D, 4 * H)) / math.sqrt(c.D))
    inp['bias'] = f32(0.5 * r.standard_normal(4 * H))
    w1 = r.integers(-2, 3, (H, F)) / 64.0
    sign = np.where(r.permutation(F) % 2 == 0, 1.0, -1.0)
    b1 = sign * (FUSED_MARGIN + np.abs(w1).sum(0))
    _, h = _cell(inp['x'], inp['wx'], inp['bias'])
  else:
    h = r.integers(-1024, 1025, (N, H)) / 1024.0
    inp['h'] = f32(h)
    w1 = r.integers(-2, 3, (H, F)) / 8.0
    b1 = (2 * r.integers(-4096, 4096, F) + 1) / 16384.0
  inp['w1'], inp['b1'] = f32(w1), f32(b1)
  inp['hw'] = [f32(r.integers(-2, 3, (F, sz)) * (r.random((F, sz)) < 0.25) / 8.0) for sz, _, _ in c.heads]
  inp['hb'] = [f32((2 * r.integers(-65536, 65536, sz) + 1) / 262144.0) for sz, _, _ in c.heads]
  a1 = np.maximum(h @ inp['w1'].astype(np.float64) + inp['b1'].astype(np.float64), 0.0)
  tg = []
  for i, (sz, kind, _) in enumerate(c.heads):
    if kind == XENT:      # label = rint(target) + 1 = (n + i) mod size: every label, none out of range
      tg.append(f32(((np.arange(N) + i) % sz - 1).reshape(N, 1)))
    else:
      pred = a1 @ inp['hw'][i].astype(np.float64) + inp['hb'][i].astype(np.float64)
      offs = np.array([0.0, 1.0, 0.125, -1.0])[np.arange(N * sz).reshape(N, sz) % 4]
      tg.append(f32(np.rint(pred * 8.0) / 8.0 + offs))
  inp['tg'] = tg
  inp['sw'] = inp['cw'] = None
  if c.shaping:
    if c.shaping['sw']:      # weights from {0, 0.5, 1, 2}; where N > 1 the first is zero and the last is not
      sw = np.array([0.0, 0.5, 1.0, 2.0])[r.integers(0, 4, N)]
      if N == 1:
        sw[0] = 2.0
      else:
        sw[0], sw[N - 1] = 0.0, 0.5
      inp['sw'] = f32(sw)
    if c.shaping['cw']:
      inp['cw'] = f32(CLASS_W)
  return inp


def target_layout(c, inp, i):
  """-> (flat float32 buffer, element offset of sample 0's first column, row stride).  'dense': stride = the columns read.  'model'
  (graph.py:361-366): the first head reads size columns of rows one wider ((cmd, 4)), a kind-1 head the last column of rows of four
  (cmd[:, 3:]: a base 12 bytes into the row), the others the first columns of rows of K * 7 = 14 ((ee_last, K * 7)).  Every
  unread column is NaN, and so are eight floats behind the last row."""
  sz, kind, _ = c.heads[i]
  t = inp['tg'][i]
  cols = t.shape[1]
  if c.layout == 'dense':
    return t.reshape(-1).copy(), 0, cols
  stride, col = (4, 3) if kind == XENT else ((sz + 1, 0) if i == 0 else (max(14, sz + 5), 0))
  buf = np.full(c.N * stride + 8, np.nan, np.float32)
  rows = buf[:c.N * stride].reshape(c.N, stride)
  rows[:, col:col + cols] = t
  return buf, col, stride


def sample_weight_layout(c, inp):
  """-> flat float32 buffer holding sw[n] at n * sw_stride, NaN between."""
  buf = np.full((c.N - 1) * c.sw_stride + 1, np.nan, np.float32)
  buf[::c.sw_stride] = inp['sw']
  return buf


# ------------------------------------------------------------------------------------------------------------------------------
# the tail, stated once: float64 with bounds = the reference; float32 with a summation order (and a mistake) = an emulated kernel
# ------------------------------------------------------------------------------------------------------------------------------
def bf16(a):
  """float32 -> the nearest bfloat16 (round to nearest even), as float32."""
  u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
  u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
  return u.astype(np.uint32).view(np.float32)


def sum0(terms, order):
  """Sum over axis 0 in the dtype of ``terms``: 'forward', 'reversed' (one term after the other) or 'pairwise' (numpy's own)."""
  if order == 'pairwise' or terms.dtype == np.float64:
    return terms.sum(0, dtype=terms.dtype)
  acc = np.zeros(terms.shape[1:], terms.dtype)
  for k in (range(terms.shape[0]) if order == 'forward' else reversed(range(terms.shape[0]))):
    acc = acc + terms[k]
  return acc


def dot(a, b, order):
  """a [M][K] b [K][N]: every product rounded to the dtype, then summed over k in ``order``."""
  if a.dtype == np.float64:
    return a @ b
  return sum0(a.T[:, :, None] * b[:, None, :], order)


def tail_math(c, inp, h, dt=np.float64, order='forward', mistake=None, exact_inputs=True):
  """The decoder tail on ``h`` [N][H] in dtype ``dt``.  Returns (values, extra): values = dict(preds, losses[1 + nheads], and with
  ``backward`` dh, dw1, db1, dhw<i>, dhb<i>).  In float64 ``extra`` holds, per output, ``abs`` = the sum of |terms| along its
  reduction chain and ``bound`` = its rounding bound (module docstring); ``exact_inputs``: h, fc1 and the heads sit on the lattice
  (no rounding before the loss terms)."""
  f = lambda a: np.asarray(a, dt)
  N, H, F = c.N, c.H, c.F
  sizes = [sz for sz, _, _ in c.heads]
  nh, OT = len(sizes), sum(sizes)
  off = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
  w1, b1, hh = f(inp['w1']), f(inp['b1']), f(h)
  wh, bh = np.concatenate([f(w) for w in inp['hw']], 1), np.concatenate([f(b) for b in inp['hb']])
  ref = dt == np.float64
  a = np.abs
  # ---- fc1 and the heads ----
  pre = (dot(bf16(hh), bf16(w1), order) if mistake == 'bf16' else dot(hh, w1, order)) + b1
  a1 = np.maximum(pre, dt(0))
  preds = dot(a1, wh, order) + bh
  if mistake == 'swap_offsets':      # the offsets of two heads of equal size, one for the other
    i, j = [k for k in range(nh) if c.heads[k][:2] == (3, MSE)][:2]
    preds = preds.copy()
    preds[:, off[i]:off[i + 1]], preds[:, off[j]:off[j + 1]] = preds[:, off[j]:off[j + 1]].copy(), preds[:, off[i]:off[i + 1]].copy()
  if ref:
    if exact_inputs:
      e_a1, e_p = np.zeros_like(a1), np.zeros_like(preds)
    else:      # an H-term dot product plus the bias; the ReLU keeps the bound where it is open; then F terms plus the bias
      e_a1 = np.where(pre > 0, gamma(H + 1) * (a(hh) @ a(w1) + a(b1)), 0.0)
      e_p = gamma(F + 1) * (a1 @ a(wh) + a(bh)) + e_a1 @ a(wh)
  # ---- effective weights and counts ----
  shaped = c.shaping is not None
  sw = f(inp['sw']) if inp['sw'] is not None else np.ones(N, dt)
  smooth = dt(np.float32(c.shaping['smooth'])) if shaped else dt(0)
  cls_head = next((i for i, (_, k, _) in enumerate(c.heads) if k == XENT), -1) if inp['cw'] is not None else -1
  lterm, dp = np.zeros((N, nh), dt), np.zeros((N, OT), dt)
  e_lt, e_dp = np.zeros((N, nh)), np.zeros((N, OT))
  cnts = []
  for i, (sz, kind, wt) in enumerate(c.heads):
    p = preds[:, off[i]:off[i + 1]]
    ep = e_p[:, off[i]:off[i + 1]] if ref else None
    if mistake == 'dense_stride':      # targets fetched at stride = size whatever the layout says
      buf, col, _ = target_layout(c, inp, i)
      cols = inp['tg'][i].shape[1]
      t = f(np.stack([buf[col + n * cols:col + n * cols + cols] for n in range(N)]))
    else:
      t = f(inp['tg'][i])
    w = sw.copy()
    if kind == XENT:
      label = np.rint(np.nan_to_num(t[:, 0])).astype(int) + 1
      if mistake == 'dense_stride':
        label = np.clip(label, 0, sz - 1)
      if i == cls_head:
        w = w * f(inp['cw'])[label]
    cnt = int(np.count_nonzero(w)) if shaped else N
    if mistake == 'mean_over_n':
      cnt = N
    cnts.append(cnt)
    wsc = dt(np.float32(wt)) * dt(1)
    if cnt == 0:
      continue
    live = (w != 0)[:, None]
    if kind == MSE:
      d = p - t
      c2 = dt(2) / dt(cnt * sz) * wsc
      l = (d * d).sum(1, dtype=dt)
      g = d * c2 * w[:, None]
      if ref:      # d: one rounding; l: |d|^2 twice the relative error of d, sz products and sums; dp: weight product, division, 3 products
        e_d = U * a(d) + ep
        e_l = (2 * a(d) * e_d).sum(1) + gamma(sz + 1) * l
        e_g = a(c2 * w[:, None]) * e_d + (4 + DIV_U) * U * a(g)
    elif kind == HUBER:
      d = p - t
      dl = dt(np.float32(DELTA))
      ad = a(d)
      q = np.minimum(ad, dl)
      lc = dt(0.5) * q * q + dl * (ad - q)
      l = lc.sum(1, dtype=dt)
      c1 = dt(1) / dt(cnt * sz) * wsc
      g = np.where(ad <= dl, d, np.copysign(dl, d)) * c1 * w[:, None]
      if ref:      # d l / d d = clip(d): at most q; per column q q / 2, a - q, the product by delta, their sum: 4; then sz sums
        e_d = U * ad + ep
        e_l = (q * e_d).sum(1) + gamma(sz + 4) * l
        e_g = np.where(ad <= dl, a(c1 * w[:, None]) * e_d, 0.0) + (4 + DIV_U) * U * a(g)
    else:
      mx = p.max(1)
      x = p - mx[:, None]
      E = np.exp(x)
      se = E.sum(1, dtype=dt)
      lo = smooth / dt(sz)
      hi = dt(1) * (dt(1) - smooth) + lo
      y = np.where(np.arange(sz)[None, :] == label[:, None], hi, lo)
      ysum = y.sum(1, dtype=dt)
      lse = np.log(se)
      t_c = (mx + lse)[:, None] - p
      l = (y * t_c).sum(1, dtype=dt)
      invc = dt(1) / dt(cnt)
      core = E / se[:, None] * ysum[:, None] - y
      g = core * invc * wsc * w[:, None]
      if ref:
        # x = p - max: one rounding and both operands' bounds; expf(x): its allowance and e_x (d exp = exp dx); se: a sum of sz
        # positive terms: the worst relative error of a term and sz - 1 roundings; logf: its allowance and se's relative error
        epm = ep.max(1)[:, None]
        e_x = U * a(x) + 2 * epm
        rel_e = EXP_U * U + e_x
        rel_se = rel_e.max(1) + (sz - 1) * U
        e_lse = rel_se + LOG_U * U * a(lse)
        # a term (max + log se) - p: two roundings; y = hi or lo: a division and two roundings (ky); l: sz products and sums
        ky = DIV_U + 2
        e_t = (e_lse + U * a(mx + lse))[:, None] + U * a(t_c) + 2 * epm
        e_l = (y * e_t).sum(1) + gamma(sz + 1 + ky) * a(y * t_c).sum(1)
        # softmax * ysum - y: expf, se, the division, the product by ysum (sz sums of y: sz + ky); y's own ky; the difference: one;
        # then 1 / cnt (division), the weight product and three products
        soft = E / se[:, None]
        e_core = soft * (rel_e + rel_se[:, None] + (DIV_U + 1 + sz + ky) * U) + y * ky * U + U * a(core)
        e_g = e_core * a(invc * wsc * w)[:, None] + (4 + DIV_U) * U * a(g)
    lterm[:, i] = np.where(live[:, 0], l * w, dt(0))
    dp[:, off[i]:off[i + 1]] = np.where(live, g, dt(0))
    if ref:      # l * w: one more rounding
      e_lt[:, i] = np.where(live[:, 0], a(w) * e_l + U * a(l * w), 0.0)
      e_dp[:, off[i]:off[i + 1]] = np.where(live, e_g, 0.0)
  # ---- what sums over the batch ----
  rows = np.arange(N)
  if mistake == 'drop_last_sample':
    rows = rows[:-1]
  if mistake == 'drop_chunk_row':      # the last row of every full 32-sample chunk
    rows = rows[rows % HF_NC != HF_NC - 1]
  losses = np.zeros(1 + nh, dt)
  L_abs, L_e = np.zeros(1 + nh), np.zeros(1 + nh)
  for i, (sz, kind, wt) in enumerate(c.heads):
    cnt = cnts[i]
    mean = dt(0) if cnt == 0 else (dt(1) / dt(cnt) if kind == XENT else dt(1) / dt(cnt * sz))
    losses[1 + i] = sum0(lterm[rows, i], order) * mean
    if ref:      # N terms in any order, then the mean: a division and a product
      L_abs[1 + i] = a(lterm[:, i]).sum() * mean
      L_e[1 + i] = (e_lt[:, i].sum() + gamma(N) * a(lterm[:, i]).sum()) * mean + (DIV_U + 2) * U * a(losses[1 + i])
  total = dt(0)
  for i, (_, _, wt) in enumerate(c.heads):
    total = total + dt(np.float32(wt)) * losses[1 + i]
  losses[0] = total
  out = dict(preds=preds, losses=losses)
  if ref:
    wts = np.array([wt for _, _, wt in c.heads])
    L_abs[0] = (wts * a(losses[1:])).sum()
    L_e[0] = (wts * L_e[1:]).sum() + gamma(nh + 1) * L_abs[0]
    ex = dict(preds=(a1 @ a(wh) + a(bh), e_p), losses=(L_abs, L_e))
  if c.backward:
    dhw = dot(np.ascontiguousarray(a1[rows].T), dp[rows], order)
    dhb = sum0(dp[rows], order)
    g1 = dot(dp, np.ascontiguousarray(wh.T), order)
    mask = (g1 > 0) if mistake == 'mask_da1' else (a1 > 0)
    da1 = np.where(mask, g1, dt(0))
    out.update(dw1=dot(np.ascontiguousarray(hh[rows].T), da1[rows], order), db1=sum0(da1[rows], order),
               dh=dot(da1, np.ascontiguousarray(w1.T), order))
    for i in range(nh):
      out['dhw%d' % i], out['dhb%d' % i] = dhw[:, off[i]:off[i + 1]], dhb[off[i]:off[i + 1]]
    if ref:
      # sums over n: N terms; d(a1): OT terms, kept where the unit is open (exactly zero elsewhere); d(h): F terms
      A_dhw, e_dhw = a(a1).T @ a(dp), gamma(N) * (a(a1).T @ a(dp)) + a(a1).T @ e_dp + e_a1.T @ a(dp)
      A_dhb, e_dhb = a(dp).sum(0), gamma(N) * a(dp).sum(0) + e_dp.sum(0)
      A_g = np.where(mask, a(dp) @ a(wh).T, 0.0)
      e_da1 = np.where(mask, gamma(OT) * (a(dp) @ a(wh).T) + e_dp @ a(wh).T, 0.0)
      ex['dw1'] = (a(hh).T @ a(da1), gamma(N) * (a(hh).T @ a(da1)) + a(hh).T @ e_da1)
      ex['db1'] = (a(da1).sum(0), gamma(N) * a(da1).sum(0) + e_da1.sum(0))
      ex['dh'] = (a(da1) @ a(w1).T, gamma(F) * (a(da1) @ a(w1).T) + e_da1 @ a(w1).T)
      for i in range(nh):
        ex['dhw%d' % i] = (A_dhw[:, off[i]:off[i + 1]], e_dhw[:, off[i]:off[i + 1]])
        ex['dhb%d' % i] = (A_dhb[off[i]:off[i + 1]], e_dhb[off[i]:off[i + 1]])
      ex['_da1_abs'] = A_g
  if not ref:
    return out, None
  ex['_pre'], ex['_a1'] = pre, a1
  return out, ex


def legacy_cap(name, val):
  """What tests/test_kernels_gpu.py::test_heads_loss allows an element of this output today."""
  if name == 'preds':
    return 1e-5 + 1e-5 * np.abs(val)
  if name == 'losses':
    return 1e-6 + 1e-5 * np.abs(val)
  return np.full(val.shape, float(np.abs(val).max()) * 2e-5 + 1e-8)


def tail_reference(c, inp, z=None, h=None):
  """-> dict name -> (value, abs, bound), float64.  heads cases: from inp['h'].  step_heads cases: ``z`` and ``h`` are what the device
  returned for them (float32); the chain is linked there (module docstring)."""
  fused = c.entry == 'step_heads'
  if fused:
    z64, h64 = _cell(inp['x'], inp['wx'], inp['bias'])
    z_in = z64 if z is None else np.asarray(z, np.float64)
    h_in = h64 if h is None else np.asarray(h, np.float64)
  else:
    h_in = inp['h'].astype(np.float64)
  val, ex = tail_math(c, inp, h_in, exact_inputs=not fused)
  ref = {}
  for name, v in val.items():
    if fused and name == 'dh':
      continue      # the fused form keeps d(h) on chip
    A, e = ex[name]
    ref[name] = (v, A, np.minimum(e, legacy_cap(name, v)))
  if fused:
    H = c.H
    A_z = np.abs(inp['x'].astype(np.float64)) @ np.abs(inp['wx'].astype(np.float64))
    ref['z'] = (z64, A_z, gamma(c.D) * A_z)      # D products and sums, in slabs or not
    cc, hv, gates = P.lstm_gates_ref(z_in, inp['bias'])
    bc, bh, bg = P.lstm_gates_fwd_bounds(z_in, inp['bias'])
    ref['c'], ref['h'], ref['gates'] = (cc, np.abs(cc), bc), (hv, np.abs(hv), bh), (gates, np.abs(gates), bg)
    if c.backward:
      dh, e_dh = val['dh'], ex['dh'][1]
      dz, _ = P.lstm_gates_bwd_ref(z_in, inp['bias'], dh=dh)
      bdz, _ = P.lstm_gates_bwd_bounds(z_in, inp['bias'], dh=dh)
      si, tj, sf, so = (gates[:, k * H:(k + 1) * H] for k in range(4))
      tc = np.tanh(cc)
      dct = so * (1 - tc * tc)      # dz is linear in d(h): its bound travels through these factors
      J = np.concatenate([dct * tj * si * (1 - si), dct * si * (1 - tj * tj), np.zeros_like(si), tc * so * (1 - so)], 1)
      ref['dz'] = (dz, np.abs(dz), bdz + np.abs(J) * np.tile(e_dh, (1, 4)))
  return ref


def tail_compare(c, got, ref):
  """-> ({output: worst err / bound}, [problems]).  Equality for the predictions of a lattice case and for every element that is
  exactly zero in the reference term by term (the sum of |terms| is 0: a masked unit, a sample of weight zero; a sum whose terms
  cancel to 0.0 in float64 need not in float32 and stays under its bound); the per-element bound everywhere else.  A problem starts with 'nan', 'exact' or 'bound'."""
  worst, problems = {}, []
  lattice = c.entry == 'heads'
  for name, (val, A, bound) in ref.items():
    g = np.asarray(got[name], np.float64).reshape(val.shape)
    if np.isnan(g).any():
      problems.append('nan %s: %d of %d elements' % (name, int(np.isnan(g).sum()), g.size))
      worst[name] = float('inf')
      continue
    eq = np.ones(val.shape, bool) if (lattice and name == 'preds') else (A == 0)
    if (g[eq] != val[eq]).any():
      at = np.argwhere(eq & (g != val))[0]
      problems.append('exact %s: %d elements differ, first at %s: got %.9g, reference %.9g' % (
          name, int((g[eq] != val[eq]).sum()), tuple(at), g[tuple(at)], val[tuple(at)]))
    err, rest = np.abs(g - val), ~eq
    share = err[rest] / np.maximum(bound[rest], 1e-300)
    worst[name] = float(share.max()) if share.size else 0.0
    if (err[rest] > bound[rest]).any():
      at = np.argwhere(rest & (err > bound))[0]
      problems.append('bound %s: %d of %d elements, worst share %.3g, first at %s: got %.9g, reference %.9g, bound %.3e' % (
          name, int((err[rest] > bound[rest]).sum()), g.size, worst[name], tuple(at), g[tuple(at)], val[tuple(at)], bound[tuple(at)]))
  return worst, problems
