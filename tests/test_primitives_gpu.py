"""The small kernels every decoder and optimiser step runs, each against a float64 reference of its own (tests/_primitive_refs.py).

tests/test_kernels_gpu.py checks the fused kernels bitwise against the chains of launches they replace; the kernels of those chains
(geeco_gemm_f32, geeco_colsum, geeco_lstm_gates_fwd/bwd, geeco_state_concat_fwd/bwd, geeco_adam_tf, ...) are pinned here, so a
mistake in device code both sides of such a comparison share does not pass unseen.

Two kinds of input: small integers (every product and sum exact in fp32: assert_array_equal catches a dropped, doubled or misplaced
element whatever the summation order) and random floats against the reference with the per-element bounds derived in
_primitive_refs.py (tests/test_primitive_refs_cpu.py applies the same bounds to emulated mistakes).  Every output buffer carries
NaN-filled slack past its logical extent that must stay NaN; outputs that are written (not accumulated) start as NaN and must end
NaN-free; padding of inputs that must not be read is NaN as well.
"""
import numpy as np
import pytest
import torch

import _primitive_refs as R

pytestmark = pytest.mark.gpu

NAN = float('nan')


def _nan(dev, *shape):
  return torch.full(shape, NAN, dtype=torch.float32, device=dev)


def _padded(dev, a, ld=None, rows=None):
  """a [r][c] (numpy) -> device tensor [rows >= r][ld >= c] whose padding is NaN."""
  r, c = a.shape
  t = _nan(dev, rows or r, ld or c)
  t[:r, :c] = torch.from_numpy(np.ascontiguousarray(a))
  return t


def _flat(dev, a, slack=5):
  """a (numpy, any shape) -> flat device tensor with ``slack`` NaN elements behind it."""
  t = _nan(dev, a.size + slack)
  t[:a.size] = torch.from_numpy(np.ascontiguousarray(a).reshape(-1))
  return t


def _np(t):
  return t.detach().cpu().numpy().copy()


def _all_nan(t):
  return bool(torch.isnan(t).all())


def _check(got, ref, bound, what):
  print('%s: %.3f of its bound' % (what, R.worst_ratio(got, ref, bound)))
  R.assert_within(got, ref, bound, what)


# --------------------------------------------------------------------------------------------------------------------------
# Adam
# --------------------------------------------------------------------------------------------------------------------------
ADAM_GRID_CAP_N = 4 * 2048 * 256 + 4 * 300 + 3      # past the 2048-block cap: a second, ragged grid-stride round, and a tail
ADAM = dict(beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=0.125)


def _adam_ref_and_bounds(p, g, m, v, lr_t, l2):
  kw = dict(b1=ADAM['beta1'], b2=ADAM['beta2'], eps=ADAM['eps'], grad_scale=ADAM['grad_scale'], l2=l2)
  return R.adam_ref(p, g, m, v, lr_t, **kw), R.adam_bounds(p, g, m, v, lr_t, **kw)


@pytest.mark.parametrize('l2', [0.0, 1e-3])
@pytest.mark.parametrize('n', [1, 3, 4, 5, 7, 1027, ADAM_GRID_CAP_N])
def test_adam_three_steps(dev, n, l2):
  """geeco_adam_prepare + geeco_adam_tf, three steps: p, m, v of every step against adam_ref carried forward in float64 from the
  device's own previous state and the device's own lr_t (bounds: adam_bounds, per step, nothing compounds).  n = 1, 3: the n & 3
  tail alone; 5, 7, 1027: a tail behind whole float4s; 4: none; the largest: the grid-stride loop past the block cap."""
  from geeco_amd import ops
  p, g, m, v = (_flat(dev, a) for a in R.adam_inputs(n, 10 + n % 97))
  step = torch.tensor([4, -7], dtype=torch.int64, device=dev)
  scal = _nan(dev, 2)
  for t in (5, 6, 7):
    before = [_np(x[:n]) for x in (p, g, m, v)]
    ops.adam_prepare(step, 0.001, scal)
    ops.adam_tf(p, g, m, v, n, scal, l2=l2, **ADAM)
    torch.cuda.synchronize()
    assert step.tolist() == [t, -7]
    lr_t = float(scal[0])
    ref, bounds = _adam_ref_and_bounds(*before, lr_t, l2)
    for name, buf, r, b in zip('pmv', (p, m, v), ref, bounds):
      _check(buf[:n], r, b, 'adam n=%d l2=%g step %d: %s' % (n, l2, t, name))
      assert _all_nan(buf[n:]), name
    assert np.array_equal(_np(g[:n]), before[1]) and _all_nan(g[n:]) and _all_nan(scal[1:])


def test_adam_segments(dev):
  """geeco_adam_tf_segments against adam_ref (and bitwise against geeco_adam_tf over the same elements): three pieces given out of
  arena order, one a single float4, their gradients in buffers of their own, g_out set.  Between the pieces nothing moves."""
  from geeco_amd import ops
  n = 1280
  pieces = [(1240, 20), (8, 4), (16, 1200)]       # (offset, count) in floats
  l2 = 1e-3
  p0, g0, m0, v0 = R.adam_inputs(n, 20)
  p, m, v = (_flat(dev, a) for a in (p0, m0, v0))
  g_out = _nan(dev, n + 5)
  gsrc = [_flat(dev, g0[o:o + c]) for o, c in pieces]
  scal = torch.tensor([float(np.float32(R.lr_t_ref(0.001, 0.9, 0.999, 3))), NAN], device=dev)
  ops.adam_tf_segments(p, m, v, [(gs, o, c) for gs, (o, c) in zip(gsrc, pieces)], scal, g_out=g_out, l2=l2, **ADAM)
  # the one-pass kernel over the same elements
  q, qm, qv, qg = (_flat(dev, a) for a in (p0, m0, v0, g0))
  ops.adam_tf(q, qg, qm, qv, n, scal, l2=l2, **ADAM)
  torch.cuda.synchronize()
  ref, bounds = _adam_ref_and_bounds(p0, g0, m0, v0, float(scal[0]), l2)
  inside = np.zeros(n, bool)
  for o, c in pieces:
    inside[o:o + c] = True
  for name, buf, start, one_pass, r, b in zip('pmv', (p, m, v), (p0, m0, v0), (q, qm, qv), ref, bounds):
    got = _np(buf[:n])
    _check(got[inside], r[inside], b[inside], 'adam segments: ' + name)
    assert np.array_equal(got[inside], _np(one_pass[:n])[inside]), name
    assert np.array_equal(got[~inside], start[~inside]), name + ': moved outside the pieces'
    assert _all_nan(buf[n:]), name
  go = _np(g_out[:n])
  assert np.array_equal(go[inside], g0[inside]) and np.isnan(go[~inside]).all() and _all_nan(g_out[n:])
  for gs, (o, c) in zip(gsrc, pieces):
    assert np.array_equal(_np(gs[:c]), g0[o:o + c]) and _all_nan(gs[c:])


@pytest.mark.parametrize('t0', [0, 9, 999, 99999])
def test_adam_prepare(dev, t0):
  """scal[0] = lr_t of step t0 + 1 to 4 U relative (float64 pow / sqrt on the device, one rounding to float32); the counter moves by
  exactly one; nothing else is written."""
  from geeco_amd import ops
  step = torch.tensor([t0, -7], dtype=torch.int64, device=dev)
  scal = _nan(dev, 2)
  ops.adam_prepare(step, 0.001, scal)
  torch.cuda.synchronize()
  assert step.tolist() == [t0 + 1, -7] and _all_nan(scal[1:])
  ref = R.lr_t_ref(0.001, 0.9, 0.999, t0 + 1)
  _check(scal[:1], np.array([ref]), 4 * R.U * ref, 'lr_t at step %d' % (t0 + 1))


# --------------------------------------------------------------------------------------------------------------------------
# LSTM gate math
# --------------------------------------------------------------------------------------------------------------------------
GATE_SHAPES = [(1, 1), (3, 5), (2, 128), (5, 100), (9, 128)]      # N H = 1: a ragged block; 15; 256 exactly; 500; 1152 = 4.5 blocks


def _gates_fwd(ops, dev, z, bias, cp, N, H):
  c, h, gates = _nan(dev, N * H + 5), _nan(dev, N * H + 5), _nan(dev, 4 * N * H + 5)
  ops.lstm_gates_fwd_into(c, h, gates, z, bias, cp, N, H)
  return c, h, gates


@pytest.mark.parametrize('with_c', [True, False])
@pytest.mark.parametrize('N,H', GATE_SHAPES)
def test_lstm_gates_fwd(dev, N, H, with_c):
  """geeco_lstm_gates_fwd: c, h and the four gate blocks (order i, j, f, o; forget bias 1) against lstm_gates_ref with the bounds
  of lstm_gates_fwd_bounds; a third of the pre-activations saturate their gate."""
  from geeco_amd import ops
  z, bias, cp, _, _ = R.gates_inputs(N, H, 100 * N + H)
  cp = cp if with_c else None
  dz, db, dcp = _flat(dev, z), _flat(dev, bias), (_flat(dev, cp) if with_c else None)
  c, h, gates = _gates_fwd(ops, dev, dz, db, dcp, N, H)
  torch.cuda.synchronize()
  ref, bounds = R.lstm_gates_ref(z, bias, cp), R.lstm_gates_fwd_bounds(z, bias, cp)
  for name, buf, r, b in zip(('c', 'h', 'gates'), (c, h, gates), ref, bounds):
    _check(buf[:r.size].reshape(r.shape), r, b, 'gates fwd N=%d H=%d c_prev=%s: %s' % (N, H, with_c, name))
    assert _all_nan(buf[r.size:]), name


@pytest.mark.parametrize('N,H', GATE_SHAPES)
def test_lstm_gates_bwd(dev, N, H):
  """geeco_lstm_gates_bwd behind geeco_lstm_gates_fwd, in the argument combinations the decoder's backward loop issues, against
  autograd through the oracle's cell in float64 (lstm_gates_bwd_ref; bounds: lstm_gates_bwd_bounds, which carry the forward's):
    last step   dc = None, dc_prev written;
    middle step dc and dc_prev both given -- as two buffers, and as the decoder gives them, ONE buffer (same result required);
    first step  c_prev = None, dc_prev = None;
    and dh = None."""
  from geeco_amd import ops
  z, bias, cp, dh, dc = R.gates_inputs(N, H, 200 * N + H)
  dv = {k: _flat(dev, a) for k, a in dict(z=z, bias=bias, cp=cp, dh=dh, dc=dc).items()}

  def run(with_c, with_dh, with_dc, want_dcp, alias=False):
    c, h, gates = _gates_fwd(ops, dev, dv['z'], dv['bias'], dv['cp'] if with_c else None, N, H)
    dz = _nan(dev, 4 * N * H + 5)
    dc_in = dv['dc'].clone() if with_dc else None
    dcp = dc_in if alias else (_nan(dev, N * H + 5) if want_dcp else None)
    ops.lstm_gates_bwd_into(dz, dcp, gates, dv['cp'] if with_c else None, c, dv['dh'] if with_dh else None, dc_in, N, H)
    torch.cuda.synchronize()
    args = (z, bias, cp if with_c else None, dh if with_dh else None, dc if with_dc else None)
    (rz, rcp), (bz, bcp) = R.lstm_gates_bwd_ref(*args), R.lstm_gates_bwd_bounds(*args)
    what = 'gates bwd N=%d H=%d c_prev=%s dh=%s dc=%s alias=%s' % (N, H, with_c, with_dh, with_dc, alias)
    _check(dz[:4 * N * H].reshape(N, 4 * H), rz, bz, what + ': dz')
    assert _all_nan(dz[4 * N * H:])
    if dcp is not None:
      assert with_c      # (dc_prev = dct sf is the gradient of the c_prev the reference differentiates)
      _check(dcp[:N * H].reshape(N, H), rcp, bcp, what + ': dc_prev')
      assert _all_nan(dcp[N * H:])
    if with_dc and not alias:
      assert np.array_equal(_np(dc_in[:N * H]), dc.reshape(-1))      # an input
    return dz, dcp

  run(True, True, False, True)                       # last step
  dz2, dcp2 = run(True, True, True, True)            # middle step, two buffers
  dz1, dcp1 = run(True, True, True, True, alias=True)      # ... as the decoder runs it: dc_prev IS dc
  assert torch.equal(dz1[:4 * N * H], dz2[:4 * N * H]) and torch.equal(dcp1[:N * H], dcp2[:N * H])
  run(False, True, True, False)                      # first step
  run(True, False, True, True)                       # dh = None
  run(False, True, False, False)                     # the one-step decoder: only dh


def test_lstm_three_step_chain(dev):
  """T = 3, N = 3, H = 8, D = 5 through the loops of LSTMDecoder._forward_chain / backward: the hoisted input projection, then per
  step gemm_into(accumulate=True) (z[t] += h[t-1] Wh) + lstm_gates_fwd_into; backward per step lstm_gates_bwd_into (dc_prev and dc
  one buffer) + gemm_into(tb=True) (dh = dz[t] Wh^T).  Against float64 autograd through three oracle cells: c, h and dz of every
  step, and the dh / dc buffers as step 0's backward finds them.  Bound: LSTM_CHAIN_ATOL (derived in _primitive_refs.py)."""
  from geeco_amd import ops
  r = np.random.default_rng(7)
  T, N, D, H = 3, 3, 5, 8
  u = lambda lim, *s: r.uniform(-lim, lim, s).astype(np.float32)
  x, Wx, Wh, bias, dh_last = u(1, T, N, D), u(0.25, D, 4 * H), u(0.125, H, 4 * H), u(0.25, 4 * H), u(1, N, H)
  t = lambda a: torch.from_numpy(a).to(dev)
  xs, W, b = t(x), t(np.concatenate([Wx, Wh], 0)), t(bias)
  dWx, dWh = W[:D], W[D:]
  z, dz, gates = _nan(dev, T + 1, N, 4 * H), _nan(dev, T + 1, N, 4 * H), _nan(dev, T + 1, N, 4 * H)
  c, h = _nan(dev, T + 1, N, H), _nan(dev, T + 1, N, H)
  ws = torch.empty(max(ops.gemm_ws_bytes(T * N, 4 * H, D), ops.gemm_ws_bytes(N, 4 * H, H), ops.gemm_ws_bytes(N, H, 4 * H)) // 4 + 4,
                   dtype=torch.float32, device=dev)
  ops.gemm_into(z, xs, dWx, T * N, 4 * H, D, D, 4 * H, 4 * H, ws=ws)
  for k in range(T):
    if k > 0:
      ops.gemm_into(z[k], h[k - 1], dWh, N, 4 * H, H, H, 4 * H, 4 * H, accumulate=True, ws=ws)
    ops.lstm_gates_fwd_into(c[k], h[k], gates[k], z[k], b, c[k - 1] if k > 0 else None, N, H)
  dh, dc = _nan(dev, N + 1, H), _nan(dev, N + 1, H)
  dh[:N] = t(dh_last)
  at_step0 = None
  for k in range(T - 1, -1, -1):
    if k == 0:
      at_step0 = (dh.clone(), dc.clone())
    ops.lstm_gates_bwd_into(dz[k], dc if k > 0 else None, gates[k], c[k - 1] if k > 0 else None, c[k], dh, None if k == T - 1 else dc, N, H)
    if k > 0:
      ops.gemm_into(dh, dz[k], dWh, N, H, 4 * H, 4 * H, 4 * H, H, tb=True, ws=ws)
  torch.cuda.synchronize()
  ref = R.lstm_chain_ref(x, Wx, Wh, bias, dh_last)
  for k in range(T):
    for name, buf in (('c', c), ('h', h), ('dz', dz)):
      _check(buf[k], ref[name][k], R.LSTM_CHAIN_ATOL, 'chain step %d: %s' % (k, name))
  _check(at_step0[0][:N], ref['dh0'], R.LSTM_CHAIN_ATOL, 'chain: dh at step 0')
  _check(at_step0[1][:N], ref['dc0'], R.LSTM_CHAIN_ATOL, 'chain: dc at step 0')
  for buf in (z, dz, gates, c, h):
    assert _all_nan(buf[T])
  assert _all_nan(dh[N:]) and _all_nan(dc[N:])


# --------------------------------------------------------------------------------------------------------------------------
# state concat
# --------------------------------------------------------------------------------------------------------------------------
CONCAT_CASES = [(1, (6,), 0, 3), (1, (6,), 1, 3), (2, (8, 5), 1, 7), (2, (8, 5), 2, 7), (3, (8, 4, 6), 2, 7), (3, (256, 128, 64), 0, 7),
                (1, (5,), 1, 0)]
CELLS = 4


def _concat_inputs(N, chs, J, seed):
  """Small integers (copies, one multiply, one subtraction or addition: exact).  pre: the features before their ReLU, a third exact
  zeros, a third negative."""
  r = np.random.default_rng(seed)
  ints = lambda *s: torch.tensor(r.integers(-8, 9, s).astype(np.float32))
  pre = [ints(N, 2, 2, ch) * torch.tensor(r.integers(0, 3, (N, 2, 2, ch)) > 0) for ch in chs]
  return pre, ints(N, J), ints(N, 2, 2, chs[0]), ints


@pytest.mark.parametrize('sub', [False, True])
@pytest.mark.parametrize('N', [1, 5])
@pytest.mark.parametrize('nfeat,chs,jnt_pos,J', CONCAT_CASES)
def test_state_concat_fwd(dev, nfeat, chs, jnt_pos, J, N, sub):
  """geeco_state_concat_fwd against state_concat_ref (torch.cat as the oracle's state_concatenation / representation_concatenation /
  _v2 build their layouts): every position of the joint block, unequal channel counts, J = 0, ``sub_from``, joint rows read at a
  stride (the newest row of a window [N][2J + 1]) and a state row longer than cells * Ctot.  Exact."""
  from geeco_amd import ops
  pre, jnt, tgt, _ = _concat_inputs(N, chs, J, 300 + N + 10 * jnt_pos + sum(chs))
  Ctot = sum(chs) + J
  stride = CELLS * Ctot + 3
  jbuf = _nan(dev, N, 2 * J + 1)
  jbuf[:, J + 1:] = jnt.to(dev)
  state = _nan(dev, N + 1, stride)
  feats = [_flat(dev, p.numpy()) for p in pre]
  sub_from = _flat(dev, tgt.numpy()) if sub else None
  ops.state_concat_fwd_into(state, feats, list(chs), jnt_pos, jbuf[:, J + 1:] if J else jbuf, 2 * J + 1, J, N, CELLS, stride,
                            sub_from=sub_from)
  torch.cuda.synchronize()
  ref = R.state_concat_ref(pre, jnt, jnt_pos, sub_from=tgt if sub else None)
  assert ref.shape == (N, CELLS * Ctot)
  np.testing.assert_array_equal(_np(state[:N, :CELLS * Ctot]), ref.numpy())
  assert _all_nan(state[:N, CELLS * Ctot:]) and _all_nan(state[N])
  for f, p in zip(feats, pre):
    assert _all_nan(f[p.numel():])


@pytest.mark.parametrize('scale', [1.0, -1.0])
@pytest.mark.parametrize('accumulate', [False, True])
@pytest.mark.parametrize('N', [1, 5])
@pytest.mark.parametrize('nfeat,chs,jnt_pos,J', CONCAT_CASES)
def test_state_concat_bwd(dev, nfeat, chs, jnt_pos, J, N, accumulate, scale):
  """geeco_state_concat_bwd against autograd through relu features and state_concat_ref: features with exact zeros and negatives
  (the gate is > 0), scale 1 / -1, written into NaN or accumulated onto a non-zero buffer, the last feature's buffer withheld (a
  None entry) when there are several.  The joint columns and the slack of d(state) are NaN on the device: reading one would show."""
  from geeco_amd import ops
  pre, jnt, _, ints = _concat_inputs(N, chs, J, 400 + N + 10 * jnt_pos + sum(chs))
  Ctot = sum(chs) + J
  stride = CELLS * Ctot + 3
  dstate = ints(N, CELLS * Ctot)
  joint = torch.zeros(Ctot, dtype=torch.bool)
  off = sum(chs[:jnt_pos])
  joint[off:off + J] = True
  dsd = _nan(dev, N + 1, stride)
  dsd[:N, :CELLS * Ctot] = torch.where(joint.repeat(CELLS), torch.tensor(NAN), dstate).to(dev)
  base = [ints(N, 2, 2, ch) for ch in chs]
  ref = R.state_concat_bwd_ref(pre, jnt, jnt_pos, dstate, scale=scale, base=base if accumulate else None)
  feats = [_flat(dev, torch.relu(p).numpy()) for p in pre]
  dfeats = [_flat(dev, b.numpy()) if accumulate else _nan(dev, b.numel() + 5) for b in base]
  withheld = nfeat - 1 if nfeat > 1 else None
  before = dfeats[withheld].clone() if withheld is not None else None
  ops.state_concat_bwd_into([None if f == withheld else d for f, d in enumerate(dfeats)], dsd, stride, feats, list(chs), jnt_pos, J, N,
                            CELLS, accumulate=accumulate, scale=scale)
  torch.cuda.synchronize()
  for f in range(nfeat):
    n = pre[f].numel()
    if f == withheld:
      assert torch.equal(torch.nan_to_num(dfeats[f], nan=12345.0), torch.nan_to_num(before, nan=12345.0))
      continue
    np.testing.assert_array_equal(_np(dfeats[f][:n]), ref[f].reshape(-1).numpy().astype(np.float32))
    assert _all_nan(dfeats[f][n:])


# --------------------------------------------------------------------------------------------------------------------------
# GEMM
# --------------------------------------------------------------------------------------------------------------------------
GEMM_CASES = [      # M, N, K, slabs of the split-K plan
    (1, 1, 1, 1),
    (3, 512, 128, 2),       # the recurrent product z[t] += h[t-1] Wh
    (5, 7, 63, 1), (5, 7, 64, 1), (5, 7, 65, 1),
    (65, 63, 130, 2),       # ragged tiles both ways, a ragged last slab (80 + 50)
    (64, 64, 1040, 13),     # several slabs (the slab sum's unrolled eight and its remainder)
    (130, 520, 40, 1),      # many tiles, unsplit
]


@pytest.mark.parametrize('M,N,K,S', GEMM_CASES)
def test_gemm_forms(dev, M, N, K, S):
  """geeco_gemm_f32 in all four (ta, tb) forms, overwriting and accumulating, every leading dimension 3 larger than needed (the
  operands' padding NaN: never read), unsplit and split-K (``S`` asserted through geeco_gemm_ws_bytes so each case provably takes the
  form it is named for).  Integer operands: exact; standard-normal operands: the bound of test_kernels_gpu.py::test_gemm."""
  from geeco_amd import ops
  nbytes = ops.gemm_ws_bytes(M, N, K)
  assert nbytes == (S * M * N * 4 if S > 1 else 16), (nbytes, S)
  ws = torch.empty(nbytes // 4 + 4, dtype=torch.float32, device=dev)
  r = np.random.default_rng(M + N + K)
  for kind in ('int', 'float'):
    draw = (lambda *s: r.integers(-4, 5, s).astype(np.float32)) if kind == 'int' else (lambda *s: r.standard_normal(s).astype(np.float32))
    for ta in (False, True):
      for tb in (False, True):
        A, B = draw(*((K, M) if ta else (M, K))), draw(*((N, K) if tb else (K, N)))
        dA, dB = _padded(dev, A, A.shape[1] + 3), _padded(dev, B, B.shape[1] + 3)
        for accumulate in (False, True):
          base = draw(M, N) if accumulate else None
          C = _nan(dev, M + 1, N + 3)
          if accumulate:
            C[:M, :N] = torch.from_numpy(base)
          ops.gemm_into(C, dA, dB, M, N, K, A.shape[1] + 3, B.shape[1] + 3, N + 3, ta, tb, accumulate, ws)
          torch.cuda.synchronize()
          ref = R.gemm_ref(A, B, ta, tb, M, N, K, base)
          what = 'gemm %dx%dx%d ta=%d tb=%d acc=%d %s' % (M, N, K, ta, tb, accumulate, kind)
          if kind == 'int':
            assert np.abs(ref).max() < 2 ** 24
            np.testing.assert_array_equal(_np(C[:M, :N]), ref, err_msg=what)
          else:
            R.assert_within(C[:M, :N], ref, R.gemm_bound(ref, K), what)
          assert _all_nan(C[:M, N:]) and _all_nan(C[M]), what


# --------------------------------------------------------------------------------------------------------------------------
# reductions
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('accumulate', [False, True])
@pytest.mark.parametrize('M,N,lda', [(1, 1, 1), (7, 5, 9), (8, 256, 256), (13, 300, 304), (96, 512, 512)])
def test_colsum(dev, M, N, lda, accumulate):
  """geeco_colsum: M below, at and off the multiples of 8 its row loop unrolls by, lda > N (the padding NaN), N off the multiples
  of its 256-column blocks, overwriting NaN or accumulating.  Integers: exact; floats: colsum_bound ((M + 1) U sum |terms|)."""
  from geeco_amd import ops
  r = np.random.default_rng(M * N)
  for kind in ('int', 'float'):
    draw = (lambda *s: r.integers(-8, 9, s).astype(np.float32)) if kind == 'int' else (lambda *s: r.standard_normal(s).astype(np.float32))
    a, base = draw(M, N), draw(N)
    da = _padded(dev, a, lda, M + 1)
    out = _flat(dev, base, 3) if accumulate else _nan(dev, N + 3)
    ops.colsum_into(out, da, lda, M, N, accumulate=accumulate)
    torch.cuda.synchronize()
    b = base if accumulate else None
    ref = R.colsum_ref(a, M, N, b)
    if kind == 'int':
      np.testing.assert_array_equal(_np(out[:N]), ref)
    else:
      _check(out[:N], ref, R.colsum_bound(a, M, N, b), 'colsum %dx%d acc=%d' % (M, N, accumulate))
    assert _all_nan(out[N:])


@pytest.mark.parametrize('n', [1, 255, 2048, 2049, 1024 * 2048 + 77])
def test_sumsq(dev, n):
  """geeco_sumsq: one ragged block; one full block; a second, ragged one; past the 1024-block cap with a ragged last round.  Run
  twice into the same ``out`` (which starts as garbage): overwritten, not accumulated.  +-1: the sum is the count, exact; standard
  normal: sumsq_rel_bound.  The NaN behind the input is never read."""
  from geeco_amd import ops
  x = np.random.default_rng(n).standard_normal(n).astype(np.float32)
  for kind, vals in (('int', np.where(x < 0, -1.0, 1.0).astype(np.float32)), ('float', x)):
    p = _flat(dev, vals, 3)
    out = torch.tensor([123.0, NAN], device=dev)
    for _ in range(2):
      ops.sumsq_into(out, p, n)
    torch.cuda.synchronize()
    ref = R.sumsq_ref(vals)
    if kind == 'int':
      assert float(out[0]) == ref == n
    else:
      _check(out[:1], np.array([ref]), R.sumsq_rel_bound(n) * ref, 'sumsq n=%d' % n)
    assert _all_nan(out[1:])


# --------------------------------------------------------------------------------------------------------------------------
# plumbing (copies: exact)
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('A,B,Bd,C', [(9, 3, 4, 32), (2, 4, 4, 5), (1, 1, 3, 1)])
def test_pad_mid(dev, A, B, Bd, C):
  from geeco_amd import ops
  src = np.random.default_rng(A + C).integers(-8, 9, (A, B, C)).astype(np.float32)
  dst = _nan(dev, A * Bd * C + 5)
  ops.pad_mid_into(dst, _flat(dev, src), A, B, Bd, C)
  torch.cuda.synchronize()
  np.testing.assert_array_equal(_np(dst[:A * Bd * C]).reshape(A, Bd, C), R.pad_mid_ref(src, Bd))
  assert _all_nan(dst[A * Bd * C:])


@pytest.mark.parametrize('Cin,Cout', [(1, 1), (20, 36), (33, 31), (64, 128)])
def test_transpose_hwio(dev, Cin, Cout):
  """geeco_transpose_hwio: ragged 32 x 32 tiles both ways, two encoders at unequal, padded strides."""
  from geeco_amd import ops
  G, per = 2, 9 * Cin * Cout
  gs_w, gs_wt = per + 5, per + 11
  w = np.random.default_rng(Cin).integers(-99, 100, (G, 3, 3, Cin, Cout)).astype(np.float32)
  dw = _padded(dev, w.reshape(G, per), gs_w)
  dwt = _nan(dev, G + 1, gs_wt)
  ops.transpose_hwio_into(dwt, dw, G, gs_w, gs_wt, Cin, Cout)
  torch.cuda.synchronize()
  np.testing.assert_array_equal(_np(dwt[:G, :per]).reshape(G, 3, 3, Cout, Cin), R.transpose_taps_ref(w))
  assert _all_nan(dwt[:G, per:]) and _all_nan(dwt[G])


@pytest.mark.parametrize('HW', [1, 255, 257])
@pytest.mark.parametrize('C1,C2,Cpad', [(3, 0, 4), (3, 1, 4), (4, 0, 4), (3, 1, 6), (2, 0, 3)])
def test_pack_pixels(dev, C1, C2, Cpad, HW):
  """geeco_pack_pixels: the float4 store (Cpad == 4) and the channel loop, with and without a second source, zero padding, sample
  strides larger than a sample (the padding NaN)."""
  from geeco_amd import ops
  N = 2
  r = np.random.default_rng(HW + C1)
  src = r.integers(1, 100, (N, HW, C1)).astype(np.float32)
  src2 = r.integers(1, 100, (N, HW, C2)).astype(np.float32) if C2 else None
  s1, s2 = HW * C1 + 3, HW * C2 + 2
  d1 = _padded(dev, src.reshape(N, -1), s1)
  d2 = _padded(dev, src2.reshape(N, -1), s2) if C2 else None
  dst = _nan(dev, N * HW * Cpad + 5)
  ops.pack_pixels_into(dst, d1, s1, N, HW, C1, Cpad, src2=d2, src2_sample_stride=s2 if C2 else 0, C2=C2)
  torch.cuda.synchronize()
  np.testing.assert_array_equal(_np(dst[:N * HW * Cpad]).reshape(N, HW, Cpad), R.pack_pixels_ref(src, src2, Cpad))
  assert _all_nan(dst[N * HW * Cpad:])


@pytest.mark.parametrize('E', [4, 1020, 1028])
@pytest.mark.parametrize('u8', [True, False])
def test_gather_windows(dev, u8, E):
  """geeco_gather_windows: uint8 frames / 255 bitwise numpy's float32(u8) / float32(255); float frames at divisor 1 a bitwise copy;
  overlapping windows whose starts are out of order; a frame of one float4, one short of a block's 1024 and one float4 past it."""
  from geeco_amd import ops
  F, K, starts = 6, 3, [2, 0, 3, 1]
  N = len(starts)
  r = np.random.default_rng(E)
  src = r.integers(0, 256, (F, E)).astype(np.uint8) if u8 else r.standard_normal((F, E)).astype(np.float32)
  dsrc = torch.from_numpy(src).to(dev)
  out = _nan(dev, N * K * E + 5)
  ops.gather_windows_into(out, dsrc, torch.tensor(starts, dtype=torch.int32, device=dev), N, K, E, divisor=255.0 if u8 else 1.0)
  torch.cuda.synchronize()
  ref = R.gather_windows_ref(src, starts, K, 255.0 if u8 else 1.0)
  assert ref.dtype == np.float32
  np.testing.assert_array_equal(_np(out[:N * K * E]).reshape(N, K, E).view(np.uint32), ref.view(np.uint32))
  assert _all_nan(out[N * K * E:])


def test_every_u8_ingest_path_is_the_one_conversion(dev):
  """Every entry point that turns resident uint8 frames into floats gives numpy.float32(v) / numpy.float32(255) BITWISE for all 256
  byte values: the division form of csrc/frame_ingest.h in the gathers, the frame pack and the predictor's pack and push, at
  8 x 12 (their 4-byte / 4-pixel paths) and at 5 x 5 (one element or pixel at a time), and the Newton form in the one-pass input
  stage's copy of the current frame.  The frames start with arange(256)."""
  from geeco_amd import ops

  def same(got, want, what):
    np.testing.assert_array_equal(_np(got).reshape(-1).view(np.uint32), np.ascontiguousarray(want, np.float32).reshape(-1).view(np.uint32), what)

  def i32(a):
    return torch.tensor(a, dtype=torch.int32, device=dev)

  r, K, J = np.random.default_rng(255), 2, 3
  for H, W, F in ((8, 12, 2), (5, 5, 4)):
    HW, fe, what = H * W, H * W * 3, '%d x %d' % (H, W)
    f = r.integers(0, 256, size=F * fe, dtype=np.uint8)
    f[:256] = np.arange(256, dtype=np.uint8)
    want = (f.astype(np.float32) / np.float32(255)).reshape(F, H, W, 3)
    N = F // K                                   # windows of K consecutive frames: together every byte of f
    buf = torch.zeros(F * fe + 1, dtype=torch.uint8, device=dev)
    buf[1:] = torch.from_numpy(f)
    src, off1 = buf[1:].clone(), buf[1:]         # the same frames 4-byte aligned (a fresh allocation) and 1 byte past alignment
    assert src.data_ptr() % 4 == 0 and off1.data_ptr() % 4 == 1
    addr = lambda t: torch.tensor([t.data_ptr() + n * K * fe for n in range(N)], dtype=torch.int64, device=dev)
    kind = i32([0] * N)
    if fe % 4 == 0:
      out = _nan(dev, N * K * fe)
      ops.gather_windows_into(out, src, i32([n * K for n in range(N)]), N, K, fe, 255.0)
      same(out, want, what + ' gather_windows')
      for t, name in ((src, 'aligned'), (off1, 'offset by 1 byte')):
        out = _nan(dev, N * K * fe)
        ops.gather_windows_by_address_into(out, addr(t), kind, N, K, fe)
        same(out, want, what + ' gather_windows_by_address, ' + name)
    for dx in (0, 1):
      out = _nan(dev, N * K * fe)
      ops.gather_windows_augmented_into(out, addr(src), kind, i32([[0, dx]] * N), None, N, K, H, W, 3)
      shifted = np.zeros_like(want)
      shifted[:, :, dx:] = want[:, :, :W - dx]
      same(out, shifted, what + ' gather_windows_augmented, dx = %d' % dx)
    padded = np.zeros((F, H, W, 4), np.float32)
    padded[..., :3] = want
    frames = src.view(F, HW, 3)
    x_in = _nan(dev, F, HW, 4)
    ops.pack_frames_by_address_into(x_in, torch.tensor([src.data_ptr() + i * fe for i in range(F)], dtype=torch.int64, device=dev), F, HW, True)
    same(x_in, padded, what + ' pack_frames_by_address')
    x_in = _nan(dev, F, HW, 4)
    ops.predict_pack_newest_into(x_in, frames, F, HW, 3)
    same(x_in, padded, what + ' predict_pack_newest')
    rgb, jw = _nan(dev, F, K, HW, 3), _nan(dev, F, K, J)
    ops.predict_push_dense_into(rgb, None, jw, frames, torch.zeros(F, J, device=dev), i32([1] * F), i32([0] * (F + 1)), F, K, HW, 3, J)
    same(rgb, np.repeat(want[:, None], K, axis=1), what + ' predict_push_dense')
    if HW % 4 == 0:                              # the window's LAST frame is the current one: the arange frame goes there
      win = torch.cat([src[fe:2 * fe], src[:fe]])
      imgs = [_nan(dev, 1, H, W, 4) for _ in range(3)]
      ptr = torch.tensor([win.data_ptr()], dtype=torch.int64, device=dev)
      ops.goal_dynimgs_u8_into(imgs[0], imgs[1], imgs[2], ptr, ptr, K, 1, HW, ops.goal_dynimgs_ws(1, HW, dev))
      same(imgs[0], padded[:1], what + ' goal_dynimgs_u8 cur_out')
