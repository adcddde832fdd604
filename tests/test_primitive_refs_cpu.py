"""The references of tests/_primitive_refs.py against the oracle, and their bounds against wrong kernels (no GPU).

Two halves.  (1) Every reference that restates something the oracle (or a vector TensorFlow publishes) also states agrees with it
in float64.  (2) Every bound tests/test_primitives_gpu.py imports is applied here to mistakes a kernel could make, each emulated in
numpy and rounded to float32 like a kernel's output: each must be rejected, and the unperturbed reference rounded to float32 must be
accepted -- a bound that accepted one of them would let that kernel pass on the GPU.
"""
import numpy as np
import pytest
import torch

import _primitive_refs as R
from oracle import geeco_oracle as O

f32 = lambda a: np.asarray(a, np.float64).astype(np.float32)


# --------------------------------------------------------------------------------------------------------------------------
# (1) the references agree with the oracle
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_c', [True, False])
def test_gates_ref_is_the_oracles_cell(with_c):
  N, H, D = 3, 5, 4
  r = np.random.default_rng(0)
  x, h, c = r.standard_normal((N, D)), r.standard_normal((N, H)), r.standard_normal((N, H)) if with_c else np.zeros((N, H))
  kernel, bias = r.standard_normal((D + H, 4 * H)), r.standard_normal(4 * H)
  t = lambda a: torch.tensor(a, dtype=torch.float64)
  c2, h2 = O.lstm_cell(t(x), t(c), t(h), t(kernel), t(bias))
  z = np.concatenate([x, h], 1) @ kernel
  rc, rh, gates = R.lstm_gates_ref(z, bias, c if with_c else None)
  np.testing.assert_allclose(rc, c2.numpy(), rtol=1e-12, atol=0)
  np.testing.assert_allclose(rh, h2.numpy(), rtol=1e-12, atol=0)
  # the gate blocks, in the order i, j, f, o, rebuild the cell
  si, tj, sf, so = (gates[:, k * H:(k + 1) * H] for k in range(4))
  np.testing.assert_allclose(sf * c + si * tj, c2.numpy(), rtol=1e-12, atol=0)
  np.testing.assert_allclose(so * np.tanh(c2.numpy()), h2.numpy(), rtol=1e-12, atol=0)


def test_gates_ref_reproduces_the_vector_tf_publishes():
  from test_oracle_kat import TF_BASIC_LSTM_STATE, tf_basic_lstm_case
  x, state, kernel, bias = (t.numpy() for t in tf_basic_lstm_case())
  c1, h1, _ = R.lstm_gates_ref(np.concatenate([x, state[:, 2:4]], 1) @ kernel, bias, state[:, 0:2])
  c2, h2, _ = R.lstm_gates_ref(np.concatenate([h1, state[:, 6:8]], 1) @ kernel, bias, state[:, 4:6])
  np.testing.assert_allclose(np.concatenate([c1, h1, c2, h2], 1), TF_BASIC_LSTM_STATE, atol=2e-7, rtol=0)


def test_gates_bwd_ref_is_autograd_and_matches_the_closed_form():
  """lstm_gates_bwd_ref IS autograd through O.lstm_cell; the hand-derived closed form is only checked against it here."""
  z, bias, cp, dh, dc = R.gates_inputs(3, 5, 1)
  H = 5
  dz, dcp = R.lstm_gates_bwd_ref(z, bias, cp, dh, dc)
  c, h, gates = R.lstm_gates_ref(z, bias, cp)
  si, tj, sf, so = (gates[:, k * H:(k + 1) * H] for k in range(4))
  tc = np.tanh(c)
  dct = dc + dh * so * (1 - tc * tc)
  closed = np.concatenate([dct * tj * si * (1 - si), dct * si * (1 - tj * tj), dct * cp * sf * (1 - sf), dh * tc * so * (1 - so)], 1)
  np.testing.assert_allclose(dz, closed, rtol=1e-9, atol=1e-15)
  np.testing.assert_allclose(dcp, dct * sf, rtol=1e-12, atol=0)
  # absent arguments are zeros
  dz0, none = R.lstm_gates_bwd_ref(z, bias, None, dh, None)
  assert none is None
  np.testing.assert_allclose(dz0[:, 2 * H:3 * H], 0, atol=0)      # no c_prev: the forget gate has no gradient


def test_state_concat_ref_is_the_oracles_three_layouts():
  r = np.random.default_rng(2)
  N, J = 3, 7
  t = lambda *s: torch.tensor(r.standard_normal(s))
  a, b, c, jnt = t(N, 2, 2, 8), t(N, 2, 2, 5), t(N, 2, 2, 6), t(N, J)
  eq = lambda x, y: np.testing.assert_allclose(x.numpy(), y.numpy(), rtol=1e-12, atol=0)
  eq(R.state_concat_ref([a], jnt, 1), O.state_concatenation(a, jnt))
  eq(R.state_concat_ref([a, b], jnt, 1), O.representation_concatenation(a, b, jnt))
  eq(R.state_concat_ref([a, b, c], jnt, 2), O.representation_concatenation_v2(a, b, jnt, c))
  tgt = t(N, 2, 2, 8)
  eq(R.state_concat_ref([a], jnt, 1, sub_from=tgt), O.state_concatenation(tgt - a, jnt))      # the 'residual' target mode


def test_adam_ref_is_the_oracles_step_and_tfs_protocol():
  from test_oracle_kat import TF_ADAM_GRADS, TF_ADAM_VARS, tf_adam_update_numpy
  # constants a float32 represents exactly: the float32-carried constants are then the mathematical ones
  b1, b2, eps, lr = 0.875, 1 - 2.0 ** -8, 2.0 ** -27, 0.001
  p, g, m, v = (x.astype(np.float64) for x in R.adam_inputs(64, 3))
  for t in (1, 2, 7):
    op, om, ov = p.copy(), m.copy(), v.copy()
    lr_t = O.adam_step_tf(op, g, om, ov, t, lr, b1, b2, eps)
    np.testing.assert_allclose(R.lr_t_ref(float(np.float32(lr)), b1, b2, t), float(np.float32(lr)) / lr * lr_t, rtol=1e-12)
    rp, rm, rv = R.adam_ref(p, g, m, v, lr_t, b1, b2, eps)
    for got, ref in ((rp, op), (rm, om), (rv, ov)):
      np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0)
    p, m, v = rp, rm, rv
  # TF's own protocol (default betas, which float32 does not represent): the float64-constant form of the same function
  p, m, v, g = np.array(sum(TF_ADAM_VARS, [])), np.zeros(4), np.zeros(4), np.array(sum(TF_ADAM_GRADS, []))
  tp, tm, tv = p.copy(), m.copy(), v.copy()
  for t in (1, 2, 3):
    tp, tm, tv = tf_adam_update_numpy(tp, g, t, tm, tv)
    p, m, v = R.adam_ref(p, g, m, v, 0.001 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t), const=np.float64)
    for got, ref in ((p, tp), (m, tm), (v, tv)):
      np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0)


def test_trivial_refs():
  a = np.arange(12.0).reshape(3, 4)
  np.testing.assert_array_equal(R.colsum_ref(a, 2, 3), [4, 6, 8])
  np.testing.assert_array_equal(R.colsum_ref(a, 2, 3, base=np.ones(4)), [5, 7, 9])
  assert R.sumsq_ref([1, -2, 3]) == 14.0
  np.testing.assert_array_equal(R.pad_mid_ref(np.ones((2, 1, 2)), 2), [[[1, 1], [0, 0]]] * 2)
  w = np.arange(2 * 9 * 2 * 3.0).reshape(2, 3, 3, 2, 3)
  assert R.transpose_taps_ref(w).shape == (2, 3, 3, 3, 2) and R.transpose_taps_ref(w)[1, 2, 0, 2, 1] == w[1, 2, 0, 1, 2]
  np.testing.assert_array_equal(R.pack_pixels_ref(np.ones((1, 2, 2)), 2 * np.ones((1, 2, 1)), 4), [[[1, 1, 2, 0]] * 2])
  src = np.arange(12, dtype=np.uint8).reshape(6, 2)
  np.testing.assert_array_equal(R.gather_windows_ref(src, [3, 0], 2, 1), [[[6, 7], [8, 9]], [[0, 1], [2, 3]]])
  assert R.gather_windows_ref(src, [3], 1, 255)[0, 0, 1] == np.float32(7) / np.float32(255)
  A, B = np.arange(6.0).reshape(2, 3), np.arange(12.0).reshape(3, 4)
  np.testing.assert_array_equal(R.gemm_ref(A.T.copy(), B.T.copy(), True, True, 2, 4, 3), A @ B)


# --------------------------------------------------------------------------------------------------------------------------
# (2) the bounds reject wrong kernels
# --------------------------------------------------------------------------------------------------------------------------
ADAM_KW = dict(b1=0.9, b2=0.999, eps=1e-8, grad_scale=0.125, l2=1e-3)


def _adam_wrong(kind, p, g, m, v, lr_t, b1, b2, eps, grad_scale, l2):
  b1, omb1, b2, omb2, eps, gs, l2 = R._adam_consts(b1, b2, eps, grad_scale, l2, np.float32)
  p, g, m, v = (np.asarray(x, np.float64) for x in (p, g, m, v))
  if kind == 'b2_099':
    b2, omb2 = 0.99, 0.01
  if kind == 'no_grad_scale':
    gs = 1.0
  gg = g * gs + (0.0 if kind == 'l2_after' else l2 * p)
  m2 = b1 * m + omb1 * gg
  v2 = b2 * v + omb2 * gg * gg
  den = np.sqrt(v2 + eps) if kind == 'eps_inside' else np.sqrt(v2) + eps
  p2 = p - lr_t * m2 / den
  if kind == 'l2_after':
    p2 = p2 - lr_t * l2 * p
  if kind == 'tail_untouched':
    k = len(p) & 3
    p2[-k:], m2[-k:], v2[-k:] = p[-k:], m[-k:], v[-k:]
  return p2, m2, v2


@pytest.mark.parametrize('n', [7, 1027])
def test_adam_bounds_reject_wrong_updates(n):
  p, g, m, v = R.adam_inputs(n, 4)
  lr_t = float(np.float32(R.lr_t_ref(0.001, 0.9, 0.999, 3)))
  ref = R.adam_ref(p, g, m, v, lr_t, **ADAM_KW)
  bounds = R.adam_bounds(p, g, m, v, lr_t, **ADAM_KW)
  ok = lambda out: all(R.within(f32(o), r, b) for o, r, b in zip(out, ref, bounds))
  assert ok(ref)
  for kind in ('eps_inside', 'b2_099', 'l2_after', 'no_grad_scale', 'tail_untouched'):
    assert not ok(_adam_wrong(kind, p, g, m, v, lr_t, **ADAM_KW)), kind
  # each mistake is caught where it is made: the parameters alone show the misplaced epsilon, the second moment alone shows b2
  assert not R.within(f32(_adam_wrong('eps_inside', p, g, m, v, lr_t, **ADAM_KW)[0]), ref[0], bounds[0])
  assert not R.within(f32(_adam_wrong('b2_099', p, g, m, v, lr_t, **ADAM_KW)[2]), ref[2], bounds[2])
  assert not R.within(f32(_adam_wrong('l2_after', p, g, m, v, lr_t, **ADAM_KW)[1]), ref[1], bounds[1])


def test_lr_t_bound_rejects_a_step_counter_off_by_one():
  for t in (1, 10, 1000, 100000):
    ref = R.lr_t_ref(0.001, 0.9, 0.999, t)
    assert abs(float(np.float32(ref)) - ref) <= 4 * R.U * ref
    if t < 100000:      # (by then both corrections have run out: lr_t == lr; the GPU test reads the counter itself as well)
      assert abs(R.lr_t_ref(0.001, 0.9, 0.999, t + 1) - ref) > 4 * R.U * ref


@pytest.mark.parametrize('with_c', [True, False])
def test_gate_bounds_reject_wrong_cells(with_c):
  N, H = 5, 100
  z, bias, cp, dh, dc = R.gates_inputs(N, H, 5)
  cp = cp if with_c else None
  ref, bounds = R.lstm_gates_ref(z, bias, cp), R.lstm_gates_fwd_bounds(z, bias, cp)
  ok = lambda out: all(R.within(f32(o), r, b) for o, r, b in zip(out, ref, bounds))
  assert ok(ref)
  assert not ok(R.lstm_gates_ref(z, bias, cp, forget_bias=0.0))
  assert not R.within(f32(R.lstm_gates_ref(z, bias, cp, forget_bias=0.0)[2]), ref[2], bounds[2])      # seen in the gates alone
  swapped = z.copy()
  swapped[:, H:2 * H], swapped[:, 2 * H:3 * H] = z[:, 2 * H:3 * H], z[:, H:2 * H]
  sb = bias.copy()
  sb[H:2 * H], sb[2 * H:3 * H] = bias[2 * H:3 * H], bias[H:2 * H]
  assert not ok(R.lstm_gates_ref(swapped, sb, cp))
  if with_c:      # ... and in c and h alone
    for k in (0, 1):
      assert not R.within(f32(R.lstm_gates_ref(z, bias, cp, forget_bias=0.0)[k]), ref[k], bounds[k])


def test_gate_bwd_bounds_reject_wrong_gradients():
  N, H = 5, 100
  z, bias, cp, dh, dc = R.gates_inputs(N, H, 6)
  (dz, dcp), (bz, bcp) = R.lstm_gates_bwd_ref(z, bias, cp, dh, dc), R.lstm_gates_bwd_bounds(z, bias, cp, dh, dc)
  assert R.within(f32(dz), dz, bz) and R.within(f32(dcp), dcp, bcp)
  sf = R.lstm_gates_ref(z, bias, cp)[2][:, 2 * H:3 * H]
  assert not R.within(f32(dcp / sf), dcp, bcp)                                      # dc_prev without the sf factor
  dz0, dcp0 = R.lstm_gates_bwd_ref(z, bias, cp, dh, dc, forget_bias=0.0)
  assert not R.within(f32(dz0), dz, bz) and not R.within(f32(dcp0), dcp, bcp)        # forget bias 0
  dz_nodc, _ = R.lstm_gates_bwd_ref(z, bias, cp, dh, None)
  assert not R.within(f32(dz_nodc), dz, bz)                                          # the incoming dc dropped
  # a forward off by a few ulp is what the backward's bound allows for: gates rounded to float32 stay inside
  c, h, gates = (f32(x).astype(np.float64) for x in R.lstm_gates_ref(z, bias, cp))
  si, tj, sf32, so = (gates[:, k * H:(k + 1) * H] for k in range(4))
  tc = np.tanh(c)
  dct = dc + dh * so * (1 - tc * tc)
  from_f32 = np.concatenate([dct * tj * si * (1 - si), dct * si * (1 - tj * tj), dct * cp * sf32 * (1 - sf32), dh * tc * so * (1 - so)], 1)
  assert R.within(f32(from_f32), dz, bz) and R.within(f32(dct * sf32), dcp, bcp)


def _chain_case():
  r = np.random.default_rng(7)
  T, N, D, H = 3, 3, 5, 8
  u = lambda lim, *s: r.uniform(-lim, lim, s).astype(np.float32)
  return u(1, T, N, D), u(0.25, D, 4 * H), u(0.125, H, 4 * H), u(0.25, 4 * H), u(1, N, H)


def test_chain_bound_rejects_wrong_chains():
  x, Wx, Wh, bias, dh = _chain_case()
  ref = R.lstm_chain_ref(x, Wx, Wh, bias, dh)
  flat = lambda d: np.concatenate([a.ravel() for a in d['dz'] + d['c'] + d['h'] + [d['dh0'], d['dc0']]])
  assert R.within(f32(flat(ref)), flat(ref), R.LSTM_CHAIN_ATOL)
  # a recurrent product that overwrites z instead of adding to it = no input projection after step 0
  x0 = x.copy(); x0[1:] = 0
  assert not R.within(f32(flat(R.lstm_chain_ref(x0, Wx, Wh, bias, dh))), flat(ref), R.LSTM_CHAIN_ATOL)
  # the recurrent product left out
  assert not R.within(f32(flat(R.lstm_chain_ref(x, Wx, 0 * Wh, bias, dh))), flat(ref), R.LSTM_CHAIN_ATOL)
  # each of the quantities compared alone shows a dc that is dropped between steps (dz of step 0 without the cell path)
  dz0_no_c = R.lstm_gates_bwd_ref(x[0] @ Wx.astype(np.float64), bias, None, ref['dh0'], None)[0]
  assert not R.within(f32(dz0_no_c), ref['dz'][0], R.LSTM_CHAIN_ATOL)
  with_c = R.lstm_gates_bwd_ref(x[0] @ Wx.astype(np.float64), bias, None, ref['dh0'], ref['dc0'])[0]
  assert R.within(f32(with_c), ref['dz'][0], R.LSTM_CHAIN_ATOL)      # (and dh0 / dc0 are what step 0's backward is given)


def test_concat_equality_rejects_misplaced_columns_and_a_wrong_relu_gate():
  r = np.random.default_rng(8)
  N, chs, J, jnt_pos = 5, (8, 5), 7, 1
  ints = lambda *s: torch.tensor(r.integers(-8, 9, s).astype(np.float32))
  pre = [ints(N, 2, 2, c) for c in chs]
  for p in pre:
    p[..., ::3] = 0.0      # exact zeros
  jnt = ints(N, J)
  feats = [torch.relu(p) for p in pre]
  state = R.state_concat_ref(feats, jnt, jnt_pos).numpy()
  Ctot = sum(chs) + J
  off = chs[0]
  cols = list(range(Ctot))
  cols.insert(off + J, cols.pop(off))      # the joint block one column early
  wrong = state.reshape(N, 4, Ctot)[:, :, cols].reshape(N, -1)
  assert not np.array_equal(wrong, state) and np.array_equal(np.sort(wrong, 1), np.sort(state, 1))
  dstate = ints(N, 4 * Ctot)
  dstate[dstate == 0] = 1.0
  ref = R.state_concat_bwd_ref(pre, jnt, jnt_pos, dstate, scale=-1.0)
  d3 = dstate.reshape(N, 2, 2, Ctot)
  slices = [d3[..., :chs[0]], d3[..., chs[0] + J:]]
  for f in range(2):
    right = torch.where(feats[f] > 0, -slices[f], torch.zeros(()))
    loose = torch.where(feats[f] >= 0, -slices[f], torch.zeros(()))
    assert np.array_equal(right.numpy(), ref[f].numpy()) and not np.array_equal(loose.numpy(), ref[f].numpy())
  # the joint columns of dstate influence nothing
  d2 = dstate.clone().reshape(N, 4, Ctot)
  d2[:, :, off:off + J] += 5.0
  for a, b in zip(R.state_concat_bwd_ref(pre, jnt, jnt_pos, d2.reshape(N, -1), scale=-1.0), ref):
    assert torch.equal(a, b)


def test_colsum_bound_rejects_dropped_rows():
  M, N, lda = 13, 300, 304
  r = np.random.default_rng(9)
  for a in (r.standard_normal((M, lda)).astype(np.float32), r.integers(-8, 9, (M, lda)).astype(np.float32)):
    ref, bound = R.colsum_ref(a, M, N), R.colsum_bound(a, M, N)
    assert R.within(f32(ref), ref, bound)
    assert not R.within(f32(R.colsum_ref(a, M - M % 8, N)), ref, bound)
    assert not np.array_equal(R.colsum_ref(a, M - M % 8, N), ref)
  base = r.standard_normal(lda).astype(np.float32)
  assert not R.within(f32(ref), R.colsum_ref(a, M, N, base), R.colsum_bound(a, M, N, base))      # accumulate ignored


def test_sumsq_bound_rejects_a_dropped_block_and_an_accumulated_second_run():
  for n in (255, 2049, 1024 * 2048 + 77):
    p = np.random.default_rng(n).standard_normal(n).astype(np.float32)
    ref = R.sumsq_ref(p)
    tol = R.sumsq_rel_bound(n) * ref
    assert abs(float(np.float32(ref)) - ref) <= tol
    # a piece left out: the ragged end at the small sizes; at the largest the float bound (1033 U of 2.1e6) sees one block's 2048
    # elements, and the 77 of the ragged end are what the +-1 inputs are for (the sum is then the count, exact below 2**24)
    assert abs(R.sumsq_ref(p[:-(77 if n < 4096 else 2048)]) - ref) > tol
    ones = np.where(p < 0, -1.0, 1.0)
    assert R.sumsq_ref(ones) == n < 2 ** 24 and R.sumsq_ref(ones[:-77]) != n
    assert abs(2 * ref - ref) > tol                                # out accumulated over two runs
