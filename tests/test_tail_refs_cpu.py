"""What tests/test_decoder_tail_variants_gpu.py relies on, shown without a GPU: the inputs of every case of _tail_refs.CASES have the
lattice properties claimed for them, the float64 statement of the tail agrees with the autograd one of _loss_shaping_ref, the case
table holds every instantiation and edge it was written for, and ``tail_compare`` -- the function the device test asserts on --
accepts a float32 numpy emulation of the tail in two summation orders and rejects emulated wrong kernels.  The emulation is
_tail_refs.tail_math in float32: that measures the reference's bounds and the comparison, never the kernels.
"""
import ctypes

import numpy as np
import pytest
import torch

import _loss_shaping_ref as L
import _primitive_refs as P
import _tail_refs as R

CASES = R.CASES
SMALL = [c for c in CASES if c.N <= 128]
ids = lambda c: c.id

_memo = {}


def inputs(c):
  if c.index not in _memo:
    _memo[c.index] = R.tail_inputs(c)
  return _memo[c.index]


def emulate(c, order, mistake=None):
  """-> (got, ref): the case in float32 numpy (the fused form with its slab sum, gate math and gate backward) and the reference
  linked to it as the device test links it."""
  inp = inputs(c)
  f32 = np.float32
  if c.entry == 'heads':
    got, _ = R.tail_math(c, inp, inp['h'], f32, order, mistake)
    return got, R.tail_reference(c, inp)
  H = c.H
  chunks = np.array_split(np.arange(c.D), c.S)
  if mistake == 'drop_slab':
    chunks = chunks[:-1]
  z = np.zeros((c.N, 4 * H), f32)
  for ks in chunks:
    z = z + R.dot(inp['x'][:, ks], inp['wx'][ks], order)
  x = z + inp['bias']
  sig = lambda v: f32(1) / (f32(1) + np.exp(-v))
  si, tj, sf, so = sig(x[:, :H]), np.tanh(x[:, H:2 * H]), sig(x[:, 2 * H:3 * H] + f32(1)), sig(x[:, 3 * H:])
  cn = si * tj
  tc = np.tanh(cn)
  h = so * tc
  got, _ = R.tail_math(c, inp, h, f32, order, None if mistake == 'drop_slab' else mistake)
  got.update(z=z, c=cn, h=h, gates=np.concatenate([si, tj, sf, so], 1))
  if c.backward:
    dh = got.pop('dh')
    dct = dh * so * (f32(1) - tc * tc)
    got['dz'] = np.concatenate([dct * tj * si * (f32(1) - si), dct * si * (f32(1) - tj * tj), np.zeros_like(si),
                                dh * tc * so * (f32(1) - so)], 1)
  return got, R.tail_reference(c, inp, z=z, h=h)


# ------------------------------------------------------------------------------------------------------------------------------
# the inputs
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', CASES, ids=ids)
def test_lattice_properties(c):
  inp = inputs(c)
  f64 = lambda a: np.asarray(a, np.float64)
  if c.entry == 'heads':
    h = f64(inp['h'])
    margin = R.LATTICE_MARGIN
  else:
    _, h = R._cell(inp['x'], inp['wx'], inp['bias'])
    margin = R.FUSED_MARGIN
    assert np.abs(h).max() < 1.0
  pre = h @ f64(inp['w1']) + f64(inp['b1'])
  assert np.abs(pre).min() >= margin, np.abs(pre).min()
  assert 0.3 < np.mean(pre > 0) < 0.7, np.mean(pre > 0)                      # about half of fc1 on each side of 0
  val, ex = R.tail_math(c, inp, h, exact_inputs=c.entry == 'heads')
  assert np.abs(val['preds']).max() <= 8.0
  if c.entry == 'heads':
    # float32 in forward, reversed and pairwise order gives the float64 fc1 output and predictions bit for bit
    for order in ('forward', 'reversed', 'pairwise'):
      pre32 = R.dot(inp['h'], inp['w1'], order) + inp['b1']
      assert pre32.dtype == np.float32 and np.array_equal(pre32.astype(np.float64), pre), order
      a1 = np.maximum(pre32, np.float32(0))
      wh, bh = np.concatenate(inp['hw'], 1), np.concatenate(inp['hb'])
      p32 = R.dot(a1, wh, order) + bh
      assert p32.dtype == np.float32 and np.array_equal(p32.astype(np.float64), val['preds']), order
  off = np.concatenate([[0], np.cumsum([sz for sz, _, _ in c.heads])]).astype(int)
  dl = float(np.float32(R.DELTA))
  for i, (sz, kind, _) in enumerate(c.heads):
    t = f64(inp['tg'][i])
    if kind == R.XENT:
      labels = np.rint(t[:, 0]).astype(int) + 1
      assert labels.min() >= 0 and labels.max() < sz and len(set(labels.tolist())) == min(c.N, sz)
    else:
      d = np.abs(val['preds'][:, off[i]:off[i + 1]] - t)
      assert np.array_equal(t * 8, np.rint(t * 8))                            # targets on the lattice
      assert ((d < 0.25) | (d > 0.875)).all()                                 # ... and the residuals far from delta
      if kind == R.HUBER:
        assert c.N * sz >= 2 and (d <= dl).any() and (d > dl).any(), i
  if inp['sw'] is not None and c.N > 1:
    assert (inp['sw'] == 0).any() and inp['sw'][-1] != 0
  # an element that is exactly zero in the reference is zero term by term: it is compared by equality, not under a bound
  ref = R.tail_reference(c, inp)
  for name, (v, A, bound) in ref.items():
    if name in ('z', 'c', 'h', 'gates', 'dz'):
      continue
    assert not v[A == 0].any(), name
    if name == 'preds' and c.entry == 'heads':
      assert not bound.any()                                                   # lattice predictions: equality
    else:
      assert (bound[v != 0] > 0).all(), name
  zero = {k: v.copy() for k, v in val.items()}
  if c.backward and c.entry == 'heads' and (ref['dh'][1] == 0).any():
    zero['dh'][ref['dh'][1] == 0] = 1e-30                                     # far inside any bound, but not equal
    _, problems = R.tail_compare(c, zero, ref)
    assert [p.split(' ')[:2] for p in problems] == [['exact', 'dh:']], problems


@pytest.mark.parametrize('c', SMALL, ids=ids)
def test_reference_is_the_autograd_one(c):
  """tail_math in float64 against _loss_shaping_ref.tail_reference (torch autograd): two statements of the same mathematics."""
  inp = inputs(c)
  h = inp['h'].astype(np.float64) if c.entry == 'heads' else R._cell(inp['x'], inp['wx'], inp['bias'])[1]
  val, _ = R.tail_math(c, inp, h, exact_inputs=False)
  t = lambda a: torch.tensor(np.asarray(a, np.float64))
  kw = {}
  if c.shaping:
    kw = dict(sample_weights=t(inp['sw']) if inp['sw'] is not None else None, class_weights=R.CLASS_W if inp['cw'] is not None else None,
              smoothing=float(np.float32(c.shaping['smooth'])), deltas=[float(np.float32(R.DELTA))] * len(c.heads))
  ref = L.tail_reference(t(h), t(inp['w1']), t(inp['b1']), [t(w) for w in inp['hw']], [t(b) for b in inp['hb']], c.heads,
                         [t(x) for x in inp['tg']], **kw)
  close = lambda a, b, what: np.testing.assert_allclose(np.asarray(a), b.numpy(), rtol=1e-11, atol=1e-13, err_msg=what)
  close(val['preds'], ref['preds'], 'preds')
  close(val['losses'][0], ref['total'], 'total')
  close(val['losses'][1:], ref['parts'], 'parts')
  if c.backward:
    g = ref['grads']
    close(val['dh'], g['h'], 'dh'); close(val['dw1'], g['w1'], 'dw1'); close(val['db1'], g['b1'], 'db1')
    for i in range(len(c.heads)):
      close(val['dhw%d' % i], g['hw'][i], 'dhw'); close(val['dhb%d' % i], g['hb'][i], 'dhb')


# ------------------------------------------------------------------------------------------------------------------------------
# the comparison
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', CASES, ids=ids)
def test_float32_in_two_orders_is_accepted(c):
  for order in ('forward', 'pairwise'):
    got, ref = emulate(c, order)
    worst, problems = R.tail_compare(c, got, ref)
    assert not problems, (order, problems)
    assert set(worst) == set(ref) and all(np.isfinite(v) for v in worst.values())
    print('%s, %s: float32 uses at most %.4f of a bound (%s)' % (c.id, order, max(worst.values()), max(worst, key=worst.get)))


# mistake -> what tail_compare has to report on every case marked for it ('any': at least one problem of any kind)
MISTAKES = {
    'drop_last_sample': 'bound',      # the last sample left out of a batch sum
    'drop_chunk_row': 'bound',        # the last row of a 32-sample chunk left out
    'mean_over_n': 'bound',           # a mean over N where it is over the non-zero count
    'dense_stride': 'any',            # a target read at stride = size in the model layout (NaN columns, or a neighbour's value)
    'swap_offsets': 'exact',          # the offsets of two equal-sized heads swapped: lattice predictions are compared by equality
    'drop_slab': 'bound',             # one slab left out of the fused slab sum
    'bf16': 'any',                    # fc1 products rounded to bf16: equality on a lattice case, the bound on a fused one
    'mask_da1': 'any',                # the ReluGrad mask taken from d(a1) instead of a1
}


def test_every_mistake_has_a_case():
  for m in MISTAKES:
    assert any(m in c.marks for c in CASES), m
  assert {m for c in CASES for m in c.marks} == set(MISTAKES)
  assert {c.entry for c in CASES if 'bf16' in c.marks} == {'heads', 'step_heads'}


@pytest.mark.parametrize('name,c', [(m, c) for c in CASES for m in c.marks], ids=lambda v: v if isinstance(v, str) else v.id)
def test_mistake_is_rejected(name, c):
  got, ref = emulate(c, 'forward', name)
  _, problems = R.tail_compare(c, got, ref)
  kinds = {p.split(' ')[0] for p in problems}
  assert problems and (MISTAKES[name] == 'any' or MISTAKES[name] in kinds), (name, problems)
  if name == 'mask_da1':      # seen in the gradients alone
    assert all(p.split(' ')[1].rstrip(':') in ('dh', 'dw1', 'db1') for p in problems), problems
  if name == 'drop_slab':
    assert any(p.startswith('bound z') for p in problems), problems


def test_no_bound_is_looser_than_test_heads_loss():
  for c in SMALL[::3]:
    for name, (v, _, bound) in R.tail_reference(c, inputs(c)).items():
      if name not in ('z', 'c', 'h', 'gates', 'dz'):
        assert (bound <= R.legacy_cap(name, v)).all(), (c.id, name)


def test_gamma_and_the_allowances():
  assert R.gamma(1) == R.U / (1 - R.U) and R.gamma(4096) < 4096 * R.U * 1.001
  assert (R.EXP_U, R.DIV_U, R.LOG_U) == (P.EXP_U, P.DIV_U, P.EXP_U)


# ------------------------------------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------------------------------------
def test_the_cases_hold_the_edges():
  heads = [c for c in CASES if c.entry == 'heads']
  fused = [c for c in CASES if c.entry == 'step_heads']
  ps = [c for c in heads if R.per_sample(c.H, c.F, c.heads)]
  wg = [c for c in heads if not R.per_sample(c.H, c.F, c.heads)]
  OT = lambda c: sum(sz for sz, _, _ in c.heads)
  sh = lambda c: c.shaping is not None
  # per-sample kernel with its own finish: Hfc x H, unshaped and shaped; both tables; forward only
  for F in (64, 128):
    for H in (1, 100, 127, 128):
      assert {sh(c) for c in ps if (c.H, c.F) == (H, F) and c.backward} == {False, True}, (H, F)
  for table in (R.CART, R.VEL, R.CART_S, R.VEL_S):
    assert {c.backward for c in ps if c.heads == table} == {0, 1}, table
  assert all(c.names[-1] == 'heads_finish_kernel' and c.names[0].startswith('heads_sample_kernel<false') for c in ps)
  # single-workgroup kernel: H = 129, Hfc = 96, unshaped and shaped, N past 1024 at H <= 16
  assert {sh(c) for c in wg if c.H == 129 and c.F == 128} == {False, True}
  assert {sh(c) for c in wg if c.F == 96} == {False, True} and any(not c.backward for c in wg)
  assert {c.N for c in wg if c.H <= 16} >= {1025, 4096}
  assert all(c.names == ['heads_loss_kernel<shaped>' if sh(c) else 'heads_loss_kernel'] for c in wg)
  # chunk and count edges of the finish roles and shaped_counts
  assert {c.N for c in ps if c.backward} >= {1, 31, 32, 33, 65}
  big = [c for c in ps if c.N in (1025, 4096)]
  assert {c.N for c in big} == {1025, 4096} and all((c.H, c.F) == (8, 64) and c.shaping == R.FULL for c in big)
  assert all(c.H <= 16 for c in CASES if c.N > 128)
  # width edges
  for group in (ps, wg):
    assert any(OT(c) == 32 and len(c.heads) == 5 and 16 in [sz for sz, _, _ in c.heads] for c in group)
    assert any(c.heads == [(1, R.MSE, 1.0)] for c in group)
  assert any(OT(c) == 32 for c in fused)
  assert any(R.XENT not in [k for _, k, _ in c.heads[:2]] and len(c.heads) > 2 and c.heads[2][1] == R.XENT for c in ps)
  two = [c for c in ps if [k for _, k, _ in c.heads].count(R.XENT) == 2]
  assert {sh(c) for c in two} == {False, True} and all(not (c.shaping or {}).get('cw') for c in two)
  # fused one-step decoder: the four instantiations, H, deferred, forward only, the slab counts
  assert {(c.F, sh(c)) for c in fused} == {(64, False), (64, True), (128, False), (128, True)}
  assert {(c.F, sh(c)) for c in fused if c.backward} == {(64, False), (64, True), (128, False), (128, True)}
  assert {c.H for c in fused} == {128, 100} and {c.deferred for c in fused if c.backward} == {False, True}
  assert {c.H for c in fused if c.deferred} == {128, 100} and any(not c.backward for c in fused)
  for c in fused:
    assert c.S == R.gemm_plan(c.N, 4 * c.H, c.D) and not (c.deferred and not c.backward)
    assert ('lstm_step_bwd_heads_kernel' in c.names) == c.deferred and ('heads_finish_kernel' in c.names) == (not c.deferred)
  S = {c.S for c in fused}
  assert 1 in S and any(1 < s < 16 for s in S) and any(s > 16 and s % 16 for s in S), S
  # layouts: the model's strided targets in both modes, sample weights at stride 3
  for group in (ps, wg, fused):
    assert any(c.layout == 'model' for c in group)
    assert any(c.layout == 'model' and R.XENT in [k for _, k, _ in c.heads] for c in group)
  assert any(c.layout == 'model' and c.heads in (R.VEL, R.VEL_S) for c in ps)
  for group in (ps, wg, fused):
    assert any(c.sw_stride == 3 and c.shaping and c.shaping['sw'] for c in group)
  assert all(c.sw_stride == 1 or (c.shaping and c.shaping['sw']) for c in CASES)
  assert len({c.id for c in CASES}) == len(CASES)


def test_the_model_layout_is_strided_and_poisoned():
  c = next(c for c in CASES if c.layout == 'model' and c.heads == R.CART_S and c.entry == 'heads' and c.N > 1)
  inp = inputs(c)
  for i, (sz, kind, _) in enumerate(c.heads):
    buf, col, stride = R.target_layout(c, inp, i)
    cols = inp['tg'][i].shape[1]
    assert stride > cols and np.isnan(buf[c.N * stride:]).all()
    rows = buf[:c.N * stride].reshape(c.N, stride)
    assert np.array_equal(rows[:, col:col + cols], inp['tg'][i]) and np.isnan(np.delete(rows, np.s_[col:col + cols], 1)).all()
    assert (col, stride) == ((3, 4) if kind == R.XENT else (0, 4 if i == 0 else 14))
  c = next(c for c in CASES if c.sw_stride == 3)
  buf = R.sample_weight_layout(c, inputs(c))
  assert np.array_equal(buf[::3], inputs(c)['sw']) and np.isnan(buf[1::3]).all() and np.isnan(buf[2::3]).all()


def test_gemm_plan_is_the_library_s():
  from geeco_amd import _native
  lib = _native.load()
  for c in CASES:
    if c.entry == 'step_heads':
      assert lib.geeco_gemm_ws_bytes(c.N, 4 * c.H, c.D) == (c.S * c.N * 4 * c.H * 4 if c.S > 1 else 16), c.id


def test_refusals_need_no_gpu():
  """N = 4097, a 17-wide head and OT = 33 come back as -1 with their message before any launch, from both entry points."""
  from geeco_amd import _native
  lib = _native.load()
  one = ctypes.c_void_p(256)

  def call(N, sizes, step):
    nh = len(sizes)
    parr = (ctypes.c_void_p * nh)(*[256] * nh)
    heads = (nh, parr, parr, (ctypes.c_int * nh)(*sizes), (ctypes.c_int * nh)(*[0] * nh), (ctypes.c_float * nh)(*[1.0] * nh), parr,
             (ctypes.c_int64 * nh)(*sizes))
    if step:
      return lib.geeco_lstm_step_heads_fwd_bwd(one, 64, one, 32, one, one, one, one, one, N, 8, 64, one, one, one, *heads, 1.0, 64, one,
                                               one, 0, None, None, None, None, None, one, None, None)
    return lib.geeco_heads_loss_fwd_bwd(one, one, one, *heads, 1.0, N, 8, 64, one, one, 0, None, None, None, None, None, one, None)
  for step in (False, True):
    assert call(4097, [3], step) == -1 and b'bad dims' in lib.geeco_last_error()
    assert call(0, [3], step) == -1
    assert call(4, [17], step) == -1 and b'size 17' in lib.geeco_last_error()
    assert call(4, [16, 16, 1], step) == -1 and b'33 outputs > 32' in lib.geeco_last_error()
    assert call(4, [1] * 6, step) == -1 and b'nheads=6' in lib.geeco_last_error()
