"""The launch-variant table of the input-gradient pass (tests/_input_grad_ref.py: CASES), on the host: it holds every instantiation
and edge that tests/test_input_grad_variants_gpu.py is there to launch, its inputs are what the generators promise, and the
comparison the GPU test uses rejects wrong kernels while it passes the float64 reference rounded to float32.  No GPU needed."""
import ctypes

import numpy as np
import pytest

import _input_grad_ref as R
import _relu_taps as T

CONV = [c for c in R.CASES if c.entry == 'conv1']
PACK = [c for c in R.CASES if c.entry == 'pack']
DYN = [c for c in R.CASES if c.entry == 'dynimg']
_inputs = {}


def inputs(c):
  if c.index not in _inputs:
    _inputs[c.index] = R.input_grad_inputs(c)
  return _inputs[c.index]


def _need(what, found):
  """Every edge by the id of a case that holds it."""
  assert found, 'no case holds: ' + what
  print('%-62s %s' % (what, found[0].id))


def test_ids_are_unique_and_indexed():
  assert [c.index for c in R.CASES] == list(range(len(R.CASES))) and len({c.id for c in R.CASES}) == len(R.CASES)
  assert len(CONV) + len(PACK) + len(DYN) == len(R.CASES)


def test_conv1_cases_hold_every_edge():
  geo = {c.index: R.conv1_geometry(c) for c in CONV}
  for Cin in (3, 4):
    _need('conv1_dgrad_kernel<%d>' % Cin, [c for c in CONV if c.Cin == Cin])
    for H, W in ((1, 1), (8, 32), (9, 33), (7, 31), (16, 64), (17, 65)):
      _need('cin%d at %d x %d' % (Cin, H, W), [c for c in CONV if (c.Cin, c.H, c.W) == (Cin, H, W)])
    for form in ('g1', 'dense', 'padded', 'shared_w'):
      _need('cin%d, group form %s' % (Cin, form), [c for c in CONV if c.Cin == Cin and c.form == form])
  for F in (1, 2):
    _need('F = %d' % F, [c for c in CONV if c.F == F])
  # the tile counts: one tile, exactly one tile, one pixel more in both directions, a short tile, 2 x 2 full tiles, 3 x 3 with ragged edges
  for ty, tx, H, W in ((1, 1, 1, 1), (1, 1, 8, 32), (2, 2, 9, 33), (1, 1, 7, 31), (2, 2, 16, 64), (3, 3, 17, 65)):
    _need('%d x %d tiles at %d x %d' % (ty, tx, H, W),
          [c for c in CONV if (geo[c.index]['tiles_y'], geo[c.index]['tiles_x'], c.H, c.W) == (ty, tx, H, W)])
  for c in CONV:
    g = geo[c.index]
    assert g['gs_dz'] % 4 == 0 and g['gs_dx'] % 4 == 0      # the entry point's own condition
    if c.form == 'g1':
      assert (g['G'], g['gs_dz'], g['gs_w'], g['gs_dx']) == (1, 0, 0, 0)      # as the encoder calls it
    if c.form == 'padded':
      assert g['gs_dz'] > g['n_dz'] and g['gs_w'] > g['n_w'] and g['gs_dx'] > g['n_dx'] and (g['gs_dz'] - g['n_dz']) % 4 == 0
    if c.form == 'shared_w':
      assert g['G'] == 2 and g['gs_w'] == 0 and inputs(c)['w'].shape[0] == 1
  exact = [c for c in CONV if c.exact]
  _need('small integers: every product and sum exact', exact)
  for c in exact:
    w, dz = inputs(c)['w'].astype(np.float64), inputs(c)['dz']
    assert np.array_equal(w, np.round(w)) and np.array_equal(dz, np.round(dz)) and 9 * 32 * np.abs(w).max() * np.abs(dz).max() < 2 ** 24
    # asymmetric in ky, kx, ci and co: a mirrored or transposed tap changes the result
    assert not np.array_equal(w, w[:, ::-1]) and not np.array_equal(w, w[:, :, ::-1])
    assert not np.array_equal(w, w[..., ::-1, :]) and not np.array_equal(w, w[..., ::-1])
    assert not np.array_equal(w, np.swapaxes(w, 1, 2))


def test_pack_cases_hold_every_edge():
  for shape in ((3, 0, 4), (3, 1, 4), (4, 0, 4), (3, 1, 8), (1, 2, 3)):
    _need('(C1, C2, Cpad) = %s' % (shape,), [c for c in PACK if (c.C1, c.C2, c.Cpad) == shape])
  for HW in (1, 255, 256, 257):
    _need('HW = %d' % HW, [c for c in PACK if c.HW == HW])
  _need('strided sample views', [c for c in PACK if c.K > 1])
  _need('only d_src', [c for c in PACK if c.form == 'src'])
  _need('only d_src2', [c for c in PACK if c.form == 'src2'])
  _need('C2 = 1 with d_src2 null', [c for c in PACK if c.form == 'c2_null' and c.C2 == 1])
  for acc in ((0, 0), (1, 0), (0, 1), (1, 1)):
    _need('(accumulate, accumulate2) = %s' % (acc,), [c for c in PACK if c.form == 'both' and c.acc == acc])
  _need('Cpad > C1 + C2', [c for c in PACK if c.Cpad > c.C1 + c.C2])
  for c in PACK:
    g = inputs(c)['g']
    used = np.zeros(c.Cpad, bool)
    if c.form != 'src2':
      used[:c.C1] = True
    if c.form in ('both', 'src2'):
      used[c.C1:c.C1 + c.C2] = True
    assert np.isnan(g[..., ~used]).all() and not np.isnan(g[..., used]).any(), c.id      # NaN in every channel >= C1 + C2 (and unread)


def test_dynimg_cases_hold_every_edge():
  geo = {c.index: R.dyn_geometry(c) for c in DYN}
  V = lambda c: geo[c.index]['V']
  _need('dynimg_bwd_*_kernel<4> at the dense aligned layout', [c for c in DYN if V(c) == 4 and not c.lay])
  # (dense strides are multiples of HW * C: they fail the test with it, and the layout gives no reason of its own)
  _need('<1> by HW * C = 75', [c for c in DYN if 'total' in geo[c.index]['reasons'] and not c.lay and geo[c.index]['total'] == 75])
  for reason in ('sample_stride', 'frame_stride', 'd_sample_stride', 'd_frame_stride', 'frames', 'd_frames', 'frames2', 'd_frames2'):
    own = [c for c in DYN if geo[c.index]['reasons'] == {reason}]
    _need('<1> by %s alone' % reason, own)
    assert any(c.twin for c in own), reason      # ... with the same values through <4> as well
  c = [c for c in DYN if geo[c.index]['reasons'] == {'sample_stride'}][0]
  assert geo[c.index]['ss'] % 4 == 2 and geo[c.index]['total'] % 4 == 0
  for c in DYN:
    if c.twin:
      assert geo[c.index]['V'] == 1 and 'total' not in geo[c.index]['reasons'] and R.dyn_geometry(R.dense_twin(c))['V'] == 4
  # blocks
  for v in (4, 1):
    for nblk in (1, 2, 5):
      _need('V = %d, nblk = %d' % (v, nblk), [c for c in DYN if V(c) == v and geo[c.index]['nblk'] == nblk])
    unit = 256 * v
    _need('V = %d: exactly one block' % v, [c for c in DYN if V(c) == v and geo[c.index]['total'] == unit])
    _need('V = %d: one unit more' % v, [c for c in DYN if V(c) == v and geo[c.index]['total'] == unit + v])
    _need('V = %d: a ragged last block' % v, [c for c in DYN if V(c) == v and geo[c.index]['nblk'] > 2 and geo[c.index]['total'] % unit])
    uniq = [c for c in DYN if V(c) == v and c.kind == 'planted' and all(len(p) == 1 for p in c.mins + c.maxs)]
    blk = lambda c, pos: pos[0] // (256 * V(c))
    last = lambda c: geo[c.index]['nblk'] - 1
    _need('V = %d: min and max in one block' % v, [c for c in uniq if geo[c.index]['nblk'] >= 1 and blk(c, c.mins[0]) == blk(c, c.maxs[0])])
    _need('V = %d: min and max in different blocks' % v, [c for c in uniq if blk(c, c.mins[0]) != blk(c, c.maxs[0])])
    _need('V = %d: an extremum in the last ragged block' % v,
          [c for c in uniq if geo[c.index]['total'] % unit and last(c) > 0 and last(c) in (blk(c, c.mins[0]), blk(c, c.maxs[0]))])
    _need('V = %d: min in block 0, max in the last' % v, [c for c in uniq if last(c) > 0 and blk(c, c.mins[0]) == 0 and blk(c, c.maxs[0]) == last(c)])
    _need('V = %d: nothing planted (the recomputed extrema)' % v, [c for c in DYN if V(c) == v and c.kind == 'random'])
  # ties
  planted = [c for c in DYN if c.kind == 'planted']
  blocks = lambda c, pos: {p // (256 * V(c)) for p in pos}
  _need('two maxima in one block', [c for c in planted if len(c.maxs[0]) == 2 and len(blocks(c, c.maxs[0])) == 1])
  _need('two maxima in different blocks', [c for c in planted if len(c.maxs[0]) == 2 and len(blocks(c, c.maxs[0])) == 2])
  _need('three minima over three blocks', [c for c in planted if len(c.mins[0]) == 3 and len(blocks(c, c.mins[0])) == 3])
  _need('a tie for both extrema at once', [c for c in planted if len(c.mins[0]) > 1 and len(c.maxs[0]) > 1])
  for v in (4, 1):
    _need('V = %d: the flat sample' % v, [c for c in DYN if V(c) == v and c.kind == 'flat' and c.K > 1])
  # shapes
  for K in (1, 2, 3, 4, 16, R.DYN_MAXK):
    _need('K = %d' % K, [c for c in DYN if c.K == K and not c.two])
  _need('K = 1 under accumulate', [c for c in DYN if c.K == 1 and c.acc[0]])
  _need('K = 3 under accumulate', [c for c in DYN if c.K == 3 and c.acc[0]])
  for shape in ((1, 3), (2, 4), (3, 4), (4, 4), (3, 8), (4, 8)):
    _need('(C, Cpad) = %s' % (shape,), [c for c in DYN if (c.C, c.Cpad) == shape])
  for N in (1, 3):
    _need('N = %d' % N, [c for c in DYN if c.N == N])
  for c in DYN:
    if c.N == 3:      # each sample with its extrema in different blocks
      assert all(blocks(c, c.mins[n]) != blocks(c, c.maxs[n]) for n in range(3)), c.id
  two = [c for c in DYN if c.two]
  for outs in ('both', 'd1', 'd2'):
    _need('two-frame form, outputs: %s' % outs, [c for c in two if c.outs == outs])
  for acc in ((0, 0), (1, 0), (0, 1), (1, 1)):
    _need('two-frame form, (accumulate, accumulate2) = %s' % (acc,), [c for c in two if c.outs == 'both' and c.acc == acc])
  assert all(geo[c.index]['total'] <= 6000 for c in DYN)


def test_workspace_is_the_entry_points_formula():
  from geeco_amd import _native
  lib = ctypes.CDLL(_native.LIB_PATH)
  lib.geeco_dynimg_bwd_ws_bytes.restype = ctypes.c_int64
  lib.geeco_dynimg_bwd_ws_bytes.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int]
  for c in DYN:
    geo = R.dyn_geometry(c)
    assert lib.geeco_dynimg_bwd_ws_bytes(c.N, c.HW, c.C) == geo['ws_bytes'], c.id
    assert geo['rec_floats'] * 4 <= geo['ws_bytes'] and geo['ws_bytes'] % 16 == 0, c.id


def test_dynimg_input_conditions():
  for c in DYN:
    inp = inputs(c)      # (check_dyn_inputs ran inside: margins, positions, bitwise ties)
    R.check_dyn_inputs(c, inp['frames'])
    assert np.isnan(inp['gp'][..., c.C:]).all() and np.array_equal(inp['gp'][..., :c.C].reshape(c.N, -1), inp['g']), c.id
    if c.kind != 'flat':
      assert R.extrema_margin(inp['frames']) >= R.MARGIN or any(len(p) > 1 for p in c.mins + c.maxs), c.id
    for n, pos in [(n, p) for n in range(c.N) for p in ((c.mins or [[]] * c.N)[n], (c.maxs or [[]] * c.N)[n]) if len(p) > 1]:
      assert len(set(inp['g'][n, pos].tolist())) == 1      # equal g at tied elements: their outputs are bitwise equal
    a = R.alpha64(c.K)
    assert (a == 0).any() == (c.K == 1)      # (the reference's coefficients: only K = 1 has a zero one; K = 3 is (-4/3, 2/3, 2/3))


def _f32(d):
  return {k: v.astype(np.float32) for k, v in d.items()}


@pytest.mark.parametrize('c', DYN, ids=lambda c: c.id)
def test_dynimg_reference_passes_and_is_the_restatement(c):
  inp = inputs(c)
  d = R.dyn_eval(c, inp)
  ref = R.input_grad_reference(c, inp)
  worst, problems = R.input_grad_compare(c, _f32(R.dyn_split(c, d)), ref)
  assert not problems and max(worst.values()) <= 1, (c.id, problems)
  # the element-wise restatement is dynimg_bwd_ref (whose tensordot may order its sums differently: to 1e-12 of the largest)
  full = R.dynimg_bwd_ref(inp['g'], inp['frames'])
  if c.K > 1 and not any(len(p) > 1 for p in (c.mins or []) + (c.maxs or [])) and c.kind != 'flat':
    assert np.abs(full - d).max() <= 1e-12 * np.abs(d).max()
  if c.K == 1:
    assert not d.any() and not full.any()
  # every bound is a small multiple of its element: a bound that swallows a relative 1e-5 would prove nothing
  for k, r in ref.items():
    ordinary = ~r['eq'] & (np.abs(r['val']) > 0)
    if c.kind == 'planted':
      assert (r['bound'][ordinary] > 0).all()


@pytest.mark.parametrize('c', CONV + PACK, ids=lambda c: c.id)
def test_conv1_and_pack_references_pass(c):
  inp = inputs(c)
  ref = R.input_grad_reference(c, inp)
  worst, problems = R.input_grad_compare(c, {k: r['val'].astype(np.float32) for k, r in ref.items()}, ref)
  assert not problems and max(worst.values()) <= 1, (c.id, problems)
  if c.entry == 'pack':      # a stale copy (the accumulate flag ignored) and a channel shifted by one are both seen
    for k, r in ref.items():
      start = (inp['a0'] if k == 'd_src' else inp['b0']).copy()
      if not np.array_equal(start.astype(np.float64), r['val']):
        assert R.input_grad_compare(c, {kk: (start if kk == k else rr['val'].astype(np.float32)) for kk, rr in ref.items()}, ref)[1]


@pytest.mark.parametrize('mistake', R.CONV_MISTAKES)
def test_conv1_mistakes_are_rejected(mistake):
  hit = 0
  for c in CONV:
    if mistake == 'halo-column-zeroed' and c.W <= R.C1D_TX:
      continue      # one tile per row: no seam
    if c.H * c.W == 1 and mistake == 'kx-mirrored':
      continue      # a single pixel sees the centre tap alone
    inp = inputs(c)
    wrong = R.conv1_eval(c, inp, mistake).astype(np.float32)
    _, problems = R.input_grad_compare(c, dict(dx=wrong), R.input_grad_reference(c, inp))
    assert problems, (mistake, c.id)
    hit += 1
  assert hit >= 4


@pytest.mark.parametrize('mistake', R.DYN_MISTAKES)
def test_dynimg_mistakes_are_rejected(mistake):
  """Each emulated wrong kernel, in every case it touches.  'ordinary-rel-1e-5' (every ordinary element off by a relative 1e-5)
  is the one that PASSES the rel_max / rel_l2 <= 2e-5 test of tests/test_input_grad_gpu.py -- asserted below -- since both norms are
  relative to the extremum elements, tens of times larger than an ordinary one."""
  hit = []
  for c in DYN:
    inp = inputs(c)
    wrong = R.dyn_eval(c, inp, mistake)
    if wrong is None:
      continue
    ref = R.input_grad_reference(c, inp)
    _, problems = R.input_grad_compare(c, _f32(R.dyn_split(c, wrong)), ref)
    assert problems, (mistake, c.id)
    hit.append(c.id)
    if mistake == 'ordinary-rel-1e-5':
      right = R.dyn_eval(c, inp)
      assert T.rel_max(wrong, right) <= T.GRAD_TOL and T.rel_l2(wrong, right) <= T.GRAD_TOL, c.id      # today's test lets it through
  print('%s: rejected in %d cases, first %s' % (mistake, len(hit), hit[:3]))
  assert len(hit) >= (1 if mistake == 'cpad4-for-8' else 3), (mistake, hit)
