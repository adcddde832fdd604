"""The opt-in per-variable statistics on the GPU: the two launches of csrc/varstats.hip against the float64 restatement
tests/_varstats_ref.py, the model's ``variable_stats()`` against the arenas copied to the host, and the Estimator surface on top.

Counts, extrema and classes are integers or selections: they must be EXACTLY the reference's.  Roundings of the float32 sums
(U = 2^-24 each), counted from the reduction order csrc/varstats.hip documents, longest path:
  a term             G = g * grad_scale is one rounded product (1 U on G, 2 U on G^2); the square itself is not rounded on its own (one
                     FMA per element adds it to the running sum).  A parameter is exact.  u = m / (sqrtf(v) + eps) is a square root, a
                     sum and a quotient, 3 U on u and 6 U on u^2, + 1 U for every second-order term: TERM = 2 (gradient), 0 (parameter),
                     7 (update) for a sum of squares; 1, 0 for a signed sum
  inside a chunk     16 serial additions per thread (4 float4s) + 6 levels of the wave butterfly + 3 additions of the 4 wave sums = 25
  over the chunks    ceil(chunks of the variable / 256) serial additions per thread + 6 + 3
Every term of a sum of squares is >= 0, so the bound is relative to the sum: ((1 + U)^count - 1) S; for a signed sum it is relative to
the sum of magnitudes.  The largest variable here (70 001 elements, 18 chunks) has count = 7 + 25 + 10 = 42: 2.5e-6, below the 1e-5
the clipping feature promises for its norm.

A half-covered variable is NOT refused: its uncovered elements have no gradient and are in none of the gradient's fields
(``grad_covered`` counts the others), as include/geeco_hip.h documents.
"""
import json
import os

import numpy as np
import pytest
import torch

import _guard_ref as G
import _primitive_refs as R
import _varstats_ref as V

pytestmark = pytest.mark.gpu

NAN = float('nan')
U = R.U
CH = 4096
IN_CHUNK = 16 + 6 + 3
COUNTS = [1, 3, 4, 5, CH - 1, CH, CH + 1, 3 * CH + 7, 70001]
EPS = 1e-8
GSCALE = 0.3            # no power of two: the product rounds

_CASES = {}


def _bound(count, scale):
  return ((1.0 + U) ** count - 1.0) * scale


def _roundings(term, n):
  return term + IN_CHUNK + (-(-(-(-n // CH)) // 256) + 6 + 3)


def _table(nvar):
  """(variables, arena size): counts cycling through COUNTS (rotated so that a table of 5 holds the tails), 0 / 4 / 8 pad floats between."""
  variables, off = [], 0
  for i in range(nvar):
    cnt = COUNTS[(i * 4 + 2) % len(COUNTS)] if nvar > 1 else 70001
    variables.append((off, cnt))
    off = -(-(off + cnt) // 4) * 4 + 4 * (i % 3)
  return variables, off + 4


def _case(nvar):
  """The table and p, g, m, v as numpy float32 with NaN in every pad, once per size and left unchanged.  One gradient in 7 is an exact
  zero, one in 11 of those a -0.0."""
  if nvar not in _CASES:
    variables, n = _table(nvar)
    r = np.random.default_rng(3000 + nvar)
    arenas = [np.full(n, np.nan, np.float32) for _ in range(4)]
    for off, cnt in variables:
      p, g, m = (r.standard_normal(cnt).astype(np.float32) for _ in range(3))
      g *= np.float32(0.1)
      g[::7] = 0.0
      g[::77] = -0.0
      v = (r.standard_normal(cnt).astype(np.float32) * np.float32(0.1)) ** 2
      for a, x in zip(arenas, (p, g, m * np.float32(0.1), v)):
        a[off:off + cnt] = x
    _CASES[nvar] = (variables, n) + tuple(arenas)
  return _CASES[nvar]


def _dev(dev, a, slack=5):
  t = torch.full((a.size + slack,), NAN, dtype=torch.float32, device=dev)
  t[:a.size] = torch.from_numpy(a)
  return t


def _run(dev, variables, n, p, m, v, segments, gscale=GSCALE, eps=EPS):
  """The two launches into buffers with slack behind them that must come back untouched; the records as numpy."""
  from geeco_amd import ops
  table_h = ops.variable_stats_table(variables)
  nch = (table_h.size - 2 * len(variables)) // 2
  table = torch.from_numpy(table_h).to(dev)
  ws_words = ops.variable_stats_ws_bytes(nch) // 4
  ws = torch.full((ws_words + 4,), 0x5a5a5a5a, dtype=torch.int32, device=dev)
  nbytes = len(variables) * ops.VARSTATS_DTYPE.itemsize
  out = torch.full((nbytes + 16,), 0xab, dtype=torch.uint8, device=dev)
  ops.variable_stats(out, ws, table, p, m, v, segments, n, variables, nch, grad_scale=gscale, eps=eps)
  torch.cuda.synchronize()
  assert bool((ws[ws_words:] == 0x5a5a5a5a).all()) and bool((out[nbytes:] == 0xab).all())
  for t in (p, m, v):
    assert torch.isnan(t[n:]).all()
  return out[:nbytes].cpu().numpy().view(ops.VARSTATS_DTYPE).copy()


def _check_tensor(got, want, n, term_sq, term_sum, what):
  assert int(got['nonfinite']) == want['nonfinite'] and int(got['zeros']) == want['zeros'], what
  np.testing.assert_array_equal(got['neg'], want['neg'], err_msg=str(what))
  np.testing.assert_array_equal(got['pos'], want['pos'], err_msg=str(what))
  assert float(got['min']) == want['min'] and float(got['max']) == want['max'], what
  c_sq, c_sum = _roundings(term_sq, n), _roundings(term_sum, n)
  assert c_sq * U < 1e-5, c_sq
  assert abs(float(got['sumsq']) - want['sumsq']) <= _bound(c_sq, want['sumsq']), (what, float(got['sumsq']), want['sumsq'], c_sq)
  assert abs(float(got['sum']) - want['sum']) <= _bound(c_sum, want['abs_sum']), (what, float(got['sum']), want['sum'], c_sum)


def _check_records(recs, variables, p0, g0, m0, v0, covered, gscale=GSCALE, eps=EPS):
  worst = 0.0
  for i, ((off, cnt), rec) in enumerate(zip(variables, recs)):
    sl = slice(off, off + cnt)
    want = V.record(g0[sl], covered[sl], p0[sl], m0[sl], v0[sl], gscale, eps)
    assert int(rec['grad_covered']) == want['grad_covered'], i
    _check_tensor(rec['grad'], want['grad'], cnt, 2, 1, ('gradient', i, cnt))
    _check_tensor(rec['param'], want['param'], cnt, 0, 0, ('parameter', i, cnt))
    wu, c = want['update'], _roundings(7, cnt)
    assert int(rec['update_nonfinite']) == wu['nonfinite'], i
    assert abs(float(rec['update_sumsq']) - wu['sumsq']) <= _bound(c, wu['sumsq']), (i, cnt, float(rec['update_sumsq']), wu['sumsq'])
    assert abs(float(rec['update_max_abs']) - wu['max_abs']) <= _bound(4, wu['max_abs']), (i, cnt)
    if want['grad']['sumsq'] > 0:
      worst = max(worst, abs(float(rec['grad']['sumsq']) - want['grad']['sumsq']) / want['grad']['sumsq'] / U)
  return worst


# ================================================================================================
# kernels
# ================================================================================================
@pytest.mark.parametrize('nvar', [1, 5, 64])
def test_records_against_float64(dev, nvar):
  """Every field of every record against the restatement; the pads between the variables and the slack behind every buffer are NaN and
  stay out of everything (a read of one would show in a count or poison a sum)."""
  variables, n, p0, g0, m0, v0 = _case(nvar)
  assert sorted({c for _, c in variables}) == sorted(set(COUNTS)) or nvar < 9
  p, g, m, v = (_dev(dev, a) for a in (p0, g0, m0, v0))
  recs = _run(dev, variables, n, p, m, v, [(g, 0, n)])
  covered = np.ones(n, bool)
  worst = _check_records(recs, variables, p0, g0, m0, v0, covered)
  print('nvar=%d: %d floats; the gradient sum of squares is off by at most %.2f U' % (nvar, n, worst))
  for rec in recs:
    assert int(rec['grad']['nonfinite']) == 0 and int(rec['param']['nonfinite']) == 0 and int(rec['update_nonfinite']) == 0
  assert sum(int(r['grad']['zeros']) for r in recs) == sum(len(range(0, c, 7)) for _, c in variables)
  # a power-of-two scale is exact: the gradient's terms then round like the parameter's
  recs1 = _run(dev, variables, n, p, m, v, [(g, 0, n)], gscale=1.0)
  _check_records(recs1, variables, p0, g0, m0, v0, covered, gscale=1.0)


def _special_values():
  f = np.float32
  edges = [f(2.0) ** f(e) for e in range(-33, 9)]
  below = [np.nextafter(x, f(0.0)) for x in edges]
  vals = [f(np.nan), f(np.inf), f(-np.inf), f(-0.0), f(0.0), f(1e-45), f(-1e-45), f(1e-39), f(127.9), f(-127.9)]
  vals += edges + below + [-x for x in edges] + [-x for x in below]
  return np.array(vals, np.float32)


def test_special_values_are_counted_exactly_and_poison_nothing(dev):
  """NaN, +-Inf, -0.0, denormals and both sides of every class edge at the first, last and tail positions of the 4097-element variable
  (the last one alone in its chunk), in the gradient and in the parameters: counts and classes exact, the sums those of the other
  elements, and the records of the neighbouring variables bit for bit what they were."""
  variables, n, p0, g0, m0, v0 = _case(5)
  target = next(i for i, (_, c) in enumerate(variables) if c == CH + 1)
  off, cnt = variables[target]
  vals = _special_values()
  k = vals.size // 2
  pos = np.concatenate([np.arange(k), cnt - (vals.size - k) + np.arange(vals.size - k)])      # the first elements; the last ones, chunk tail included
  assert pos.size == vals.size and pos.max() == cnt - 1 and len(set(pos)) == pos.size and CH in pos and CH - 1 in pos
  g1, p1 = g0.copy(), p0.copy()
  g1[off + pos] = vals
  p1[off + pos[::-1]] = vals
  p, g, m, v = (_dev(dev, a) for a in (p0, g0, m0, v0))
  before = _run(dev, variables, n, p, m, v, [(g, 0, n)], gscale=1.0)
  p, g = _dev(dev, p1), _dev(dev, g1)
  after = _run(dev, variables, n, p, m, v, [(g, 0, n)], gscale=1.0)
  covered = np.ones(n, bool)
  _check_records(after, variables, p1, g1, m0, v0, covered, gscale=1.0)
  rec = after[target]
  for t in (rec['grad'], rec['param']):
    assert int(t['nonfinite']) == 3 and int(t['zeros']) >= 2
    assert np.isfinite(float(t['sum'])) and np.isfinite(float(t['sumsq'])) and float(t['max']) == 256.0 and float(t['min']) == -256.0
  # ... as if the planted non-finite elements were absent: the reference of the variable with them deleted
  keep = np.ones(cnt, bool)
  keep[pos[:3]] = False
  assert not np.isfinite(g1[off + pos[:3]]).any()
  want = V.tensor(g1[off:off + cnt][keep])
  assert want['nonfinite'] == 0 and abs(float(rec['grad']['sumsq']) - want['sumsq']) <= _bound(_roundings(0, cnt), want['sumsq'])
  for i in range(len(variables)):
    if i != target:
      assert before[i].tobytes() == after[i].tobytes(), i
  assert before[target].tobytes() != after[target].tobytes()


N5 = _table(5)[1]


def _cuts(k):
  """k pieces of [0, N5) cut at offsets that are no multiples of 4 and lie inside variables, in a shuffled order."""
  variables, n = _table(5)
  at = sorted(set(int(0.93 * n * j / k) | 1 for j in range(1, k)))      # odd offsets
  assert len(at) == k - 1 and any(off < a < off + cnt for a in at for off, cnt in variables)
  bounds = [0] + at + [n]
  pieces = [(a, b - a) for a, b in zip(bounds, bounds[1:])]
  return pieces[1::2] + pieces[0::2]


def _pieces(dev, g, g0, cuts, own):
  out = []
  for i, (off, cnt) in enumerate(cuts):
    src = torch.from_numpy(g0[off:off + cnt].copy()).to(dev) if i == own else g[off:off + cnt]
    out.append((src, off, cnt))
  return out


@pytest.mark.parametrize('k', [2, 3, 8])
def test_any_partition_of_the_gradient_gives_the_same_records(dev, k):
  """Bit for bit the one-piece records, whatever the cuts, the order of the pieces and where a piece's gradients live; and the same
  bits from call to call."""
  variables, n, p0, g0, m0, v0 = _case(5)
  p, g, m, v = (_dev(dev, a) for a in (p0, g0, m0, v0))
  one = _run(dev, variables, n, p, m, v, [(g, 0, n)])
  again = _run(dev, variables, n, p, m, v, [(g, 0, n)])
  assert one.tobytes() == again.tobytes()
  cuts = _cuts(k)
  assert len(cuts) == k and sum(c for _, c in cuts) == n and any(o % 4 for o, _ in cuts)
  for own in (0, k - 1):
    got = _run(dev, variables, n, p, m, v, _pieces(dev, g, g0, cuts, own))
    assert got.tobytes() == one.tobytes(), (k, own)


def test_uncovered_and_half_covered_variables(dev):
  """A variable no piece touches has grad_covered == 0 and empty gradient fields, its parameter and update fields those of the full
  call; a half-covered variable is not refused: its record describes the covered elements."""
  variables, n, p0, g0, m0, v0 = _case(5)
  p, g, m, v = (_dev(dev, a) for a in (p0, g0, m0, v0))
  full = _run(dev, variables, n, p, m, v, [(g, 0, n)])
  absent, half = 1, 3
  (o1, c1), (o3, c3) = variables[absent], variables[half]
  mid = o3 + c3 // 2 + 1
  segments = [(g[:o1], 0, o1), (g[o1 + c1:mid], o1 + c1, mid - o1 - c1), (g[o3 + c3:n], o3 + c3, n - o3 - c3)]
  covered = np.zeros(n, bool)
  for _, o, c in segments:
    covered[o:o + c] = True
  got = _run(dev, variables, n, p, m, v, segments)
  _check_records(got, variables, p0, g0, m0, v0, covered)
  a = got[absent]
  assert int(a['grad_covered']) == 0 and float(a['grad']['sum']) == 0.0 and float(a['grad']['sumsq']) == 0.0
  assert float(a['grad']['min']) == np.inf and float(a['grad']['max']) == -np.inf and int(a['grad']['neg'].sum() + a['grad']['pos'].sum()) == 0
  assert a['param'].tobytes() == full[absent]['param'].tobytes() and float(a['update_sumsq']) == float(full[absent]['update_sumsq'])
  assert 0 < int(got[half]['grad_covered']) == mid - o3 < c3
  for i in (0, 2, 4):
    assert got[i].tobytes() == full[i].tobytes(), i


def test_bad_arguments_launch_nothing(dev):
  from geeco_amd import _native, ops
  variables, n, p0, g0, m0, v0 = _case(5)
  p, g, m, v = (_dev(dev, a) for a in (p0, g0, m0, v0))
  table_h = ops.variable_stats_table(variables)
  nch = (table_h.size - 10) // 2
  table = torch.from_numpy(table_h).to(dev)
  ws = torch.zeros(ops.variable_stats_ws_bytes(nch) // 4, dtype=torch.int32, device=dev)
  out = torch.full((5 * ops.VARSTATS_DTYPE.itemsize,), 0xab, dtype=torch.uint8, device=dev)
  seg = [(g, 0, n)]

  def refused(match, **kw):
    a = dict(out=out, ws=ws, table=table, p=p, m=m, v=v, segments=seg, n=n, variables=variables, nchunks=nch)
    a.update(kw)
    with pytest.raises(_native.GeecoNativeError, match=match):
      ops.variable_stats(**a)

  for null in ('out', 'ws', 'table', 'p', 'm', 'v'):
    refused('null pointer', **{null: None})
  refused('aligned', p=p[1:])
  refused('multiple of 4', variables=[(variables[0][0] + 2, 1)] + variables[1:])
  refused('overlap', variables=variables[:1] + [(variables[1][0], variables[2][0] - variables[1][0] + 4)] + variables[2:])
  refused('outside the arena', variables=variables[:4] + [(variables[4][0], n)])
  refused('chunks', nchunks=nch - 1)
  refused('outside the arena', segments=[(g, 4, n)])
  refused('overlap', segments=[(g, 0, 8), (g, 4, 8)])
  refused('eps', eps=-1.0)
  with pytest.raises((ValueError, _native.GeecoNativeError)):      # nvar < 1
    ops.variable_stats(out, ws, table, p, m, v, seg, n, [], 0)
  lib = _native.load()
  import ctypes
  nine = (_native.AdamSegment * 9)()
  for i in range(9):
    nine[i].g, nine[i].p_off, nine[i].count = g.data_ptr(), 4 * i, 4
  offs, cnts = (ctypes.c_int64 * 5)(*[o for o, _ in variables]), (ctypes.c_int64 * 5)(*[c for _, c in variables])
  vp = lambda t: ctypes.c_void_p(t.data_ptr())
  for nseg, nvar in ((9, 5), (0, 5), (1, 0), (1, -1)):
    rc = lib.geeco_variable_stats(vp(p), vp(m), vp(v), nine, nseg, n, 1.0, 1e-8, offs, cnts, nvar, vp(table), nch, vp(ws), vp(out), None)
    assert rc == _native.GEECO_EINVAL, (nseg, nvar)
  torch.cuda.synchronize()
  assert bool((out == 0xab).all()) and bool((ws == 0).all())


# ================================================================================================
# through the model
# ================================================================================================
def _tensors(d):
  return {k: torch.from_numpy(v) for k, v in d.items()}


# e2e_vmc and the goal model of tests/_guard_ref.py (batch 4), and geeco-f at the smallest shape tests/test_model_gpu.py runs it at
# (three encoders behind the one-pass input stage, K = 3, 136 x 136, batch 2)
MODELS = list(G.MODELS) + ['geeco-f']
_MODEL_CASES = {}


def _model_case(name):
  """(cfg, goal, P, feats, labels), once per model and left unchanged."""
  if name in G.MODELS:
    return G.case(name)[1:]
  if name not in _MODEL_CASES:
    from geeco_amd.params import create_e2evmc_config
    from oracle import geeco_oracle as O
    ocfg = O.make_config(window_size=3, img_height=136, img_width=136, batch_size=2, lr=1e-3, proc_obs='dynimg', proc_tgt='dyndiff')
    P = O.init_params(O.model_param_shapes(ocfg, True), seed=1)
    feats, labels = O.synthetic_batch(ocfg, True, 2, seed=3, H=136, W=136)
    _MODEL_CASES[name] = (create_e2evmc_config(ocfg._asdict()), True, P, feats, labels)
  return _MODEL_CASES[name]


def _model(dev, name, feats=None, **kw):
  from geeco_amd import graph
  cfg, goal, P, f, labels = _model_case(name)
  model = (graph.GoalE2EVMC if goal else graph.E2EVMC)(cfg, f['rgb'].shape[0], dev, training=True, **kw)
  model.store.load_numpy(P)
  model.load_batch(_tensors(f if feats is None else feats), _tensors(labels))
  return model


def _host(model):
  s = model.store
  return {k: getattr(s, k).detach().cpu().numpy().copy() for k in ('params', 'grads', 'adam_m', 'adam_v')}


def _check_model_stats(model, stats, before, multipliers=None, applied=True):
  """``stats`` against float64 from the arenas on the host; ``before``: the parameters before the step."""
  s, h = model.store, _host(model)
  lr_t = float(model.scal[0])
  assert list(stats) == list(s.shapes)
  for name, d in stats.items():
    off, cnt = s.offsets[name], int(np.prod(s.shapes[name]))
    sl = slice(off, off + cnt)
    mul = 1.0 if multipliers is None else multipliers[name]
    want = V.record(h['grads'][sl], np.ones(cnt, bool), h['params'][sl], h['adam_m'][sl], h['adam_v'][sl], 1.0, EPS)
    rel = lambda term: _bound(_roundings(term, cnt), 1.0)
    wn = np.sqrt(want['param']['sumsq'])
    assert abs(d['weight_norm'] - wn) <= rel(0) * wn and d['weight_nonfinite'] == 0, name
    assert d['weight_max_abs'] == max(abs(want['param']['min']), abs(want['param']['max'])), name
    if mul == 0.0:
      assert d['grad_norm'] is None and d['grad_nonfinite'] is None and d['update_norm'] == 0.0, name
      continue
    gn = np.sqrt(want['grad']['sumsq'])
    assert abs(d['grad_norm'] - gn) <= rel(0) * gn and d['grad_nonfinite'] == want['grad']['nonfinite'], name      # grad_scale = 1: exact terms
    assert d['grad_zero_fraction'] == want['grad']['zeros'] / cnt, name
    assert d['grad_max_abs'] == max(abs(want['grad']['min']), abs(want['grad']['max'])), name
    assert abs(d['grad_mean'] * cnt - want['grad']['sum']) <= _bound(_roundings(0, cnt), want['grad']['abs_sum']) + 1e-12 * want['grad']['abs_sum'], name
    if not applied:
      assert d['update_norm'] == 0.0, name
      continue
    un = lr_t * mul * np.sqrt(want['update']['sumsq'])
    assert abs(d['update_norm'] - un) <= rel(7) * un, (name, d['update_norm'], un)
    # the step Adam just took: p' = fl(p - fl(fl(lr m) / fl(fl(sqrt v) + eps))): the quotient is lr u within 4 U (one more with a
    # multiplier, lr_k = fl(lr mul)), the difference rounds once more, by at most U |p'| <= U (|p| + |lr u|) per element.
    # Hence | ||p' - p|| - update_norm | <= 2 U ||p|| + (roundings of the sum + 5) U update_norm.
    moved = np.linalg.norm(h['params'][sl].astype(np.float64) - before[sl].astype(np.float64))
    bound = 2.0 * U * np.linalg.norm(before[sl].astype(np.float64)) + _bound(_roundings(7, cnt) + 5, un)
    assert abs(moved - d['update_norm']) <= bound, (name, moved, d['update_norm'], bound)
    if wn > 0:
      assert d['update_ratio'] == d['update_norm'] / d['weight_norm'], name


@pytest.mark.parametrize('name', MODELS)
def test_model_statistics_after_one_step(dev, name):
  """One training step: every variable's statistics against float64 from the arenas copied to the host, and update_norm against
  ||p_after - p_before||; then the same step with the gradient in pieces, as backward_and_apply hands the early and the late bucket to
  the optimiser beside the fused encoder bottom: the recorded pieces give the same statistics, checked against the host again."""
  model = _model(dev, name, variable_stats='histograms')
  with pytest.raises(RuntimeError, match='no optimiser step'):
    model.variable_stats()
  before = model.store.params.detach().cpu().numpy().copy()
  model.train_step()
  stats = model.variable_stats()
  _check_model_stats(model, stats, before)
  assert stats == model.variable_stats()      # asking changes nothing
  for n, d in stats.items():
    cnt = int(np.prod(model.store.shapes[n]))
    assert d['histograms']['weights']['num'] == cnt and d['histograms']['gradients']['num'] == cnt
    hw = d['histograms']['weights']
    assert sum(hw['neg']) + sum(hw['pos']) + hw['zeros'] == cnt
  off = _model(dev, name)
  assert off.stats_plan is None and off.step_pieces is None
  with pytest.raises(RuntimeError, match='variable_stats'):
    off.variable_stats()
  # the step in two pieces beside the encoder bottom: the same statistics from the recorded pieces
  from geeco_amd.runtime import gradient_buckets
  twin = _model(dev, name, variable_stats=True)
  early, late = gradient_buckets(twin.store)
  before_twin = twin.store.params.detach().cpu().numpy().copy()
  twin.forward(backward_too=True)
  twin.backward_and_apply(early, late)
  assert len(twin.step_pieces) == len(early) + len(late) > 1
  assert [q[1:] for q in twin.step_pieces] == [tuple(x) for x in list(early) + list(late)]
  if name == 'geeco-f':
    assert len(twin.step_pieces) > 2 and len(model.store.shapes) == 60      # three encoders: their conv1 / conv2 are pieces of their own
  got = twin.variable_stats()
  _check_model_stats(twin, got, before_twin)
  for n in stats:
    assert got[n] == {k: v for k, v in stats[n].items() if k != 'histograms'}, n


def test_model_statistics_on_shared_frames(dev):
  import test_shared_frames_gpu as SF
  from geeco_amd import graph
  from geeco_amd.params import create_e2evmc_config
  ocfg, goal, P, feats, labels, win, tgt, _ = SF._case(dev, 'goal residual', 'two episodes')
  F = 4 + 2 * (SF.K3 - 1) + 2
  table, index, tindex, _ = win.frame_table(F, tgt, dev)
  model = graph.GoalE2EVMC(create_e2evmc_config(ocfg._asdict()), 4, dev, training=True, shared_frames=F, variable_stats=True)
  model.store.load_numpy(P)
  f = {k: torch.from_numpy(v) for k, v in feats.items() if k not in ('rgb', 'target_rgb')}
  f.update(frame_table=torch.from_numpy(table), frame_index=torch.from_numpy(index), target_index=torch.from_numpy(tindex))
  model.load_batch(f, _tensors(labels))
  before = model.store.params.detach().cpu().numpy().copy()
  model.train_step()
  _check_model_stats(model, model.variable_stats(), before)


def test_multipliers_and_frozen_variables(dev):
  mults = {'LSTMDecoder/fc1/': 0.0, 'Encoder/': 0.1}
  model = _model(dev, 'e2e_vmc', variable_stats=True, lr_multipliers=mults)
  plain = _model(dev, 'e2e_vmc', variable_stats=True)
  before = model.store.params.detach().cpu().numpy().copy()
  model.train_step()
  plain.train_step()
  stats, ref = model.variable_stats(), plain.variable_stats()
  _check_model_stats(model, stats, before, multipliers=model.lr_multipliers)
  tenth = float(np.float32(0.1))
  seen = {0.0: 0, tenth: 0, 1.0: 0}
  for n, d in stats.items():
    mul = model.lr_multipliers[n]
    seen[mul] += 1
    if mul == 0.0:
      o, c = model.store.offsets[n], int(np.prod(model.store.shapes[n]))
      assert 'fc1' in n and d['grad_norm'] is None and d['update_norm'] == 0.0 and ref[n]['update_norm'] > 0.0
      assert np.array_equal(model.store.params[o:o + c].cpu().numpy(), before[o:o + c])      # frozen: it did not move (its weight_norm is checked above)
    else:
      # the same gradient, hence the same moments and the same sums: the multiplier is all that differs
      assert d['grad_norm'] == ref[n]['grad_norm'], n
      assert d['update_norm'] == pytest.approx(mul * ref[n]['update_norm'], rel=1e-12), n
  assert seen[0.0] == 2 and seen[tenth] == 16 and seen[1.0] > 0


def test_per_variable_norms_add_up_to_the_clipped_norm(dev):
  """clip_norm with l2 = 0: the sum of the per-variable grad_norm^2 is clip_out[1]^2 within the roundings of both reductions: the
  statistics' (25 + 10 for its largest variable, exact terms at grad_scale = 1) and the clipping's (25 + ceil(chunks / 256) + 9, + 1 for
  its square root, doubled by squaring it again, + 1 for the float32 norm squared on the host in float64: none)."""
  model = _model(dev, 'e2e_vmc', variable_stats=True, clip_norm=0.01)
  assert float(model.cfg.l2_regularizer) == 0.0
  model.train_step()
  stats = model.variable_stats()
  total = sum(d['grad_norm'] ** 2 for d in stats.values())
  norm = float(model.clip_out[1])
  largest = max(int(np.prod(s)) for s in model.store.shapes.values())
  count = _roundings(0, largest) + (IN_CHUNK + -(-model.clip_ws.numel() // 256) + 9) + 2
  print('sum of grad_norm^2 %.9g, clip_out[1]^2 %.9g, %d roundings allowed, off by %.2f U' % (total, norm * norm, count, abs(total - norm * norm) / total / U))
  assert abs(total - norm * norm) <= _bound(count, total)
  assert 0.0 < float(model.clip_out[0]) < 1.0


def test_a_nan_frame_is_traced_to_the_variable(dev):
  """skip_nonfinite with a NaN planted in one input frame: the step is skipped, update_norm is 0 everywhere, the first conv kernel of
  the encoder that saw the frame reports non-finite gradient elements, and the error of a limit of 1 names it."""
  from geeco_amd import estimator as est
  _, _, _, _, feats, _ = G.case('e2e_vmc')
  bad = {k: v.copy() for k, v in feats.items()}
  bad['rgb'][1, 0, 40, 50, 1] = np.nan
  model = _model(dev, 'e2e_vmc', feats=bad, variable_stats=True, skip_nonfinite=1)
  before = model.store.params.detach().clone()
  model.train_step()
  stats = model.variable_stats()
  assert model.guard.tolist() == [0, 1, 1] and torch.equal(before.view(torch.int32), model.store.params.view(torch.int32))
  assert all(d['update_norm'] == 0.0 for d in stats.values())
  first = 'VMC/ConvEncoder/conv1/kernel'
  assert stats[first]['grad_nonfinite'] > 0
  assert np.isfinite(stats[first]['weight_norm']) and stats[first]['weight_nonfinite'] == 0
  bad_vars = model.nonfinite_gradient_variables(stats)
  assert first in bad_vars and all(v > 0 for v in bad_vars.values())
  with pytest.raises(RuntimeError, match=r'nothing was saved; non-finite gradient elements of the last skipped step: .*%s: %d' % (first, bad_vars[first])):
    est.check_skipped_steps(model)
  # without the option the text is what it was
  twin = _model(dev, 'e2e_vmc', feats=bad, skip_nonfinite=1)
  twin.train_step()
  with pytest.raises(RuntimeError, match=r'in a row\); nothing was saved$'):
    est.check_skipped_steps(twin)


# ================================================================================================
# Estimator
# ================================================================================================
def _events(model_dir):
  return [json.loads(l) for l in open(os.path.join(model_dir, 'events.jsonl'))]


def _event_file(model_dir):
  from geeco_amd.tfrecord import read_records
  from test_variable_stats_cpu import _decode_event
  path = [os.path.join(model_dir, f) for f in os.listdir(model_dir) if f.startswith('events.out.tfevents')]
  assert len(path) == 1
  return [_decode_event(bytes(r)) for r in read_records(path[0], compression=None)]


class _CountingLibrary:
  def __init__(self, lib):
    self._lib, self.calls = lib, []

  def __getattr__(self, name):
    fn = getattr(self._lib, name)
    if not name.startswith('geeco_') or name == 'geeco_last_error' or name.endswith('_bytes') or name.endswith('_floats'):
      return fn

    def counted(*a):
      self.calls.append(name)
      return fn(*a)
    return counted


def test_estimator_logs_statistics_and_histograms(dev, tmp_path, monkeypatch):
  from geeco_amd import _native
  from geeco_amd import estimator as est
  from geeco_amd import input_fn as I
  from geeco_amd.params import create_e2evmc_config
  from geeco_amd.variables import model_variable_shapes
  root = str(tmp_path / 'ds')
  I.write_synthetic_dataset(root, 2, episode_length=9, img_hw=(G.H, G.H), seed=5)
  batches = list(I.pickplace_input_fn(root, 'default', 'train', window_size=G.K3, batch_size=4, num_threads=2))
  assert len(batches) == 3
  cfg = create_e2evmc_config(dict(window_size=G.K3, img_height=G.H, img_width=G.H, batch_size=4))
  shapes = model_variable_shapes(cfg, False)
  plain = {'e2evmc_config': cfg, 'log_steps': 2, 'debug': False}

  def run(tag, **extra):
    md = str(tmp_path / tag)
    est._SummarySaverHook._writers.pop(md, None)
    e = est.Estimator(est.e2evmc_model_fn, md, est.RunConfig(init_seed=4), dict(plain, **extra))
    e.train(input_fn=lambda: iter(batches))
    est._SummarySaverHook._writers.pop(md).close()
    return e, md

  e, md = run('on', variable_stats='histograms')
  ev = _events(md)
  assert [line['global_step'] for line in ev] == [2]
  assert list(ev[0]['variables']) == list(shapes) and 'nonfinite_variables' not in ev[0]
  for n, d in ev[0]['variables'].items():
    assert d['grad_norm'] > 0 and d['grad_nonfinite'] == 0 and d['update_norm'] > 0 and 'histograms' not in d, n
  records = _event_file(md)[1:]
  assert len(records) == 2
  tags = set(records[0]['scalars'])
  for n in shapes:
    assert {'grad_norm/' + n, 'weight_norm/' + n, 'grad_zero_fraction/' + n} <= tags, n
    assert ('update_ratio/' + n in tags) == (ev[0]['variables'][n]['update_ratio'] is not None), n
    if n.endswith('/kernel'):      # (a bias that is still all zero has no ratio)
      assert records[0]['scalars']['update_ratio/' + n] == pytest.approx(ev[0]['variables'][n]['update_ratio'], rel=1e-6), n
    cnt = float(np.prod(shapes[n]))
    for kind in ('gradients/', 'weights/'):
      h = records[1]['histograms'][kind + n]
      assert h[3] == cnt and h[7].sum() == cnt and len(h[6]) == len(h[7]) == 82, (kind, n)
  assert 'loss' in tags and len(records[1]['histograms']) == 2 * len(shapes)
  # without the option: neither, and the same loss line
  e0, md0 = run('off')
  ev0 = _events(md0)
  assert len(ev0) == 1 and 'variables' not in ev0[0] and ev0[0]['loss'] == ev[0]['loss']
  rec0 = _event_file(md0)[1:]
  assert len(rec0) == 1 and not rec0[0]['histograms'] and all(t.startswith('loss') for t in rec0[0]['scalars'])
  assert torch.equal(e0._store.params, e._store.params)
  # the step itself, as the Estimator's runner takes it (backward_and_apply: the early bucket beside the encoder bottom, the late one
  # behind it): the same launches with the option on and off, and no allocation in it
  from geeco_amd.runtime import TrainStepRunner
  on = next(iter(e._specs.values()))[0].model
  off = next(iter(e0._specs.values()))[0].model
  runners = [TrainStepRunner(m, use_graph=False) for m in (on, off)]
  assert all(r.beside_bottom for r in runners)
  for r in runners:
    r.step()      # (the first eager step of a runner creates its streams and events)
  counter = _CountingLibrary(_native.load())
  monkeypatch.setattr(_native, '_lib', counter)
  calls = []
  for r in runners:
    del counter.calls[:]
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    r.step()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == held
    calls.append(list(counter.calls))
  monkeypatch.undo()
  assert calls[0] == calls[1] and 'geeco_variable_stats' not in calls[0] and calls[0].count('geeco_adam_tf_segments') == 2
  assert len(on.step_pieces) > 1 and on._open_pieces == [] and off.step_pieces is None


def test_more_than_one_rank_is_refused(dev, monkeypatch):
  from geeco_amd import dist as gdist
  from geeco_amd import estimator as est
  from geeco_amd.params import create_e2evmc_config
  cfg = create_e2evmc_config(dict(window_size=2, img_height=136, img_width=136, batch_size=2))
  monkeypatch.setattr(gdist, 'world_size', lambda: 2)
  feats = {'rgb': torch.zeros(2, 2, 136, 136, 3, device=dev)}
  with pytest.raises(ValueError, match=r"params\['variable_stats'\] is single-GPU: with 2 ranks"):
    est.e2evmc_model_fn(feats, {}, est.ModeKeys.TRAIN, {'e2evmc_config': cfg, 'variable_stats': True})
