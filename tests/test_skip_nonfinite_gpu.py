"""The opt-in skipping of optimiser steps whose gradient is not finite on the GPU: the two entry points of csrc/guard.hip,
the sum of squares in front of them, the step that calls them, and the Estimator / data-parallel surface on top.  Reference:
tests/_guard_ref.py; tests/test_skip_nonfinite_cpu.py has checked in float64 that the poisoned batch used here has a non-finite
gradient and the clean one a finite one.

Nearly every comparison is bit for bit (an applied step IS the step without the option, a skipped step changes nothing), so there
are no tolerances to derive; the one exception is the two-rank run against one process, held to the bound of tests/test_dp_gpu.py.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import _guard_ref as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float('nan'), float('inf')
CH = 4096                       # GEECO_CLIP_CHUNK of csrc/clip.hip
ADAM = dict(beta1=0.9, beta2=0.999, eps=1e-8)
LR_T = 1e-3
ONE = np.float32(1.0).view(np.uint32)

_INPUTS = {}


def _inputs(n):
  """p, g, m, v, shadow as numpy float32, once per size and left unchanged."""
  if n not in _INPUTS:
    r = np.random.default_rng(3000 + n % 1013)
    p, g, m, s = (r.standard_normal(n).astype(np.float32) for _ in range(4))
    v = (r.standard_normal(n).astype(np.float32)) ** 2
    _INPUTS[n] = (p, g * np.float32(0.1), m * np.float32(0.1), v * np.float32(0.01), s)
  return _INPUTS[n]


def _dev(dev, a, slack=5):
  """numpy array -> flat device tensor with ``slack`` NaN elements behind it (they must stay NaN)."""
  t = torch.full((a.size + slack,), NAN, dtype=torch.float32, device=dev)
  t[:a.size] = torch.from_numpy(a)
  return t


def _bits(t):
  return t.detach().cpu().numpy().view(np.uint32)


def _guard(dev, verdict, total, row):
  """guard[3] with two sentinel words behind it (they must stay)."""
  return torch.tensor([verdict, total, row, -7, -7], dtype=torch.int64, device=dev)


def _scalars(dev, t=5):
  scal = torch.zeros(4, dtype=torch.float32, device=dev)
  scal[0] = LR_T
  return scal, torch.full((1,), t, dtype=torch.int64, device=dev)


# ================================================================================================
# geeco_guard_decide
# ================================================================================================
def _decide(dev, partials, nch, clip, guard):
  from geeco_amd import ops
  out2 = torch.full((2 + 3,), NAN, dtype=torch.float32, device=dev)
  ops.guard_decide(out2, guard, partials, nch, clip)
  torch.cuda.synchronize()
  assert torch.isnan(out2[2:]).all() and guard[3:].tolist() == [-7, -7]
  return out2


@pytest.mark.parametrize('nch', [1, 3, 256, 257, 1844])
def test_the_decision(dev, nch):
  """Finite partials: out2 bitwise geeco_clip_scale's (clip > 0) or [1.0f, norm] (clip == 0), the norm bitwise the restatement's,
  guard = {1, T, 0}.  One NaN, one +Inf or a sum that overflows, at the first, the last and a middle partial: guard = {0, T + 1, C + 1},
  out2 = [0, norm as computed].  A finite call after that ends the row and keeps the total.  Slack behind every buffer stays."""
  from geeco_amd import ops
  r = np.random.default_rng(nch)
  x0 = (r.random(nch, dtype=np.float32) + np.float32(0.5)) * np.float32(3.0)
  partials = _dev(dev, x0, slack=3)
  norm = G.norm_f32(x0)
  T, C = 4, 2
  for clip in (float(np.float32(0.1 * norm)), float(np.float32(1.001 * norm)), 0.0):
    guard = _guard(dev, 0, T, C)
    out2 = _decide(dev, partials, nch, clip, guard)
    want, want_guard = G.decide(x0, clip, [0, T, C])
    assert guard[:3].tolist() == want_guard == [1, T, 0], (nch, clip)
    np.testing.assert_array_equal(_bits(out2[:2]), want.view(np.uint32), err_msg='out2 against the restatement, clip=%g' % clip)
    assert (0.0 < float(want[0]) < 1.0) if clip == float(np.float32(0.1 * norm)) else _bits(out2[:1])[0] == ONE
    if clip > 0.0:
      ref = torch.full((2,), NAN, dtype=torch.float32, device=dev)
      ops.clip_scale(ref, partials, nch, clip)
      np.testing.assert_array_equal(_bits(out2[:2]), _bits(ref), err_msg='out2 against geeco_clip_scale, clip=%g' % clip)
  # non-finite sums.  (One finite partial cannot overflow: nch = 1 has no such case.)
  guard = _guard(dev, 1, T, 0)
  state = [1, T, 0]
  places = sorted({0, nch // 2, nch - 1})
  for kind in ('nan', 'inf') + (('overflow',) if nch > 1 else ()):
    for at in places:
      x = x0.copy()
      if kind == 'overflow':
        x[at] = x[(at + 1) % nch] = np.float32(3e38)
      else:
        x[at] = np.float32(NAN if kind == 'nan' else INF)
      for clip in (0.0, 0.5):
        out2 = _decide(dev, _dev(dev, x, slack=3), nch, clip, guard)
        want, state = G.decide(x, clip, state)
        assert state[0] == 0 and guard[:3].tolist() == state, (nch, kind, at, clip)
        assert _bits(out2[:1])[0] == 0, (kind, at)                                      # +0.0f
        got = float(out2[1])
        assert (np.isnan(got) if kind == 'nan' else got == INF), (kind, at, got)
  skipped = state[1] - T
  assert skipped == state[2] == 2 * len(places) * (3 if nch > 1 else 2)
  out2 = _decide(dev, partials, nch, 0.0, guard)
  assert guard[:3].tolist() == [1, T + skipped, 0] and float(out2[0]) == 1.0 and _bits(out2[1:2])[0] == norm.view(np.uint32)
  assert torch.isnan(partials[nch:]).all()


# ================================================================================================
# geeco_adam_tf_segments_guard
# ================================================================================================
N_BIG = 3 * CH + 7
# offsets are multiples of 4; the last piece of each ends in a scalar tail (1, 3 and 3 elements)
PIECES = {5: [(4, 1), (0, 4)], 1027: [(512, 515), (0, 256), (256, 256)], N_BIG: [(2 * CH, CH + 7), (0, CH), (CH, CH)]}


@pytest.mark.parametrize('ema', [False, True], ids=['plain', 'shadow arena'])
@pytest.mark.parametrize('n', [5, 1027, N_BIG])
def test_adam_behind_the_decision(dev, n, ema):
  """guard[0] = 1: clip_dev[0] = 1.0f is bitwise geeco_adam_tf[_ema] on the whole arena and geeco_adam_tf_segments[_ema] on its
  multiple-of-4 part; clip_dev[0] = s < 1 is bitwise geeco_adam_tf_segments_clip.  guard[0] = 0: p, m, v and the shadow arena keep every
  bit, the slack words behind them included, and g_out holds the gradient.  As one piece and in pieces with scalar tails."""
  from geeco_amd import ops
  p0, g0, m0, v0, s0 = _inputs(n)
  one = torch.tensor([1.0, 3.0], dtype=torch.float32, device=dev)
  part = torch.tensor([0.37, 3.0], dtype=torch.float32, device=dev)
  applied, skipped = _guard(dev, 1, 0, 0), _guard(dev, 0, 1, 1)
  layouts = (('one piece', lambda g: [(g, 0, n)]), ('pieces', lambda g: [(g[off:off + cnt], off, cnt) for off, cnt in PIECES[n]]))
  for gscale, l2 in ((1.0, 0.0), (0.125, 1e-3)):
    kw = dict(grad_scale=gscale, l2=l2, **ADAM)
    scal, step = _scalars(dev)
    ekw = dict(global_step=step, decay=0.99) if ema else {}

    def fresh(g_np=g0):
      return [_dev(dev, x) for x in (p0, g_np, m0, v0, s0)]

    def guarded(pieces_of, clip_dev, guard, g_np=g0):
      p, g, m, v, s = fresh(g_np)
      g_out = torch.full((n + 5,), NAN, device=dev)
      ops.adam_tf_segments_guard(p, m, v, pieces_of(g), scal, clip_dev, guard, ema=s if ema else None, g_out=g_out, **ekw, **kw)
      return p, g_out, m, v, s

    # applied, scale 1: the unclipped kernels
    ref = fresh()
    if ema:
      ops.adam_tf_ema(ref[0], ref[1], ref[2], ref[3], ref[4], n, scal, step, 0.99, **kw)
    else:
      ops.adam_tf(ref[0], ref[1], ref[2], ref[3], n, scal, **kw)
    for what, pieces_of in layouts:
      got = guarded(pieces_of, one, applied)
      torch.cuda.synchronize()
      for name, x, y in zip(('p', 'g_out', 'm', 'v', 'shadow'), got, ref):
        np.testing.assert_array_equal(_bits(x), _bits(y), err_msg='applied, s = 1, %s, %s: n=%d l2=%g' % (name, what, n, l2))
    assert not np.array_equal(_bits(ref[0][:n]), p0.view(np.uint32))      # (the update did run)
    n4 = n & ~3
    seg = fresh()
    segs = [(seg[1][:n4], 0, n4)]
    if ema:
      ops.adam_tf_segments_ema(seg[0], seg[2], seg[3], seg[4], segs, scal, step, 0.99, **kw)
    else:
      ops.adam_tf_segments(seg[0], seg[2], seg[3], segs, scal, **kw)
    got = guarded(lambda g: [(g[:n4], 0, n4)], one, applied)
    torch.cuda.synchronize()
    for name, x, y in zip(('p', 'm', 'v', 'shadow'), (got[0], got[2], got[3], got[4]), (seg[0], seg[2], seg[3], seg[4])):
      np.testing.assert_array_equal(_bits(x), _bits(y), err_msg='%s against the segments entry point: n=%d' % (name, n))
    # applied, scale < 1: the clipped kernel
    for what, pieces_of in layouts:
      clipped = fresh()
      c_out = torch.full((n + 5,), NAN, device=dev)
      ops.adam_tf_segments_clip(clipped[0], clipped[2], clipped[3], pieces_of(clipped[1]), scal, part, ema=clipped[4] if ema else None,
                                g_out=c_out, **ekw, **kw)
      got = guarded(pieces_of, part, applied)
      torch.cuda.synchronize()
      for name, x, y in zip(('p', 'g_out', 'm', 'v', 'shadow'), got, (clipped[0], c_out, clipped[2], clipped[3], clipped[4])):
        np.testing.assert_array_equal(_bits(x), _bits(y), err_msg='applied, s = 0.37, %s, %s: n=%d' % (name, what, n))
      assert not np.array_equal(_bits(got[0]), _bits(ref[0]))               # (the scale did act)
    # skipped: nothing but g_out moves, whatever the gradient holds
    bad = g0.copy()
    bad[0] = bad[n - 1] = np.float32(NAN)
    bad[n // 2] = np.float32(INF)
    zero = torch.tensor([0.0, NAN], dtype=torch.float32, device=dev)
    for what, pieces_of in layouts:
      p, g_out, m, v, s = guarded(pieces_of, zero, skipped, bad)
      torch.cuda.synchronize()
      for name, x, x0 in (('p', p, p0), ('m', m, m0), ('v', v, v0), ('shadow', s, s0)):
        np.testing.assert_array_equal(_bits(x), _bits(_dev(dev, x0)), err_msg='skipped, %s, %s: n=%d' % (name, what, n))
      np.testing.assert_array_equal(_bits(g_out), _bits(_dev(dev, bad)), err_msg='skipped, g_out, %s: n=%d' % (what, n))
    # ... and without a g_out there is nothing to write at all
    p, g, m, v, s = fresh(bad)
    ops.adam_tf_segments_guard(p, m, v, layouts[1][1](g), scal, zero, skipped, ema=s if ema else None, **ekw, **kw)
    torch.cuda.synchronize()
    for name, x, x0 in (('p', p, p0), ('g', g, bad), ('m', m, m0), ('v', v, v0), ('shadow', s, s0)):
      np.testing.assert_array_equal(_bits(x), _bits(_dev(dev, x0)), err_msg='skipped, no g_out, %s: n=%d' % (name, n))
  assert applied.tolist() == [1, 0, 0, -7, -7] and skipped.tolist() == [0, 1, 1, -7, -7]      # the kernel only reads the verdict


# ================================================================================================
# the sum of squares in front of the decision
# ================================================================================================
def test_what_no_piece_covers_cannot_cause_a_skip_and_a_tail_can(dev):
  """A NaN in a stretch of the gradient arena that no piece covers adds 0: the step is applied.  A NaN in the last element of a piece's
  scalar tail skips it."""
  from geeco_amd import ops
  n = N_BIG
  g0 = _inputs(n)[1]
  nch = ops.clip_ws_floats(n)
  # the eight pieces of tests/test_clip_gpu.py; (6001, 2195) starts at an odd offset, (12292, 3) is all tail
  cuts = [(8196, 4), (0, 4), (6001, 2195), (12292, 3), (2000, 2100), (8200, 4092), (4, 1996), (4100, 1901)]
  assert sorted(c[0] for c in cuts)[-1] + 3 == n and sum(c[1] for c in cuts) == n

  def verdict(g_np, use):
    g = _dev(dev, g_np)
    partials = torch.full((nch + 3,), NAN, dtype=torch.float32, device=dev)
    ops.grad_sumsq_segments(partials, None, [(g[off:off + cnt], off, cnt) for off, cnt in use], n, grad_scale=0.125)
    guard = _guard(dev, 1, 0, 0)
    out2 = _decide(dev, partials, nch, 0.0, guard)
    assert torch.isnan(partials[nch:]).all()
    return guard[:3].tolist(), out2

  holes = [c for c in cuts if c[0] not in (2000, 12292)]       # [2000, 4100) and the last three elements belong to no piece
  bad = g0.copy()
  bad[2000] = bad[3000] = bad[4099] = bad[12292] = bad[n - 1] = np.float32(NAN)
  zeroed = g0.copy()
  zeroed[2000:4100] = 0
  zeroed[12292:] = 0
  got, out_holes = verdict(bad, holes)
  want, out_zero = verdict(zeroed, [(0, n)])
  assert got == want == [1, 0, 0] and np.array_equal(_bits(out_holes[:2]), _bits(out_zero[:2])) and np.isfinite(float(out_holes[1]))
  assert G.total_grad_is_finite(zeroed, zeroed, 0.125) and not G.total_grad_is_finite(bad, bad, 0.125)
  # every element covered: the NaN in the last element of the tail decides
  tail = g0.copy()
  tail[n - 1] = np.float32(NAN)
  got, out2 = verdict(tail, cuts)
  assert got == [0, 1, 1] and float(out2[0]) == 0.0 and np.isnan(float(out2[1]))
  assert verdict(g0, cuts)[0] == [1, 0, 0]


# ================================================================================================
# the step
# ================================================================================================
CLIP = 0.01             # below the norm of every clean step these tests take (tests/test_clip_gpu.py)


def _tensors(d):
  return {k: torch.from_numpy(v) for k, v in d.items()}


def _model(dev, name, **kw):
  from geeco_amd import graph
  _, cfg, goal, P, feats, labels = G.case(name)
  model = (graph.GoalE2EVMC if goal else graph.E2EVMC)(cfg, 4, dev, training=True, **kw)
  model.store.load_numpy(P)
  model.load_batch(_tensors(feats), _tensors(labels))
  return model


def _load(model, name, poisoned):
  _, _, _, _, feats, labels = G.case(name)
  model.load_batch(_tensors(feats), _tensors(G.poisoned(labels) if poisoned else labels))


def _state(model):
  s = model.store
  out = {k: getattr(s, k).detach().clone() for k in ('params', 'adam_m', 'adam_v')}
  if s.ema is not None:
    out['ema'] = s.ema.detach().clone()
  return out


def _assert_state(model, state, what):
  for k, v in state.items():
    assert torch.equal(getattr(model.store, k).view(torch.int32), v.view(torch.int32)), (what, k)


def _same_state(a, b, what=''):
  for name in ('params', 'adam_m', 'adam_v', 'grads') + (('ema',) if a.store.ema is not None else ()):
    assert torch.equal(getattr(a.store, name).view(torch.int32), getattr(b.store, name).view(torch.int32)), (what, name)
  assert int(a.store.global_step.item()) == int(b.store.global_step.item()), what


OPTIONS = {'alone': {}, 'with clip_norm': dict(clip_norm=CLIP), 'with ema_decay': dict(ema_decay=0.9)}


@pytest.mark.parametrize('options', list(OPTIONS))
@pytest.mark.parametrize('name', list(G.MODELS))
def test_clean_batches_take_the_step_of_the_model_without_the_option(dev, name, options):
  """Two steps: p, m, v, g, the shadow arena and the counter bit for bit those of the model built without skip_nonfinite; under
  clip_norm also [s, norm]; nothing was skipped."""
  kw = OPTIONS[options]
  a, b = _model(dev, name, skip_nonfinite=True, **kw), _model(dev, name, **kw)
  assert a.skip_limit == 100 and a.guard.tolist() == [0, 0, 0] and a.clip_ws is not None and a.clip_out.numel() == 2
  assert b.skip_limit is None and b.guard is None and (a.store.ema is not None) == ('ema_decay' in kw)
  for _ in range(2):
    a.train_step()
    b.train_step()
  torch.cuda.synchronize()
  _same_state(a, b, options)
  assert a.guard.tolist() == [1, 0, 0] and np.isfinite(float(a.clip_out[1])) and float(a.clip_out[1]) > CLIP
  if 'clip_norm' in kw:
    assert torch.equal(a.clip_out.view(torch.int32), b.clip_out.view(torch.int32)) and 0.0 < float(a.clip_out[0]) < 1.0
  else:
    assert float(a.clip_out[0]) == 1.0


@pytest.mark.parametrize('name', list(G.MODELS))
def test_a_poisoned_step_updates_nothing_and_training_goes_on(dev, name):
  """Clean, poisoned, clean.  After the poisoned step params, m, v and the shadow arena are bitwise those after the clean step alone,
  the counter is 2 and guard = {0, 1, 1}.  After the third the state is bitwise that of a twin without the option that took the two
  clean steps with its counter raised by one in between: a skipped step is a step with no update.  Without the option the
  poisoned step leaves NaN in the whole arena."""
  a = _model(dev, name, skip_nonfinite=True, ema_decay=0.9)
  a.train_step()
  torch.cuda.synchronize()
  after_one = _state(a)
  assert a.guard.tolist() == [1, 0, 0]
  _load(a, name, True)
  a.train_step()
  torch.cuda.synchronize()
  _assert_state(a, after_one, 'after the poisoned step')
  assert int(a.store.global_step.item()) == 2 and a.guard.tolist() == [0, 1, 1]
  assert float(a.clip_out[0]) == 0.0 and not np.isfinite(float(a.clip_out[1]))
  assert not bool(torch.isfinite(a.store.grads).all()) and not np.isfinite(float(a.loss))      # the device saw what the oracle saw
  _load(a, name, False)
  a.train_step()
  torch.cuda.synchronize()
  assert a.guard.tolist() == [1, 1, 0] and int(a.store.global_step.item()) == 3
  twin = _model(dev, name, ema_decay=0.9)
  twin.train_step()
  torch.cuda.synchronize()
  _assert_state(twin, after_one, 'the twin after one step')
  twin.store.global_step.add_(1)
  twin.train_step()
  torch.cuda.synchronize()
  _same_state(a, twin, 'after the third step')
  for k in ('params', 'adam_m', 'adam_v', 'ema'):
    assert bool(torch.isfinite(getattr(a.store, k)).all()), k
  assert not torch.equal(a.store.params, after_one['params'])
  # what the option is for: the same two steps without it
  _load(twin, name, True)
  twin.train_step()
  torch.cuda.synchronize()
  for k in ('params', 'adam_m', 'adam_v', 'ema'):
    assert float(torch.isnan(getattr(twin.store, k)).float().mean()) > 0.5, k


class _CountingLibrary:
  """Stands in for the loaded library: records the calls of every entry point that is handed a stream (each is one launch or a fixed few)."""

  def __init__(self, lib):
    self._lib, self.calls = lib, []

  def __getattr__(self, name):
    fn = getattr(self._lib, name)
    if not name.startswith('geeco_') or name in ('geeco_last_error', 'geeco_clip_ws_floats') or name.endswith('_bytes'):
      return fn

    def counted(*a):
      self.calls.append(name)
      return fn(*a)
    return counted


def test_the_schedules_skip_alike_with_the_same_launches(dev, monkeypatch):
  """train_step, backward_and_apply and a replayed TrainStepRunner(use_graph=True) over clean, poisoned, clean: the same state bit for
  bit and the same guard; the calls of a step are the same list on a clean and on a poisoned batch (the step stays one graph)."""
  from geeco_amd import _native
  from geeco_amd.runtime import TrainStepRunner, gradient_buckets
  name = 'e2e_vmc'
  a, b, c = (_model(dev, name, skip_nonfinite=True, ema_decay=0.9) for _ in range(3))
  early, late = gradient_buckets(a.store)
  assert early and late and b.can_apply_beside_bottom()
  runner = TrainStepRunner(c, use_graph=True, warmup=1)      # step 1 eager, step 2 captured and replayed, step 3 replayed
  assert runner.beside_bottom

  def beside():
    b.forward(backward_too=True)
    b.backward_and_apply(early, late)

  counter = _CountingLibrary(_native.load())
  calls = {'train_step': [], 'backward_and_apply': []}
  for poisoned in (False, True, False):
    for m in (a, b, c):
      _load(m, name, poisoned)
    monkeypatch.setattr(_native, '_lib', counter)
    for what, step in (('train_step', a.train_step), ('backward_and_apply', beside)):
      del counter.calls[:]
      step()
      torch.cuda.synchronize()
      calls[what].append(list(counter.calls))
    monkeypatch.undo()
    runner.step()
    torch.cuda.synchronize()
    want = [0, 1, 1] if poisoned else [1, int(a.guard[1]), 0]
    for what, m in (('train_step', a), ('backward_and_apply', b), ('replayed', c)):
      assert m.guard.tolist() == want, (what, poisoned)
  _same_state(a, b, 'backward_and_apply against train_step')
  _same_state(a, c, 'the replayed step against train_step')
  assert a.guard.tolist() == [1, 1, 0] and int(a.store.global_step.item()) == 3
  assert runner._graphs is not None and len(runner._graphs) == 1
  assert b._clip_calls == [] and not b._prepared
  for what, per_step in calls.items():
    assert per_step[0] == per_step[1] == per_step[2], what
  new = ('geeco_grad_sumsq_segments', 'geeco_guard_decide', 'geeco_adam_tf_segments_guard')
  assert [calls['train_step'][1].count(x) for x in new] == [1, 1, 1]
  assert [calls['backward_and_apply'][1].count(x) for x in new] == [1, 1, 2]


def test_a_model_without_the_option_is_untouched(dev, monkeypatch):
  """No guard, no clip buffers, none of the new entry points: the calls of a step are those of the guarded step minus the two launches in
  front of the optimiser pass, in both schedules; a model with clip_norm alone calls what it called."""
  from geeco_amd import _native
  from geeco_amd.runtime import gradient_buckets
  off, on, clip = _model(dev, 'e2e_vmc'), _model(dev, 'e2e_vmc', skip_nonfinite=5), _model(dev, 'e2e_vmc', clip_norm=CLIP)
  assert off.skip_limit is None and off.guard is None and off.clip_ws is None and off.clip_out is None and off._clip_calls == []
  assert on.skip_limit == 5 and clip.guard is None and clip.clip_ws is not None
  early, late = gradient_buckets(off.store)
  counter = _CountingLibrary(_native.load())
  monkeypatch.setattr(_native, '_lib', counter)
  guard = ('geeco_grad_sumsq_segments', 'geeco_guard_decide', 'geeco_adam_tf_segments_guard')
  clipping = ('geeco_grad_sumsq_segments', 'geeco_clip_scale', 'geeco_adam_tf_segments_clip')

  def calls_of(step):
    del counter.calls[:]
    step()
    torch.cuda.synchronize()
    return list(counter.calls)

  def beside(m):
    m.forward(backward_too=True)
    m.backward_and_apply(early, late)

  plain_off, plain_on, plain_clip = calls_of(off.train_step), calls_of(on.train_step), calls_of(clip.train_step)
  assert plain_off.count('geeco_adam_tf') == 1 and not any(c in plain_off for c in guard + clipping)
  assert [plain_on.count(c) for c in guard] == [1, 1, 1] and not any(c in plain_on for c in ('geeco_adam_tf',) + clipping[1:])
  assert len(plain_on) == len(plain_off) + 2
  assert [c for c in plain_on if c not in guard] == [c for c in plain_off if c != 'geeco_adam_tf']
  assert [plain_clip.count(c) for c in clipping] == [1, 1, 1] and not any(c in plain_clip for c in guard[1:])
  side_off, side_on = calls_of(lambda: beside(off)), calls_of(lambda: beside(on))
  assert side_off.count('geeco_adam_tf_segments') == 2 and not any(c in side_off for c in guard + clipping)
  assert [side_on.count(c) for c in guard] == [1, 1, 2] and 'geeco_adam_tf_segments' not in side_on
  assert len(side_on) == len(side_off) + 2


# ================================================================================================
# Estimator
# ================================================================================================
def _events(model_dir):
  return [json.loads(l) for l in open(os.path.join(model_dir, 'events.jsonl'))]


def test_estimator_skips_logs_and_gives_up(dev, tmp_path):
  """Three steps of e2e_vmc on a two-episode synthetic dataset whose second batch is poisoned.  With params['skip_nonfinite'] every
  events.jsonl line carries skipped_steps and grad_norm, the final checkpoint is finite and equals the live store, and
  last_train_stats counts the skip; with a limit of 1 train() raises RuntimeError at the skipped step and writes no checkpoint;
  without the option the key is not written (and the checkpoint is NaN: what the option is for)."""
  from geeco_amd import estimator as est
  from geeco_amd import input_fn as I
  from geeco_amd.graph import build_store
  from geeco_amd.params import create_e2evmc_config
  root = str(tmp_path / 'ds')
  I.write_synthetic_dataset(root, 2, episode_length=9, img_hw=(G.H, G.H), seed=5)
  batches = list(I.pickplace_input_fn(root, 'default', 'train', window_size=G.K3, batch_size=4, num_threads=2))
  assert len(batches) == 3
  feats, labels = batches[1]
  batches[1] = (feats, G.poisoned(labels))
  assert np.isfinite(labels['cmd']).all() and np.isnan(batches[1][1]['cmd'][0, 0])
  cfg = create_e2evmc_config(dict(window_size=G.K3, img_height=G.H, img_width=G.H, batch_size=4))
  plain = {'e2evmc_config': cfg, 'log_steps': 1, 'debug': False}

  def run(tag, **extra):
    md = str(tmp_path / tag)
    e = est.Estimator(est.e2evmc_model_fn, md, est.RunConfig(init_seed=4), dict(plain, **extra))
    e.train(input_fn=lambda: iter(batches))
    return e, md

  e, md = run('on', skip_nonfinite=True)
  ev = _events(md)
  print('events:', [(line['global_step'], line['skipped_steps'], line['grad_norm'], line['loss']) for line in ev])
  assert [line['global_step'] for line in ev] == [1, 2, 3] and [line['skipped_steps'] for line in ev] == [0, 1, 1]
  assert np.isfinite(ev[0]['grad_norm']) and not np.isfinite(ev[1]['grad_norm']) and np.isfinite(ev[2]['grad_norm'])
  assert np.isfinite(ev[0]['loss']) and not np.isfinite(ev[1]['loss']) and np.isfinite(ev[2]['loss'])
  assert e.last_train_stats['skipped_steps'] == 1 and e.last_train_stats['steps'] == 3
  back = build_store(cfg, False, 'cpu')
  est.load_checkpoint(back, est.latest_checkpoint(md))
  for name in ('params', 'adam_m', 'adam_v', 'global_step'):
    assert torch.equal(getattr(back, name), getattr(e._store, name).cpu()), name
    assert bool(torch.isfinite(getattr(back, name).float()).all()), name
  assert int(back.global_step.item()) == 3
  # a limit of one skipped step: the run stops where it happens, and nothing is saved
  md1 = str(tmp_path / 'limit')
  e1 = est.Estimator(est.e2evmc_model_fn, md1, est.RunConfig(init_seed=4), dict(plain, skip_nonfinite=1))
  with pytest.raises(RuntimeError, match=r'1 optimiser steps in a row were skipped.*nan'):
    e1.train(input_fn=lambda: iter(batches))
  assert est.latest_checkpoint(md1) is None and len(_events(md1)) == 1
  # without the option: no key, and the NaN gets everywhere
  e0, md0 = run('off')
  assert not any('skipped_steps' in line or 'grad_norm' in line for line in _events(md0)) and 'skipped_steps' not in e0.last_train_stats
  assert _events(md0)[0]['loss'] == ev[0]['loss']
  assert float(torch.isnan(e0._store.params).float().mean()) > 0.5


# ================================================================================================
# data parallel: two ranks sharing the test GPU over gloo (the harness of tests/test_dp_gpu.py)
# ================================================================================================
def _dp_batch(step, lo, hi):
  """The global batch of tests/test_dp_gpu.py; in step 2 (of 1..3) row 2 -- the first row of rank 1's shard, no row of rank 0's -- is poisoned."""
  import test_dp_gpu as D
  feats, labels = D._batch(4)
  if step == 2:
    labels = G.poisoned(labels, row=2)
  return {k: torch.from_numpy(v[lo:hi]) for k, v in feats.items()}, {k: torch.from_numpy(v[lo:hi]) for k, v in labels.items()}


def _dp_worker(rank, world, port, q):
  sys.path.insert(0, ROOT)
  sys.path.insert(0, os.path.join(ROOT, 'tests'))
  import test_dp_gpu as D
  D._child_watchdog()
  os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
  from geeco_amd import dist as gdist
  from geeco_amd import graph
  from geeco_amd.params import create_e2evmc_config
  from geeco_amd.runtime import TrainStepRunner
  torch.cuda.set_device(0)
  gdist.init_from_env('gloo')
  lo, hi = gdist.shard_bounds(4)
  model = graph.GoalE2EVMC(create_e2evmc_config(D.KW), hi - lo, 'cuda:0', training=True, skip_nonfinite=True)
  if rank == 0:
    model.store.initialize(seed=9)
  gdist.broadcast_variables(model.store)
  runner = TrainStepRunner(model, use_graph=True, warmup=1)     # the default form: step 1 eager, steps 2-3 replayed
  assert runner.dp and runner.split_adam
  guards, local_nan = [], []
  for step in (1, 2, 3):
    model.load_batch(*_dp_batch(step, lo, hi))
    runner.step()
    torch.cuda.synchronize()
    guards.append(model.guard.tolist())
    local_nan.append(bool(torch.isnan(model.inputs['cmd']).any()))
  q.put((rank, model.store.params.detach().cpu().numpy(), guards, local_nan, gdist.replicas_identical(model.store)))
  torch.distributed.destroy_process_group()


def test_two_ranks_skip_together(dev):
  """A NaN in ONE rank's shard survives the SUM of the exchange: both ranks skip step 2, stay bitwise identical, and end where the
  single process ends on the global batch (at the tolerance tests/test_dp_gpu.py holds three unguarded steps to; here only two of
  the three move anything)."""
  import test_dp_gpu as D
  from geeco_amd import graph
  from geeco_amd.params import create_e2evmc_config
  ctx = mp.get_context('spawn')
  q = ctx.Queue()
  port = 28600 + os.getpid() % 1000
  procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
  for p in procs:
    p.start()
  res = sorted(D._results(procs, q, 2), key=lambda t: t[0])
  for p in procs:
    p.join(timeout=60)
    assert p.exitcode == 0
  model = graph.GoalE2EVMC(create_e2evmc_config(D.KW), 4, dev, training=True, skip_nonfinite=True)
  model.store.initialize(seed=9)
  guards = []
  for step in (1, 2, 3):
    model.load_batch(*_dp_batch(step, 0, 4))
    model.train_step()
    torch.cuda.synchronize()
    guards.append(model.guard.tolist())
  ref = model.store.params.detach().cpu().numpy()
  assert guards == [[1, 0, 0], [0, 1, 1], [1, 1, 0]]
  assert res[0][2] == res[1][2] == guards
  assert res[0][3] == [False, False, False] and res[1][3] == [False, True, False]      # only rank 1 held the NaN
  assert res[0][4] and res[1][4]
  np.testing.assert_array_equal(res[0][1].view(np.uint32), res[1][1].view(np.uint32))  # replicas stay identical
  assert np.isfinite(ref).all() and np.isfinite(res[0][1]).all()
  np.testing.assert_allclose(res[0][1], ref, rtol=0, atol=3e-4)
  frac_close = np.mean(np.abs(res[0][1] - ref) < 2e-5)
  assert frac_close > 0.99, frac_close
