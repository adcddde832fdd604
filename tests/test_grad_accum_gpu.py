"""The opt-in gradient accumulation over micro-batches on the GPU: the accumulate launch of csrc/grad_accum.hip, the three
forms of the micro-step, their composition with every optimiser-side option, and the Estimator surface on top.

Kernel reference: tests/_grad_accum_ref.py (numpy float32: one IEEE addition per element, so the comparison is by bits, NaN for NaN).
Model reference, from code that predates the option: a model built WITHOUT it on the same weights runs forward + backward per
micro-batch, its gradient arenas are added in float32 in order on the host, and the sum goes through the existing optimiser entry
points with grad_scale = 1 / A.  Nothing is reordered on either side, so the comparison is by bits there too."""
import json
import os

import numpy as np
import pytest
import torch

import _grad_accum_ref as GA

pytestmark = pytest.mark.gpu

NAN = float('nan')
ADAM = dict(beta1=0.9, beta2=0.999, eps=1e-8)


def _bits(t):
  return t.detach().cpu().numpy().view(np.uint32)


# ================================================================================================
# the kernel
# ================================================================================================
BIG = 2097152 + 1031      # past one pass of the 2048 x 256 x 4 grid, with a tail
SIZES = [1, 3, 4, 7, 1029, BIG]
SLACK = 5


def _launch(dev, acc0, g, cuts, overwrite, n):
  """One launch: every piece from a source buffer of its own with NaN slack behind it.  Returns (accumulator, sources, their originals)."""
  from geeco_amd import ops
  acc = torch.from_numpy(acc0).to(dev)
  srcs, origs = [], []
  for off, cnt in cuts:
    o = np.full(cnt + SLACK, np.nan, np.float32)
    o[:cnt] = g[off:off + cnt]
    origs.append(o)
    srcs.append(torch.from_numpy(o).to(dev))
  ops.grad_accumulate_segments(acc, [(s, off, cnt) for s, (off, cnt) in zip(srcs, cuts)], n, overwrite)
  torch.cuda.synchronize()
  return acc.cpu().numpy(), [s.cpu().numpy() for s in srcs], origs


@pytest.mark.parametrize('overwrite', [True, False], ids=['overwrite', 'add'])
@pytest.mark.parametrize('n', SIZES)
def test_any_partition_is_the_one_piece_result_and_numpys_float32(dev, n, overwrite):
  """1..8 pieces at multiples of 4: bitwise numpy's float32 result and bitwise the one-piece call; the slack past n keeps every bit and
  the sources are unchanged.  Overwrite runs onto an all-NaN accumulator (it must not be read), add onto random contents."""
  g = GA.special_floats(n, 100 + n % 97)
  acc0 = np.full(n + SLACK, np.nan, np.float32) if overwrite else np.random.default_rng(n).standard_normal(n + SLACK).astype(np.float32)
  want = GA.accumulate(acc0, [(g, 0, n)], overwrite)
  one, _, _ = _launch(dev, acc0, g, [(0, n)], overwrite, n)
  assert GA.same_floats(one, want)
  assert GA.same_floats(one[n:], acc0[n:])
  if overwrite:
    assert np.array_equal(np.isnan(one[:n]), np.isnan(g))      # finite wherever the gradient is: the NaNs it held are gone
  seen = set()
  for pieces in (2, 3, 5, 8):
    cuts = GA.partition(n, pieces, 7 * pieces + n % 13)
    if len(cuts) in seen:
      continue
    seen.add(len(cuts))
    assert 1 <= len(cuts) <= 8 and sum(c for _, c in cuts) == n and all(off % 4 == 0 for off, _ in cuts)
    got, srcs, origs = _launch(dev, acc0, g, cuts, overwrite, n)
    assert GA.same_floats(got, one), (n, cuts[:3])
    for s, o in zip(srcs, origs):
      assert GA.same_floats(s, o)
  assert n < 8 or 8 in seen or n == 7


@pytest.mark.parametrize('overwrite', [True, False], ids=['overwrite', 'add'])
def test_an_uncovered_stretch_keeps_every_bit(dev, overwrite):
  n = 1029
  g = GA.special_floats(n, 3)
  acc0 = GA.special_floats(n + SLACK, 4)
  cuts = [(512, 517), (0, 256)]                       # [256, 512) belongs to no piece
  got, _, _ = _launch(dev, acc0, g, cuts, overwrite, n)
  assert GA.same_floats(got, GA.accumulate(acc0, [(g[off:off + cnt], off, cnt) for off, cnt in cuts], overwrite))
  assert GA.same_floats(got[256:512], acc0[256:512]) and GA.same_floats(got[n:], acc0[n:])
  assert not GA.same_floats(got[:256], acc0[:256])


def test_refusals_leave_the_accumulator_alone(dev):
  """Every refusal returns non-zero with its message and launches nothing."""
  import ctypes
  from geeco_amd import _native, ops
  lib = _native.load()
  fn, E = lib.geeco_grad_accumulate_segments, _native.GEECO_EINVAL
  err = lambda: (lib.geeco_last_error() or b'').decode()
  n = 64
  acc0 = GA.special_floats(n + SLACK, 9)
  acc = torch.from_numpy(acc0).to(dev)
  g = torch.ones(n + 8, device=dev)
  ap, gp = ctypes.c_void_p(acc.data_ptr()), g.data_ptr()
  stream = ops._stream()

  def segs(*pieces):
    arr = (_native.AdamSegment * max(len(pieces), 1))()
    for a, (src, off, cnt) in zip(arr, pieces):
      a.g, a.p_off, a.count = src, off, cnt
    return arr

  refused = [
      ('null accumulator', (None, segs((gp, 0, 8)), 1, n, 0), 'bad arguments'),
      ('null table', (ap, None, 1, n, 0), 'bad arguments'),
      ('null source', (ap, segs((0, 0, 8)), 1, n, 0), 'piece 0'),
      ('no piece', (ap, segs((gp, 0, 8)), 0, n, 0), 'pieces'),
      ('nine pieces', (ap, segs(*[(gp + 32 * k, 4 * k, 4) for k in range(9)]), 9, n, 0), 'pieces'),
      ('misaligned offset', (ap, segs((gp, 2, 8)), 1, n, 0), 'multiple of 4'),
      ('misaligned source', (ap, segs((gp + 4, 0, 8)), 1, n, 0), '16-byte aligned'),
      ('misaligned accumulator', (ctypes.c_void_p(acc.data_ptr() + 4), segs((gp, 0, 8)), 1, n, 0), '16-byte aligned'),
      ('count 0', (ap, segs((gp, 0, 0)), 1, n, 0), 'count >= 1'),
      ('past n', (ap, segs((gp, 60, 8)), 1, n, 0), 'outside the accumulator'),
      ('at n', (ap, segs((gp, 64, 1)), 1, n, 0), 'outside the accumulator'),
      ('source in its own range', (ap, segs((acc.data_ptr() + 16, 0, 8)), 1, n, 0), 'overlaps'),
      ('source across the end of its range', (ap, segs((acc.data_ptr() + 16, 8, 8)), 1, n, 1), 'overlaps'),
  ]
  for what, args, message in refused:
    assert fn(*args, stream) == E and message in err(), (what, err())
  with pytest.raises(ValueError):
    ops.grad_accumulate_segments(acc[:32], [(g, 0, 8)], n, False)
  torch.cuda.synchronize()
  assert GA.same_floats(acc.cpu().numpy(), acc0)
  assert fn(ap, segs((gp, 0, 8)), 1, n, 0, stream) == 0      # ... and the good call goes through
  torch.cuda.synchronize()
  assert GA.same_floats(acc.cpu().numpy(), GA.accumulate(acc0, [(np.ones(8, np.float32), 0, 8)], False))


# ================================================================================================
# the model
# ================================================================================================
def _tensors(d):
  return {k: torch.from_numpy(v) for k, v in d.items()}


def _load(model, batch):
  model.load_batch(_tensors(batch[0]), _tensors(batch[1]))


def _model(dev, name, **kw):
  from geeco_amd import graph
  _, cfg, goal, P = GA.case(name)
  model = (graph.GoalE2EVMC if goal else graph.E2EVMC)(cfg, 4, dev, training=True, **kw)
  model.store.load_numpy(P)
  return model


def _buckets(model):
  from geeco_amd.runtime import gradient_buckets
  return gradient_buckets(model.store)


STATE = ('params', 'adam_m', 'adam_v', 'ema')


def _state(model):
  """Everything a micro-step that applies nothing must leave alone, as bits."""
  s = model.store
  out = {k: _bits(getattr(s, k)).copy() for k in STATE if getattr(s, k) is not None}
  out['global_step'] = s.global_step.cpu().numpy().copy()
  out['scal'] = _bits(model.scal).copy()
  for k in ('clip_out', 'guard'):
    if getattr(model, k) is not None:
      out[k] = getattr(model, k).cpu().numpy().copy().view(np.uint8)
  return out


def _assert_state(got, want, what):
  assert sorted(got) == sorted(want)
  for k in want:
    assert np.array_equal(got[k], want[k]), (what, k)


class _Reference:
  """The optimiser step of a group from code that predates the option: ``model`` is built without it."""

  def __init__(self, model, A):
    self.model, self.A = model, A
    self.kw = dict(grad_scale=1.0 / A, l2=float(model.cfg.l2_regularizer))

  def summed(self, batches, load=_load):
    """The micro-batches' gradient arenas added in float32, in order, on the host; on the device again."""
    m, acc = self.model, None
    for b in batches:
      load(m, b)
      m.forward(backward_too=True)
      m.backward()
      torch.cuda.synchronize()
      g = m.store.grads.cpu().numpy().copy()
      acc = g if acc is None else acc + g
    return torch.from_numpy(acc).to(m.store.grads.device)

  def prepare(self):
    from geeco_amd import ops
    m = self.model
    if m.lr_schedule is None:
      ops.adam_prepare(m.store.global_step, float(m.cfg.lr), m.scal)
    else:
      ops.adam_prepare_schedule(m.store.global_step, m._lr_arg, m.scal)

  def step(self, batches, load=_load):
    """adam_prepare + adam_tf (adam_tf_ema with a shadow arena) on the summed gradient; the weight copies follow."""
    from geeco_amd import ops
    m, s = self.model, self.model.store
    g = self.summed(batches, load)
    self.prepare()
    if s.ema is not None:
      ops.adam_tf_ema(s.params, g, s.adam_m, s.adam_v, s.ema, s.size, m.scal, s.global_step, m.ema_decay, **self.kw)
    else:
      ops.adam_tf(s.params, g, s.adam_m, s.adam_v, s.size, m.scal, **self.kw)
    m._refresh_after_update()
    torch.cuda.synchronize()
    return g


def _same_arenas(on, ref, what, names=('params', 'adam_m', 'adam_v')):
  for k in names:
    assert np.array_equal(_bits(getattr(on.store, k)), _bits(getattr(ref.store, k))), (what, k)


@pytest.mark.parametrize('captured', [False, True], ids=['eager', 'captured'])
@pytest.mark.parametrize('A', [2, 3])
@pytest.mark.parametrize('name', ['e2e_vmc', 'goal dynimg'])
def test_a_group_is_the_reference_step_on_the_summed_gradient(dev, name, A, captured):
  """Three optimiser steps through TrainStepRunner (captured: the first group runs eagerly, the second and third are replays of the
  three forms' graphs), each bitwise the reference continued; the first A - 1 calls change no bit outside the accumulator."""
  from geeco_amd.runtime import TrainStepRunner
  on, off = _model(dev, name, grad_accum_steps=A), _model(dev, name)
  assert on.store.accum is not None and on.store.accum.numel() == on.store.size and on.store.accum.data_ptr() % 16 == 0
  assert not on.store.accum.any() and on.store.accum_count == 0
  batches = GA.micro_batches(name, A)
  runner = TrainStepRunner(on, use_graph=captured, warmup=1)
  assert runner.beside_bottom
  ref = _Reference(off, A)
  for step in (1, 2, 3):
    before = _state(on)
    for a, b in enumerate(batches):
      _load(on, b)
      applied = runner.step()
      torch.cuda.synchronize()
      assert applied == (a == A - 1) and runner.applied == applied and on.store.accum_count == (a + 1) % A
      if a < A - 1:
        _assert_state(_state(on), before, 'step %d, micro-step %d' % (step, a))
        assert int(on.store.global_step.item()) == step - 1
    g = ref.step(batches)
    assert int(on.store.global_step.item()) == step == int(off.store.global_step.item())
    assert np.array_equal(_bits(on.store.accum), _bits(g)), 'the accumulator is the float32 sum, step %d' % step
    _same_arenas(on, off, 'step %d' % step)
    assert np.array_equal(_bits(on.scal[:1]), _bits(off.scal[:1]))
    assert not np.array_equal(_bits(on.store.params), before['params'])
  if captured:
    assert sorted(runner._graphs) == (['first', 'last'] if A == 2 else ['first', 'last', 'middle'])
  else:
    assert runner._graphs is None
  # the losses: the mean over the group's micro-batches, summed on the device (the reference ran the same forwards one step of weights later)
  parts = {k: float(v) for k, v in on.loss_parts().items()}
  assert set(parts) == {k for k in off.loss_parts()} and np.isfinite(parts['loss']) and parts['loss'] > 0.0


@pytest.mark.parametrize('name', ['e2e_vmc', 'goal dynimg'])
def test_the_two_layouts_give_the_same_bits(dev, name):
  """backward_and_apply(form) beside the bottom against the plain order (backward, one accumulate launch, the optimiser step)."""
  A = 3
  a, b = _model(dev, name, grad_accum_steps=A), _model(dev, name, grad_accum_steps=A)
  assert a.can_apply_beside_bottom()
  batches = GA.micro_batches(name, A)
  for _ in range(2):
    for i, batch in enumerate(batches):
      _load(a, batch)
      _load(b, batch)
      assert a.micro_step(_buckets(a)) == b.micro_step() == (i == A - 1)
  torch.cuda.synchronize()
  _same_arenas(a, b, 'beside the bottom against plain', ('params', 'adam_m', 'adam_v', 'accum', 'grads'))
  assert int(a.store.global_step.item()) == int(b.store.global_step.item()) == 2
  assert {k: float(v) for k, v in a.loss_parts().items()} == {k: float(v) for k, v in b.loss_parts().items()}


def _run_group(on, batches, buckets=True, load=_load):
  for b in batches:
    load(on, b)
    applied = on.micro_step(_buckets(on) if buckets else None)
  torch.cuda.synchronize()
  assert applied and on.store.accum_count == 0


CLIP = 0.01             # below the norm of the steps these tests take (asserted)


def test_clip_norm_sees_the_summed_gradient(dev):
  from geeco_amd import ops
  name, A = 'e2e_vmc', 2
  on, off = _model(dev, name, grad_accum_steps=A, clip_norm=CLIP), _model(dev, name)
  batches = GA.micro_batches(name, A)
  before = _state(on)
  _load(on, batches[0])
  assert not on.micro_step(_buckets(on))
  torch.cuda.synchronize()
  _assert_state(_state(on), before, 'first micro-step under clip_norm')
  _load(on, batches[1])
  assert on.micro_step(_buckets(on))
  ref = _Reference(off, A)
  g, s = ref.summed(batches), off.store
  ref.prepare()
  ws, out2 = torch.zeros(ops.clip_ws_floats(s.size), device=dev), torch.zeros(2, device=dev)
  ops.grad_sumsq_segments(ws, s.params, [(g, 0, s.size)], s.size, **ref.kw)
  ops.clip_scale(out2, ws, ws.numel(), CLIP)
  ops.adam_tf_segments_clip(s.params, s.adam_m, s.adam_v, [(g, 0, s.size)], off.scal, out2, **ref.kw)
  torch.cuda.synchronize()
  assert np.array_equal(_bits(on.clip_out), _bits(out2)) and float(out2[1]) > CLIP and 0.0 < float(out2[0]) < 1.0
  _same_arenas(on, off, 'clipped')


def test_ema_moves_once_per_optimiser_step(dev):
  name, A = 'e2e_vmc', 2
  on, off = _model(dev, name, grad_accum_steps=A, ema_decay=0.9), _model(dev, name, ema_decay=0.9)
  batches = GA.micro_batches(name, A)
  for step in (1, 2):
    shadow = _bits(on.store.ema).copy()
    _load(on, batches[0])
    assert not on.micro_step(_buckets(on))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(on.store.ema), shadow)
    _load(on, batches[1])
    assert on.micro_step(_buckets(on))
    _Reference(off, A).step(batches)
    assert not np.array_equal(_bits(on.store.ema), shadow)
    _same_arenas(on, off, 'step %d' % step, ('params', 'adam_m', 'adam_v', 'ema'))


def test_the_schedule_follows_optimiser_steps(dev):
  from geeco_amd import ops
  name, A = 'e2e_vmc', 2
  sched = dict(kind='exponential', decay_steps=1, decay_rate=0.5)
  on, off = _model(dev, name, grad_accum_steps=A, lr_schedule=sched), _model(dev, name, lr_schedule=sched)
  batches = GA.micro_batches(name, A)
  ref = _Reference(off, A)
  assert float(on.scal[2]) == 0.0
  for step in (0, 1):
    rate = float(on.scal[2])
    _load(on, batches[0])
    on.micro_step(_buckets(on))
    torch.cuda.synchronize()
    assert float(on.scal[2]) == rate and int(on.store.global_step.item()) == step      # a micro-step that applies nothing: no schedule step
    _load(on, batches[1])
    on.micro_step(_buckets(on))
    ref.step(batches)
    assert float(on.scal[2]) == float(np.float32(ops.lr_schedule_eval(on.lr_schedule, step))) == float(off.scal[2])
    _same_arenas(on, off, 'scheduled step %d' % step)
  assert float(on.scal[2]) == float(np.float32(0.5 * 1e-3))


def test_a_frozen_bottom_is_neither_read_nor_accumulated(dev):
  """--freeze_encoder_bottom: conv1 / conv2 keep every bit of params, adam_m, adam_v and accum (filled with NaN here: an add would show);
  the rest is the reference."""
  name, A = 'goal dynimg', 2
  on, off = _model(dev, name, grad_accum_steps=A, lr_multipliers={'/conv[12]/': 0.0}), _model(dev, name)
  assert on.backward_cut == 'no_bottom' and not on.can_apply_beside_bottom()
  s = on.store
  frozen = np.ones(s.size, bool)
  for lo, cnt, _ in on.lr_runs:
    frozen[lo:lo + cnt] = False
  assert frozen.any() and not frozen.all()
  s.accum.fill_(NAN)
  s.adam_m[torch.from_numpy(frozen).to(dev)] = 0.25
  before = {k: _bits(getattr(s, k)).copy() for k in ('params', 'adam_m', 'adam_v', 'accum')}
  batches = GA.micro_batches(name, A)
  _run_group(on, batches, buckets=False)
  _Reference(off, A).step(batches)
  for k in ('params', 'adam_m', 'adam_v', 'accum'):
    assert np.array_equal(_bits(getattr(s, k))[frozen], before[k][frozen]), k
  for k in ('params', 'adam_m', 'adam_v'):
    assert np.array_equal(_bits(getattr(s, k))[~frozen], _bits(getattr(off.store, k))[~frozen]), k
  assert not torch.isnan(s.accum[torch.from_numpy(~frozen).to(dev)]).any() and int(s.global_step.item()) == 1


def test_variable_stats_report_the_averaged_accumulated_gradient(dev):
  """grad_norm per variable: the existing statistics pass on the reference's summed gradient with grad_scale = 1 / A, bitwise (its record
  does not depend on the pieces), and the float64 norm of sum / A at 1e-5."""
  from geeco_amd import ops
  name, A = 'e2e_vmc', 2
  on, off = _model(dev, name, grad_accum_steps=A, variable_stats=True), _model(dev, name)
  batches = GA.micro_batches(name, A)
  _run_group(on, batches)
  stats = on.variable_stats()
  g, s = _Reference(off, A).summed(batches), off.store
  plan = ops.VariableStatsPlan([(s.offsets[n], int(np.prod(s.shapes[n]))) for n in s.shapes], dev)
  plan.run(s.params, s.adam_m, s.adam_v, [(g, 0, s.size)], s.size, grad_scale=1.0 / A)
  host = g.cpu().numpy().astype(np.float64) / A
  for rec, n in zip(plan.records(), s.shapes):
    assert stats[n]['grad_norm'] == float(np.sqrt(float(rec['grad']['sumsq']))), n
    o, c = s.offsets[n], int(np.prod(s.shapes[n]))
    want = float(np.sqrt(np.sum(host[o:o + c] ** 2)))
    assert abs(stats[n]['grad_norm'] - want) <= 1e-5 * want and want > 0.0, n


def test_shared_frames_take_the_plain_layout(dev):
  import test_shared_frames_gpu as S
  A = 2
  cases = [S._case(dev, 'e2e_vmc', b) for b in ('one episode', 'two episodes')]
  ocfg, goal, P = cases[0][:3]
  from geeco_amd import graph
  from geeco_amd.params import create_e2evmc_config
  F = 4 + 2 * (S.K3 - 1)
  cfg = create_e2evmc_config(ocfg._asdict())

  def batch_of(case):
    _, _, _, feats, labels, win, tgt, _ = case
    table, index, _, _ = win.frame_table(F, tgt, dev)
    f = {k: v for k, v in feats.items() if k not in ('rgb', 'target_rgb')}
    f.update(frame_table=table, frame_index=index)
    return f, labels

  batches = [batch_of(c) for c in cases]
  models = []
  for kw in (dict(grad_accum_steps=A), {}):
    m = graph.E2EVMC(cfg, 4, dev, training=True, shared_frames=F, **kw)
    m.store.load_numpy(P)
    models.append(m)
  on, off = models
  _run_group(on, batches, buckets=False)
  _Reference(off, A).step(batches)
  _same_arenas(on, off, 'shared frames')
  assert int(on.store.global_step.item()) == 1


def test_a_skipped_group_leaves_a_clean_accumulator(dev):
  """A NaN pixel in micro-batch 2 of 2: verdict 0, nothing but the counter moves; the next group on clean data is the reference step --
  overwrite mode cleared the accumulator of its NaNs with no zeroing pass."""
  name, A = 'e2e_vmc', 2
  on, off = _model(dev, name, grad_accum_steps=A, skip_nonfinite=True, ema_decay=0.9), _model(dev, name, ema_decay=0.9)
  batches = GA.micro_batches(name, A)
  bad = ({k: v.copy() for k, v in batches[1][0].items()}, batches[1][1])
  bad[0]['rgb'][1, 0, 40, 40, 1] = np.nan
  before = _state(on)
  _run_group(on, [batches[0], bad])
  assert on.guard.tolist() == [0, 1, 1] and int(on.store.global_step.item()) == 1 and torch.isnan(on.store.accum).any()
  after = _state(on)
  for k in STATE:
    assert np.array_equal(after[k], before[k]), k
  _run_group(on, batches)
  assert on.guard.tolist() == [1, 1, 0] and int(on.store.global_step.item()) == 2 and not torch.isnan(on.store.accum).any()
  off.store.global_step.fill_(1)      # the skipped step advanced the counter; the reference takes its step at t = 2
  _Reference(off, A).step(batches)
  _same_arenas(on, off, 'the group after a skipped one', ('params', 'adam_m', 'adam_v', 'ema'))


class _CountingLibrary:
  """Stands in for the loaded library: records the calls of every entry point that is handed a stream."""

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


def test_a_model_without_the_option_is_untouched(dev, monkeypatch):
  """grad_accum_steps None or 1: no accumulator, and the launches of a step are those of a model that never heard of the option, in both
  layouts; the option's forms are that list with the accumulate launch in (first) or in front of (last) the optimiser's launches."""
  from geeco_amd import _native
  new = 'geeco_grad_accumulate_segments'
  never, none, one, on = _model(dev, 'e2e_vmc'), _model(dev, 'e2e_vmc', grad_accum_steps=None), _model(dev, 'e2e_vmc', grad_accum_steps=1), \
      _model(dev, 'e2e_vmc', grad_accum_steps=2)
  batch = GA.micro_batches('e2e_vmc', 1)[0]
  for m in (never, none, one, on):
    _load(m, batch)
  for m in (never, none, one):
    assert m.grad_accum is None and m.store.accum is None and m.store.accum_loss_sum is None and m.micro_step_form() is None
  counter = _CountingLibrary(_native.load())
  monkeypatch.setattr(_native, '_lib', counter)

  def calls_of(step):
    del counter.calls[:]
    step()
    torch.cuda.synchronize()
    return list(counter.calls)

  def beside(m):
    m.forward(backward_too=True)
    m.backward_and_apply(*_buckets(m))

  plain, side = calls_of(never.train_step), calls_of(lambda: beside(never))
  assert plain.count('geeco_adam_tf') == 1 and side.count('geeco_adam_tf_segments') == 2 and new not in plain + side
  for m in (none, one):
    assert calls_of(m.train_step) == plain and calls_of(lambda: beside(m)) == side
  first, last = calls_of(lambda: on.micro_step(_buckets(on))), calls_of(lambda: on.micro_step(_buckets(on)))
  assert first.count(new) == 2 and 'geeco_adam_tf_segments' not in first and len(first) == len(side)
  assert last.count(new) == 2 and last.count('geeco_adam_tf_segments') == 2 and len(last) == len(side) + 2
  first, last = calls_of(on.micro_step), calls_of(on.micro_step)
  assert first.count(new) == 1 and 'geeco_adam_tf' not in first and len(first) == len(plain)
  assert last.count(new) == 1 and last.count('geeco_adam_tf') == 1 and len(last) == len(plain) + 1


def test_more_than_one_rank_is_refused(dev, monkeypatch):
  from geeco_amd import dist as gdist
  from geeco_amd import estimator as est
  from geeco_amd.runtime import TrainStepRunner
  on = _model(dev, 'e2e_vmc', grad_accum_steps=2)
  with pytest.raises(ValueError, match='grad_accum_steps is single-GPU'):
    TrainStepRunner(on, dp=True)
  monkeypatch.setattr(gdist, 'world_size', lambda: 2)
  with pytest.raises(ValueError, match='grad_accum_steps is single-GPU'):
    TrainStepRunner(on)
  _, cfg, _, _ = GA.case('e2e_vmc')
  with pytest.raises(ValueError, match=r"params\['grad_accum_steps'\] is single-GPU"):
    est.e2evmc_model_fn({'rgb': torch.zeros(4, GA.K3, GA.H, GA.H, 3, device=dev)}, None, est.ModeKeys.TRAIN,
                        {'e2evmc_config': cfg, 'grad_accum_steps': 2})


# ================================================================================================
# Estimator
# ================================================================================================
def _events(model_dir):
  return [json.loads(l) for l in open(os.path.join(model_dir, 'events.jsonl'))]


def test_estimator_counts_optimiser_steps(dev, tmp_path):
  """A = 2 on the tiny synthetic dataset: global_step = batches // 2, one events.jsonl line per optimiser step numbered by global_step, the
  logged loss the mean of the step's two micro-batch losses (against forward-only losses of a model without the option on the same
  weights, rtol 1e-6 as the other Estimator loss checks), steps=3 runs six batches, and a half group waits for the next train()."""
  from geeco_amd import estimator as est
  from geeco_amd import graph
  from geeco_amd import input_fn as I
  from geeco_amd.params import create_e2evmc_config
  root = str(tmp_path / 'ds')
  I.write_synthetic_dataset(root, 2, episode_length=9, img_hw=(GA.H, GA.H), seed=5)
  batches = list(I.pickplace_input_fn(root, 'default', 'train', window_size=GA.K3, batch_size=4, num_threads=2))
  assert len(batches) == 3 and all(int(f['rgb'].shape[0]) == 4 for f, _ in batches)
  cfg = create_e2evmc_config(dict(window_size=GA.K3, img_height=GA.H, img_width=GA.H, batch_size=4))
  params = {'e2evmc_config': cfg, 'log_steps': 1, 'debug': False, 'grad_accum_steps': 2}

  probe = graph.E2EVMC(cfg, 4, dev, training=True)      # no option: forward-only losses on given weights

  def loss_on(weights, batch):
    probe.store.params.copy_(weights)
    probe.store._params_rewritten()
    probe.load_batch({k: torch.as_tensor(v) for k, v in batch[0].items()}, {k: torch.as_tensor(v) for k, v in batch[1].items()})
    probe.forward(backward_too=False)
    return float(probe.loss)

  # six batches, then steps=3 of a longer input
  md = str(tmp_path / 'six')
  e = est.Estimator(est.e2evmc_model_fn, md, est.RunConfig(init_seed=4), dict(params))
  fresh = graph.build_store(cfg, False, dev)
  fresh.initialize(seed=4)
  w0 = fresh.params.clone()
  e.train(input_fn=lambda: iter(batches + batches), steps=1)
  assert e.last_train_stats['steps'] == 1 and e.last_train_stats['micro_steps'] == 2 and int(e._store.global_step.item()) == 1
  w1 = e._store.params.clone()
  e.train(input_fn=lambda: iter(batches[2:] + batches + batches[:1]))      # five batches: two steps and a half group
  assert e.last_train_stats == dict(e.last_train_stats, steps=2, micro_steps=5) and int(e._store.global_step.item()) == 3
  assert e._store.accum_count == 1
  ev = _events(md)
  assert [line['global_step'] for line in ev] == [1, 2, 3]
  np.testing.assert_allclose(ev[0]['loss'], np.mean([loss_on(w0, batches[0]), loss_on(w0, batches[1])]), rtol=1e-6)
  np.testing.assert_allclose(ev[1]['loss'], np.mean([loss_on(w1, batches[2]), loss_on(w1, batches[0])]), rtol=1e-6)
  # the half group is completed by the next call: 2 + 5 + 1 = 8 batches, four optimiser steps
  e.train(input_fn=lambda: iter(batches[:1]))
  assert int(e._store.global_step.item()) == 4 and e._store.accum_count == 0 and e.last_train_stats['micro_steps'] == 1
  assert [line['global_step'] for line in _events(md)] == [1, 2, 3, 4]
  # steps=3 runs six batches of a longer input
  md = str(tmp_path / 'steps')
  e = est.Estimator(est.e2evmc_model_fn, md, est.RunConfig(init_seed=4), dict(params))
  e.train(input_fn=lambda: iter(batches * 4), steps=3)
  assert e.last_train_stats['steps'] == 3 and e.last_train_stats['micro_steps'] == 6 and int(e._store.global_step.item()) == 3
  # an odd batch count, twice: total batches // 2
  md = str(tmp_path / 'odd')
  e = est.Estimator(est.e2evmc_model_fn, md, est.RunConfig(init_seed=4), dict(params))
  e.train(input_fn=lambda: iter(batches))
  assert int(e._store.global_step.item()) == 1 and e._store.accum_count == 1
  e.train(input_fn=lambda: iter(batches))
  assert int(e._store.global_step.item()) == 3 and e._store.accum_count == 0
  assert [line['global_step'] for line in _events(md)] == [1, 2, 3]
