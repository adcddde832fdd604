"""Fine-tuning on the GPU: geeco_adam_tf_segments_scaled (bitwise the existing Adam entry points at multiplier 1, the
float64 reference of tests/_primitive_refs.py at other multipliers, graph replay), the models' optimiser step and cut points, and the
Estimator's warm start.  tests/_finetune_ref.py restates the semantics."""
import collections
import json
import os

import numpy as np
import pytest
import torch

import _clip_ref as C
import _finetune_ref as F
import _primitive_refs as R

pytestmark = pytest.mark.gpu

ADAM = dict(beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=0.125)      # tests/test_primitives_gpu.py
REF = dict(b1=0.9, b2=0.999, eps=1e-8, grad_scale=0.125)
L2 = 1e-3
N_ARENA = 4096 + 7
PIECES = [(0, 4), (16, 12), (64, 1028), (2048, 2055)]      # (offset, count): a single float4 .. a piece that ends in a 3-element tail
SENTINELS = np.array([0x7fc01234, 0xffc00001, 0x7f800001, 0xdeadbeef, 0x00000001, 0x80000000, 0x7f7fffff], np.uint32)
_ARENA = {}


def _arena():
  """p, g, m, v, ema (float32 numpy) of the kernel tests, built once: R.adam_inputs inside the pieces, sentinel bit patterns (NaN
  payloads among them) in every gap of p, m, v and ema."""
  if not _ARENA:
    p, g, m, v = R.adam_inputs(N_ARENA, 31)
    ema = (p + np.float32(0.01) * np.random.default_rng(5).standard_normal(N_ARENA).astype(np.float32)).astype(np.float32)
    inside = np.zeros(N_ARENA, bool)
    for o, c in PIECES:
      inside[o:o + c] = True
    fill = SENTINELS[np.arange(N_ARENA) % SENTINELS.size].view(np.float32)
    for a in (p, m, v, ema):
      a[~inside] = fill[~inside]
    _ARENA.update(p=p, g=g, m=m, v=v, ema=ema, inside=inside)
  return _ARENA


def _dev(dev, a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t):
  return t.detach().cpu().numpy().view(np.uint32).copy()


def _state(dev, ema, g_out):
  A = _arena()
  st = {k: _dev(dev, A[k]) for k in ('p', 'm', 'v')}
  st['ema'] = _dev(dev, A['ema']) if ema else None
  st['g_out'] = torch.from_numpy(SENTINELS[np.arange(N_ARENA) % SENTINELS.size].view(np.float32).copy()).to(dev) if g_out else None
  return st


def _sources(dev):
  """Every piece's gradients in a buffer of its own (16-byte aligned: a fresh allocation)."""
  A = _arena()
  return [_dev(dev, A['g'][o:o + c]) for o, c in PIECES]


def _scalars(dev, t=5):
  scal = torch.tensor([float(np.float32(R.lr_t_ref(0.001, 0.9, 0.999, t))), 0.0, 0.0, 0.0], dtype=torch.float32, device=dev)
  return scal, torch.tensor([t], dtype=torch.int64, device=dev)


def _existing(dev, st, srcs, scal, step, clip, guard):
  """The update through the entry points that existed before: _guard / _clip where a guard / a scale is given, else
  geeco_adam_tf_segments[_ema] for the whole-float4 pieces and geeco_adam_tf[_ema] on the piece with the tail."""
  from geeco_amd import ops
  segs = [(s, o, c) for s, (o, c) in zip(srcs, PIECES)]
  ema = dict(ema=st['ema'], global_step=step, decay=0.9) if st['ema'] is not None else {}
  if guard is not None:
    one = clip if clip is not None else torch.ones(2, dtype=torch.float32, device=dev)
    ops.adam_tf_segments_guard(st['p'], st['m'], st['v'], segs, scal, one, guard, g_out=st['g_out'], l2=L2, **ema, **ADAM)
  elif clip is not None:
    ops.adam_tf_segments_clip(st['p'], st['m'], st['v'], segs, scal, clip, g_out=st['g_out'], l2=L2, **ema, **ADAM)
  else:
    whole, (src, off, cnt) = segs[:3], segs[3]
    assert cnt % 4 == 3 and all(c % 4 == 0 for _, _, c in whole)
    sl = slice(off, off + cnt)
    if st['ema'] is not None:
      ops.adam_tf_segments_ema(st['p'], st['m'], st['v'], st['ema'], whole, scal, step, 0.9, g_out=st['g_out'], l2=L2, **ADAM)
      ops.adam_tf_ema(st['p'][sl], src, st['m'][sl], st['v'][sl], st['ema'][sl], cnt, scal, step, 0.9, l2=L2, **ADAM)
    else:
      ops.adam_tf_segments(st['p'], st['m'], st['v'], whole, scal, g_out=st['g_out'], l2=L2, **ADAM)
      ops.adam_tf(st['p'][sl], src, st['m'][sl], st['v'][sl], cnt, scal, l2=L2, **ADAM)
    if st['g_out'] is not None:
      st['g_out'][sl].copy_(src)


@pytest.mark.parametrize('g_out', [False, True], ids=['no g_out', 'g_out'])
@pytest.mark.parametrize('guard', [None, 1, 0], ids=['no guard', 'applied', 'skipped'])
@pytest.mark.parametrize('clip', [False, True], ids=['no clip', 'clip'])
@pytest.mark.parametrize('ema', [False, True], ids=['plain', 'shadow arena'])
def test_every_multiplier_one_is_bitwise_the_existing_entry_point(dev, ema, clip, guard, g_out):
  """p, m, v, the shadow arena and g_out as unsigned integers, the whole arena: the pieces equal what the existing entry point leaves,
  the gaps (sentinels, NaN payloads among them) keep every bit.  A verdict of 0 writes g_out alone."""
  from geeco_amd import ops
  A = _arena()
  srcs = _sources(dev)
  scal, step = _scalars(dev)
  clip_dev = torch.tensor([0.37, 9.0], dtype=torch.float32, device=dev) if clip else None
  guard_dev = torch.tensor([guard, 3, 1], dtype=torch.int64, device=dev) if guard is not None else None
  a, b = _state(dev, ema, g_out), _state(dev, ema, g_out)
  kw = dict(ema=a['ema'], global_step=step, decay=0.9) if ema else {}
  ops.adam_tf_segments_scaled(a['p'], a['m'], a['v'], [(s, o, c) for s, (o, c) in zip(srcs, PIECES)], [1.0] * len(PIECES), scal,
                              clip_dev=clip_dev, guard=guard_dev, g_out=a['g_out'], l2=L2, **kw, **ADAM)
  _existing(dev, b, srcs, scal, step, clip_dev, guard_dev)
  torch.cuda.synchronize()
  inside = A['inside']
  for k in ('p', 'm', 'v') + (('ema',) if ema else ()):
    got, want, start = _bits(a[k]), _bits(b[k]), A[k].view(np.uint32)
    assert np.array_equal(got, want), k
    assert np.array_equal(got[~inside], start[~inside]), k + ': a gap moved'
    assert np.array_equal(got[inside], start[inside]) == (guard == 0), k
  if g_out:
    got = _bits(a['g_out'])
    assert np.array_equal(got, _bits(b['g_out']))
    assert np.array_equal(got[inside], A['g'].view(np.uint32)[inside])
    assert np.array_equal(got[~inside], SENTINELS[np.arange(N_ARENA) % SENTINELS.size][~inside])
  if guard_dev is not None:
    assert guard_dev.tolist() == [guard, 3, 1]


MULS = (1.0, 0.1, 3.0, 0.5)


def test_two_steps_at_four_multipliers_against_float64(dev):
  """adam_prepare + the scaled update, twice: every piece's p, m, v against adam_ref at float32(lr_t * multiplier), carried forward
  from the device's own previous state, within adam_bounds -- reference and tolerance of geeco_adam_tf's test.  The shadow arena
  follows the new parameters as the EMA kernels' does; the gaps do not move."""
  from geeco_amd import ops
  from geeco_amd.variables import ema_decay_at
  A = _arena()
  srcs = _sources(dev)
  st = _state(dev, True, False)
  step = torch.tensor([4], dtype=torch.int64, device=dev)
  scal = torch.zeros(4, dtype=torch.float32, device=dev)
  segs = [(s, o, c) for s, (o, c) in zip(srcs, PIECES)]
  for t in (5, 6):
    before = {k: st[k].detach().cpu().numpy().copy() for k in ('p', 'm', 'v', 'ema')}
    ops.adam_prepare(step, 0.001, scal)
    ops.adam_tf_segments_scaled(st['p'], st['m'], st['v'], segs, MULS, scal, ema=st['ema'], global_step=step, decay=0.9, l2=L2, **ADAM)
    torch.cuda.synchronize()
    assert step.tolist() == [t]
    lr_t = float(scal[0])
    d = ema_decay_at(0.9, t)
    for (o, c), mul in zip(PIECES, MULS):
      sl = slice(o, o + c)
      ref, bounds = F.adam_ref(before['p'][sl], A['g'][sl], before['m'][sl], before['v'][sl], lr_t, mul, l2=L2, **REF)
      for name, r, b in zip('pmv', ref, bounds):
        got = st[name][sl].detach().cpu().numpy()
        print('step %d piece (%d, %d) x %g: %s %.3f of its bound' % (t, o, c, mul, name, R.worst_ratio(got, r, b)))
        R.assert_within(got, r, b, 'piece (%d, %d) x %g step %d: %s' % (o, c, mul, t, name))
      pn = st['p'][sl].detach().cpu().numpy()
      want = (pn + (before['ema'][sl] - pn) * d).astype(np.float32)       # ema' = p' + (ema - p') d_t, the EMA kernels' form
      np.testing.assert_allclose(st['ema'][sl].detach().cpu().numpy(), want, rtol=0, atol=2 * R.U * float(np.abs(want).max() + np.abs(pn).max()))
    for k in ('p', 'm', 'v', 'ema'):
      assert np.array_equal(_bits(st[k])[~A['inside']], A[k].view(np.uint32)[~A['inside']]), k
  o, c = PIECES[2]
  assert not np.array_equal(_bits(st['p'])[o:o + c], A['p'].view(np.uint32)[o:o + c])


def test_a_replayed_graph_follows_the_device_counter(dev):
  """adam_prepare + the scaled update captured once and replayed three times equals three eager calls bit for bit: lr_t is read
  from the device at every replay, not frozen at capture."""
  from geeco_amd import ops
  from geeco_amd.runtime import capture_graphs
  srcs = _sources(dev)
  segs = [(s, o, c) for s, (o, c) in zip(srcs, PIECES)]
  runs = []
  for graph in (False, True):
    st = _state(dev, True, True)
    step = torch.tensor([0], dtype=torch.int64, device=dev)
    scal = torch.zeros(4, dtype=torch.float32, device=dev)

    def one():
      ops.adam_prepare(step, 0.001, scal)
      ops.adam_tf_segments_scaled(st['p'], st['m'], st['v'], segs, MULS, scal, ema=st['ema'], global_step=step, decay=0.9, g_out=st['g_out'],
                                  l2=L2, **ADAM)

    lrs = []
    replay = capture_graphs([one])[0] if graph else one
    for _ in range(3):
      replay()
      torch.cuda.synchronize()
      lrs.append(float(scal[0]))
    assert step.tolist() == [3] and len(set(lrs)) == 3, lrs
    runs.append((st, lrs))
  (a, la), (b, lb) = runs
  assert la == lb
  for k in ('p', 'm', 'v', 'ema', 'g_out'):
    assert np.array_equal(_bits(a[k]), _bits(b[k])), k


# ================================================================================================
# the models
# ================================================================================================
def _tensors(d):
  return {k: torch.from_numpy(v) for k, v in d.items()}


def _model(dev, name, **kw):
  from geeco_amd import graph
  _, cfg, goal, P, feats, labels = F.case(name)
  model = (graph.GoalE2EVMC if goal else graph.E2EVMC)(cfg, F.N, dev, training=True, **kw)
  model.store.load_numpy(P)
  model.load_batch(_tensors(feats), _tensors(labels))
  return model


def _var_bits(store, which, name):
  arena = getattr(store, which)
  o, c = store.offsets[name], int(np.prod(store.shapes[name]))
  return arena[o:o + c].view(torch.int32)


class _CountingLibrary:
  """Stands in for the loaded library: records the calls of every entry point (tests/test_skip_nonfinite_gpu.py)."""

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


def _calls_of(step):
  """The library calls of ``step()``, in order."""
  from geeco_amd import _native
  lib = _native.load()
  counter = _CountingLibrary(lib)
  _native._lib = counter
  try:
    step()
    torch.cuda.synchronize()
  finally:
    _native._lib = lib
  return counter.calls


def _encoder_layers(model, monkeypatch):
  """Records (kind, layer) of every filter- and input-gradient launch the encoder stack is asked for."""
  seen = []
  for kind in ('launch_wgrad', 'launch_dgrad'):
    real = getattr(model.enc, kind)
    monkeypatch.setattr(model.enc, kind, lambda l, *a, _real=real, _kind=kind, **kw: (seen.append((_kind, l)), _real(l, *a, **kw))[1])
  return seen


BOTTOM = ('geeco_conv2_dgrad_conv1_wgrad_bits', 'geeco_conv2_dgrad_conv1_wgrad', 'geeco_conv2_dgrad_conv1_wgrad_partial')


@pytest.mark.parametrize('name', list(F.MODELS))
def test_bottom_frozen_one_step_from_equal_weights(dev, name, monkeypatch):
  """Every trainable variable's p, m, v and averaged weight is bitwise that of the model without the option; every frozen one's is
  bitwise its initial value; the fused bottom, conv2's filter gradient and conv3's input gradient are never launched."""
  a, b = _model(dev, name, lr_multipliers={'/conv[12]/': 0}, ema_decay=0.9), _model(dev, name, ema_decay=0.9)
  assert a.backward_cut == 'no_bottom' and b.backward_cut == 'full' and b.lr_runs is None and not a.can_apply_beside_bottom()
  assert len(a.lr_runs) == (3 if name == 'geeco-f' else 1)
  start = {k: getattr(a.store, k).detach().clone() for k in ('params', 'adam_m', 'adam_v', 'ema')}
  layers = _encoder_layers(a, monkeypatch)
  calls_a = _calls_of(a.train_step)
  calls_b = _calls_of(b.train_step)
  frozen = [n for n in a.store.shapes if a.lr_multipliers[n] == 0.0]
  assert len(frozen) == 4 * len([n for n in a.store.shapes if n.endswith('/conv1/kernel')])
  for n in a.store.shapes:
    for k in ('params', 'adam_m', 'adam_v', 'ema'):
      got = _var_bits(a.store, k, n)
      if n in frozen:
        o = a.store.offsets[n]
        assert torch.equal(got, start[k][o:o + got.numel()].view(torch.int32)), (n, k)
      else:
        assert torch.equal(got, _var_bits(b.store, k, n)), (n, k)
  assert int(a.store.global_step.item()) == 1
  lo, cnt, _ = a.lr_runs[-1]
  for k in ('params', 'adam_m', 'adam_v'):      # (the trainable part did move)
    assert not torch.equal(getattr(a.store, k)[lo:lo + cnt], start[k][lo:lo + cnt]), k
  assert not any(c in BOTTOM for c in calls_a) and any(c in BOTTOM for c in calls_b)
  assert layers and not [x for x in layers if x in (('launch_wgrad', 0), ('launch_wgrad', 1), ('launch_dgrad', 1), ('launch_dgrad', 2))]
  assert calls_a.count('geeco_adam_tf_segments_scaled') == 1 and 'geeco_adam_tf_ema' not in calls_a
  # a strict subset of the launches of the full step
  extra = collections.Counter(calls_a) - collections.Counter(calls_b)
  del extra['geeco_adam_tf_segments_scaled'], extra['geeco_dynimg_alpha']      # (the second: a host-side table, filled once per process)
  print('%s: %d library calls with the bottom frozen, %d without the option' % (name, len(calls_a), len(calls_b)))
  assert not extra and len(calls_a) < len(calls_b), extra


def test_encoders_frozen_graph_and_eager(dev, monkeypatch):
  """geeco-f with every encoder frozen: no encoder backward launch at all; three steps through TrainStepRunner (captured) and three
  eager train_steps leave bitwise the same decoder variables; the encoders' part of every arena is bitwise initial."""
  from geeco_amd.runtime import TrainStepRunner
  name = 'geeco-f'
  a, b = _model(dev, name, lr_multipliers={'Encoder/': 0}), _model(dev, name, lr_multipliers={'Encoder/': 0})
  assert a.backward_cut == 'decoder_only' and len(a.lr_runs) == 1
  start = {k: getattr(a.store, k).detach().clone() for k in ('params', 'adam_m', 'adam_v')}

  def never(*args, **kw):
    raise AssertionError('an encoder backward half was asked for')
  for m in (a, b):
    monkeypatch.setattr(m.enc, 'backward_upper', never)
    monkeypatch.setattr(m.enc, 'backward_bottom', never)
  calls = _calls_of(a.train_step)
  assert not [c for c in calls if 'wgrad' in c or 'dgrad' in c or 'conv_top_bwd' in c], calls
  a.train_step()
  a.train_step()
  runner = TrainStepRunner(b, use_graph=True, warmup=1)
  assert not runner.beside_bottom
  for _ in range(3):
    runner.step()
  torch.cuda.synchronize()
  assert runner._graphs is not None and len(runner._graphs) == 1
  assert int(a.store.global_step.item()) == int(b.store.global_step.item()) == 3
  lo, cnt, mul = a.lr_runs[0]
  assert mul == 1.0 and lo + cnt == a.store.size and lo == a.store.offsets['GoalVMC/LSTMDecoder/lstm_cell/kernel']
  for k in ('params', 'adam_m', 'adam_v'):
    x, y = getattr(a.store, k).view(torch.int32), getattr(b.store, k).view(torch.int32)
    assert torch.equal(x, y), k
    assert torch.equal(x[:lo], start[k][:lo].view(torch.int32)), k + ': an encoder variable moved'
    assert not torch.equal(x[lo:], start[k][lo:].view(torch.int32)), k
  assert bool(torch.isfinite(a.store.params).all())


CLIP = 0.01             # below the norm of every clean step these models take (tests/test_clip_gpu.py)


@pytest.mark.parametrize('name', list(F.MODELS))
def test_encoders_at_a_tenth_against_float64(dev, name):
  """forward + backward, the device's gradient copied, then the optimiser step: every variable against adam_ref at
  float32(lr_t * its multiplier) within adam_bounds.  With clip_norm below the norm, clip_out[1] is the float64 norm over the
  TRAINABLE pieces only (the tolerance of tests/test_clip_gpu.py's step test: 60 U)."""
  table = {'Encoder/conv[45]/': 0, 'Encoder/': 0.1}      # (conv4 / conv5 frozen ABOVE the cut: their gradients are computed, not applied)
  m = _model(dev, name, lr_multipliers=table)
  assert m.backward_cut == 'full'
  m.forward(backward_too=True)
  m.backward()
  torch.cuda.synchronize()
  before = {k: m.store.to_numpy(k) for k in ('params', 'grads', 'adam_m', 'adam_v')}
  m.apply_gradients()
  torch.cuda.synchronize()
  lr_t = float(m.scal[0])
  after = {k: m.store.to_numpy(k) for k in ('params', 'adam_m', 'adam_v')}
  mults = F.multipliers(table, m.store.shapes)
  assert mults == m.lr_multipliers and set(mults.values()) == {0.0, float(np.float32(0.1)), 1.0}
  for n, mul in mults.items():
    if mul == 0.0:
      for k in after:
        assert np.array_equal(after[k][n].view(np.uint32), before[k][n].view(np.uint32)), (n, k)
      continue
    flat = lambda k: before[k][n].reshape(-1)
    ref, bounds = F.adam_ref(flat('params'), flat('grads'), flat('adam_m'), flat('adam_v'), lr_t, mul, b1=0.9, b2=0.999, eps=1e-8)
    for k, r, b in zip(('params', 'adam_m', 'adam_v'), ref, bounds):
      R.assert_within(after[k][n].reshape(-1), r, b, '%s x %g: %s' % (n, mul, k))
  # ... and under clip_norm
  c = _model(dev, name, lr_multipliers=table, clip_norm=CLIP)
  c.train_step()
  torch.cuda.synchronize()
  g, p = c.store.to_numpy('grads'), c.store.to_numpy('params')
  sq_train = sum(float(np.sum(C.total_grad(p[n], g[n]) ** 2)) for n, mul in mults.items() if mul != 0.0)
  sq_all = sum(float(np.sum(C.total_grad(p[n], g[n]) ** 2)) for n in mults)
  norm = float(np.sqrt(sq_train))
  print('%s: norm over the trainable pieces %.6g (device %.6g), over every variable %.6g' % (name, norm, float(c.clip_out[1]), np.sqrt(sq_all)))
  assert norm > CLIP and 0.0 < float(c.clip_out[0]) < 1.0
  assert abs(float(c.clip_out[1]) - norm) <= 60 * R.U * norm
  assert abs(np.sqrt(sq_all) - norm) > 1000 * R.U * norm      # the frozen variables' gradients would have shown


def test_a_nan_in_a_frozen_slot_cannot_cause_a_skip_and_a_trainable_one_does(dev):
  name = 'e2e_vmc'
  m = _model(dev, name, lr_multipliers={'/conv[12]/': 0}, skip_nonfinite=True)
  frozen, trainable = 'VMC/ConvEncoder/conv1/kernel', 'VMC/ConvEncoder/conv5/bias'
  # the bottom is not run: the frozen variables' gradient slots keep what is written there
  m.store.grad(frozen).view(-1)[7] = float('nan')
  start = m.store.params.detach().clone()
  m.train_step()
  torch.cuda.synchronize()
  assert m.guard.tolist() == [1, 0, 0] and np.isfinite(float(m.clip_out[1]))
  assert bool(torch.isnan(m.store.grad(frozen).view(-1)[7])) and not torch.equal(m.store.params, start)
  assert bool(torch.isfinite(m.store.params).all())
  # a NaN in a trainable variable's gradient, in front of the optimiser step alone
  state = {k: getattr(m.store, k).detach().clone() for k in ('params', 'adam_m', 'adam_v')}
  m.forward(backward_too=True)
  m.backward()
  m.store.grad(trainable).view(-1)[3] = float('nan')
  m.apply_gradients()
  torch.cuda.synchronize()
  assert m.guard.tolist() == [0, 1, 1] and not np.isfinite(float(m.clip_out[1]))
  for k, v in state.items():
    assert torch.equal(getattr(m.store, k).view(torch.int32), v.view(torch.int32)), k


def test_a_model_without_the_option_is_untouched(dev):
  """lr_multipliers None, empty or all ones: no runs, the full backward, the calls of a step are the same list in the same order as
  the model built without the argument, in both schedules, and the parameters are bitwise the same; none calls the new entry point."""
  from geeco_amd.runtime import gradient_buckets
  name = 'e2e_vmc'
  off = _model(dev, name)
  same = [_model(dev, name, lr_multipliers=None), _model(dev, name, lr_multipliers={}), _model(dev, name, lr_multipliers={'Encoder/': 1.0, 'fc1': 1})]
  early, late = gradient_buckets(off.store)

  def beside(m):
    m.forward(backward_too=True)
    m.backward_and_apply(early, late)

  plain_off, side_off = _calls_of(off.train_step), _calls_of(lambda: beside(off))
  assert plain_off.count('geeco_adam_tf') == 1 and side_off.count('geeco_adam_tf_segments') == 2
  assert 'geeco_adam_tf_segments_scaled' not in plain_off + side_off
  for m in same:
    assert m.lr_multipliers is None and m.lr_runs is None and m.backward_cut == 'full' and m.can_apply_beside_bottom()
    assert _calls_of(m.train_step) == plain_off
    assert _calls_of(lambda: beside(m)) == side_off
    for k in ('params', 'adam_m', 'adam_v', 'grads'):
      assert torch.equal(getattr(m.store, k).view(torch.int32), getattr(off.store, k).view(torch.int32)), k
  # the option on, full backward: beside the bottom with the buckets cut at the runs, bitwise the plain path
  on_a, on_b = _model(dev, name, lr_multipliers={'Encoder/': 0.1}), _model(dev, name, lr_multipliers={'Encoder/': 0.1})
  assert on_a.can_apply_beside_bottom() and on_a.backward_cut == 'full'
  side_on = _calls_of(lambda: beside(on_a))
  plain_on = _calls_of(on_b.train_step)
  assert side_on.count('geeco_adam_tf_segments_scaled') == 2 and plain_on.count('geeco_adam_tf_segments_scaled') == 1
  assert len(side_on) == len(side_off) and len(plain_on) == len(plain_off)
  for k in ('params', 'adam_m', 'adam_v', 'grads'):
    assert torch.equal(getattr(on_a.store, k).view(torch.int32), getattr(on_b.store, k).view(torch.int32)), k


# ================================================================================================
# Estimator
# ================================================================================================
def _events(model_dir):
  return [json.loads(l) for l in open(os.path.join(model_dir, 'events.jsonl'))]


def test_estimator_warm_start_and_frozen_encoders(dev, tmp_path, monkeypatch):
  """Two steps and a checkpoint; a second Estimator warm-started from that directory with the encoders frozen starts at step 0 with
  the first run's weights, trains two steps, keeps the encoder variables bitwise and moves the decoder's; events.jsonl carries the
  trainable / frozen line; more than one rank, or shared_frames, is refused with the key."""
  from geeco_amd import dist as gdist
  from geeco_amd import estimator as est
  from geeco_amd import input_fn as I
  from geeco_amd.params import create_e2evmc_config
  root = str(tmp_path / 'ds')
  I.write_synthetic_dataset(root, 2, episode_length=9, img_hw=(F.H, F.H), seed=5)
  batches = list(I.pickplace_input_fn(root, 'default', 'train', window_size=F.K, batch_size=4, num_threads=2))[:2]
  cfg = create_e2evmc_config(dict(window_size=F.K, img_height=F.H, img_width=F.H, batch_size=4))
  plain = {'e2evmc_config': cfg, 'log_steps': 1, 'debug': False}
  md1, md2 = str(tmp_path / 'first'), str(tmp_path / 'second')
  e1 = est.Estimator(est.e2evmc_model_fn, md1, est.RunConfig(init_seed=4), dict(plain))
  e1.train(input_fn=lambda: iter(batches))
  first = e1._store.to_numpy('params')
  assert int(e1._store.global_step.item()) == 2 and est.latest_checkpoint(md1) is not None
  e2 = est.Estimator(est.e2evmc_model_fn, md2, est.RunConfig(init_seed=99), dict(plain, lr_multipliers={'Encoder/': 0}), warm_start_from=md1)
  seen = {}
  real = est.Estimator._restore_once

  def restore(self):
    real(self)
    seen.setdefault('step', int(self._store.global_step.item()))
    seen.setdefault('params', self._store.to_numpy('params'))
    seen.setdefault('m', float(self._store.adam_m.abs().sum()))
  monkeypatch.setattr(est.Estimator, '_restore_once', restore)
  e2.train(input_fn=lambda: iter(batches))
  assert seen['step'] == 0 and seen['m'] == 0.0
  second = e2._store.to_numpy('params')
  assert int(e2._store.global_step.item()) == 2
  for n in first:
    assert np.array_equal(seen['params'][n], first[n]), n
    if 'Encoder/' in n:
      assert np.array_equal(second[n].view(np.uint32), first[n].view(np.uint32)), n
    else:
      assert not np.array_equal(second[n], first[n]), n
  ev = _events(md2)
  total = e2._store.count_parameters()
  frozen = sum(int(np.prod(s)) for n, s in e2._store.shapes.items() if 'Encoder/' in n)
  assert ev[0]['frozen_parameters'] == frozen and ev[0]['trainable_parameters'] == total - frozen and ev[0]['backward_cut'] == 'decoder_only'
  assert ev[0]['global_step'] == 0 and [line['global_step'] for line in ev[1:]] == [1, 2]
  assert not any('trainable_parameters' in line for line in _events(md1))
  # the scope limits
  feats = {'rgb': torch.zeros(4, F.K, F.H, F.H, 3, device=dev)}
  with pytest.raises(ValueError, match=r"params\['lr_multipliers'\] with params\['shared_frames'\]"):
    est.e2evmc_model_fn(feats, None, est.ModeKeys.TRAIN, dict(plain, lr_multipliers={'Encoder/': 0}, shared_frames=True))
  monkeypatch.setattr(gdist, 'world_size', lambda: 2)
  with pytest.raises(ValueError, match=r"params\['lr_multipliers'\] is single-GPU: with 2 ranks"):
    est.e2evmc_model_fn(feats, None, est.ModeKeys.TRAIN, dict(plain, lr_multipliers={'Encoder/': 0}))
