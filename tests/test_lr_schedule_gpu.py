"""The learning-rate schedules on the GPU: the two entry points that do the optimiser's prepare work under a schedule,
the step that calls them -- captured once and replayed -- and the Estimator / command-line surface on top.
Reference: tests/_lr_schedule_ref.py (float64, parameters rounded to float32 as the device holds them).

Tolerances: scal[0] = lr_t is double arithmetic on the device (pow, cos, sqrt) and ONE rounding to float32: 4 U relative, the bound of
tests/test_primitives_gpu.py::test_adam_prepare for the same arithmetic.  scal[2] = lr(s) is the float32 nearest to the reference's
double (for 'piecewise' the value itself); the device's pow / cos may differ from the host's in the last bits of the double, which
moves the float32 only when the double sits within ~1e-16 relative of a rounding boundary -- none of the cases here does.
The models are the smallest of tests/test_clip_gpu.py's whole-step tests (136 x 136, K = 3, N = 4)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _lr_schedule_ref as L
import _primitive_refs as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float('nan')
U = R.U

W, DS = 5, 7
KINDS = {
    'constant': L.schedule('constant', base_lr=1e-3, warmup_steps=W),
    'exponential': L.schedule('exponential', base_lr=1e-3, warmup_steps=W, decay_steps=1000, decay_rate=0.96),      # (0.96^100 at 99999: a normal float32)
    'exponential, staircase': L.schedule('exponential', base_lr=1e-3, warmup_steps=W, decay_steps=DS, decay_rate=0.96, staircase=True),
    'cosine': L.schedule('cosine', base_lr=3e-4, warmup_steps=W, decay_steps=DS, alpha=0.1),
    'piecewise': L.schedule('piecewise', warmup_steps=W, boundaries=(DS, 2 * DS, 99990), values=(1e-3, 1e-4, 1e-2, 3e-5)),
}
STARTS = {'0': 0, 'w - 1': W - 1, 'w': W, 'a boundary': W + DS, '99999': 99999}      # the counter before the call (= s)
# (the staircase with 7-step periods has left float32's range long before 99999 -- 0.96^14285: it is checked up to the boundary)
CASES = [(k, s) for k in KINDS for s in STARTS if (k, s) != ('exponential, staircase', '99999')]


def _f32(x):
  return np.float32(x)


def _bits(t):
  return t.detach().cpu().numpy().view(np.uint32)


def _scal_and_step(dev, t0):
  """scal: four NaNs and a NaN guard of three behind them (the entry point gets the first four); the counter and a guard."""
  buf = torch.full((7,), NAN, dtype=torch.float32, device=dev)
  return buf, buf[:4], torch.tensor([t0, -7], dtype=torch.int64, device=dev)


def _check_scalars(buf, step, sch, s, what):
  """scal[0], scal[2] against the reference at s completed updates; the counter moved by one; everything else still NaN."""
  got = buf.cpu().numpy()
  lr_t, lr = L.lr_t_at(sch, s), L.lr_at(sch, s)
  print('%s s=%d: lr_t %.9g (ref %.9g, off by %.2f U), lr %.9g (ref %.9g)' % (what, s, got[0], lr_t, abs(float(got[0]) - lr_t) / (U * lr_t), got[2], lr))
  assert step.tolist() == [s + 1, -7], what
  assert abs(float(got[0]) - lr_t) <= 4 * U * lr_t, (what, s, got[0], lr_t)
  assert got[2] == _f32(lr), (what, s, got[2], lr)
  assert np.isnan(got[1]) and np.isnan(got[3:]).all(), (what, got)


# ================================================================================================
# the entry points
# ================================================================================================
@pytest.mark.parametrize('kind,start', CASES)
def test_adam_prepare_schedule(dev, kind, start):
  from geeco_amd import ops
  sch, s = KINDS[kind], STARTS[start]
  buf, scal, step = _scal_and_step(dev, s)
  ops.adam_prepare_schedule(step, sch, scal)
  torch.cuda.synchronize()
  _check_scalars(buf, step, sch, s, kind)


_SLABS = [(1, 5, 8, 4, True), (2, 17, 1024, 8, True), (3, 3, 36, 12, False), (1, 16, 64, 64, True)]      # groups, S, KC, Cout, bias


def _slab_inputs(dev):
  r = np.random.default_rng(77)
  return [torch.from_numpy(r.standard_normal(g * S * (KC + Cout)).astype(np.float32)).to(dev) for g, S, KC, Cout, _ in _SLABS]


def _pending(dev, parts):
  """The slab sums of _SLABS as pending items (S >= 16: the kernel's split form), their outputs NaN with a NaN guard of 5 floats."""
  from geeco_amd import _native
  items, outs = [], []
  for part, (g, S, KC, Cout, bias) in zip(parts, _SLABS):
    dw = torch.full((g * KC + 5,), NAN, dtype=torch.float32, device=dev)
    db = torch.full((g * Cout + 5,), NAN, dtype=torch.float32, device=dev)
    items.append(_native.SlabReduce(part.data_ptr(), dw.data_ptr(), db.data_ptr() if bias else None, KC, Cout, KC, S, Cout, g, 0))
    outs += [dw, db]
  return items, outs


@pytest.mark.parametrize('kind', ['cosine', 'piecewise'])
def test_slab_reduce_batch_with_a_schedule(dev, kind):
  """The sums are bitwise those of the plain launch over the same slabs (and the guards stay NaN); scal[0] / scal[2] are bitwise those
  of adam_prepare_schedule from the same counter, with pending items and with none."""
  from geeco_amd import ops
  sch = KINDS[kind]
  parts = _slab_inputs(dev)
  plain_items, plain = _pending(dev, parts)
  ops.slab_reduce_batch(plain_items)
  assert plain_items == []
  for s in (0, W - 1, W + DS + 1):
    buf0, scal0, step0 = _scal_and_step(dev, s)
    ops.adam_prepare_schedule(step0, sch, scal0)
    for n in (len(_SLABS), 0):
      items, outs = _pending(dev, parts)
      buf, scal, step = _scal_and_step(dev, s)
      names = ops.kernel_trace(lambda: ops.slab_reduce_batch(items[:n], (step, ops.lr_schedule_struct(sch), scal)))
      torch.cuda.synchronize()
      assert names == ['wgrad_reduce_batch_schedule_kernel'], names
      np.testing.assert_array_equal(_bits(buf), _bits(buf0), err_msg='scal, n=%d s=%d' % (n, s))
      assert step.tolist() == step0.tolist() == [s + 1, -7]
      for i, (a, b) in enumerate(zip(outs, plain)):
        if n:
          np.testing.assert_array_equal(_bits(a), _bits(b), err_msg='output %d' % i)
        else:
          assert torch.isnan(a).all()
    _check_scalars(buf, step, sch, s, kind + ', riding')
  for (g, S, KC, Cout, bias), dw, db in zip(_SLABS, plain[0::2], plain[1::2]):      # (the plain sums did run, inside their bounds)
    assert torch.isfinite(dw[:g * KC]).all() and torch.isnan(dw[g * KC:]).all()
    assert (torch.isfinite(db[:g * Cout]).all() if bias else torch.isnan(db).all()) and torch.isnan(db[g * Cout:]).all()
  # the schedule as the dictionary, too
  buf, scal, step = _scal_and_step(dev, 3)
  ops.slab_reduce_batch([], (step, sch, scal))
  torch.cuda.synchronize()
  _check_scalars(buf, step, sch, 3, kind + ', dictionary')


# ================================================================================================
# the step
# ================================================================================================
H, K3, N = 136, 3, 4
LR = 1e-3
# two warm-up steps, then tenfold up and tenfold down: s = 0, 1 warm up to 1e-3; s = 2, 3 run 1e-3; s = 4, 5 run 1e-2; from s = 6 on 1e-3
PIECEWISE = {'kind': 'piecewise', 'warmup_steps': 2, 'boundaries': [1, 3], 'values': [1e-3, 1e-2, 1e-3]}
COSINE = {'kind': 'cosine', 'warmup_steps': 2, 'decay_steps': 3}
STEPS = 7               # one eager step, as the runner warms up before it captures, and six replays: s = 0 .. 6, the jump down at s = 6
_CASE = []


def _case():
  """(ocfg, cfg, P, feats, labels) of e2e_vmc, once and left unchanged."""
  if not _CASE:
    from geeco_amd.params import create_e2evmc_config
    from oracle import geeco_oracle as O
    ocfg = O.make_config(window_size=K3, img_height=H, img_width=H, batch_size=N, lr=LR)
    P = O.init_params(O.model_param_shapes(ocfg, False), seed=1)
    feats, labels = O.synthetic_batch(ocfg, False, N, seed=3, H=H, W=H)
    _CASE.append((ocfg, create_e2evmc_config(ocfg._asdict()), P, feats, labels))
  return _CASE[0]


def _model(dev, **kw):
  from geeco_amd import graph
  ocfg, cfg, P, feats, labels = _case()
  model = graph.E2EVMC(cfg, N, dev, training=True, **kw)
  model.store.load_numpy(P)
  model.load_batch({k: torch.from_numpy(v) for k, v in feats.items()}, {k: torch.from_numpy(v) for k, v in labels.items()})
  return model


def _normalised(schedule, lr=LR):
  from geeco_amd.variables import check_lr_schedule
  return check_lr_schedule(schedule, lr)


def _check_step_scalars(model, sch, s, what):
  got = model.scal.cpu().numpy()
  lr_t, lr = L.lr_t_at(sch, s), L.lr_at(sch, s)
  print('%s s=%d: lr %.9g (ref %.9g), lr_t %.9g (ref %.9g)' % (what, s, got[2], lr, got[0], lr_t))
  assert got[2] == _f32(lr), (what, s, got[2], lr)
  assert abs(float(got[0]) - lr_t) <= 4 * U * lr_t, (what, s, got[0], lr_t)
  assert int(model.store.global_step.item()) == s + 1


@pytest.mark.parametrize('name', ['piecewise', 'cosine'])
def test_a_captured_step_follows_the_schedule(dev, name):
  """The test that fails without the feature: the step is captured ONCE (behind the runner's one eager warm-up step) and replayed six
  times with no host call in between; after every step scal[2] is the reference lr(s) and scal[0] the reference lr_t -- a rate
  handed over as a launch argument would be frozen at the capture's."""
  from geeco_amd.runtime import TrainStepRunner
  schedule = PIECEWISE if name == 'piecewise' else COSINE
  sch = _normalised(schedule)
  model = _model(dev, lr_schedule=schedule)
  runner = TrainStepRunner(model, use_graph=True, warmup=1)
  rates = []
  for s in range(STEPS):
    runner.step()
    torch.cuda.synchronize()
    assert (runner._graphs is not None) == (s >= 1)
    _check_step_scalars(model, sch, s, name)
    rates.append(float(model.scal[2]))
  assert len(runner._graphs) == 1
  if name == 'piecewise':
    assert rates == [float(_f32(x)) for x in (0.5e-3, 1e-3, 1e-3, 1e-3, 1e-2, 1e-2, 1e-3)]
  else:      # warm-up to 1e-3, cosine down to 0 at u = 3 and 0 from there on
    assert rates[1] == rates[2] == float(_f32(1e-3)) and rates[2] > rates[3] > rates[4] > rates[5] == rates[6] == 0.0


def test_trajectory_against_the_oracle(dev):
  """The same seven steps against the float64 oracle stepped with cfg.lr = lr(s): the parameters after EVERY step within the project's
  bound for a post-Adam comparison, atol = 2.5 lr(s) (tests/test_model_gpu.py); and on the first step behind the jump down (s = 6)
  no parameter moves by 2.5 lr(s) or more -- a device that were one step late would move them by ten times lr(s)."""
  from geeco_amd.runtime import TrainStepRunner
  from oracle import geeco_oracle as O
  ocfg, _, P, feats, labels = _case()
  sch = _normalised(PIECEWISE)
  model = _model(dev, lr_schedule=PIECEWISE)
  runner = TrainStepRunner(model, use_graph=True, warmup=1)
  ref = O.OracleTrainer(ocfg, False, P, dtype=torch.float64)
  before = model.store.to_numpy('params')
  for s in range(STEPS):
    lr = L.lr_at(sch, s)
    ref.cfg = ref.cfg._replace(lr=lr)
    ref.train_step(feats, labels)
    runner.step()
    torch.cuda.synchronize()
    got = model.store.to_numpy('params')
    worst = max(float(np.abs(got[k] - v.numpy()).max()) for k, v in ref.P.items())
    moved = max(float(np.abs(got[k] - before[k]).max()) for k in got)
    print('s=%d lr=%g: worst parameter difference to the oracle %.3g (%.2f lr), largest move %.3g (%.2f lr)' % (s, lr, worst, worst / lr, moved,
                                                                                                          moved / lr))
    for k, v in ref.P.items():
      np.testing.assert_allclose(got[k], v.numpy(), rtol=0, atol=2.5 * lr, err_msg='%s after step s=%d' % (k, s))
    if s == 6:
      assert lr == float(_f32(1e-3)) and L.lr_at(sch, 5) == float(_f32(1e-2))
      assert 0.25 * lr < moved < 2.5 * lr, (moved, lr)
    before = got


def _same_state(a, b, what=''):
  for name in ('params', 'adam_m', 'adam_v', 'grads'):
    assert torch.equal(getattr(a.store, name).view(torch.int32), getattr(b.store, name).view(torch.int32)), (what, name)
  assert int(a.store.global_step.item()) == int(b.store.global_step.item()), what


def test_a_constant_piecewise_schedule_is_the_plain_model(dev):
  """Every value = cfg.lr, no warm-up: parameters, m and v bitwise the plain model's after three steps (train_step, and the schedule with
  the optimiser beside the encoder bottom); scal[0] bitwise too, scal[2] = float32(cfg.lr) against the plain model's untouched 0."""
  from geeco_amd.runtime import gradient_buckets
  flat = {'kind': 'piecewise', 'boundaries': [1], 'values': [LR, LR]}
  plain, on, beside = _model(dev), _model(dev, lr_schedule=flat), _model(dev, lr_schedule=flat)
  early, late = gradient_buckets(plain.store)
  assert plain.lr_schedule is None and on.lr_schedule is not None and beside.can_apply_beside_bottom()
  for _ in range(3):
    plain.train_step()
    on.train_step()
    beside.forward(backward_too=True)
    beside.backward_and_apply(early, late)
  torch.cuda.synchronize()
  _same_state(on, plain, 'constant piecewise against no schedule')
  _same_state(beside, plain, 'constant piecewise, backward_and_apply, against no schedule')
  assert _bits(on.scal[:1]) == _bits(plain.scal[:1]) and float(on.scal[2]) == float(_f32(LR)) and float(plain.scal[2]) == 0.0
  assert int(on.store.global_step.item()) == 3
  # forward / backward / apply_gradients one by one: apply_gradients launches the prepare work itself (geeco_adam_prepare_schedule)
  apart = _model(dev, lr_schedule=flat)
  for _ in range(3):
    apart.forward(backward_too=True)
    apart.backward()
    apart.apply_gradients()
  torch.cuda.synchronize()
  _same_state(apart, plain, 'apply_gradients preparing by itself')


LAUNCHING = ['slab_reduce_batch', 'adam_prepare', 'adam_prepare_schedule', 'adam_tf', 'adam_tf_ema', 'adam_tf_segments', 'adam_tf_segments_ema',
             'adam_tf_segments_clip', 'grad_sumsq_segments', 'clip_scale', 'derive_conv_weights', 'sumsq_into', 'check_input_stage']


def test_same_launch_count(dev, monkeypatch):
  """With the option on, train_step and backward_and_apply issue the calls they issue with it off, one for one by name (every
  launching function of ops behind a recording wrapper, as profiles/encoder_plan/step_calls.py lists them): the schedule rides where
  the constant rode.  apply_gradients by itself: geeco_adam_prepare_schedule in geeco_adam_prepare's place."""
  from geeco_amd import ops
  from geeco_amd.runtime import gradient_buckets
  off, on = _model(dev), _model(dev, lr_schedule=PIECEWISE)
  early, late = gradient_buckets(off.store)
  calls = []

  def recording(name, fn):
    def f(*a, **k):
      lr = a[1][1] if name == 'slab_reduce_batch' and len(a) > 1 and a[1] is not None else None
      calls.append(name + (':schedule' if lr is not None and not isinstance(lr, float) else ':lr' if lr is not None else ''))
      return fn(*a, **k)
    return f

  names = sorted(n for n in dir(ops) if n.endswith('_into')) + LAUNCHING
  for n in names:
    monkeypatch.setattr(ops, n, recording(n, getattr(ops, n)))

  def calls_of(step):
    del calls[:]
    step()
    torch.cuda.synchronize()
    return list(calls)

  def beside(m):
    m.forward(backward_too=True)
    m.backward_and_apply(early, late)

  def apart(m):
    m.forward(backward_too=True)
    m.backward()
    m.apply_gradients()

  for what, step in (('train_step', lambda m: m.train_step()), ('backward_and_apply', beside)):
    a, b = calls_of(lambda: step(off)), calls_of(lambda: step(on))
    assert len(a) == len(b) and len(a) > 10, what
    assert a.count('slab_reduce_batch:lr') == 1 and b.count('slab_reduce_batch:schedule') == 1 and 'slab_reduce_batch:lr' not in b, what
    assert [c.replace(':schedule', ':lr') for c in b] == a, what
    assert not any(c.startswith('adam_prepare') for c in a + b), what
  a, b = calls_of(lambda: apart(off)), calls_of(lambda: apart(on))
  assert a.count('adam_prepare') == 1 and b.count('adam_prepare_schedule') == 1 and 'adam_prepare' not in b
  assert [c.replace('adam_prepare_schedule', 'adam_prepare') for c in b] == a


def test_with_averaged_weights_and_clipping(dev):
  """ema_decay and clip_norm both on: the step runs (the shadow arena moves, the norm is logged, the update is the clipped one) and the
  sequence of scal[2] is bitwise the schedule-only model's."""
  from geeco_amd.graph import build_store
  _, cfg, _, _, _ = _case()
  sch = _normalised(PIECEWISE)
  alone = _model(dev, lr_schedule=PIECEWISE)
  both = _model(dev, lr_schedule=PIECEWISE, ema_decay=0.9, clip_norm=0.01, store=build_store(cfg, False, dev, ema=True))
  seq = {'alone': [], 'both': []}
  for s in range(5):
    for tag, m in (('alone', alone), ('both', both)):
      m.train_step()
      torch.cuda.synchronize()
      _check_step_scalars(m, sch, s, tag)
      seq[tag].append(_bits(m.scal[2:3])[0])
  assert seq['alone'] == seq['both']
  assert 0.0 < float(both.clip_out[0]) < 1.0 and float(both.clip_out[1]) > 0.01
  assert not torch.equal(both.store.ema, both.store.params) and not torch.equal(both.store.params, alone.store.params)
  assert torch.isfinite(both.store.params).all() and torch.isfinite(both.store.ema).all()


# ================================================================================================
# Estimator and command line
# ================================================================================================
def _events(model_dir):
  return [json.loads(l) for l in open(os.path.join(model_dir, 'events.jsonl'))]


def test_estimator_logs_the_rate_and_resumes_the_schedule(dev, tmp_path):
  """Three steps, a checkpoint, a NEW Estimator on the same model_dir, one more step: its learning_rate in events.jsonl is the
  reference lr(3) -- the schedule is a function of the restored counter.  Without the option the key is not written."""
  from geeco_amd import estimator as est
  from geeco_amd.input_fn import synthetic_batches
  from geeco_amd.params import create_e2evmc_config
  cfg = create_e2evmc_config(dict(window_size=K3, img_height=H, img_width=H, batch_size=N, lr=LR))
  schedule = {'kind': 'exponential', 'warmup_steps': 2, 'decay_steps': 1, 'decay_rate': 0.5}
  sch = _normalised(schedule)
  params = {'e2evmc_config': cfg, 'log_steps': 1, 'debug': False, 'lr_schedule': schedule}
  md = str(tmp_path / 'run')
  e = est.Estimator(est.e2evmc_model_fn, md, est.RunConfig(init_seed=4), params)
  e.train(input_fn=synthetic_batches(N, K3, 3, (H, H), 3, False, seed=5))
  first = _events(md)
  assert [line['learning_rate'] for line in first] == [float(_f32(L.lr_at(sch, s))) for s in range(3)]
  assert os.path.basename(est.latest_checkpoint(md)) == 'model.ckpt-3'
  again = est.Estimator(est.e2evmc_model_fn, md, est.RunConfig(init_seed=4), params)
  again.train(input_fn=synthetic_batches(N, K3, 1, (H, H), 3, False, seed=6))
  ev = _events(md)
  print('learning_rate per step:', [line['learning_rate'] for line in ev])
  assert len(ev) == 4 and ev[3]['global_step'] == 4
  assert ev[3]['learning_rate'] == float(_f32(L.lr_at(sch, 3))) == float(_f32(LR)) * 0.5
  off = str(tmp_path / 'off')
  e = est.Estimator(est.e2evmc_model_fn, off, est.RunConfig(init_seed=4), {k: v for k, v in params.items() if k != 'lr_schedule'})
  e.train(input_fn=synthetic_batches(N, K3, 2, (H, H), 3, False, seed=5))
  assert len(_events(off)) == 2 and not any('learning_rate' in line for line in _events(off))
  assert _events(off)[0]['loss'] == first[0]['loss']


def test_train_script_with_a_cosine_schedule(dev, tmp_path):
  md = str(tmp_path / 'run')
  cmd = [sys.executable, os.path.join(ROOT, 'scripts', 'train_e2evmc.py'), '--dataset_dir', 'synthetic:6:136x136', '--model_dir', md,
         '--window_size', '3', '--batch_size', '4', '--train_epochs', '1', '--log_steps', '1', '--num_best_ckpt', '1',
         '--lr_schedule', 'cosine', '--lr_warmup_steps', '2', '--lr_decay_steps', '4']
  os.makedirs(md)
  from geeco_amd.params import create_e2evmc_config
  cfg = create_e2evmc_config(dict(window_size=3, img_height=136, img_width=136, batch_size=4, lr=3e-4))
  with open(os.path.join(md, 'e2evmc_config.json'), 'w') as f:      # (the image size comes through a pre-seeded config: restart protocol)
    json.dump(cfg._asdict(), f)
  out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
  assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
  sch = _normalised({'kind': 'cosine', 'warmup_steps': 2, 'decay_steps': 4}, cfg.lr)
  ev = _events(md)
  print('learning_rate per step:', [line['learning_rate'] for line in ev])
  assert [line['global_step'] for line in ev] == [1, 2, 3, 4, 5, 6]
  assert [line['learning_rate'] for line in ev] == [float(_f32(L.lr_at(sch, s))) for s in range(6)]
