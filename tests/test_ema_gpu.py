"""The opt-in averaged weights on the GPU: the two Adam entry points that keep the shadow arena, the step that calls
them, and the Estimator / checkpoint / predictor surface on top.

The shadow update is tf.train.ExponentialMovingAverage's (zero_debias=False, num_updates=global_step), all in float32:
    d_t = min(decay, (1 + t) / (10 + t));    s' = s - (s - p') (1 - d_t),   p' = the parameter the step has just written.
``_shadow_ref`` restates the two lines in float64, fed the device's own p' and the float32 d_t.  Bound of the kernel tests: 2 ulp of
max(|s|, |p'|) per element -- derived, not measured: the update is one subtraction and one FMA (csrc/misc.hip: ema_element), the
subtraction's rounding (0.5 ulp(s - p') <= 1 ulp of the max) scaled by d_t < 1, the FMA's 0.5 ulp(s') <= 0.5 ulp of the max.
"""
import json
import os
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float('nan')
ADAM = dict(beta1=0.9, beta2=0.999, eps=1e-8)
SIZES = [1, 3, 4, 5, 1027, 2101251]      # the last: more than 2048 blocks x 256 threads x 4, so the grid-stride loop runs, tail of 3
# both sides of the min; the ramp (1 + t) / (10 + t) passes decay = 0.99 at t = 890 (at t = 89 .. 91 it is still 0.909 .. 0.911)
STEPS = [1, 5, 89, 90, 91, 889, 890, 891, 10**6]
LR_T = 1e-3


def _decay_f32(decay, t):
  """d_t in numpy.float32 arithmetic: float32 division of two float32 values, then the min."""
  t = np.float32(t)
  return min(np.float32(decay), (np.float32(1) + t) / (np.float32(10) + t))


def _shadow_ref(s, p_new, d):
  """float64 restatement of the update, from the float32 shadow, the device's new parameters and the float32 d_t."""
  s, p_new = s.astype(np.float64), p_new.astype(np.float64)
  return s - (s - p_new) * (1.0 - np.float64(d))


def _ulp_of_max(s, p_new):
  return np.spacing(np.maximum(np.abs(s), np.abs(p_new)).astype(np.float32)).astype(np.float64)


_INPUTS = {}


def _inputs(n, seed=0):
  """p, g, m, v, ema as numpy float32 (v >= 0; the shadow independent of p: either sign, any distance).  Computed once per size."""
  if (n, seed) not in _INPUTS:
    r = np.random.default_rng(1000 + 7 * seed + n % 1013)
    p, g, m, s = (r.standard_normal(n).astype(np.float32) for _ in range(4))
    v = (r.standard_normal(n).astype(np.float32)) ** 2
    _INPUTS[(n, seed)] = tuple(a for a in (p, g * np.float32(0.1), m * np.float32(0.1), v * np.float32(0.01), s))
  return _INPUTS[(n, seed)]


def _dev(dev, a, slack=5):
  """numpy array -> flat device tensor with ``slack`` NaN elements behind it (they must stay NaN)."""
  t = torch.full((a.size + slack,), NAN, dtype=torch.float32, device=dev)
  t[:a.size] = torch.from_numpy(a)
  return t


def _scalars(dev, t):
  scal = torch.zeros(4, dtype=torch.float32, device=dev)
  scal[0] = LR_T
  return scal, torch.full((1,), t, dtype=torch.int64, device=dev)


def _bits(t):
  return t.detach().cpu().numpy().view(np.uint32)


@pytest.mark.parametrize('n', SIZES)
def test_adam_is_unchanged_by_the_shadow_arena(dev, n):
  """(1) After geeco_adam_tf_ema, p, m, v are bit for bit what geeco_adam_tf leaves from the same inputs (and the slack behind every
  arena is untouched)."""
  from geeco_amd import ops
  p0, g0, m0, v0, s0 = _inputs(n)
  for l2 in (0.0, 1e-3):
    for gscale in (1.0, 0.125):
      scal, step = _scalars(dev, 5)
      a = [_dev(dev, x) for x in (p0, g0, m0, v0)]
      b = [_dev(dev, x) for x in (p0, g0, m0, v0, s0)]
      ops.adam_tf(a[0], a[1], a[2], a[3], n, scal, grad_scale=gscale, l2=l2, **ADAM)
      ops.adam_tf_ema(b[0], b[1], b[2], b[3], b[4], n, scal, step, 0.99, grad_scale=gscale, l2=l2, **ADAM)
      torch.cuda.synchronize()
      for name, x, y in zip('pgmv', a, b):
        np.testing.assert_array_equal(_bits(x), _bits(y), err_msg='%s n=%d l2=%g gscale=%g' % (name, n, l2, gscale))
      assert not np.array_equal(_bits(a[0][:n]), p0.view(np.uint32))      # (the update did run)
      assert torch.isnan(b[4][n:]).all() and not torch.isnan(b[4][:n]).any()


@pytest.mark.parametrize('t', STEPS)
@pytest.mark.parametrize('n', SIZES)
def test_shadow_arithmetic(dev, n, t):
  """(2) The shadow arena against the float64 restatement, every element within 2 ulp of max(|s|, |p'|)."""
  from geeco_amd import ops
  p0, g0, m0, v0, s0 = _inputs(n)
  d = _decay_f32(0.99, t)
  for l2 in (0.0, 1e-3):
    for gscale in (1.0, 0.125):
      scal, step = _scalars(dev, t)
      b = [_dev(dev, x) for x in (p0, g0, m0, v0, s0)]
      ops.adam_tf_ema(b[0], b[1], b[2], b[3], b[4], n, scal, step, 0.99, grad_scale=gscale, l2=l2, **ADAM)
      p_new, got = b[0][:n].cpu().numpy(), b[4][:n].cpu().numpy()
      err = np.abs(got.astype(np.float64) - _shadow_ref(s0, p_new, d)) / _ulp_of_max(s0, p_new)
      print('n=%d t=%d l2=%g gscale=%g d_t=%.9g: max error %.3f ulp' % (n, t, l2, gscale, d, err.max()))
      assert err.max() <= 2.0
      assert int(step.item()) == t       # the counter is read, never written


@pytest.mark.parametrize('t', STEPS + [2**24 + 1])
def test_decay_schedule_is_exact(dev, t):
  """(2) d_t itself, exactly: with p = g = m = v = 0 the new parameter is 0, and a shadow of 1 becomes 0 + (1 - 0) d_t = d_t with no
  rounding.  Against numpy.float32 arithmetic (2**24 + 1: the counter's conversion to float32 rounds)."""
  from geeco_amd import ops
  n = 7
  z = np.zeros(n, np.float32)
  for decay in (0.99, 0.5, 0.999999):
    scal, step = _scalars(dev, t)
    b = [_dev(dev, x) for x in (z, z, z, z, np.ones(n, np.float32))]
    ops.adam_tf_ema(b[0], b[1], b[2], b[3], b[4], n, scal, step, decay, **ADAM)
    assert torch.equal(b[0][:n], torch.zeros(n, device=dev))
    want = np.full(n, _decay_f32(decay, t), np.float32)
    np.testing.assert_array_equal(_bits(b[4][:n]), want.view(np.uint32), err_msg='t=%d decay=%g' % (t, decay))


def _partitions(n):
  """{name: [(offset, count)]}: offsets and counts multiples of 4, a 4-float piece, gaps no piece covers (the 1-piece case: a gap
  on either side), pieces given out of arena order.  n = 2 101 252: the long pieces run the grid-stride loop."""
  return {
      '1 piece': [(8, n - 20)],
      '2 pieces': [(n - 8, 4), (0, n - 16)],
      '8 pieces': [(4096, 1024), (0, 4), (8, 2052), (n - 4, 4), (3000, 1000), (1000000, 1100000), (5120, 994000), (2064, 900)],
  }


@pytest.mark.parametrize('with_g_out', [False, True], ids=['no g_out', 'g_out'])
@pytest.mark.parametrize('pieces', ['1 piece', '2 pieces', '8 pieces'])
def test_any_partition_gives_the_one_pass_result(dev, pieces, with_g_out):
  """(3) geeco_adam_tf_segments_ema leaves p, m, v, ema bitwise equal to the one-pass geeco_adam_tf_ema on the covered elements
  and every uncovered element of the four arenas untouched; g_out receives the pieces' gradients and nothing else."""
  from geeco_amd import ops
  n = 2101252
  segs = _partitions(n)[pieces]
  covered = np.zeros(n, bool)
  for off, cnt in segs:
    assert off % 4 == 0 and cnt % 4 == 0 and not covered[off:off + cnt].any()
    covered[off:off + cnt] = True
  assert not covered.all()
  p0, g0, m0, v0, s0 = _inputs(n)
  scal, step = _scalars(dev, 7)
  one = [_dev(dev, x) for x in (p0, g0, m0, v0, s0)]
  ops.adam_tf_ema(one[0], one[1], one[2], one[3], one[4], n, scal, step, 0.99, grad_scale=0.5, l2=1e-3, **ADAM)
  seg = [_dev(dev, x) for x in (p0, m0, v0, s0)]
  g_out0 = np.random.default_rng(5).standard_normal(n).astype(np.float32)
  g_out = _dev(dev, g_out0) if with_g_out else None
  sources = [(torch.from_numpy(g0[off:off + cnt]).to(dev), off, cnt) for off, cnt in segs]      # every piece its own gradient buffer
  ops.adam_tf_segments_ema(seg[0], seg[1], seg[2], seg[3], sources, scal, step, 0.99, g_out=g_out, grad_scale=0.5, l2=1e-3, **ADAM)
  torch.cuda.synchronize()
  for name, got, ref, init in zip(('p', 'm', 'v', 'ema'), seg, (one[0], one[2], one[3], one[4]), (p0, m0, v0, s0)):
    got, ref = _bits(got), _bits(ref)
    np.testing.assert_array_equal(got[:n][covered], ref[:n][covered], err_msg=name + ' (covered)')
    np.testing.assert_array_equal(got[:n][~covered], init.view(np.uint32)[~covered], err_msg=name + ' (uncovered)')
    np.testing.assert_array_equal(got[n:], ref[n:], err_msg=name + ' (slack)')
  if with_g_out:
    want = np.where(covered, g0, g_out0)
    np.testing.assert_array_equal(_bits(g_out[:n]), want.view(np.uint32))


def test_argument_refusals(dev):
  """(4) A null or misaligned shadow arena and a decay outside (0, 1) return GEECO_EINVAL with a message; nothing is launched
  (every arena is as it was).  The same calls with a valid arena and decay are the tests above."""
  import ctypes
  from geeco_amd import _native
  from geeco_amd.ops import _p, _stream
  lib = _native.load()
  n = 64
  arenas0 = _inputs(n)
  scal, step = _scalars(dev, 3)

  def attempt(ema_of, decay, segments):
    a = dict(zip(('p', 'g', 'm', 'v', 'ema'), (_dev(dev, x, slack=8) for x in arenas0)))
    ema = ema_of(a['ema'])
    if segments:
      seg = (_native.AdamSegment * 1)()
      seg[0].g, seg[0].p_off, seg[0].count = _p(a['g']), 0, n
      rc = lib.geeco_adam_tf_segments_ema(_p(a['p']), None, _p(a['m']), _p(a['v']), ema, seg, 1, _p(scal), _p(step), decay, 0.9, 0.999,
                                          1e-8, 1.0, 0.0, _stream())
    else:
      rc = lib.geeco_adam_tf_ema(_p(a['p']), _p(a['g']), _p(a['m']), _p(a['v']), ema, n, _p(scal), _p(step), decay, 0.9, 0.999, 1e-8,
                                 1.0, 0.0, _stream())
    msg = (lib.geeco_last_error() or b'').decode()
    torch.cuda.synchronize()
    for x0, k in zip(arenas0, ('p', 'g', 'm', 'v', 'ema')):
      np.testing.assert_array_equal(_bits(a[k][:n]), x0.view(np.uint32), err_msg=k + ' was written')
    return rc, msg

  whole = lambda e: _p(e)
  for segments, who in ((False, 'adam_tf_ema'), (True, 'adam_tf_segments_ema')):
    rc, msg = attempt(lambda e: None, 0.9, segments)
    assert rc == _native.GEECO_EINVAL and who in msg and 'null' in msg, (rc, msg)
    rc, msg = attempt(lambda e: ctypes.c_void_p(e.data_ptr() + 4), 0.9, segments)
    assert rc == _native.GEECO_EINVAL and who in msg and 'aligned' in msg, (rc, msg)
    for decay in (0.0, 1.0, -0.1, 1.5, NAN):
      rc, msg = attempt(whole, decay, segments)
      assert rc == _native.GEECO_EINVAL and who in msg and 'decay' in msg, (decay, rc, msg)


# ---- the step ----------------------------------------------------------------------------------------------------------------------

def _model(dev, goal, P, feats, labels, cfg, **kw):
  from geeco_amd import graph
  N = feats['rgb'].shape[0]
  model = (graph.GoalE2EVMC if goal else graph.E2EVMC)(cfg, N, dev, training=True, **kw)
  model.store.load_numpy(P)
  model.load_batch({k: torch.from_numpy(v) for k, v in feats.items()}, {k: torch.from_numpy(v) for k, v in labels.items()})
  return model


def _restart(model, P):
  """The state of step 0 again, in place (the captured graph keeps its pointers): what the warm-up steps moved is put back."""
  s = model.store
  s.load_numpy(P)           # (the shadow arena restarts from the parameters)
  for t in (s.adam_m, s.adam_v, s.grads, s.global_step):
    t.zero_()
  model.enc.refresh_derived()
  model._prepared = False


@pytest.mark.parametrize('goal', [True, False], ids=['geeco-f', 'e2e_vmc'])
def test_three_replayed_steps(dev, goal):
  """(5) K = 2, N = 2 at 136 x 136 -- the smallest size this suite builds models at: the encoder's seven stride-2 layers must end
  on the 2 x 2 state grid, so check_image_size refuses anything under 129 pixels (16 x 16 cannot be built).  Three captured and
  replayed steps with ema_decay = 0.9 leave params, adam_m, adam_v and the losses bitwise equal to three steps with the option
  off; the shadow arena equals the float64 recurrence over the three device parameter snapshots within 3 x the bound of the kernel
  test; the schedule with the optimiser beside the encoder bottom gives bitwise the plain schedule's shadow arena."""
  from geeco_amd.params import create_e2evmc_config
  from geeco_amd.runtime import TrainStepRunner
  from oracle import geeco_oracle as O
  kw = dict(window_size=2, img_height=136, img_width=136, batch_size=2, lr=1e-3)
  if goal:
    kw.update(proc_obs='dynimg', proc_tgt='dyndiff')
  ocfg = O.make_config(**kw)
  cfg = create_e2evmc_config(ocfg._asdict())
  P = O.init_params(O.model_param_shapes(ocfg, goal), seed=1)
  feats, labels = O.synthetic_batch(ocfg, goal, 2, seed=3, H=136, W=136)

  def three_steps(ema_decay, beside):
    m = _model(dev, goal, P, feats, labels, cfg, ema_decay=ema_decay)
    r = TrainStepRunner(m, use_graph=True, warmup=2)
    assert r.beside_bottom
    r.beside_bottom = beside
    r.prepare()               # two eager steps, then the capture
    assert r._graphs is not None and len(r._graphs) == 1
    _restart(m, P)
    start = m.store.params.clone()
    losses, snaps = [], []
    for _ in range(3):
      r.step()
      torch.cuda.synchronize()
      losses.append(float(m.loss))
      snaps.append(m.store.params.cpu().numpy().copy())
    assert int(m.store.global_step.item()) == 3
    return m, losses, snaps, start.cpu().numpy()

  on, l_on, snaps, start = three_steps(0.9, True)
  off, l_off, _, _ = three_steps(None, True)
  assert off.store.ema is None and on.store.ema is not None
  assert l_on == l_off
  for name in ('params', 'adam_m', 'adam_v', 'grads'):
    assert torch.equal(getattr(on.store, name), getattr(off.store, name)), name
  # the float64 recurrence over the device's parameter snapshots, s_0 = p_0
  s = start.astype(np.float64)
  scale = np.abs(start)
  for t, p_t in enumerate(snaps, 1):
    s = _shadow_ref(s, p_t, _decay_f32(0.9, t))
    scale = np.maximum(scale, np.maximum(np.abs(s), np.abs(p_t)))
  got = on.store.ema.cpu().numpy()
  err = np.abs(got.astype(np.float64) - s) / np.spacing(scale.astype(np.float32)).astype(np.float64)
  print('shadow arena after three steps: max error %.3f ulp' % err.max())
  assert err.max() <= 3 * 2.0
  assert not np.array_equal(got, snaps[-1])          # (it is an average, not a copy)
  plain, l_plain, _, _ = three_steps(0.9, False)
  assert l_plain == l_on
  assert torch.equal(plain.store.ema, on.store.ema) and torch.equal(plain.store.params, on.store.params)


# ---- Estimator, checkpoints, predictors --------------------------------------------------------------------------------------------

def test_estimator_evaluates_and_exports_the_averaged_weights(dev, tmp_path):
  """(6) Train a few steps with params['ema_decay'], evaluate: the loss is that of a model whose parameters were overwritten with
  the shadow arena (rtol 1e-4, atol 2e-5: the tolerance of the batched-versus-batch-1 comparisons) and not the raw weights' loss;
  the .pt file and the TF bundle round-trip the shadow tensors bitwise; predictors with use_ema=True return that model's commands
  and raise KeyError on a checkpoint without shadow tensors."""
  from geeco_amd import estimator as est
  from geeco_amd import tf_checkpoint
  from geeco_amd.graph import build_store
  from geeco_amd.input_fn import synthetic_batches
  from geeco_amd.params import create_e2evmc_config
  from geeco_amd.predictor import GoalE2EVMCPredictor
  kw = dict(proc_obs='dynimg', proc_tgt='dyndiff', window_size=3, img_height=136, img_width=136, batch_size=4, lr=1e-3)
  cfg = create_e2evmc_config(kw)
  plain = {'e2evmc_config': cfg, 'log_steps': 100, 'debug': False}
  train_in = synthetic_batches(4, 3, 4, (136, 136), 3, True, seed=5)
  eval_in = synthetic_batches(4, 3, 2, (136, 136), 3, True, seed=6)
  md = str(tmp_path / 'run')
  e = est.Estimator(est.goal_e2evmc_model_fn, md, est.RunConfig(save_tf_bundle=True), dict(plain, ema_decay=0.9))
  e.train(input_fn=train_in)
  json.dump(cfg._asdict(), open(os.path.join(md, 'e2evmc_config.json'), 'w'))
  ev = e.evaluate(input_fn=eval_in)
  assert ev['global_step'] == 4
  store = e._store
  assert store.ema is not None and not torch.equal(store.ema, store.params)
  shadow, raw = store.to_numpy('ema'), store.to_numpy('params')

  # a model directory whose PARAMETERS are the shadow arena (no shadow tensors of its own), as .pt and as a bundle
  swapped = str(tmp_path / 'swapped')
  os.makedirs(swapped)
  st = build_store(cfg, True, 'cpu')
  st.load_numpy(shadow)
  st.global_step.fill_(4)
  est.save_checkpoint(st, swapped, keep_max=2, tf_bundle=True)
  json.dump(cfg._asdict(), open(os.path.join(swapped, 'e2evmc_config.json'), 'w'))
  ev_swapped = est.Estimator(est.goal_e2evmc_model_fn, swapped, est.RunConfig(), plain).evaluate(input_fn=eval_in)
  ev_raw = est.Estimator(est.goal_e2evmc_model_fn, md, est.RunConfig(), plain).evaluate(input_fn=eval_in)      # option off: the raw weights
  print('eval loss: averaged %.9g, swapped-in %.9g, raw %.9g' % (ev['loss'], ev_swapped['loss'], ev_raw['loss']))
  for k in ('loss', 'cmd_ee', 'pos_ee', 'pos_obj'):
    np.testing.assert_allclose(ev[k], ev_swapped[k], rtol=1e-4, atol=2e-5, err_msg=k)
  assert ev['loss'] != ev_raw['loss']

  # both checkpoint forms carry the shadow tensors, bitwise
  prefix = est.latest_checkpoint(md)
  t = tf_checkpoint.read_checkpoint(prefix)
  for name in store.shapes:
    np.testing.assert_array_equal(t[name + '/ExponentialMovingAverage'].view(np.uint32), shadow[name].view(np.uint32), err_msg=name)
    np.testing.assert_array_equal(t[name].view(np.uint32), raw[name].view(np.uint32), err_msg=name)
  only_bundle = str(tmp_path / 'bundle_only')
  os.makedirs(only_bundle)
  for fn in os.listdir(md):
    if not fn.endswith('.pt'):
      shutil.copy(os.path.join(md, fn), only_bundle)
  for directory in (md, only_bundle):
    back = build_store(cfg, True, 'cpu', ema=True)
    est.load_checkpoint(back, est.latest_checkpoint(directory))
    assert torch.equal(back.ema.view(torch.int32), store.ema.cpu().view(torch.int32)), directory
    assert torch.equal(back.params.view(torch.int32), store.params.cpu().view(torch.int32)), directory
  # ... and a resumed run evaluates the same averaged weights
  ev2 = est.Estimator(est.goal_e2evmc_model_fn, only_bundle, est.RunConfig(), dict(plain, ema_decay=0.9)).evaluate(input_fn=eval_in)
  assert ev2['loss'] == ev['loss']

  # predictors
  r = np.random.default_rng(3)
  frames, jnts = r.random([3, 136, 136, 3], dtype=np.float32), r.standard_normal([3, 7]).astype(np.float32)
  tgt = r.random([136, 136, 3], dtype=np.float32)

  def run(model_dir, **pkw):
    p = GoalE2EVMCPredictor(model_dir, **pkw)
    p.set_goal(tgt)
    return [p.predict(frames[i], jnts[i]) for i in range(3)]
  want = run(swapped)
  for directory in (md, only_bundle):
    for a, b in zip(run(directory, use_ema=True), want):
      for k in b:
        np.testing.assert_array_equal(a[k], b[k], err_msg='%s: %s' % (directory, k))
  assert any(not np.array_equal(a['cmd_ee'], b['cmd_ee']) for a, b in zip(run(md), want))      # (use_ema=False: the raw weights)
  first = next(iter(store.shapes)) + '/ExponentialMovingAverage'
  with pytest.raises(KeyError, match=first):
    GoalE2EVMCPredictor(swapped, use_ema=True)                    # a .pt file without shadow tensors
  os.remove(est.latest_checkpoint(swapped) + '.pt')
  with pytest.raises(KeyError, match=first):
    GoalE2EVMCPredictor(swapped, use_ema=True)                    # a bundle without them
