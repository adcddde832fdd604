"""Opt-in loss shaping on the GPU: the shaped decoder-tail kernels against the fp64 restatement (tests/_loss_shaping_ref.py),
neutral shaping against the unshaped entry points bit for bit, the fused one-step decoder against the separate shaped entry points, the
whole models, and the Estimator.  Tolerances of the kernel cases are those of tests/test_kernels_gpu.py::test_heads_loss."""
import json
import os

import numpy as np
import pytest
import torch

import _loss_shaping_ref as R

pytestmark = pytest.mark.gpu

CLASS_W = [1.0, 0.25, 2.0]
SMOOTH, DELTA = 0.1, 0.5


def _close(got, ref, rtol, atol, what):
  got, ref = got.detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
  err = (got - ref).abs()
  bound = atol + rtol * ref.abs()
  assert bool((err <= bound).all()), '%s: max error %.3e (bound %.3e)' % (what, float(err.max()), float(bound.max()))


def _heads(mode, huber):
  """[(size, kind, weight)] of test_heads_loss, with kind 2 on the heads ``huber`` lists."""
  heads = [(3, 0, 1.0), (3, 1, 1.0), (3, 0, 0.5), (3, 0, 0.5)] if mode == 'cartesian' else \
          [(7, 0, 1.0), (3, 0, 1.0), (2, 0, 1.0), (3, 0, 1.0), (3, 0, 1.0)]
  return [(sz, 2 if i in huber else kind, wt) for i, (sz, kind, wt) in enumerate(heads)]


def _sample_weights(N, g, all_zero=False):
  """Weights from {0, 0.5, 1, 2}; where N > 1 at least one zero and one non-zero."""
  if all_zero:
    return torch.zeros(N)
  w = torch.tensor([0.0, 0.5, 1.0, 2.0])[torch.randint(0, 4, (N,), generator=g)]
  if N == 1:
    w[0] = 2.0
  else:
    w[0], w[N - 1] = 0.0, 0.5
  return w


class _Tail:
  """Inputs of one decoder-tail case on the host (float32) and on the device, with the output buffers of a call."""

  def __init__(self, dev, N, mode, H, F, huber, seed, labels=None):
    self.dev, self.N, self.H, self.F = dev, N, H, F
    self.heads = _heads(mode, huber)
    g = torch.Generator().manual_seed(seed)
    self.g = g
    self.h = torch.randn(N, H, generator=g)
    self.w1, self.b1 = torch.randn(H, F, generator=g) * 0.1, torch.randn(F, generator=g) * 0.1
    self.hw = [torch.randn(F, sz, generator=g) * 0.1 for sz, _, _ in self.heads]
    self.hb = [torch.randn(sz, generator=g) * 0.1 for sz, _, _ in self.heads]
    self.tg = [torch.randint(-1, 2, (N, 1), generator=g).float() if kind == 1 else torch.randn(N, sz, generator=g)
               for sz, kind, _ in self.heads]
    if labels is not None:
      self.tg[1] = torch.tensor(labels, dtype=torch.float32).reshape(N, 1)
    d = lambda t: t.to(dev).contiguous()
    self.dev_in = (d(self.h), d(self.w1), d(self.b1), [d(t) for t in self.hw], [d(t) for t in self.hb])
    self.meta = ([sz for sz, _, _ in self.heads], [k for _, k, _ in self.heads], [w for _, _, w in self.heads], [d(t) for t in self.tg],
                 [t.shape[1] for t in self.tg])
    self.OT = sum(self.meta[0])

  def outputs(self):
    dev, N, H, F = self.dev, self.N, self.H, self.F
    nan = lambda *s: torch.full(s, float('nan'), device=dev)
    return dict(preds=nan(N, self.OT), losses=torch.zeros(8, device=dev), dh=nan(N, H), dw1=nan(H, F), db1=nan(F),
                dhw=[nan(F, sz) for sz in self.meta[0]], dhb=[nan(sz) for sz in self.meta[0]])

  def run(self, shaping=None, meta=None):
    from geeco_amd import ops
    o = self.outputs()
    ws = torch.empty(ops.heads_ws_bytes(self.N, self.H, self.F) // 4 + 4, device=self.dev)
    o['names'] = ops.kernel_trace(lambda: ops.heads_loss_into(
        o['preds'], o['losses'], *self.dev_in, *(meta or self.meta), 1.0, self.N, self.H, self.F, ws, dh=o['dh'], d_fc1_w=o['dw1'],
        d_fc1_b=o['db1'], d_heads_w=o['dhw'], d_heads_b=o['dhb'], shaping=shaping))
    torch.cuda.synchronize()
    return o


def _check_against_reference(case, out, ref):
  nh = len(case.heads)
  _close(out['preds'], ref['preds'], 1e-5, 1e-5, 'preds')
  _close(out['losses'][0], ref['total'], 1e-5, 1e-6, 'loss')
  _close(out['losses'][1:1 + nh], ref['parts'], 1e-5, 1e-6, 'per-head losses')
  scale = lambda t: float(t.abs().max()) * 2e-5 + 1e-8
  g = ref['grads']
  _close(out['dh'], g['h'], 0, scale(g['h']), 'dh')
  _close(out['dw1'], g['w1'], 0, scale(g['w1']), 'd fc1/kernel')
  _close(out['db1'], g['b1'], 0, scale(g['b1']), 'd fc1/bias')
  for i in range(nh):
    _close(out['dhw'][i], g['hw'][i], 0, scale(g['hw'][i]), 'd head kernel %d' % i)
    _close(out['dhb'][i], g['hb'][i], 0, scale(g['hb'][i]), 'd head bias %d' % i)
  for k, v in out.items():
    for t in (v if isinstance(v, list) else [v]):
      assert k == 'names' or not torch.isnan(t).any(), k


def _shaped_names(H, F):
  return ['heads_sample_kernel<false, shaped>', 'heads_finish_kernel'] if (H <= 128 and F in (64, 128)) else ['heads_loss_kernel<shaped>']


# (33: a second partial wave of samples in the finish sums; (9, 100, 64): G = 16; (5, 160, 128): the single-workgroup kernel)
KERNEL_CASES = [(1, 'cartesian', 128, 128), (7, 'cartesian', 128, 128), (33, 'cartesian', 128, 128), (5, 'velocity', 128, 128),
                (9, 'cartesian', 100, 64), (5, 'cartesian', 160, 128)]


@pytest.mark.parametrize('N,mode,H,F', KERNEL_CASES)
def test_shaped_tail_against_fp64(dev, N, mode, H, F):
  """(tests/test_decoder_tail_variants_gpu.py holds every shaped instantiation, launch form, size edge and layout under a bound per
  element.)"""
  from geeco_amd import ops
  cart = mode == 'cartesian'
  huber = (0, 3) if cart else (0, 2)      # Huber on two regression heads, weighted MSE on the others
  case = _Tail(dev, N, mode, H, F, huber, seed=200 + N if N > 1 else 205)      # (seeds at which every Huber head has both branches)
  sw = _sample_weights(N, case.g)
  assert N == 1 or (bool((sw == 0).any()) and bool((sw != 0).any()))
  deltas = [DELTA if k == 2 else 0.0 for k in case.meta[1]]
  ref = R.tail_reference(case.h, case.w1, case.b1, case.hw, case.hb, case.heads, case.tg, sample_weights=sw,
                         class_weights=CLASS_W if cart else None, smoothing=SMOOTH if cart else 0.0, deltas=deltas)
  # both Huber branches occur (delta = 0.5 against N(0, 1) residuals)
  off = np.cumsum([0] + case.meta[0])
  for i in huber:
    a = (ref['preds'][:, off[i]:off[i + 1]] - case.tg[i].double()).abs()
    assert bool((a <= DELTA).any()) and bool((a > DELTA).any()), i
  swd, cwd = sw.to(dev), torch.tensor(CLASS_W, device=dev)
  shaping = ops.loss_shaping(swd, cwd if cart else None, SMOOTH if cart else 0.0, deltas)
  out = case.run(shaping)
  assert out['names'] == _shaped_names(H, F), out['names']
  _check_against_reference(case, out, ref)
  # the launch list is the unshaped call's, apart from the names (MSE in place of Huber: the unshaped entry point refuses kind 2)
  plain = case.run(None, ([case.meta[0], [min(k, 1) for k in case.meta[1]]] + list(case.meta[2:])))
  assert len(plain['names']) == len(out['names']) and plain['names'] != out['names']


@pytest.mark.parametrize('N,H,F', [(7, 128, 128), (5, 160, 128)])
def test_all_weights_zero_gives_zero_loss_and_exactly_zero_gradients(dev, N, H, F):
  from geeco_amd import ops
  case = _Tail(dev, N, 'cartesian', H, F, (0,), seed=300 + N)
  deltas = [DELTA, 0.0, 0.0, 0.0]
  shaping = ops.loss_shaping(torch.zeros(N, device=dev), torch.tensor(CLASS_W, device=dev), SMOOTH, deltas)
  out = case.run(shaping)
  ref = R.tail_reference(case.h, case.w1, case.b1, case.hw, case.hb, case.heads, case.tg, sample_weights=torch.zeros(N),
                         class_weights=CLASS_W, smoothing=SMOOTH, deltas=deltas)
  assert float(ref['total']) == 0.0 and not ref['grads']['h'].any()
  _close(out['preds'], ref['preds'], 1e-5, 1e-5, 'preds')
  assert out['losses'][:5].tolist() == [0.0] * 5
  for k in ('dh', 'dw1', 'db1', 'dhw', 'dhb'):
    for t in (out[k] if isinstance(out[k], list) else [out[k]]):
      assert not torch.isnan(t).any() and not t.any(), k
  # class weights alone can zero every sample of the gripper head while the regression heads keep their mean over N
  only = ops.loss_shaping(None, torch.zeros(3, device=dev), 0.0, deltas)
  out = case.run(only)
  ref = R.tail_reference(case.h, case.w1, case.b1, case.hw, case.hb, case.heads, case.tg, class_weights=[0.0, 0.0, 0.0], deltas=deltas)
  assert float(out['losses'][2]) == 0.0 and not out['dhw'][1].any() and not out['dhb'][1].any()
  _check_against_reference(case, out, ref)


@pytest.mark.parametrize('H,F', [(128, 128), (160, 128)])
def test_out_of_range_label(dev, H, F):
  """An out-of-range label keeps an all-zero one-hot (eps / C everywhere once smoothed) and takes class weight 0 only when class
  weights are given."""
  from geeco_amd import ops
  N = 6
  case = _Tail(dev, N, 'cartesian', H, F, (), seed=41, labels=[-1, 0, 2, 1, -3, 0])      # labels + 1: 3 and -2 are out of range
  sw = torch.tensor([1.0, 2.0, 0.5, 1.0, 1.0, 0.0])
  for cw in (None, CLASS_W):
    ref = R.tail_reference(case.h, case.w1, case.b1, case.hw, case.hb, case.heads, case.tg, sample_weights=sw, class_weights=cw,
                           smoothing=SMOOTH)
    out = case.run(ops.loss_shaping(sw.to(dev), torch.tensor(cw, device=dev) if cw else None, SMOOTH))
    _check_against_reference(case, out, ref)
  # count of the gripper head: 5 non-zero sample weights without the table, 3 with it (two labels out of range)
  per = -(R.smoothed_one_hot(torch.round(case.tg[1][:, 0]).long() + 1, 3, SMOOTH) * torch.log_softmax(ref['preds'][:, 3:6], 1)).sum(1)
  gathered = torch.tensor([1.0, 0.25, 0.0, 2.0, 0.0, 0.25], dtype=torch.float64)
  _close(out['losses'][2], (sw.double() * gathered * per).sum() / 3, 1e-5, 1e-6, 'gripper loss over 3 samples')


@pytest.mark.parametrize('N,H,F', [(33, 128, 128), (5, 160, 128)])
def test_neutral_shaping_is_the_unshaped_path_bit_for_bit(dev, N, H, F):
  from geeco_amd import ops
  ones = lambda n: torch.ones(n, device=dev)
  # (an out-of-range label is part of the identity wherever no class table is given; with a table its effective weight is 0, not 1)
  for labels, shapings in ((([3] + [0, 1, -1] * N)[:N], (lambda: ops.loss_shaping(ones(N), None, 0.0), lambda: ops.loss_shaping())),
                           (([0, 1, -1] * N)[:N], (lambda: ops.loss_shaping(ones(N), ones(3), 0.0),))):
    case = _Tail(dev, N, 'cartesian', H, F, (), seed=500 + N, labels=labels)
    plain = case.run(None)
    for shaping in shapings:
      out = case.run(shaping())
      assert out['names'] == _shaped_names(H, F) and out['names'] != plain['names']
      for k in ('preds', 'losses', 'dh', 'dw1', 'db1', 'dhw', 'dhb'):
        for u, v in zip(plain[k] if isinstance(plain[k], list) else [plain[k]], out[k] if isinstance(out[k], list) else [out[k]]):
          assert not torch.isnan(v).any() and torch.equal(u, v), k


@pytest.mark.parametrize('D', [40, 3100])      # unsplit gate product; split-K (39 slabs), as test_lstm_step_heads_one_launch_per_sample
@pytest.mark.parametrize('deferred', [True, False])
def test_fused_one_step_decoder_is_the_shaped_separate_entry_points(dev, D, deferred):
  from geeco_amd import _native, ops
  N, H, F = 7, 128, 128
  r = np.random.default_rng(131 + D)
  case = _Tail(dev, N, 'cartesian', H, F, (0, 3), seed=600 + D)
  t = lambda a: torch.tensor(np.asarray(a, np.float32), device=dev)
  x, w, bias = t(r.standard_normal([N, D])), t(r.standard_normal([D + H, 4 * H]) / np.sqrt(D)), t(r.standard_normal([4 * H]))
  sw = _sample_weights(N, case.g).to(dev)
  cw = torch.tensor(CLASS_W, device=dev)
  shaping = lambda: ops.loss_shaping(sw, cw, SMOOTH, [DELTA, 0.0, 0.0, DELTA])
  _, w1, b1, hw, hb = case.dev_in
  gws = torch.empty(max(ops.gemm_ws_bytes(N, 4 * H, D), ops.lstm_step_bwd_ws_bytes(N, D, 4 * H)) // 4 + 4, device=dev)
  hws = torch.empty(ops.heads_ws_bytes(N, H, F) // 4 + 4, device=dev)
  nan = lambda *s: torch.full(s, float('nan'), device=dev)

  def outputs():
    return dict(z=nan(N, 4 * H), c=nan(N, H), h=nan(N, H), gates=nan(N, 4 * H), preds=nan(N, case.OT), losses=torch.zeros(8, device=dev),
                dz=nan(N, 4 * H), dw1=nan(H, F), db1=nan(F), dhw=[torch.full_like(a, float('nan')) for a in hw],
                dhb=[torch.full_like(a, float('nan')) for a in hb], dwx=torch.zeros(D, 4 * H, device=dev), dbx=nan(4 * H), dx=nan(N, D))
  a = outputs()
  dh = torch.empty(N, H, device=dev)
  ops.lstm_input_step_fwd_into(a['z'], a['c'], a['h'], a['gates'], x, w[:D], bias, N, H, D, D, 4 * H, gws)
  ops.heads_loss_into(a['preds'], a['losses'], a['h'], w1, b1, hw, hb, *case.meta, 1.0, N, H, F, hws, dh=dh, d_fc1_w=a['dw1'],
                      d_fc1_b=a['db1'], d_heads_w=a['dhw'], d_heads_b=a['dhb'], shaping=shaping())
  ops.lstm_gates_bwd_into(a['dz'], None, a['gates'], None, a['c'], dh, None, N, H)
  ops.lstm_step_bwd_into(a['dwx'], a['dbx'], a['dx'], x, a['dz'], w[:D], N, D, 4 * H, 4 * H, gws)
  torch.cuda.synchronize()
  b = outputs()
  hws2 = torch.empty_like(hws)
  pend = _native.HeadsFinish() if deferred else None
  names = ops.kernel_trace(lambda: ops.lstm_step_heads_into(
      b['z'], b['c'], b['h'], b['gates'], x, w[:D], bias, N, H, D, D, 4 * H, gws, b['preds'], b['losses'], w1, b1, hw, hb, *case.meta, 1.0, F,
      hws2, dz=b['dz'], d_fc1_w=b['dw1'], d_fc1_b=b['db1'], d_heads_w=b['dhw'], d_heads_b=b['dhb'], pending=pend, shaping=shaping()))
  assert names == ['gemm_f32_kernel', 'heads_sample_kernel<true, shaped>'] + ([] if deferred else ['heads_finish_kernel']), names
  names = ops.kernel_trace(lambda: ops.lstm_step_bwd_into(b['dwx'], b['dbx'], b['dx'], x, b['dz'], w[:D], N, D, 4 * H, 4 * H, gws,
                                                         pending=pend))
  assert ('lstm_step_bwd_heads_kernel' in names) == deferred, names
  torch.cuda.synchronize()
  for k in a:
    for u, v in zip(a[k] if isinstance(a[k], list) else [a[k]], b[k] if isinstance(b[k], list) else [b[k]]):
      assert not torch.isnan(v).any() and torch.equal(u, v), k
  # and the separate entry points are what the fp64 reference says
  ref = R.tail_reference(a['h'], case.w1, case.b1, case.hw, case.hb, case.heads, case.tg, sample_weights=sw.cpu(), class_weights=CLASS_W,
                         smoothing=SMOOTH, deltas=[DELTA, 0.0, 0.0, DELTA])
  _close(a['losses'][0], ref['total'], 1e-5, 1e-6, 'loss')
  _close(dh, ref['grads']['h'], 0, float(ref['grads']['h'].abs().max()) * 2e-5 + 1e-8, 'dh')


# ================================================================================================
# whole models
# ================================================================================================
SHAPING = {'sample_weights': True, 'grp_class_weights': CLASS_W, 'label_smoothing': SMOOTH, 'huber_delta': DELTA}
MODEL_CASES = [('e2e_vmc', dict(window_size=1), False), ('geeco-f', dict(proc_obs='dynimg', proc_tgt='dyndiff', window_size=1), True)]
N_MODEL, HW = 3, 136


def _model(dev, cfg_kw, goal, seed=1, **kw):
  from geeco_amd import graph
  from geeco_amd.params import create_e2evmc_config
  from oracle import geeco_oracle as O
  ocfg = O.make_config(**dict(cfg_kw, img_height=HW, img_width=HW, batch_size=N_MODEL))
  P = O.init_params(O.model_param_shapes(ocfg, goal), seed=seed)
  feats, labels = O.synthetic_batch(ocfg, goal, N_MODEL, seed=seed + 2, H=HW, W=HW)
  model = (graph.GoalE2EVMC if goal else graph.E2EVMC)(create_e2evmc_config(ocfg._asdict()), N_MODEL, dev, training=True, **kw)
  model.store.load_numpy(P)
  model.load_batch({k: torch.from_numpy(v) for k, v in feats.items()}, {k: torch.from_numpy(v) for k, v in labels.items()})
  return model


def _model_reference(model, weights):
  """The reference losses fed the model's own predictions and targets."""
  d = model.decoder
  preds = [p.detach().double().cpu() for p in d.predictions().values()]
  targets = [t[:, :sz].detach().double().cpu() for t, (_, _, sz, _, _) in zip(d.targets, d.heads)]
  heads = [(sz, kind, wt) for _, _, sz, kind, wt in d.heads]
  ls = model.loss_shaping
  return R.heads_losses(preds, heads, targets, sample_weights=weights, class_weights=ls['grp_class_weights'], smoothing=ls['label_smoothing'],
                        deltas=[ls['huber_delta'].get(h[1], 0.0) for h in d.heads])


def _check_loss_parts(model, weights):
  total, parts = _model_reference(model, weights)
  got = model.loss_parts()
  _close(got['loss'], total, 1e-5, 1e-6, 'loss')
  for (_, key, _, _, _), ref in zip(model.decoder.heads, parts):
    _close(got['loss_' + key.replace('logits_', '')], ref, 1e-5, 1e-6, 'loss_' + key)
  return float(total)


@pytest.mark.parametrize('name,cfg_kw,goal', MODEL_CASES, ids=[c[0] for c in MODEL_CASES])
def test_model_reports_the_shaped_losses_and_reads_the_weights_at_replay(dev, name, cfg_kw, goal):
  from geeco_amd.runtime import TrainStepRunner
  model = _model(dev, cfg_kw, goal, loss_shaping=SHAPING)
  assert [h[3] for h in model.decoder.heads] == [2, 1, 2, 2] and 'sample_weight' in model.label_keys
  assert model.inputs['sample_weight'].tolist() == [1.0] * N_MODEL      # ones until fed
  w0 = torch.tensor([2.0, 0.0, 0.5])
  model.inputs['sample_weight'].copy_(w0)
  model.train_step()
  torch.cuda.synchronize()
  first = _check_loss_parts(model, w0)
  assert first > 0
  # two replays of ONE captured step with different contents of the bound weight buffer
  runner = TrainStepRunner(model, use_graph=True)
  for _ in range(8):
    runner.step()
    if runner._graphs is not None:
      break
  assert runner._graphs is not None
  seen = []
  for w in (torch.tensor([0.0, 1.0, 1.0]), torch.tensor([2.0, 0.5, 0.0])):
    model.inputs['sample_weight'].copy_(w)
    graphs = runner._graphs
    runner.step()
    torch.cuda.synchronize()
    assert runner._graphs is graphs
    seen.append(_check_loss_parts(model, w))
  # (the parameters moved between the two, but so little that equal weights would give nearly equal losses: the weights were read)
  assert abs(seen[0] - seen[1]) > 1e-3 * abs(seen[0])


def test_all_zero_weights_train_like_a_zero_gradient(dev):
  """sample_weights with an all-zero vector and l2_regularizer = 0: m, v and p are bit-equal to an Adam step on a zero gradient."""
  cfg_kw, goal = MODEL_CASES[0][1], MODEL_CASES[0][2]
  model = _model(dev, cfg_kw, goal, loss_shaping={'sample_weights': True})
  model.inputs['sample_weight'].zero_()
  model.train_step()
  torch.cuda.synchronize()
  assert float(model.loss) == 0.0 and not model.store.grads.any()
  twin = _model(dev, cfg_kw, goal)
  twin.forward(backward_too=True)
  twin.backward(adam_prepare=True)
  twin.store.grads.zero_()
  twin.apply_gradients()
  torch.cuda.synchronize()
  for k in ('params', 'adam_m', 'adam_v'):
    assert torch.equal(getattr(model.store, k), getattr(twin.store, k)), k
  assert int(model.store.global_step.item()) == int(twin.store.global_step.item()) == 1


# ================================================================================================
# Estimator
# ================================================================================================
def _events(model_dir):
  with open(os.path.join(model_dir, 'events.jsonl')) as f:
    return [json.loads(line) for line in f]


def test_estimator_trains_and_evaluates_with_shaped_losses(dev, tmp_path):
  from geeco_amd import estimator as est
  from geeco_amd import input_fn as I
  from geeco_amd.params import create_e2evmc_config
  cfg = create_e2evmc_config(dict(window_size=2, img_height=HW, img_width=HW, batch_size=3))
  weigh = lambda f, l: (np.arange(len(f['step'])) % 3).astype(np.float64)      # 0, 1, 2
  source = lambda mode, **kw: (lambda: I.pickplace_input_fn('synthetic:4:%dx%d' % (HW, HW), 'default', mode, window_size=2, batch_size=3, **kw))

  def run(tag, shaping, **kw):
    md = str(tmp_path / tag)
    est._SummarySaverHook._writers.pop(md, None)
    params = {'e2evmc_config': cfg, 'log_steps': 2, 'debug': False}
    if shaping:
      params['loss_shaping'] = shaping
    e = est.Estimator(est.e2evmc_model_fn, md, est.RunConfig(init_seed=4), params)
    e.train(input_fn=source('train', **kw))
    res = e.evaluate(input_fn=source('eval', **kw))
    est._SummarySaverHook._writers.pop(md).close()
    return e, md, res

  e1, md1, shaped = run('on', SHAPING, sample_weight=weigh)
  first = _events(md1)[0]
  assert first['loss_shaping'] == {'sample_weights': True, 'grp_class_weights': CLASS_W, 'label_smoothing': SMOOTH,
                                   'huber_delta': {'cmd_ee': DELTA, 'pos_ee': DELTA, 'pos_obj': DELTA}}
  assert sum('loss_shaping' in line for line in _events(md1)) == 1
  # an unshaped Estimator evaluating the SAME checkpoint: another loss, the same metric values
  e0 = est.Estimator(est.e2evmc_model_fn, md1, est.RunConfig(init_seed=4), {'e2evmc_config': cfg, 'log_steps': 2, 'debug': False})
  plain = e0.evaluate(input_fn=source('eval'))
  assert set(plain) == set(shaped)
  assert abs(plain['loss'] - shaped['loss']) > 1e-3 * abs(plain['loss'])
  for k in plain:
    if k not in ('loss', 'global_step'):
      assert plain[k] == shaped[k], k
  # the evaluation model took the option too (the reference builds the same loss in both modes): its last batch's loss is the reference's
  spec = next(sp for key, sp in e1._specs.items() if key[0] == est.ModeKeys.EVAL)[0]
  assert spec.model.loss_shaping is not None and not spec.model.training
  _check_loss_parts(spec.model, spec.model.inputs['sample_weight'].cpu())
  # a missing labels['sample_weight'] is a KeyError naming it
  e2 = est.Estimator(est.e2evmc_model_fn, None, est.RunConfig(init_seed=4), {'e2evmc_config': cfg, 'loss_shaping': {'sample_weights': True}})
  with pytest.raises(KeyError, match='sample_weight'):
    e2.train(input_fn=source('train'))


def test_weights_are_single_gpu_and_the_rest_is_not(dev, monkeypatch):
  from geeco_amd import dist as gdist
  from geeco_amd import estimator as est
  from geeco_amd.params import create_e2evmc_config
  cfg = create_e2evmc_config(dict(window_size=2, img_height=HW, img_width=HW, batch_size=2))
  monkeypatch.setattr(gdist, 'world_size', lambda: 2)
  feats = {'rgb': torch.zeros(2, 2, HW, HW, 3, device=dev)}
  for shaping, named in (({'sample_weights': True}, 'sample_weights'), ({'grp_class_weights': CLASS_W}, 'grp_class_weights')):
    for mode in (est.ModeKeys.TRAIN, est.ModeKeys.EVAL):
      with pytest.raises(ValueError, match=r"params\['loss_shaping'\]\['%s'\] is single-GPU: with 2 ranks" % named):
        est.e2evmc_model_fn(feats, {}, mode, {'e2evmc_config': cfg, 'loss_shaping': shaping})
  # label smoothing and Huber pass the check: the model is built and the next thing missing is an input
  for shaping in ({'label_smoothing': SMOOTH}, {'huber_delta': DELTA}):
    with pytest.raises(KeyError, match="missing input 'jnt_state'"):
      est.e2evmc_model_fn(feats, {}, est.ModeKeys.TRAIN, {'e2evmc_config': cfg, 'loss_shaping': shaping})
