"""Whole-graph parity on the GPU: forward outputs, loss, every variable's gradient and the
post-Adam weights of geeco_amd (HIP) vs the fp64 CPU oracle on the same seeded inputs/weights.

Tolerances (fp32 HIP vs fp64 oracle): loss, loss parts, predictions, dynamic images against the PLAIN oracle: loss 1e-4
relative (BASELINE.json north_star).  Gradients -- ONE standard, the full-size test's (tests/_relu_taps.py): the
oracle's backward under the device's ReLU decisions (``oracle.ReluTap``: every proc_obs x proc_tgt branch and the K-step
e2e_vmc), every variable to 2e-5 of max |g| AND 2e-5 in relative L2, and every decision in which the device differs from
the fp64 oracle on a pre-activation |z| <= 2e-5.  (Rounds 1-3 bounded these cases by max(2e-4, 4 x the fp32 CPU oracle's
error) capped at 1e-2 -- a yardstick that compares two samples of a heavy-tailed quantity; gone.)  Adam step 1
moves every weight by ~lr * sign(g) so weights are compared with atol = 2.5 * lr ("Adam step-1 sign
sensitivity").
"""
import numpy as np
import pytest
import torch

from oracle import geeco_oracle as O
import _relu_taps as T

pytestmark = pytest.mark.gpu


def _mk(cfg_kw, goal, N, H, seed=1):
  cfg_kw = dict(cfg_kw, img_height=H, img_width=H, batch_size=N)
  ocfg = O.make_config(**cfg_kw)
  shapes = O.model_param_shapes(ocfg, goal)
  P = O.init_params(shapes, seed=seed)
  # non-zero biases so that bias paths are exercised
  r = np.random.default_rng(seed + 1)
  for k in P:
    if k.endswith('/bias'):
      P[k] = (0.05 * r.standard_normal(P[k].shape)).astype(np.float32)
  feats, labels = O.synthetic_batch(ocfg, goal, N, seed=seed + 2, H=H, W=H)
  return ocfg, P, feats, labels


def _build(ocfg, goal, P, feats, labels, dev):
  from geeco_amd import graph
  from geeco_amd.params import create_e2evmc_config
  cfg = create_e2evmc_config(ocfg._asdict())
  N = feats['rgb'].shape[0]
  model = (graph.GoalE2EVMC if goal else graph.E2EVMC)(cfg, N, dev, training=True)
  assert list(model.store.shapes.keys()) == list(P.keys())
  model.store.load_numpy(P)
  model.load_batch({k: torch.from_numpy(v) for k, v in feats.items()}, {k: torch.from_numpy(v) for k, v in labels.items()})
  return model


def _rel_max(a, b):
  a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
  return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


CASES = [
    ('geeco-f rgb', dict(proc_obs='dynimg', proc_tgt='dyndiff', window_size=4), True, 2, 160),
    ('geeco-f rgbd', dict(proc_obs='dynimg', proc_tgt='dyndiff', window_size=3, img_channels=4, lambda_aux=0.5), True, 2, 136),
    ('e2e_vmc rgb', dict(window_size=3), False, 2, 144),
    ('geeco-f rgb 256', dict(proc_obs='dynimg', proc_tgt='dyndiff', window_size=16), True, 2, 256),
    # BASELINE.json configs[0] (the reference's own CPU-runnable case, and bench.py's cpu_baseline workload): batch 4, seq_len 16
    ('geeco-f rgb 256 N=4', dict(proc_obs='dynimg', proc_tgt='dyndiff', window_size=16, batch_size=4), True, 4, 256),
    # remaining goal_e2evmc branches (graph.py:362-385), velocity heads (:240-249, 430-450), L2 regulariser
    ('goal seq constant', dict(proc_obs='sequence', proc_tgt='constant', window_size=2), True, 2, 136),
    ('goal seq residual', dict(proc_obs='sequence', proc_tgt='residual', window_size=3), True, 2, 136),
    ('goal seq dyndiff', dict(proc_obs='sequence', proc_tgt='dyndiff', window_size=2), True, 2, 136),
    ('e2e_vmc velocity', dict(window_size=2, control_mode='velocity'), False, 3, 136),
    ('geeco-f l2', dict(proc_obs='dynimg', proc_tgt='dyndiff', window_size=3, l2_regularizer=1e-3), True, 2, 136),
    # unequal dim_s_obs / dim_s_dyn / dim_s_diff (train_e2evmc.py:55-61; graph.py:390,394,402): conv1-7 grouped, conv8 per encoder
    ('geeco-f dims 256/128/64', dict(proc_obs='dynimg', proc_tgt='dyndiff', window_size=3, dim_s_obs=256, dim_s_dyn=128,
                                     dim_s_diff=64), True, 2, 136),
    ('goal seq dyndiff dims 128/64', dict(proc_obs='sequence', proc_tgt='dyndiff', window_size=2, dim_s_obs=128, dim_s_diff=64),
     True, 2, 136),
    # degenerate sizes: one sample, one-frame window (alpha = [0] => the buffer image is identically 0)
    ('geeco-f N=1 K=1', dict(proc_obs='dynimg', proc_tgt='dyndiff', window_size=1), True, 1, 136),
    ('e2e_vmc N=1 K=1', dict(window_size=1), False, 1, 136),
]


@pytest.mark.parametrize('name,cfg_kw,goal,N,H', CASES, ids=[c[0] for c in CASES])
def test_train_step_parity(dev, name, cfg_kw, goal, N, H):
  ocfg, P, feats, labels = _mk(cfg_kw, goal, N, H)
  model = _build(ocfg, goal, P, feats, labels, dev)
  oracle = O.OracleTrainer(ocfg, goal, P, dtype=torch.float64)

  # ---- forward + gradients ------------------------------------------------------------------
  collect = {}
  loss_ref, parts_ref, _, pred_ref, ep_ref = oracle.loss_and_grads(feats, labels, collect)     # the plain oracle
  model.forward(backward_too=True)
  torch.cuda.synchronize()
  masks = T.snapshot_masks(model.enc)               # before the backward: nothing it reuses can alias them
  model.backward()
  torch.cuda.synchronize()
  tap, slots = T.device_tap(model, goal, masks, ocfg.img_channels)
  loss_m, _, grads_ref, _, _ = oracle.loss_and_grads(feats, labels, tap=tap)                   # under the device's decisions
  assert sorted(tap.calls.items()) == sorted({sc: sum(1 for (s2, _) in slots if s2 == sc) for sc, _ in slots}.items())
  assert abs(float(loss_m) - float(loss_ref)) <= 1e-5 * abs(float(loss_ref))     # the decisions differ at rounding level only
  if goal:
    ep = model.endpoints()
    for k in ('dynbuff', 'dyndiff'):
      if k in ep_ref:
        assert _rel_max(ep[k].cpu().numpy(), ep_ref[k].numpy()) < 2e-5, k
  preds = {k: v.cpu().numpy() for k, v in model.predictions().items()}
  for k, v in pred_ref.items():
    np.testing.assert_allclose(preds[k], v.numpy(), rtol=1e-4, atol=2e-5, err_msg=k)
  parts = {k: float(v) for k, v in model.loss_parts().items()}
  assert abs(parts['loss'] - float(loss_ref)) <= 1e-4 * abs(float(loss_ref)), (parts['loss'], float(loss_ref))
  for k, v in parts_ref.items():
    if k == 'loss_reg' and ocfg.l2_regularizer == 0.0:
      continue
    assert abs(parts[k] - float(v)) <= 1e-4 * abs(float(v)) + 1e-7, k
  grads = model.store.to_numpy('grads')
  if ocfg.l2_regularizer > 0.0:   # the HIP path folds d(loss_reg)/dv = l2 * v into the Adam kernel, not the arena
    grads = {k: g + np.float32(ocfg.l2_regularizer) * P[k] for k, g in grads.items()}
  n_dis, n_tot, worst_z = T.check_decisions(tap.stats)
  _, worst = T.check_gradients(grads, grads_ref)
  print('%s: loss %.6f (ref %.6f), worst gradient error %.2e (max-norm or rel. L2, bound %.0e) at %s; %d of %d ReLU decisions '
        'differ from the fp64 oracle, all at |z| <= %.1e' % (name, parts['loss'], float(loss_ref), worst[1], T.GRAD_TOL, worst[0],
                                                             n_dis, n_tot, worst_z))

  # ---- two optimiser steps -------------------------------------------------------------------
  lr = ocfg.lr
  for step in range(2):
    model.train_step()
    torch.cuda.synchronize()
    l_ref, _ = oracle.train_step(feats, labels)
    l_hip = float(model.loss)
    assert abs(l_hip - l_ref) <= 1e-4 * abs(l_ref), (step, l_hip, l_ref)
  assert int(model.store.global_step.item()) == 2
  Pn = model.store.to_numpy('params')
  for k, v in oracle.P.items():
    np.testing.assert_allclose(Pn[k], v.numpy(), rtol=0, atol=2.5 * lr, err_msg=k)
  # the typical weight moved by ~lr per step in the same direction as the oracle's
  if ocfg.l2_regularizer > 0.0:
    return   # with L2 every weight moves; the sign-agreement probe below assumes data gradients only
  k0 = [k for k in P if k.endswith('conv2/kernel')][0]
  moved_ref = oracle.P[k0].numpy() - P[k0]
  moved = Pn[k0] - P[k0]
  agree = np.mean(np.sign(moved) == np.sign(moved_ref))
  assert agree > 0.995, agree


def test_loss_trajectory_graph_replay(dev):
  """Ten optimiser steps through the production step runner (captured hipGraphs, multi-stream backward, fused
  kernels) on a FRESH batch every step vs the fp64 oracle trainer fed the same batches: per-step loss to 1e-4
  relative (BASELINE.json north_star).  Guards the replay path: device-resident Adam step counter, derived weight
  copies refreshed inside the Adam graph, input buffers rewritten between replays."""
  from geeco_amd.runtime import TrainStepRunner
  cfg_kw = dict(proc_obs='dynimg', proc_tgt='dyndiff', window_size=4, lr=1e-3)
  ocfg, P, feats, labels = _mk(cfg_kw, True, 2, 160)
  model = _build(ocfg, True, P, feats, labels, dev)
  oracle = O.OracleTrainer(ocfg, True, P, dtype=torch.float64)
  runner = TrainStepRunner(model, use_graph=True, warmup=2)
  losses = []
  for step in range(10):
    feats, labels = O.synthetic_batch(ocfg, True, 2, seed=100 + step, H=160, W=160)
    model.load_batch({k: torch.from_numpy(v) for k, v in feats.items()}, {k: torch.from_numpy(v) for k, v in labels.items()})
    runner.step()
    torch.cuda.synchronize()
    l_ref, _ = oracle.train_step(feats, labels)
    l_hip = float(model.loss)
    losses.append((l_hip, l_ref))
    assert abs(l_hip - l_ref) <= 1e-4 * abs(l_ref), (step, l_hip, l_ref)
  assert runner._graphs is not None                      # the last steps were graph replays
  assert int(model.store.global_step.item()) == 10
  print('loss trajectory (hip, oracle):', ['%.5f/%.5f' % p for p in losses])


@pytest.mark.parametrize('l2', [0.0, 1e-3])
def test_optimiser_step_in_pieces_is_the_one_pass_step(dev, l2):
  """geeco_adam_tf_segments (data parallel: the variables of the early bucket are updated while the late bucket is on the wire,
  conv1 / conv2 of the encoders follow with their gradients read from the staging buffer): any partition of the arena, with the
  gradients of some pieces living elsewhere, gives bitwise geeco_adam_tf's parameters and moments; ``g_out`` receives the foreign
  pieces' gradients; pieces that are not multiples of four floats are refused.
  (geeco_adam_tf itself is pinned by test_primitives_gpu.py::test_adam_three_steps, the pieces against fp64 by test_adam_segments.)"""
  from geeco_amd import ops
  r = np.random.default_rng(171)
  n = 4 * 25013
  p0 = torch.tensor(r.standard_normal(n).astype(np.float32), device=dev)
  g = torch.tensor(r.standard_normal(n).astype(np.float32), device=dev)
  m0 = torch.tensor((0.1 * r.standard_normal(n)).astype(np.float32), device=dev)
  v0 = torch.tensor((0.01 * r.random(n)).astype(np.float32), device=dev)
  scal = torch.tensor([3.1e-4, 0.0], device=dev)
  pa, ma, va = p0.clone(), m0.clone(), v0.clone()
  ops.adam_tf(pa, g, ma, va, n, scal, grad_scale=0.125, l2=l2)
  cuts = [0, 4 * 216, 4 * 3908, 4 * 3908 + 4, 4 * 20000, n]            # five pieces, one of a single float4
  pb, mb, vb = p0.clone(), m0.clone(), v0.clone()
  staged = torch.cat([g[cuts[1]:cuts[2]], g[cuts[3]:cuts[4]]]).contiguous()   # two pieces' gradients live in a buffer of their own
  g_arena = g.clone()
  g_arena[cuts[1]:cuts[2]] = float('nan')
  g_arena[cuts[3]:cuts[4]] = float('nan')
  ops.adam_tf_segments(pb, mb, vb, [(g_arena[cuts[0]:cuts[1]], cuts[0], cuts[1] - cuts[0]), (g_arena[cuts[2]:cuts[3]], cuts[2], 4),
                                    (g_arena[cuts[4]:], cuts[4], n - cuts[4])], scal, grad_scale=0.125, l2=l2)
  k = cuts[2] - cuts[1]
  ops.adam_tf_segments(pb, mb, vb, [(staged[:k], cuts[1], k), (staged[k:], cuts[3], cuts[4] - cuts[3])], scal, g_out=g_arena,
                       grad_scale=0.125, l2=l2)
  torch.cuda.synchronize()
  assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb)
  assert torch.equal(g_arena, g)
  with pytest.raises(Exception):
    ops.adam_tf_segments(pb, mb, vb, [(g, 0, 6)], scal)
  with pytest.raises(ValueError):
    ops.adam_tf_segments(pb, mb, vb, [(g, 0, 4)] * 9, scal)


@pytest.mark.parametrize('goal', [True, False], ids=['geeco-f', 'e2e_vmc'])
def test_optimiser_scalars_ride_in_the_last_slab_sum(dev, goal):
  """train_step() / the step runner let the Adam step counter and lr_t ride in the backward's last slab-sum launch
  (geeco_slab_reduce_batch_prepare) instead of a dependent launch of their own.  Same trajectory, bitwise, as forward / backward /
  apply_gradients called one by one (where apply_gradients launches geeco_adam_prepare itself), the counter advances exactly
  once per optimiser step in both, and a backward that is NOT followed by an update leaves the counter alone."""
  cfg_kw = dict(proc_obs='dynimg', proc_tgt='dyndiff', window_size=3, lr=1e-3) if goal else dict(window_size=3, lr=1e-3)
  ocfg, P, feats, labels = _mk(cfg_kw, goal, 2, 136)
  a = _build(ocfg, goal, P, feats, labels, dev)
  b = _build(ocfg, goal, P, feats, labels, dev)
  for _ in range(3):
    a.train_step()
    b.forward(backward_too=True)
    b.backward()
    b.apply_gradients()
  torch.cuda.synchronize()
  assert int(a.store.global_step.item()) == int(b.store.global_step.item()) == 3
  assert torch.equal(a.store.params, b.store.params) and torch.equal(a.store.adam_v, b.store.adam_v)
  assert float(a.scal[0]) == float(b.scal[0])
  b.forward(backward_too=True)
  b.backward()                        # no update follows: nothing may have advanced
  torch.cuda.synchronize()
  assert int(b.store.global_step.item()) == 3


@pytest.mark.parametrize('use_graph', [False, True], ids=['eager', 'hipGraph'])
@pytest.mark.parametrize('goal', [True, False], ids=['geeco-f', 'e2e_vmc'])
def test_optimiser_beside_the_encoder_bottom_is_bitwise_the_plain_step(dev, goal, use_graph):
  """The single-GPU step of runtime.TrainStepRunner runs the slab sums of conv3..conv8 and Adam's early piece (99 % of the
  arena) on a second stream beside the fused encoder-bottom backward and Adam's late piece (conv1 / conv2) behind it
  (graph._ModelBase.backward_and_apply).  Parameters, both Adam slots, the gradient arena, the step counter and every
  step's loss are bitwise those of train_step() (one slab-sum launch at the end + one Adam pass), eagerly and replayed."""
  from geeco_amd.runtime import TrainStepRunner
  cfg_kw = dict(proc_obs='dynimg', proc_tgt='dyndiff', window_size=3, lr=1e-3) if goal else dict(window_size=3, lr=1e-3)
  ocfg, P, feats, labels = _mk(cfg_kw, goal, 2, 136)
  a = _build(ocfg, goal, P, feats, labels, dev)
  b = _build(ocfg, goal, P, feats, labels, dev)
  r = TrainStepRunner(a, use_graph=use_graph, warmup=2)
  assert r.beside_bottom and a.can_apply_beside_bottom() and len(r.early) >= 1 and len(r.late) >= 1
  la, lb = [], []
  for _ in range(6):          # (warm-up steps run eagerly, the rest replayed when use_graph)
    r.step()
    b.train_step()
    torch.cuda.synchronize()
    la.append(float(a.loss))
    lb.append(float(b.loss))
  assert (r._graphs is not None) == use_graph
  assert la == lb
  assert int(a.store.global_step.item()) == int(b.store.global_step.item()) == 6
  for name in ('params', 'adam_m', 'adam_v', 'grads'):
    assert torch.equal(getattr(a.store, name), getattr(b.store, name)), name
  assert float(a.scal[0]) == float(b.scal[0])
  # the plain path through the same runner (what a model without batched slab sums gets): the same bits again
  c = _build(ocfg, goal, P, feats, labels, dev)
  rc = TrainStepRunner(c, use_graph=use_graph, warmup=2)
  rc.beside_bottom = False
  for _ in range(6):
    rc.step()
  torch.cuda.synchronize()
  assert torch.equal(a.store.params, c.store.params) and torch.equal(a.store.adam_v, c.store.adam_v)
