"""Shared-frame training on the GPU: the three kernels of csrc/shared_frames.hip against numpy / the dense
launches they replace, the whole step of the three per-frame controllers against the fp64 oracle ON THE DENSE WINDOWS and
against the dense device model, and Estimator.train / evaluate with params['shared_frames'].

Tolerances.  Pack and the forward gather move values: bitwise.  The backward sums in fp32 in one fixed order: against the
float64 scatter-sum at rtol 1e-6, in all three modes, on batches as training has them: a goal frame is never a window frame,
so every slot's terms have one sign.  One more case per mode lets target slots coincide with window slots and feeds signed
terms; sums then cancel, a relative bound on a cancelled fp32 sum is not a property of any summation, and that case alone
is held to 1e-6 of the magnitude summed, sum |term|.  Whole step: the standing rules of tests/test_model_gpu.py and
tests/_relu_taps.py, unchanged.

Frame-table capacity of the goal cases: the windows of the issue's cases hold N + 2 (K - 1) = 8 distinct frames and the goal
frame of an episode is one more resident frame (input_fn uploads it beside the windowable ones), so the goal models take
F = 8 + 2 = 10, the capacity Estimator's ``shared_frames=True`` gives them; e2e_vmc takes F = 8."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import geeco_oracle as O
import _relu_taps as T
from _table_builder_cases import window_states_bwd_ref

pytestmark = pytest.mark.gpu

CELLS = 4
J = 7


# ================================================================================================
# kernels
# ================================================================================================
@pytest.mark.parametrize('u8', [True, False], ids=['uint8', 'float32'])
@pytest.mark.parametrize('hw', [(8, 12), (5, 5)], ids=['8x12', '5x5'])
def test_pack_frames_by_address_is_bitwise(dev, u8, hw):
  from geeco_amd import ops
  HW = hw[0] * hw[1]
  r = np.random.default_rng(HW + u8)
  if u8:
    host = r.integers(0, 256, [4, HW * 3]).astype(np.uint8)
    want = host.astype(np.float32) / np.float32(255.0)
  else:
    host = r.random([4, HW * 3], dtype=np.float32)
    want = host
  flat = torch.from_numpy(host.ravel()).to(dev)
  esz = flat.element_size()
  base = flat.data_ptr()
  # frame 3 once more, one element further: an address that is NOT aligned for the 4-pixel path
  odd = torch.from_numpy(np.concatenate([host[3, :1], host[3]])).to(dev)
  slots = [base + 2 * HW * 3 * esz, base, 0, base + HW * 3 * esz, odd.data_ptr() + esz, 0]
  frames = [2, 0, None, 1, 3, None]
  table = torch.tensor(slots, dtype=torch.int64, device=dev)
  x = torch.full((len(slots), HW, 4), float('nan'), device=dev)
  ops.pack_frames_by_address_into(x, table, len(slots), HW, u8)
  torch.cuda.synchronize()
  got = x.cpu().numpy()
  for s, f in enumerate(frames):
    exp = np.zeros((HW, 4), np.float32)
    if f is not None:
      exp[:, :3] = want[f].reshape(HW, 3)
    assert np.array_equal(got[s].view(np.uint32), exp.view(np.uint32)), (s, f)


def _index_case(N, K, seed, overlap=True):
  """idx with repeats, the LAST slot referenced by nothing.  Target slots: spread over the first slots, where windows point too
  (``overlap``), or slots of their own behind the window slots, one per pair of windows, as an episode's goal frame is."""
  r = np.random.default_rng(seed)
  nw = max(1, (N * K) // 2 + 1)                # slots the windows draw from
  nt = 0 if overlap else (N + 1) // 2
  F = nw + nt + 1
  idx = r.integers(0, nw, [N, K]).astype(np.int32)
  tgt = (np.arange(N) // 2).astype(np.int32) % nw if overlap else (nw + np.arange(N) // 2).astype(np.int32)
  return F, idx, tgt


SHAPES = [(1, 1), (4, 3), (5, 16)]


def _place(t, dev, shift):
  """``t`` on the device, its base ``shift`` floats behind a 16-byte boundary"""
  buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=dev)
  assert buf.data_ptr() % 16 == 0
  out = buf[shift:shift + t.numel()].view(t.shape)
  out.copy_(t)
  return out


@pytest.mark.parametrize('mode', ['plain', 'constant', 'residual'])
@pytest.mark.parametrize('ch', [256, 64, 6])
@pytest.mark.parametrize('N,K,shift', [s + (0,) for s in SHAPES] + [(4, 3, 1)])
def test_window_states_fwd_is_the_dense_concat(dev, mode, ch, N, K, shift):
  """``shift`` = 1: the feature base sits one float off a 16-byte boundary, so ch % 4 == 0 must still take the one-float loads."""
  from geeco_amd import ops
  F, idx, tgt = _index_case(N, K, N * K + ch)
  Ctot = ch + J + (ch if mode == 'constant' else 0)
  D = CELLS * Ctot
  g = torch.Generator().manual_seed(ch + N)
  feat = _place(torch.randn(F, CELLS, ch, generator=g), dev, shift)
  jnt = torch.randn(N, K, J, generator=g).to(dev)
  idx_d, tgt_d = torch.from_numpy(idx).to(dev), torch.from_numpy(tgt).to(dev)
  got = torch.full((K, N, D), float('nan'), device=dev)
  ops.window_states_fwd_into(got, feat, idx_d, jnt, mode, F, N, K, CELLS, ch, J, D, tgt_idx=None if mode == 'plain' else tgt_d)
  want = torch.full((K, N, D), float('nan'), device=dev)
  tf = feat[tgt_d.long()].contiguous()
  for t in range(K):
    ft = feat[idx_d[:, t].long()].contiguous()
    if mode == 'plain':
      ops.state_concat_fwd_into(want[t], [ft], [ch], 1, jnt[:, t], K * J, J, N, CELLS, D)
    elif mode == 'constant':
      ops.state_concat_fwd_into(want[t], [ft, tf], [ch, ch], 1, jnt[:, t], K * J, J, N, CELLS, D)
    else:
      ops.state_concat_fwd_into(want[t], [ft], [ch], 1, jnt[:, t], K * J, J, N, CELLS, D, sub_from=tf)
  torch.cuda.synchronize()
  assert not torch.isnan(want).any()
  assert torch.equal(got.view(torch.int32), want.view(torch.int32))


BWD_CASES = [s + (False, 0) for s in SHAPES] + [(5, 16, True, 0), (4, 3, False, 1)]


@pytest.mark.parametrize('mode', ['plain', 'constant', 'residual'])
@pytest.mark.parametrize('ch', [256, 6])
@pytest.mark.parametrize('N,K,overlap,shift', BWD_CASES)
def test_window_states_bwd_is_the_scatter_sum(dev, mode, ch, N, K, overlap, shift):
  """``overlap`` False (the required bound): positive terms, goal slots that no window uses -> every slot sums terms of one
  sign (all - for a window slot of the residual mode, all + otherwise): rtol 1e-6 against float64.  ``overlap`` True: signed
  terms, goal slots that windows use too -> bounded by 1e-6 of sum |term|.  ``shift`` = 1: feat and dfeat one float off a
  16-byte boundary (the one-float instantiation with ch % 4 == 0)."""
  from geeco_amd import ops
  F, idx, tgt = _index_case(N, K, N * K + ch + 1, overlap)
  Ctot = ch + J + (ch if mode == 'constant' else 0)
  D = CELLS * Ctot
  r = np.random.default_rng(ch + K)
  dst = (r.standard_normal([K, N, D]) if overlap else 0.5 + r.random([K, N, D])).astype(np.float32)
  feat = r.standard_normal([F, CELLS, ch]).astype(np.float32)
  ref, mag = window_states_bwd_ref(dst, feat, idx, tgt, mode, J)      # the float64 scatter-sum, masked by feat > 0
  feat_d = _place(torch.from_numpy(feat), dev, shift)
  args = (torch.from_numpy(dst).to(dev), D, torch.from_numpy(idx).to(dev), feat_d, mode, F, N, K, CELLS, ch, J)
  kw = dict(tgt_idx=None if mode == 'plain' else torch.from_numpy(tgt).to(dev))
  out = [_place(torch.full((F, CELLS, ch), float('nan')), dev, shift) for _ in range(2)]
  for o in out:
    ops.window_states_bwd_into(o, *args, **kw)
  torch.cuda.synchronize()
  got = out[0].cpu().numpy()
  assert torch.equal(out[0].contiguous().view(torch.int32), out[1].contiguous().view(torch.int32))             # deterministic
  referenced = np.zeros(F, bool)
  referenced[idx.ravel()] = True
  if mode != 'plain':
    referenced[tgt] = True
  assert not referenced[F - 1]
  assert not got[~referenced].any() and not np.signbit(got[~referenced]).any()       # exact zeros
  err = np.abs(got - ref)
  print('window_states_bwd %s ch=%d N=%d K=%d overlap=%d: worst |err| / sum|term| = %.2e'
        % (mode, ch, N, K, overlap, (err / np.maximum(mag, 1e-30)).max()))
  if overlap:
    assert (err <= 1e-6 * mag).all()
  else:
    assert np.array_equal(mag, np.abs(ref))         # nothing cancels
    np.testing.assert_allclose(got, ref, rtol=1e-6, atol=0)


# ================================================================================================
# whole step
# ================================================================================================
H = 136
K3 = 3
MODES = {'e2e_vmc': (False, {}), 'goal constant': (True, dict(proc_obs='sequence', proc_tgt='constant')),
         'goal residual': (True, dict(proc_obs='sequence', proc_tgt='residual'))}
# (episode, starts) segments; every episode holds 8 windowable frames + its goal frame (a 9-frame recording)
BATCHES = {'one episode': [(0, [0, 1, 2, 5])], 'two episodes': [(0, [4, 5]), (1, [0, 1])]}

_CACHE = {}


def _case(dev, mode, batch):
  """Config, weights, the resident uint8 episodes, the DeviceWindows of the batch and its DENSE float32 windows (what the oracle
  and the dense device model read) -- built once per (mode, batch) and left unchanged."""
  key = (mode, batch)
  if key in _CACHE:
    return _CACHE[key]
  from geeco_amd.input_fn import DeviceWindows
  goal, extra = MODES[mode]
  ocfg = O.make_config(window_size=K3, img_height=H, img_width=H, batch_size=4, **extra)
  P = O.init_params(O.model_param_shapes(ocfg, goal), seed=1)
  r = np.random.default_rng(2)
  for k in P:
    if k.endswith('/bias'):
      P[k] = (0.05 * r.standard_normal(P[k].shape)).astype(np.float32)
  feats, labels = O.synthetic_batch(ocfg, goal, 4, seed=3, H=H, W=H)
  episodes = [r.integers(0, 256, [9, H, H, 3]).astype(np.uint8) for _ in range(2)]
  resident = [torch.from_numpy(e[:8].reshape(8, -1)).to(dev) for e in episodes]
  goals = [torch.from_numpy(e[8:].reshape(1, -1)).to(dev) for e in episodes]
  win, tgt = DeviceWindows(K3, (H, H, 3), 255.0), DeviceWindows(1, (H, H, 3), 255.0, squeeze_k=True)
  dense, dense_tgt = [], []
  for ep, starts in BATCHES[batch]:
    win.add(resident[ep], np.asarray(starts, np.int32))
    tgt.add(goals[ep], np.zeros(len(starts), np.int32))
    for s in starts:
      dense.append(episodes[ep][s:s + K3])
      dense_tgt.append(episodes[ep][8])
  feats['rgb'] = np.stack(dense).astype(np.float32) / np.float32(255.0)
  if goal:
    feats['target_rgb'] = np.stack(dense_tgt).astype(np.float32) / np.float32(255.0)
  _CACHE[key] = (ocfg, goal, P, feats, labels, win, tgt if goal else None, (resident, goals))
  return _CACHE[key]


def _shared_model(dev, ocfg, goal, P, feats, labels, win, tgt):
  from geeco_amd import graph
  from geeco_amd.params import create_e2evmc_config
  F = 4 + 2 * (K3 - 1) + (2 if goal else 0)
  table, index, tindex, used = win.frame_table(F, tgt, dev)
  assert used == (9 if goal and len(win.segments) == 1 else F)
  model = (graph.GoalE2EVMC if goal else graph.E2EVMC)(create_e2evmc_config(ocfg._asdict()), 4, dev, training=True, shared_frames=F)
  assert list(model.store.shapes.keys()) == list(P.keys())                # same VariableStore layout
  assert 'rgb' not in model.inputs and model.enc.Nf == F
  model.store.load_numpy(P)
  f = {k: torch.from_numpy(v) for k, v in feats.items() if k not in ('rgb', 'target_rgb')}
  f.update(frame_table=torch.from_numpy(table), frame_index=torch.from_numpy(index))
  if goal:
    f['target_index'] = torch.from_numpy(tindex)
  model.load_batch(f, {k: torch.from_numpy(v) for k, v in labels.items()})
  return model, index, tindex


def _dense_model(dev, ocfg, goal, P, feats, labels):
  from geeco_amd import graph
  from geeco_amd.params import create_e2evmc_config
  model = (graph.GoalE2EVMC if goal else graph.E2EVMC)(create_e2evmc_config(ocfg._asdict()), 4, dev, training=True)
  model.store.load_numpy(P)
  model.load_batch({k: torch.from_numpy(v) for k, v in feats.items()}, {k: torch.from_numpy(v) for k, v in labels.items()})
  return model


def _shared_tap(model, goal, masks, index, tindex):
  """The device's decisions per SLOT, handed to every oracle ``conv_encoder`` call by the slots its N frames sit in: a slot's
  decisions apply to every window position that uses it.  Oracle call order: tests/_relu_taps.py ``call_slots``."""
  enc = model.enc
  scope = enc.scopes[0]

  def slots(call):
    if goal:
      return tindex if call == 0 else index[:, call - 1]
    return index[:, call]

  def masks_fn(sc, call):
    assert sc == scope
    s = torch.from_numpy(slots(call).astype(np.int64))
    return [masks[l][0].cpu()[s] for l in range(8)]

  def inputs_fn(sc, call):
    s = torch.from_numpy(slots(call).astype(np.int64))
    return enc.x_in[0].cpu()[s][..., :3]

  return O.ReluTap(masks_fn, inputs_fn, force=True)


@pytest.mark.parametrize('batch', list(BATCHES))
@pytest.mark.parametrize('mode', list(MODES))
def test_shared_step_parity(dev, mode, batch):
  ocfg, goal, P, feats, labels, win, tgt, _keep = _case(dev, mode, batch)
  model, index, tindex = _shared_model(dev, ocfg, goal, P, feats, labels, win, tgt)
  oracle = O.OracleTrainer(ocfg, goal, P, dtype=torch.float64)
  loss_ref, parts_ref, _, pred_ref, _ = oracle.loss_and_grads(feats, labels)          # the plain oracle on the DENSE windows
  model.forward(backward_too=True)
  torch.cuda.synchronize()
  masks = T.snapshot_masks(model.enc)
  model.backward()
  torch.cuda.synchronize()
  # the pack kernel's frames are the dense windows' frames, bitwise
  x = model.enc.x_in[0].cpu().numpy()
  assert np.array_equal(x[index][..., :3], feats['rgb']) and not x[..., 3].any()
  # ---- against the fp64 oracle ----------------------------------------------------------------------
  loss = float(model.loss)
  preds = {k: v.cpu().numpy() for k, v in model.predictions().items()}
  print('%s / %s: loss %.6f (oracle %.6f)' % (mode, batch, loss, float(loss_ref)))
  assert abs(loss - float(loss_ref)) <= 1e-4 * abs(float(loss_ref))
  for k, v in pred_ref.items():
    np.testing.assert_allclose(preds[k], v.numpy(), rtol=1e-4, atol=2e-5, err_msg=k)
  parts = {k: float(v) for k, v in model.loss_parts().items()}
  for k, v in parts_ref.items():
    if k != 'loss_reg':
      assert abs(parts[k] - float(v)) <= 1e-4 * abs(float(v)) + 1e-7, k
  tap = _shared_tap(model, goal, masks, index, tindex)
  loss_m, _, grads_ref, _, _ = oracle.loss_and_grads(feats, labels, tap=tap)         # under the device's decisions
  assert tap.calls == {model.enc.scopes[0]: K3 + (1 if goal else 0)}
  assert abs(float(loss_m) - float(loss_ref)) <= 1e-5 * abs(float(loss_ref))
  grads = model.store.to_numpy('grads')
  n_dis, n_tot, worst_z = T.check_decisions(tap.stats)
  errs = {k: (T.rel_max(grads[k], g.numpy()), T.rel_l2(grads[k], g.numpy())) for k, g in grads_ref.items()}
  worst = max(errs.items(), key=lambda kv: max(kv[1]))
  print('%s / %s: worst gradient error %.2e max-norm / %.2e rel. L2 at %s (bound %.0e); %d of %d ReLU decisions differ, all at '
        '|z| <= %.1e' % (mode, batch, worst[1][0], worst[1][1], worst[0], T.GRAD_TOL, n_dis, n_tot, worst_z))
  T.check_gradients(grads, grads_ref)
  # ---- against the dense device model (the batched-vs-batch-1 tolerance: split-K follows the launch's frame count) ----
  dense = _dense_model(dev, ocfg, goal, P, feats, labels)
  dense.forward(backward_too=True)
  dense.backward()
  torch.cuda.synchronize()
  np.testing.assert_allclose(loss, float(dense.loss), rtol=1e-4, atol=2e-5)
  for k, v in dense.predictions().items():
    np.testing.assert_allclose(preds[k], v.cpu().numpy(), rtol=1e-4, atol=2e-5, err_msg=k)
  gd = dense.store.to_numpy('grads')
  print('%s / %s: shared vs dense device gradients, worst rel. L2 %.2e' % (mode, batch, max(T.rel_l2(grads[k], gd[k]) for k in gd)))


@pytest.mark.parametrize('mode', list(MODES))
def test_two_shared_steps_are_bitwise_equal(dev, mode):
  """Two optimiser steps from the same state, through backward_and_apply (the production step's form): parameters, both Adam
  slots and the gradient arena bitwise equal -- the scatter sums in one fixed order."""
  ocfg, goal, P, feats, labels, win, tgt, _keep = _case(dev, mode, 'one episode')
  from geeco_amd.runtime import gradient_buckets
  arenas = []
  for _ in range(2):
    model, _, _ = _shared_model(dev, ocfg, goal, P, feats, labels, win, tgt)
    model.forward(backward_too=True)
    early, late = gradient_buckets(model.store)
    model.backward_and_apply(early, late)
    torch.cuda.synchronize()
    s = model.store
    assert int(s.global_step.item()) == 1
    arenas.append([t.clone() for t in (s.params, s.adam_m, s.adam_v, s.grads)])
  for a, b in zip(*arenas):
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_eval_model_takes_the_option(dev):
  ocfg, goal, P, feats, labels, win, tgt, _keep = _case(dev, 'goal residual', 'two episodes')
  train, index, tindex = _shared_model(dev, ocfg, goal, P, feats, labels, win, tgt)
  train.forward(backward_too=False)
  from geeco_amd import graph
  from geeco_amd.params import create_e2evmc_config
  ev = graph.GoalE2EVMC(create_e2evmc_config(ocfg._asdict()), 4, dev, training=False, store=train.store, shared_frames=10)
  for k in ev.inputs:
    ev.inputs[k] = train.inputs[k]
  ev._bind_labels()
  ev.forward()
  torch.cuda.synchronize()
  # (the inference encoder runs conv1..conv3 without the sign-field epilogues of the training one: same values to rounding)
  np.testing.assert_allclose(ev.decoder.preds.cpu().numpy(), train.decoder.preds.cpu().numpy(), rtol=1e-5, atol=1e-6)
  np.testing.assert_allclose(float(ev.loss), float(train.loss), rtol=1e-5)


# ================================================================================================
# Estimator
# ================================================================================================
def _losses(model_dir):
  return [json.loads(l)['loss'] for l in open(os.path.join(model_dir, 'events.jsonl'))]


def test_estimator_trains_on_shared_frames(dev, tmp_path):
  """3 steps of e2e_vmc on a 2-episode dataset (2 x 6 windows, batches of 4: one episode, both, one): the loss trajectory of
  params['shared_frames']=True within 1e-4 relative of the dense-window run; evaluate works with the option on."""
  from geeco_amd import estimator as est
  from geeco_amd import input_fn as I
  from geeco_amd.params import create_e2evmc_config
  root = str(tmp_path / 'ds')
  I.write_synthetic_dataset(root, 2, episode_length=9, img_hw=(H, H), seed=5)
  kw = dict(window_size=K3, batch_size=4, device='cuda', device_keys=('rgb',), cache=False, num_threads=2)
  cfg = create_e2evmc_config(dict(window_size=K3, img_height=H, img_width=H, batch_size=4))
  runs = {}
  for shared in (False, True):
    md = str(tmp_path / ('m%d' % shared))
    params = {'e2evmc_config': cfg, 'log_steps': 1, 'debug': False}
    if shared:
      params['shared_frames'] = True
    e = est.Estimator(est.e2evmc_model_fn, md, est.RunConfig(), params)
    e.train(input_fn=lambda: I.pickplace_input_fn(root, 'default', 'train', seed=3, **kw))
    runs[shared] = (_losses(md), e.evaluate(input_fn=lambda: I.pickplace_input_fn(root, 'default', 'eval', **kw)))
    if shared:
      (spec, fbuf, _), = [v for k, v in e._specs.items() if k[0] == est.ModeKeys.TRAIN]
      assert spec.model.shared_frames == 4 + 2 * (K3 - 1) and list(fbuf) .count('rgb') == 1 and 'rgb' not in spec.model.inputs
  (dense, ev_d), (shared, ev_s) = runs[False], runs[True]
  print('loss trajectories: dense %s, shared %s; eval %s / %s' % (dense, shared, ev_d['loss'], ev_s['loss']))
  assert len(dense) == len(shared) == 3 and ev_s['global_step'] == 3
  np.testing.assert_allclose(shared, dense, rtol=1e-4)
  np.testing.assert_allclose(ev_s['loss'], ev_d['loss'], rtol=1e-4)


def test_estimator_goal_model_on_shared_frames(dev, tmp_path):
  """The goal model through the Estimator: the target stream rides in the same table (one slot per episode)."""
  from geeco_amd import estimator as est
  from geeco_amd import input_fn as I
  from geeco_amd.params import create_e2evmc_config
  root = str(tmp_path / 'ds')
  I.write_synthetic_dataset(root, 2, episode_length=7, img_hw=(H, H), seed=6)
  kw = dict(window_size=K3, batch_size=4, fetch_target=True, device='cuda', device_keys=('rgb',), cache=False, num_threads=2)
  cfg = create_e2evmc_config(dict(proc_obs='sequence', proc_tgt='residual', window_size=K3, img_height=H, img_width=H, batch_size=4))
  runs = []
  for shared in (False, True):
    md = str(tmp_path / ('m%d' % shared))
    e = est.Estimator(est.goal_e2evmc_model_fn, md, est.RunConfig(), dict({'e2evmc_config': cfg, 'log_steps': 1},
                                                                          **({'shared_frames': True} if shared else {})))
    e.train(input_fn=lambda: I.pickplace_input_fn(root, 'default', 'train', seed=3, **kw))
    runs.append(_losses(md))
  assert len(runs[0]) == 2
  np.testing.assert_allclose(runs[1], runs[0], rtol=1e-4)


def test_refusals(dev, monkeypatch):
  from geeco_amd import estimator as est
  from geeco_amd import graph
  from geeco_amd.input_fn import synthetic_batches
  from geeco_amd.params import create_e2evmc_config
  base = dict(window_size=K3, img_height=H, img_width=H, batch_size=2)
  cfg = create_e2evmc_config(base)
  # dense input
  e = est.Estimator(est.e2evmc_model_fn, None, est.RunConfig(), {'e2evmc_config': cfg, 'shared_frames': True})
  with pytest.raises(ValueError, match='DeviceWindows'):
    e.train(input_fn=synthetic_batches(2, K3, 1, (H, H), 3, False, seed=7), steps=1)
  # more than one rank
  monkeypatch.setattr(est.gdist, 'world_size', lambda: 2)
  with pytest.raises(ValueError, match='single-GPU'):
    est.e2evmc_model_fn({'rgb': torch.zeros(2, K3, H, H, 3, device=dev)}, None, est.ModeKeys.TRAIN,
                        {'e2evmc_config': cfg, 'shared_frames': True})
  monkeypatch.undo()
  # what has nothing to share
  for extra, goal, msg in ((dict(proc_obs='dynimg', proc_tgt='dyndiff'), True, 'dynimg'),
                           (dict(proc_obs='sequence', proc_tgt='dyndiff'), True, 'dyndiff'),
                           (dict(img_channels=4), False, 'RGB-D')):
    with pytest.raises(ValueError, match=msg):
      (graph.GoalE2EVMC if goal else graph.E2EVMC)(create_e2evmc_config(dict(base, **extra)), 2, dev, training=True, shared_frames=8)
