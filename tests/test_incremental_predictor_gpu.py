"""Incremental predictor on the GPU: the feature push + gather and the newest-frame pack against their specifications (bitwise),
the incremental predictors against the windowed ones and the oracle (the project's tolerance for launches of different shapes),
against themselves (bitwise: history and neighbour independence, uint8 == float32), the batch-1 classes, structure and errors."""
import numpy as np
import pytest
import torch

from oracle import geeco_oracle as O
from test_batched_predictor_gpu import _model_dir, _streams
from test_incremental_predictor_cpu import FeatureRingModel

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 2e-5      # tests/test_batched_predictor_gpu.py: batched vs batch-1 and vs the oracle
S = 136


def _classes(goal):
  from geeco_amd.batched_predictor import BatchedE2EVMCPredictor, BatchedGoalE2EVMCPredictor
  return BatchedGoalE2EVMCPredictor if goal else BatchedE2EVMCPredictor


# ---- kernels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['plain', 'constant', 'residual'])
@pytest.mark.parametrize('ch', [256, 64, 6])          # 6: the one-float path (ch % 4 != 0)
@pytest.mark.parametrize('B,K', [(1, 1), (3, 3), (5, 16)])
def test_push_features_kernel_matches_ring_model(dev, mode, ch, B, K):
  """24 calls with per-env resets and a goal change: rings, heads and the gathered states equal FeatureRingModel bitwise; a call
  with the any-bad word set leaves rings, heads and states untouched."""
  from geeco_amd import ops
  cells, J = 4, 7
  r = np.random.default_rng(1000 * B + 10 * K + ch)
  rm = FeatureRingModel(B, K, cells, ch, J, mode)
  D = cells * rm.Ctot
  stride = D + 5                                         # a row pitch wider than the row: the pad stays untouched
  states = torch.full((K, B, stride), -7.0, device=dev)
  fring = torch.zeros(B, K, cells, ch, device=dev)
  jring = torch.zeros(B, K, J, device=dev)
  heads = torch.zeros(B, dtype=torch.int32, device=dev)
  ctl = torch.zeros(B + 1, dtype=torch.int32, device=dev)
  tgt = r.standard_normal((B, cells, ch)).astype(np.float32)
  for call in range(24):
    reset = (r.random(B) < 0.25) | (call == 0)
    if call == 12:
      tgt = r.standard_normal((B, cells, ch)).astype(np.float32)
    f = r.standard_normal((B, cells, ch)).astype(np.float32)
    j = r.standard_normal((B, J)).astype(np.float32)
    td = torch.from_numpy(tgt).to(dev) if mode != 'plain' else None
    args = (torch.from_numpy(f).to(dev), torch.from_numpy(j).to(dev), torch.from_numpy(reset.astype(np.int32)).to(dev))
    if call == 7:                                        # a bad call first: nothing moves
      before = [x.clone() for x in (states, fring, jring, heads)]
      ctl[B] = 1
      ops.predict_push_features_into(states, fring, jring, heads, *args, ctl, mode, B, K, cells, ch, J, stride, tgt_feat=td)
      ctl[B] = 0
      for was, now in zip(before, (states, fring, jring, heads)):
        assert torch.equal(was, now)
    ops.predict_push_features_into(states, fring, jring, heads, *args, ctl, mode, B, K, cells, ch, J, stride, tgt_feat=td)
    want = rm.push(f, j, reset, tgt)
    torch.cuda.synchronize()
    got = states.cpu().numpy()
    np.testing.assert_array_equal(got[..., :D], want, err_msg='states call %d' % call)
    assert (got[..., D:] == -7.0).all()
    np.testing.assert_array_equal(fring.cpu().numpy(), rm.feat, err_msg='ring call %d' % call)
    np.testing.assert_array_equal(jring.cpu().numpy(), rm.jnt)
    np.testing.assert_array_equal(heads.cpu().numpy(), rm.heads)


def test_push_features_states_are_state_concat_columns(dev):
  """The gathered rows are, column for column, what state_concat_fwd_into writes for the same features (the layout the full
  models feed the decoder; state_concat_fwd_into itself: test_primitives_gpu.py::test_state_concat_fwd)."""
  from geeco_amd import ops
  B, K, cells, ch, J = 3, 1, 4, 64, 7
  r = np.random.default_rng(5)
  f, t = (torch.from_numpy(r.standard_normal((B, cells, ch)).astype(np.float32)).to(dev) for _ in range(2))
  j = torch.from_numpy(r.standard_normal((B, J)).astype(np.float32)).to(dev)
  ones = torch.ones(B, dtype=torch.int32, device=dev)
  ctl = torch.zeros(B + 1, dtype=torch.int32, device=dev)
  for mode in ('plain', 'constant', 'residual'):
    D = cells * (ch + J + (ch if mode == 'constant' else 0))
    got, want = torch.zeros(K, B, D, device=dev), torch.zeros(B, D, device=dev)
    ops.predict_push_features_into(got, torch.zeros(B, K, cells, ch, device=dev), torch.zeros(B, K, J, device=dev),
                                   torch.zeros(B, dtype=torch.int32, device=dev), f, j, ones, ctl, mode, B, K, cells, ch, J, D,
                                   tgt_feat=None if mode == 'plain' else t)
    if mode == 'constant':
      ops.state_concat_fwd_into(want, [f, t], [ch, ch], 1, j, J, J, B, cells, D)
    else:
      ops.state_concat_fwd_into(want, [f], [ch], 1, j, J, J, B, cells, D, sub_from=t if mode == 'residual' else None)
    torch.cuda.synchronize()
    assert torch.equal(got[0], want), mode


@pytest.mark.parametrize('shape', [(8, 12), (5, 5)])      # 5x5: the one-pixel path (HW % 4 != 0)
def test_pack_newest_kernel(dev, shape):
  from geeco_amd import ops
  H, W = shape
  B, r = 3, np.random.default_rng(8)
  for C, u8 in ((3, False), (4, False), (3, True)):
    f = r.integers(0, 256, (B, H, W, C), dtype=np.uint8) if u8 else r.random((B, H, W, C), dtype=np.float32)
    x = torch.full((B, H, W, 4), -3.0, device=dev)
    ops.predict_pack_newest_into(x, torch.from_numpy(f).to(dev), B, H * W, C)
    want = np.zeros((B, H, W, 4), np.float32)
    want[..., :C] = f.astype(np.float32) / np.float32(255.0) if u8 else f
    np.testing.assert_array_equal(x.cpu().numpy(), want)


# ---- predictors -----------------------------------------------------------------------------------------------------------
def _oracle_outputs(ocfg, Pt, goal, win_frames, win_jnts, tgt):
  """win_frames [K][B][H][W][C], win_jnts [K][B][J] -> the oracle's predictions in float64."""
  f = torch.tensor(win_frames.transpose(1, 0, 2, 3, 4), dtype=torch.float64)
  feats = {'rgb': f[..., :3], 'jnt_state': torch.tensor(win_jnts.transpose(1, 0, 2), dtype=torch.float64)}
  if ocfg.img_channels == 4:
    feats['depth'] = f[..., 3:4]
  if goal:
    t = torch.tensor(tgt, dtype=torch.float64)
    feats['target_rgb'] = t[..., :3]
    if ocfg.img_channels == 4:
      feats['target_depth'] = t[..., 3:4]
  ref, _ = O.model_forward(feats, Pt, ocfg, goal)
  return {k: v.numpy() for k, v in ref.items()}


def _compare(out, ref, cartesian, tag):
  for k, v in out.items():
    if k == 'cmd_grp' and cartesian:
      lg = np.sort(ref['logits_cmd_grp'], axis=-1)
      sure = lg[:, -1] - lg[:, -2] > ATOL + RTOL * np.abs(lg[:, -1])
      want = ref['logits_cmd_grp'].argmax(-1) - 1.0
      np.testing.assert_array_equal(v[sure, 0], want[sure], err_msg='cmd_grp %s' % tag)
      continue
    np.testing.assert_allclose(v, ref[k], rtol=RTOL, atol=ATOL, err_msg='%s %s' % (k, tag))


CONFIGS = [
    (False, dict(), 3, 3),
    (False, dict(), 1, 3),
    (False, dict(control_mode='velocity', img_channels=4), 3, 3),
    (True, dict(proc_obs='sequence', proc_tgt='constant'), 3, 3),
    (True, dict(proc_obs='sequence', proc_tgt='residual'), 3, 3),
    (True, dict(proc_obs='sequence', proc_tgt='residual', control_mode='velocity', img_channels=4, dim_s_obs=64), 1, 3),
    (False, dict(), 1, 16),
    (True, dict(proc_obs='sequence', proc_tgt='constant'), 3, 16),
]


@pytest.mark.parametrize('goal,extra,B,K', CONFIGS)
def test_incremental_matches_windowed_and_oracle(dev, tmp_path, goal, extra, B, K):
  """K + 5 calls, one env reset in the middle and (goal models) one env's goal changed in the middle: every output of the
  incremental predictor matches the windowed batched predictor and the float64 oracle on the same windows."""
  kw = dict(window_size=K, img_height=S, img_width=S, **extra)
  cfg, P = _model_dir(str(tmp_path), goal, kw)
  C, T = cfg.img_channels, K + 5
  r = np.random.default_rng(17 + K + B)
  frames, jnts = _streams(r, B, T, S, S, C)
  tgt = r.random((B, S, S, C), dtype=np.float32)
  inc = _classes(goal)(str(tmp_path), num_envs=B, memcap=None, device=dev, incremental=True)
  full = _classes(goal)(str(tmp_path), num_envs=B, memcap=None, device=dev)
  assert inc.window_form == 'features' and inc.num_envs == B and inc.cfg.batch_size == B
  if goal:
    inc.set_goal(tgt)
    full.set_goal(tgt)
  ocfg = O.make_config(batch_size=B, **kw)
  Pt = {k: torch.tensor(v, dtype=torch.float64) for k, v in P.items()}
  since = [[] for _ in range(B)]                            # per env: the calls since its last reset
  t_reset, t_goal, e = K + 1, K + 2, B - 1
  for t in range(T):
    if t == t_reset:
      inc.reset([e])
      full.reset([e])
      since[e] = []
    if goal and t == t_goal:
      g = r.random((S, S, C), dtype=np.float32)
      tgt[0] = g
      inc.set_goal(g, env_ids=[0])
      full.set_goal(g, env_ids=[0])
    oi, of = inc.predict(frames[t], jnts[t]), full.predict(frames[t], jnts[t])
    assert set(oi) == set(of)
    idx = np.zeros((K, B), dtype=np.int64)
    for b in range(B):
      since[b].append(t)
      w = since[b][-K:]
      idx[:, b] = [w[0]] * (K - len(w)) + w                  # first-frame padding, then slide
    wf = np.stack([frames[idx[:, b], b] for b in range(B)], axis=1)
    wj = np.stack([jnts[idx[:, b], b] for b in range(B)], axis=1)
    ref = _oracle_outputs(ocfg, Pt, goal, wf, wj, tgt)
    cart = cfg.control_mode == 'cartesian'
    for k in oi:
      assert oi[k].shape == of[k].shape and oi[k].dtype == of[k].dtype, k
    _compare(oi, ref, cart, 'vs oracle, call %d' % t)
    for k in oi:
      if k == 'cmd_grp' and cart:
        continue                                             # compared with the oracle's sure rows above
      np.testing.assert_allclose(oi[k], of[k], rtol=RTOL, atol=ATOL, err_msg='%s vs windowed, call %d' % (k, t))


@pytest.mark.parametrize('goal,extra', [(False, dict()), (True, dict(proc_obs='sequence', proc_tgt='residual'))])
def test_history_independence_bitwise(dev, tmp_path, goal, extra):
  """After sliding through 3 K + 2 calls (with a reset and a goal change on the way) the outputs equal, bit for bit, those of a
  fresh incremental predictor of the same B that was reset and fed only the last K frames: an env's output is a function of its
  window's contents, not of where the ring's head stands or of what the slots held before."""
  K, B = 3, 3
  kw = dict(window_size=K, img_height=S, img_width=S, **extra)
  cfg, _ = _model_dir(str(tmp_path), goal, kw)
  T = 3 * K + 2
  r = np.random.default_rng(23)
  frames, jnts = _streams(r, B, T, S, S, 3)
  tgt = r.random((B, S, S, 3), dtype=np.float32)
  a = _classes(goal)(str(tmp_path), num_envs=B, memcap=None, device=dev, incremental=True)
  if goal:
    a.set_goal(r.random((B, S, S, 3), dtype=np.float32))     # an earlier goal: replaced below
  for t in range(T):
    if t == 4:
      a.reset([1])
    if goal and t == 5:
      a.set_goal(tgt)
    last = a.predict(frames[t], jnts[t])
  b = _classes(goal)(str(tmp_path), num_envs=B, memcap=None, device=dev, incremental=True)
  if goal:
    b.set_goal(tgt)
  for t in range(T - K, T):
    fresh = b.predict(frames[t], jnts[t])
  for k in last:
    np.testing.assert_array_equal(last[k], fresh[k], err_msg=k)
  # ... and the same predictor, reset, gives them again (the rings' old contents do not matter)
  a.reset()
  for t in range(T - K, T):
    again = a.predict(frames[t], jnts[t])
  for k in last:
    np.testing.assert_array_equal(last[k], again[k], err_msg=k)


@pytest.mark.parametrize('goal,extra,fdt', [(False, dict(), 'float32'),
                                            (True, dict(proc_obs='sequence', proc_tgt='constant'), 'uint8')])
def test_no_leakage_between_envs(dev, tmp_path, goal, extra, fdt):
  """The same B = 3 incremental predictor run twice: env 0's stream, goal and resets are the same both times, the other envs get
  different frames and goals and are reset at other calls.  Env 0's outputs are bitwise identical."""
  K, B, T = 3, 3, 8
  kw = dict(window_size=K, img_height=S, img_width=S, **extra)
  _model_dir(str(tmp_path), goal, kw)
  p = _classes(goal)(str(tmp_path), num_envs=B, memcap=None, device=dev, frame_dtype=fdt, incremental=True)
  conv = (lambda x: x) if fdt == 'uint8' else (lambda x: x.astype(np.float32) / np.float32(255))

  def run(seed, other_resets):
    r, r0 = np.random.default_rng(seed), np.random.default_rng(99)
    res = []
    p.reset()
    if goal:
      g = r.integers(0, 256, (B, S, S, 3), dtype=np.uint8)
      g[0] = r0.integers(0, 256, (S, S, 3), dtype=np.uint8)
      p.set_goal(conv(g))
    for t in range(T):
      f = r.integers(0, 256, (B, S, S, 3), dtype=np.uint8)
      f[0] = r0.integers(0, 256, (S, S, 3), dtype=np.uint8)
      j = r.standard_normal((B, 7)).astype(np.float32)
      j[0] = r0.standard_normal(7).astype(np.float32)
      if t == 5:
        p.reset([0])
      if t in other_resets:
        p.reset(other_resets[t])
      res.append(p.predict(conv(f), j))
    return res
  a, b = run(1, {3: [2]}), run(2, {2: [1], 6: [1, 2]})
  for t in range(T):
    for k in a[t]:
      np.testing.assert_array_equal(a[t][k][0], b[t][k][0], err_msg='%s call %d' % (k, t))
    assert not np.array_equal(a[t]['cmd_ee'][1:], b[t]['cmd_ee'][1:])


@pytest.mark.parametrize('goal,extra', [(False, dict()), (True, dict(proc_obs='sequence', proc_tgt='residual'))])
def test_uint8_equals_float(dev, tmp_path, goal, extra):
  """RGB: uint8 frames and goals give bitwise the outputs of the same frames as float32 u8 / 255."""
  K, B, T = 3, 3, 6
  kw = dict(window_size=K, img_height=S, img_width=S, **extra)
  _model_dir(str(tmp_path), goal, kw)
  pu = _classes(goal)(str(tmp_path), num_envs=B, memcap=None, device=dev, frame_dtype='uint8', incremental=True)
  pf = _classes(goal)(str(tmp_path), num_envs=B, memcap=None, device=dev, incremental=True)
  assert pu.window_form == pf.window_form == 'features'
  r = np.random.default_rng(5)
  if goal:
    g = r.integers(0, 256, (B, S, S, 3), dtype=np.uint8)
    pu.set_goal(g)
    pf.set_goal(g.astype(np.float32) / np.float32(255))
  for t in range(T):
    if t == 4:
      pu.reset([1])
      pf.reset([1])
    f = r.integers(0, 256, (B, S, S, 3), dtype=np.uint8)
    j = r.standard_normal((B, 7)).astype(np.float32)
    ou, of = pu.predict(f, j), pf.predict(f.astype(np.float32) / np.float32(255), j)
    assert set(ou) == set(of)
    for k in ou:
      np.testing.assert_array_equal(ou[k], of[k], err_msg='%s call %d' % (k, t))


@pytest.mark.parametrize('goal,extra', [(False, dict()), (False, dict(control_mode='velocity', img_channels=4)),
                                        (True, dict(proc_obs='sequence', proc_tgt='constant'))])
def test_batch1_classes_incremental(dev, tmp_path, goal, extra):
  """E2EVMCPredictor / GoalE2EVMCPredictor with incremental=True against incremental=False: the same un-batched dict, a reset()
  mid-sequence pads the window again, the host-side frame assertions are the class's own."""
  from geeco_amd.predictor import E2EVMCPredictor, GoalE2EVMCPredictor
  K, T = 3, 8
  kw = dict(window_size=K, img_height=S, img_width=S, **extra)
  cfg, _ = _model_dir(str(tmp_path), goal, kw)
  C = cfg.img_channels
  cls = GoalE2EVMCPredictor if goal else E2EVMCPredictor
  pi = cls(str(tmp_path), memcap=None, device=dev, incremental=True)
  pw = cls(str(tmp_path), memcap=None, device=dev)
  assert pi.cfg == pw.cfg and pi.cfg.batch_size == 1
  r = np.random.default_rng(31)
  frames, jnts = _streams(r, 1, T, S, S, C)
  if goal:
    with pytest.raises(RuntimeError, match='set_goal'):
      pi.predict(frames[0, 0], jnts[0, 0])
    g = r.random((S, S, C + 1), dtype=np.float32)            # extra channels are cut off
    pi.set_goal(g)
    pw.set_goal(g)
  for t in range(T):
    if t == 5:
      pi.reset()
      pw.reset()
    oi, ow = pi.predict(frames[t, 0], jnts[t, 0]), pw.predict(frames[t, 0], jnts[t, 0])
    assert set(oi) == set(ow)
    for k in oi:
      assert oi[k].shape == ow[k].shape and oi[k].dtype == ow[k].dtype, k
      if k == 'cmd_grp' and cfg.control_mode == 'cartesian':
        lg = np.sort(pw._model.predictions()['logits_cmd_grp'][0].cpu().numpy())
        if lg[-1] - lg[-2] > ATOL + RTOL * abs(lg[-1]):
          assert oi[k][0] == ow[k][0], t
        continue
      np.testing.assert_allclose(oi[k], ow[k], rtol=RTOL, atol=ATOL, err_msg='%s call %d' % (k, t))
  bad = frames[0, 0].copy()
  bad[3, 3, 0] = 1.5
  with pytest.raises(AssertionError, match='Fed frame exceeds range'):
    pi.predict(bad, jnts[0, 0])
  with pytest.raises(AssertionError, match='wrong dimensions'):
    pi.predict(frames[0, 0][:100], jnts[0, 0])


def test_structure_and_errors(dev, tmp_path):
  from geeco_amd import graph
  from geeco_amd.batched_predictor import BatchedE2EVMCPredictor, BatchedGoalE2EVMCPredictor
  from geeco_amd.predictor import GoalE2EVMCPredictor
  B, K = 3, 3
  base = dict(window_size=K, img_height=S, img_width=S)
  # the two excluded model kinds say why
  _model_dir(str(tmp_path / 'f'), True, dict(proc_obs='dynimg', proc_tgt='dyndiff', **base))
  with pytest.raises(ValueError, match='dynimg'):
    BatchedGoalE2EVMCPredictor(str(tmp_path / 'f'), num_envs=B, memcap=None, device=dev, incremental=True)
  with pytest.raises(ValueError, match='dynimg'):
    GoalE2EVMCPredictor(str(tmp_path / 'f'), memcap=None, device=dev, incremental=True)
  _model_dir(str(tmp_path / 'd'), True, dict(proc_obs='sequence', proc_tgt='dyndiff', **base))
  with pytest.raises(ValueError, match='dyndiff'):
    BatchedGoalE2EVMCPredictor(str(tmp_path / 'd'), num_envs=B, memcap=None, device=dev, incremental=True)
  # the step model: the encoder sees B frames, the decoder K steps; the variable layout is the full model's
  cfg, _ = _model_dir(str(tmp_path / 'c'), True, dict(proc_obs='sequence', proc_tgt='constant', **base))
  p = BatchedGoalE2EVMCPredictor(str(tmp_path / 'c'), num_envs=B, memcap=None, device=dev, incremental=True)
  m = p._model
  assert isinstance(m, graph.GoalE2EVMCStep) and m.enc.Nf == B and m.decoder.T == K and m.decoder.N == B
  assert tuple(m.enc.x_in.shape) == (1, B, S, S, 4) and tuple(m.feat_ring.shape) == (B, K, 4, cfg.dim_s_obs)
  full = graph.GoalE2EVMC(cfg, B, dev, training=False)
  assert full.enc.Nf == (K + 1) * B
  assert m.store.offsets == full.store.offsets and m.store.size == full.store.size
  with pytest.raises(ValueError, match='inference-only'):
    graph.GoalE2EVMCStep(cfg, B, dev, training=True)
  with pytest.raises(ValueError, match='inference-only'):
    graph.E2EVMCStep(cfg, B, dev, training=True)
  # goals first; the message is the windowed predictor's
  f, j = np.zeros((B, S, S, 3), np.float32), np.zeros((B, 7), np.float32)
  with pytest.raises(RuntimeError, match=r'set_goal\(tgt_frame\) must be called before predict\(\): envs \[0, 1, 2\]'):
    p.predict(f, j)
  p.set_goal(np.zeros((S, S, 3), np.float32), env_ids=[0, 2])
  with pytest.raises(RuntimeError, match=r'envs \[1\]'):
    p.predict(f, j)
  p.set_goal(np.zeros((S, S, 3), np.float32), env_ids=[1])
  p.predict(f, j)
  for bad_call in (lambda: p.predict(f[:2], j[:2]), lambda: p.predict(f[:, :100], j), lambda: p.predict(f.astype(np.uint8), j),
                   lambda: p.set_goal(np.zeros((S, S, 2), np.float32))):
    with pytest.raises(ValueError):
      bad_call()
  assert p.frame_buffer().shape == (B, S, S, 3)
  _model_dir(str(tmp_path / 'r'), False, dict(img_channels=4, **base))
  with pytest.raises(ValueError, match='uint8'):
    BatchedE2EVMCPredictor(str(tmp_path / 'r'), num_envs=2, memcap=None, device=dev, frame_dtype='uint8', incremental=True)


def test_range_errors_leave_every_ring_alone(dev, tmp_path):
  """One env's frame at 1.1, another's NaN: the windowed predictor's AssertionError; no ring, no head moved, the pending reset is
  still pending: the next valid call gives exactly what a twin that never saw the bad call gives."""
  from geeco_amd.batched_predictor import BatchedE2EVMCPredictor
  _model_dir(str(tmp_path), False, dict(window_size=3, img_height=S, img_width=S))
  B = 3
  r = np.random.default_rng(3)
  frames, jnts = _streams(r, B, 3, S, S, 3)
  bad = frames[1].copy()
  bad[0, 10, 10, 1] = 1.1
  bad[2, 0, 5, 0] = np.nan
  pa = BatchedE2EVMCPredictor(str(tmp_path), num_envs=B, memcap=None, device=dev, incremental=True)
  pb = BatchedE2EVMCPredictor(str(tmp_path), num_envs=B, memcap=None, device=dev, incremental=True)
  pw = BatchedE2EVMCPredictor(str(tmp_path), num_envs=B, memcap=None, device=dev)
  for p in (pa, pb, pw):
    p.predict(frames[0], jnts[0])
    p.reset([1])
  m = pa._model
  before = [x.clone() for x in (m.feat_ring, m.jnt_ring, m.heads)]
  with pytest.raises(AssertionError) as ei:
    pa.predict(bad, jnts[1])
  with pytest.raises(AssertionError) as ew:
    pw.predict(bad, jnts[1])
  assert str(ei.value) == str(ew.value)
  msg = str(ei.value)
  assert 'env 0' in msg and 'env 2' in msg and 'env 1' not in msg and 'Fed frame exceeds range! Expected' in msg
  for was, now in zip(before, (m.feat_ring, m.jnt_ring, m.heads)):
    assert torch.equal(was, now)
  oa, ob = pa.predict(frames[2], jnts[2]), pb.predict(frames[2], jnts[2])
  for k in oa:
    np.testing.assert_array_equal(oa[k], ob[k], err_msg=k)
