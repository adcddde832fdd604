"""Batched predictor on the GPU: the push kernels against the window specification (bitwise), the batched predictors against B
batch-1 predictors and the oracle, isolation between envs, uint8 == float, range errors and API errors."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import geeco_oracle as O
from test_batched_predictor_cpu import WindowModel

pytestmark = pytest.mark.gpu

HW136 = (136, 136)


def _model_dir(path, goal, kw, seed=4):
  from geeco_amd import estimator as est
  from geeco_amd.graph import model_variable_shapes
  from geeco_amd.params import create_e2evmc_config
  from geeco_amd.variables import VariableStore
  cfg = create_e2evmc_config(kw)
  os.makedirs(path, exist_ok=True)
  json.dump(cfg._asdict(), open(os.path.join(path, 'e2evmc_config.json'), 'w'))
  st = VariableStore(model_variable_shapes(cfg, goal), 'cpu')
  st.initialize(seed=seed)
  est.save_checkpoint(st, str(path), keep_max=1)
  return cfg, st.to_numpy('params')


@pytest.mark.parametrize('B', [1, 3, 7, 32])
@pytest.mark.parametrize('K', [1, 2, 16])
def test_push_kernels_match_window_model(dev, B, K):
  """20 calls with random resets: dense windows (float32 RGB / RGB-D, uint8 RGB) and the mirrored uint8 ring read through its
  address table equal WindowModel bitwise; the joint-state window too."""
  from geeco_amd import ops
  r = np.random.default_rng(B * 100 + K)
  J = 7
  # 8x12: 16-byte ring units (HW * 3 % 16 == 0); 6x10: the 4-byte ring fallback; 5x5: the one-pixel dense path
  for C, u8, shape in ((3, False, (8, 12)), (4, False, (8, 12)), (3, True, (8, 12)), (3, True, (6, 10)), (3, False, (5, 5)),
                       (4, False, (5, 5))):
    H, W = shape
    HW = H * W
    rgb = torch.zeros(B, K, H, W, 3, device=dev)
    depth = torch.zeros(B, K, H, W, 1, device=dev) if C == 4 else None
    jw = torch.zeros(B, K, J, device=dev)
    ctl = torch.zeros(B + 1, dtype=torch.int32, device=dev)
    wm_rgb = WindowModel(B, K, (H, W, 3))
    wm_dep = WindowModel(B, K, (H, W, 1))
    wm_j = WindowModel(B, K, (J,))
    ring_on = u8
    if ring_on:
      ring = torch.zeros(B, 2 * K, HW * 3, dtype=torch.uint8, device=dev)
      heads = torch.zeros(B, dtype=torch.int32, device=dev)
      table = torch.zeros(B, dtype=torch.int64, device=dev)
      wm_ring = WindowModel(B, K, (HW * 3,), np.uint8)
      jr = torch.zeros(B, K, J, device=dev)
    for call in range(20):
      reset = (r.random(B) < 0.25) | (call == 0)
      if u8:
        f = r.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
        fval = f.astype(np.float32) / np.float32(255.0)
      else:
        f = r.random((B, H, W, C), dtype=np.float32)
        fval = f
      j = r.standard_normal((B, J)).astype(np.float32)
      fd, jd = torch.from_numpy(f).to(dev), torch.from_numpy(j).to(dev)
      rd = torch.from_numpy(reset.astype(np.int32)).to(dev)
      ops.predict_push_dense_into(rgb, depth, jw, fd, jd, rd, ctl, B, K, HW, C, J)
      wm_rgb.push(fval[..., :3], reset)
      if C == 4:
        wm_dep.push(fval[..., 3:4], reset)
      wm_j.push(j, reset)
      if ring_on:
        ops.predict_push_ring_into(ring, heads, table, jr, fd, jd, rd, ctl, B, K, HW, J)
        wm_ring.push(f.reshape(B, -1), reset)
      torch.cuda.synchronize()
      np.testing.assert_array_equal(rgb.cpu().numpy(), wm_rgb.dense, err_msg='rgb C=%d u8=%d call %d' % (C, u8, call))
      if C == 4:
        np.testing.assert_array_equal(depth.cpu().numpy(), wm_dep.dense)
      np.testing.assert_array_equal(jw.cpu().numpy(), wm_j.dense)
      if ring_on:
        base, stride = ring.data_ptr(), 2 * K * HW * 3
        tb = table.cpu().numpy()
        rb = ring.cpu().numpy()
        np.testing.assert_array_equal(heads.cpu().numpy(), wm_ring.heads)
        np.testing.assert_array_equal(jr.cpu().numpy(), wm_j.dense)
        for b in range(B):
          off = int(tb[b]) - base - b * stride
          assert off % (HW * 3) == 0
          s = off // (HW * 3)
          assert s == wm_ring.start[b]
          np.testing.assert_array_equal(rb[b, s:s + K], wm_ring.ring_window(b))
          np.testing.assert_array_equal(rb[b, s:s + K].reshape(K, H, W, 3).astype(np.float32) / np.float32(255.0),
                                        wm_rgb.dense[b])
    assert int(ctl.abs().sum()) == 0


def test_range_check_kernel_flags_and_blocks_the_push(dev):
  from geeco_amd import ops
  from geeco_amd.batched_predictor import range_bounds
  lo, hi = range_bounds()
  B, H, W, K, J = 4, 8, 12, 3, 7
  for C in (3, 4):
    f = np.random.default_rng(1).random((B, H, W, C), dtype=np.float32)
    f[1, 3, 4, 2] = 1.1
    f[3, 0, 0, 0] = np.nan
    if C == 4:
      f[2, 5, 5, 3] = 7.0                        # depth is not range-checked
    ctl = torch.zeros(B + 1, dtype=torch.int32, device=dev)
    fd = torch.from_numpy(f).to(dev)
    ops.predict_range_check_into(ctl, fd, B, H * W, C, lo, hi)
    assert ctl.cpu().tolist() == [0, 1, 0, 1, 1]
    rgb = torch.full((B, K, H, W, 3), 5.0, device=dev)
    depth = torch.full((B, K, H, W, 1), 5.0, device=dev) if C == 4 else None
    jw = torch.full((B, K, J), 5.0, device=dev)
    ops.predict_push_dense_into(rgb, depth, jw, fd, torch.zeros(B, J, device=dev), torch.ones(B, dtype=torch.int32, device=dev),
                                ctl, B, K, H * W, C, J)
    torch.cuda.synchronize()
    assert bool((rgb == 5.0).all()) and bool((jw == 5.0).all())


def _streams(r, B, T, H, W, C, J=7):
  frames = r.random((T, B, H, W, C), dtype=np.float32)
  jnts = r.standard_normal((T, B, J)).astype(np.float32)
  return frames, jnts


CONFIGS = [
    (True, dict(proc_obs='dynimg', proc_tgt='dyndiff')),
    (True, dict(proc_obs='sequence', proc_tgt='constant', control_mode='velocity')),
    (True, dict(proc_obs='sequence', proc_tgt='dyndiff', img_channels=4)),
    (True, dict(proc_obs='dynimg', proc_tgt='constant', control_mode='velocity', img_channels=4)),
    (False, dict()),
    (False, dict(control_mode='velocity', img_channels=4)),
]


@pytest.mark.parametrize('goal,extra', CONFIGS)
def test_batched_matches_batch1_predictors(dev, tmp_path, goal, extra):
  """B = 5 envs, each with its own frame stream, goal and resets at different calls: every env's outputs match a batch-1
  predictor fed that env's stream."""
  from geeco_amd.batched_predictor import BatchedE2EVMCPredictor, BatchedGoalE2EVMCPredictor
  from geeco_amd.predictor import E2EVMCPredictor, GoalE2EVMCPredictor
  kw = dict(window_size=3, img_height=136, img_width=136, **extra)
  cfg, _ = _model_dir(str(tmp_path), goal, kw)
  B, T, C = 5, 6, cfg.img_channels
  r = np.random.default_rng(7)
  frames, jnts = _streams(r, B, T, 136, 136, C)
  resets = {2: [1], 3: [0, 4], 4: [2]}                       # call -> envs reset before it
  tgts = r.random((B, 136, 136, C + 1), dtype=np.float32)
  bp = (BatchedGoalE2EVMCPredictor if goal else BatchedE2EVMCPredictor)(str(tmp_path), num_envs=B, memcap=None, device=dev,
                                                                         debug_images=True)
  assert bp.cfg.batch_size == B and bp.num_envs == B
  if goal:
    bp.set_goal(tgts)
  outs = []
  for t in range(T):
    if t in resets:
      bp.reset(resets[t])
    outs.append(bp.predict(frames[t], jnts[t]))
  dynimg = goal and cfg.proc_obs == 'dynimg'
  p1 = (GoalE2EVMCPredictor if goal else E2EVMCPredictor)(str(tmp_path), memcap=None, device=dev)
  for e in range(B):
    p1.reset()
    if goal:
      p1.set_goal(tgts[e])
    since_reset = 0
    for t in range(T):
      if e in resets.get(t, []):
        p1.reset()
        since_reset = 0
      o1 = p1.predict(frames[t, e], jnts[t, e])
      ob = {k: v[e] for k, v in outs[t].items()}
      assert set(o1) == set(ob), (sorted(o1), sorted(ob))
      fresh = since_reset == 0
      since_reset += 1
      for k in o1:
        assert ob[k].shape == o1[k].shape, k
        if dynimg and fresh:               # padded window: ill-conditioned dynamic image (test_predictor_gpu.py)
          assert np.isfinite(ob[k]).all(), k
          continue
        if k == 'cmd_grp' and cfg.control_mode == 'cartesian':
          lg = np.sort(p1._model.predictions()['logits_cmd_grp'][0].cpu().numpy())
          if lg[-1] - lg[-2] > 1e-3:
            assert ob[k][0] == o1[k][0], (e, t)
          continue
        np.testing.assert_allclose(ob[k], o1[k], rtol=1e-4, atol=2e-5, err_msg='%s env %d call %d' % (k, e, t))


@pytest.mark.parametrize('goal', [True, False])
def test_batched_matches_oracle(dev, tmp_path, goal):
  from geeco_amd.batched_predictor import BatchedE2EVMCPredictor, BatchedGoalE2EVMCPredictor
  kw = dict(window_size=3, img_height=136, img_width=136)
  if goal:
    kw.update(proc_obs='dynimg', proc_tgt='dyndiff')
  cfg, P = _model_dir(str(tmp_path), goal, kw)
  B, T = 3, 3
  r = np.random.default_rng(2)
  frames, jnts = _streams(r, B, T, 136, 136, 3)
  tgt = r.random((B, 136, 136, 3), dtype=np.float32)
  bp = (BatchedGoalE2EVMCPredictor if goal else BatchedE2EVMCPredictor)(str(tmp_path), num_envs=B, memcap=None, device=dev)
  if goal:
    bp.set_goal(tgt)
  ocfg = O.make_config(batch_size=B, **kw)
  Pt = {k: torch.tensor(v, dtype=torch.float64) for k, v in P.items()}
  for t in range(T):
    out = bp.predict(frames[t], jnts[t])
    idx = [max(0, t - 2 + i) for i in range(3)]                # window with first-frame padding
    feats = {'rgb': torch.tensor(frames[idx].transpose(1, 0, 2, 3, 4), dtype=torch.float64),
             'jnt_state': torch.tensor(jnts[idx].transpose(1, 0, 2), dtype=torch.float64)}
    if goal:
      feats['target_rgb'] = torch.tensor(tgt, dtype=torch.float64)
    ref, _ = O.model_forward(feats, Pt, ocfg, goal)
    noise = goal and t == 0
    for k in ('cmd_ee', 'pos_ee', 'pos_obj'):
      np.testing.assert_allclose(out[k], ref[k].numpy(), rtol=1e-4, atol=5e-2 if noise else 2e-5, err_msg='%s @%d' % (k, t))
    assert out['cmd_grp'].shape == (B, 1)
    if not noise:
      np.testing.assert_array_equal(out['cmd_grp'][:, 0], ref['logits_cmd_grp'].argmax(-1).numpy() - 1.0)


@pytest.mark.parametrize('goal,extra,fdt', [(True, dict(proc_obs='dynimg', proc_tgt='dyndiff'), 'uint8'), (False, dict(), 'float32')])
def test_no_leakage_between_envs(dev, tmp_path, goal, extra, fdt):
  """The same B = 4 predictor run twice: env 0's stream is the same both times, envs 1..3 differ.  Env 0's outputs are bitwise
  identical (ring / table / shift mistakes would mix envs)."""
  from geeco_amd.batched_predictor import BatchedE2EVMCPredictor, BatchedGoalE2EVMCPredictor
  kw = dict(window_size=3, img_height=136, img_width=136, **extra)
  _model_dir(str(tmp_path), goal, kw)
  B, T = 4, 5
  cls = BatchedGoalE2EVMCPredictor if goal else BatchedE2EVMCPredictor
  p = cls(str(tmp_path), num_envs=B, memcap=None, device=dev, frame_dtype=fdt, debug_images=True)

  def run(seed):
    r = np.random.default_rng(seed)
    r0 = np.random.default_rng(99)
    res = []
    p.reset()
    if goal:
      g = r.integers(0, 256, (B, 136, 136, 3), dtype=np.uint8)
      g[0] = r0.integers(0, 256, (136, 136, 3), dtype=np.uint8)
      p.set_goal(g if fdt == 'uint8' else g.astype(np.float32) / np.float32(255))
    for t in range(T):
      f = r.integers(0, 256, (B, 136, 136, 3), dtype=np.uint8)
      f[0] = r0.integers(0, 256, (136, 136, 3), dtype=np.uint8)
      j = r.standard_normal((B, 7)).astype(np.float32)
      j[0] = r0.standard_normal(7).astype(np.float32)
      if t == 3:
        p.reset([2])
      res.append(p.predict(f if fdt == 'uint8' else f.astype(np.float32) / np.float32(255), j))
    return res
  a, b = run(1), run(2)
  for t in range(T):
    for k in a[t]:
      np.testing.assert_array_equal(a[t][k][0], b[t][k][0], err_msg='%s call %d' % (k, t))
    assert not np.array_equal(a[t]['cmd_ee'][1:], b[t]['cmd_ee'][1:])


def test_uint8_equals_float(dev, tmp_path):
  """geeco-f RGB (the ring path): uint8 frames, and the same frames as u8 / 255.0 float32 through the dense path, give bitwise
  equal outputs, debug images included."""
  from geeco_amd.batched_predictor import BatchedGoalE2EVMCPredictor
  kw = dict(window_size=3, img_height=136, img_width=136, proc_obs='dynimg', proc_tgt='dyndiff')
  _model_dir(str(tmp_path), True, kw)
  B, T = 3, 5
  pu = BatchedGoalE2EVMCPredictor(str(tmp_path), num_envs=B, memcap=None, device=dev, frame_dtype='uint8', debug_images=True)
  pf = BatchedGoalE2EVMCPredictor(str(tmp_path), num_envs=B, memcap=None, device=dev, debug_images=True)
  assert pu.window_form == 'ring' and pf.window_form == 'dense'
  r = np.random.default_rng(5)
  g = r.integers(0, 256, (B, 136, 136, 3), dtype=np.uint8)
  pu.set_goal(g)
  pf.set_goal(g / 255.0)
  for t in range(T):
    if t == 3:
      pu.reset([1])
      pf.reset([1])
    f = r.integers(0, 256, (B, 136, 136, 3), dtype=np.uint8)
    j = r.standard_normal((B, 7)).astype(np.float32)
    ou, of = pu.predict(f, j), pf.predict((f / 255.0).astype(np.float32), j)
    assert set(ou) == set(of) == {'cmd_ee', 'cmd_grp', 'pos_ee', 'pos_obj', 'dynbuff', 'dyndiff'}
    for k in ou:
      np.testing.assert_array_equal(ou[k], of[k], err_msg='%s call %d' % (k, t))


def test_range_errors_leave_every_window_alone(dev, tmp_path):
  """One env's frame at 1.1, another's NaN: AssertionError naming both with their ranges; the next valid call gives exactly what
  it would have given without the bad call (no window moved, the pending reset still pending)."""
  from geeco_amd.batched_predictor import BatchedE2EVMCPredictor
  kw = dict(window_size=3, img_height=136, img_width=136)
  _model_dir(str(tmp_path), False, kw)
  B = 3
  r = np.random.default_rng(3)
  frames, jnts = _streams(r, B, 3, 136, 136, 3)
  bad = frames[1].copy()
  bad[0, 10, 10, 1] = 1.1
  bad[2, 0, 5, 0] = np.nan
  pa = BatchedE2EVMCPredictor(str(tmp_path), num_envs=B, memcap=None, device=dev)
  pb = BatchedE2EVMCPredictor(str(tmp_path), num_envs=B, memcap=None, device=dev)
  for p in (pa, pb):
    p.predict(frames[0], jnts[0])
    p.reset([1])
  with pytest.raises(AssertionError) as ei:
    pa.predict(bad, jnts[1])
  msg = str(ei.value)
  assert 'env 0' in msg and 'env 2' in msg and 'env 1' not in msg
  assert 'Fed frame exceeds range! Expected' in msg and '1.1' in msg and 'nan' in msg
  oa, ob = pa.predict(frames[2], jnts[2]), pb.predict(frames[2], jnts[2])
  for k in oa:
    np.testing.assert_array_equal(oa[k], ob[k], err_msg=k)


def test_api_errors(dev, tmp_path):
  from geeco_amd.batched_predictor import BatchedE2EVMCPredictor, BatchedGoalE2EVMCPredictor
  kw = dict(window_size=2, img_height=136, img_width=136, proc_obs='dynimg', proc_tgt='dyndiff')
  _model_dir(str(tmp_path / 'g'), True, kw)
  B = 3
  p = BatchedGoalE2EVMCPredictor(str(tmp_path / 'g'), num_envs=B, memcap=None, device=dev)
  f = np.zeros((B, 136, 136, 3), np.float32)
  j = np.zeros((B, 7), np.float32)
  with pytest.raises(RuntimeError, match=r'envs \[0, 1, 2\]'):
    p.predict(f, j)
  p.set_goal(np.zeros((136, 136, 3), np.float32), env_ids=[0, 2])
  with pytest.raises(RuntimeError, match=r'envs \[1\]'):
    p.predict(f, j)
  p.set_goal(np.zeros((136, 136, 3), np.float32), env_ids=[1])
  p.predict(f, j)
  with pytest.raises(ValueError):
    p.predict(f[:2], j[:2])                                    # wrong B
  with pytest.raises(ValueError):
    p.predict(f[:, :100], j)                                   # wrong frame shape
  with pytest.raises(ValueError):
    p.predict(f.astype(np.uint8), j)                           # wrong dtype for the mode
  _model_dir(str(tmp_path / 'd'), False, dict(window_size=1, img_height=136, img_width=136, img_channels=4))
  with pytest.raises(ValueError, match='uint8'):
    BatchedE2EVMCPredictor(str(tmp_path / 'd'), num_envs=2, memcap=None, device=dev, frame_dtype='uint8')
