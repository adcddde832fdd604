"""Episode replay on the GPU: the window builder against its host model (bitwise), the error reduction against float64,
the whole path against the oracle on explicitly built windows and against the batch-1 incremental predictor stepped through the same
frames, chunking, the episode lengths at the edges, ``Estimator.replay`` and scripts/replay_episodes.py on a synthetic dataset."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import _replay_ref as R
from oracle import geeco_oracle as O
from test_batched_predictor_gpu import _model_dir

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = 1e-4, 2e-5      # tests/test_predictor_gpu.py: predictions against the oracle
S = 136
U = 2.0 ** -24               # unit roundoff of float32


# ---- geeco_replay_states ----------------------------------------------------------------------------------------------------
# (ch, J, pad): 16-byte loads and stores (ch, J, stride all multiples of 4) / 16-byte loads, one-float stores (J = 7, odd stride) /
# one float everywhere (ch % 4 != 0)
LAYOUTS = [(8, 8, 4), (8, 7, 5), (6, 7, 3)]


@pytest.mark.parametrize('mode', ['plain', 'constant', 'residual'])
@pytest.mark.parametrize('K', [1, 4, 64])
@pytest.mark.parametrize('ch,J,pad', LAYOUTS)
def test_replay_states_matches_host_model_bitwise(dev, mode, K, ch, J, pad):
  """T = 1, K - 1, K, K + 1 and 37 (T * K = 2368 > 1024 at K = 64); the whole episode, and a range that starts mid-episode and ends
  ragged; the row pitch wider than the row and more rows per step than windows: everything outside the written cells keeps -7."""
  from geeco_amd import ops
  cells = 4
  D = R.state_width(mode, cells, ch, J)
  r = np.random.default_rng(1000 * K + 10 * ch + J)
  for T in sorted({1, max(K - 1, 1), K, K + 1, 37}):
    feat = r.standard_normal((T, cells, ch)).astype(np.float32)
    jnt = r.standard_normal((T, J)).astype(np.float32)
    tgt = r.standard_normal((cells, ch)).astype(np.float32)
    fd, jd = torch.from_numpy(feat).to(dev), torch.from_numpy(jnt).to(dev)
    td = torch.from_numpy(tgt).to(dev) if mode != 'plain' else None
    ranges = [(0, T)] + ([(T // 3, T - 1)] if T - 1 > T // 3 else [])
    for t0, t1 in ranges:
      n = t1 - t0
      states = torch.full((K, n + 2, D + pad), -7.0, device=dev)
      ops.replay_states_into(states, fd, jd, mode, T, t0, t1, K, cells, ch, J, tgt_feat=td)
      got = states.cpu().numpy()
      np.testing.assert_array_equal(got[:, :n, :D], R.states_ref(feat, jnt, tgt, mode, K, t0, t1), err_msg='T=%d [%d, %d)' % (T, t0, t1))
      assert (got[:, n:] == -7.0).all() and (got[:, :, D:] == -7.0).all()


def _view_4_bytes_in(a, dev):
  """``a`` on the device as a contiguous view that starts 4 bytes into its allocation (allocations are at least 16-byte aligned)."""
  buf = torch.zeros(a.size + 1, device=dev)
  buf[1:].copy_(torch.from_numpy(a).reshape(-1))
  view = buf[1:].view(a.shape)
  assert view.data_ptr() % 16 == 4 and view.is_contiguous()
  return view


@pytest.mark.parametrize('mode', ['plain', 'constant', 'residual'])
def test_replay_states_from_a_table_that_is_not_16_byte_aligned(dev, mode):
  """ch % 4 == 0, but the feature table starts 4 bytes past a 16-byte boundary: the call takes the one-float form and equals the host
  model bit for bit; the guard cells keep -7."""
  from geeco_amd import ops
  T, K, cells, ch, J, pad = 5, 4, 4, 8, 8, 4
  D = R.state_width(mode, cells, ch, J)
  r = np.random.default_rng(77)
  feat = r.standard_normal((T, cells, ch)).astype(np.float32)
  jnt = r.standard_normal((T, J)).astype(np.float32)
  tgt = r.standard_normal((cells, ch)).astype(np.float32)
  td = torch.from_numpy(tgt).to(dev) if mode != 'plain' else None
  states = torch.full((K, T + 2, D + pad), -7.0, device=dev)
  ops.replay_states_into(states, _view_4_bytes_in(feat, dev), torch.from_numpy(jnt).to(dev), mode, T, 0, T, K, cells, ch, J, tgt_feat=td)
  got = states.cpu().numpy()
  np.testing.assert_array_equal(got[:, :T, :D], R.states_ref(feat, jnt, tgt, mode, K, 0, T))
  assert (got[:, T:] == -7.0).all() and (got[:, :, D:] == -7.0).all()


def test_replay_states_columns_are_push_features_columns(dev):
  """Window t of the replay equals, bit for bit, what geeco_predict_push_features gathers after a reset at frame 0 and t pushes."""
  from geeco_amd import ops
  T, K, cells, ch, J = 7, 3, 4, 64, 7
  r = np.random.default_rng(9)
  feat = torch.from_numpy(r.standard_normal((T, cells, ch)).astype(np.float32)).to(dev)
  jnt = torch.from_numpy(r.standard_normal((T, J)).astype(np.float32)).to(dev)
  tgt = torch.from_numpy(r.standard_normal((1, cells, ch)).astype(np.float32)).to(dev)
  ctl = torch.zeros(2, dtype=torch.int32, device=dev)
  for mode in ('plain', 'constant', 'residual'):
    D = R.state_width(mode, cells, ch, J)
    got = torch.zeros(K, T, D, device=dev)
    ops.replay_states_into(got, feat, jnt, mode, T, 0, T, K, cells, ch, J, tgt_feat=None if mode == 'plain' else tgt[0])
    ring, jring = torch.zeros(1, K, cells, ch, device=dev), torch.zeros(1, K, J, device=dev)
    heads, want = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(K, 1, D, device=dev)
    for t in range(T):
      reset = torch.full((1,), int(t == 0), dtype=torch.int32, device=dev)
      ops.predict_push_features_into(want, ring, jring, heads, feat[t:t + 1], jnt[t:t + 1], reset, ctl, mode, 1, K, cells, ch, J, D,
                                     tgt_feat=None if mode == 'plain' else tgt)
      assert torch.equal(got[:, t], want[:, 0]), (mode, t)


# ---- geeco_replay_errors ----------------------------------------------------------------------------------------------------
def _error_case(control_mode, T, seed):
  from geeco_amd import replay as rp
  from geeco_amd.params import create_e2evmc_config
  cfg = create_e2evmc_config(dict(control_mode=control_mode))
  heads = rp.error_heads(cfg)
  P = sum(h[1] for h in heads)
  r = np.random.default_rng(seed)
  preds = r.standard_normal((T, P)).astype(np.float32)
  labels = r.standard_normal((T, P)).astype(np.float32)
  for off, size, kind in heads:
    if kind == 1:
      labels[:, off] = r.integers(0, size, T)
      labels[:, off + 1:off + size] = 0
      preds[0, off:off + size] = [0.25, 0.75, 0.75][:size]          # an exact tie: the first maximum (class 1) counts
      labels[0, off] = 1
      if T > 2:
        preds[2, off:off + size] = 0.5                               # all equal: class 0
        labels[2, off] = 0
        preds[T - 1, off:off + size] = [0.1, 0.3, 0.3][:size]        # tie, the recorded class is the SECOND maximum: a miss
        labels[T - 1, off] = 2
  return heads, preds, labels


@pytest.mark.parametrize('control_mode', ['cartesian', 'velocity'])
@pytest.mark.parametrize('T', [1, 257])
def test_replay_errors_against_float64(dev, control_mode, T):
  """Per frame: a head of n columns is n differences (each one rounding, so 2 u on its square), n products, n - 1 sums of
  non-negative terms and one division: within (n + 3) u of the exact value, asserted at (n + 4) u; class hits are exact.  Episode mean:
  exactly the documented order (a thread's frames ascending, 8 folds, one division), hence within (ceil(T / 256) + 8) u of the exact
  mean of the per-frame values.  Two runs are bitwise equal; a planted NaN gives NaN for that frame and head and for that head's
  episode mean, nothing else."""
  from geeco_amd import ops
  heads, preds, labels = _error_case(control_mode, T, 7 * T)
  pd, ld = torch.from_numpy(preds).to(dev), torch.from_numpy(labels).to(dev)
  runs = []
  for _ in range(2):
    of, oe = torch.full((T, len(heads)), -3.0, device=dev), torch.full((len(heads),), -3.0, device=dev)
    ops.replay_errors_into(of, oe, pd, ld, T, heads)
    runs.append((of.cpu().numpy(), oe.cpu().numpy()))
  np.testing.assert_array_equal(runs[0][0], runs[1][0])
  np.testing.assert_array_equal(runs[0][1], runs[1][1])
  frame, episode = runs[0]
  want_f, _ = R.errors_ref(preds, labels, heads)
  chain = math.ceil(T / 256) + 8
  for h, (off, size, kind) in enumerate(heads):
    if kind == 1:
      np.testing.assert_array_equal(frame[:, h], want_f[:, h])
      assert frame[0, h] == 1.0 and (T < 3 or (frame[2, h] == 1.0 and frame[T - 1, h] == 0.0))
    else:
      err = np.abs(frame[:, h] - want_f[:, h])
      print('head %d (%d columns): worst per-frame error %.3g u' % (h, size, (err / (U * want_f[:, h])).max()))
      assert (err <= (size + 4) * U * want_f[:, h]).all()
    assert episode[h] == R.episode_sum_order(frame[:, h])
    exact = frame[:, h].astype(np.float64).mean()
    assert abs(episode[h] - exact) <= chain * U * exact
  # a NaN prediction: that frame, that head
  bad_t, (off, size, _) = T // 2, heads[0]
  preds[bad_t, off + size - 1] = np.nan
  koff = next((o for o, _, k in heads if k == 1), None)
  if koff is not None and T > 1:
    preds[T - 1, koff + 1] = np.nan
  of, oe = torch.zeros(T, len(heads), device=dev), torch.zeros(len(heads), device=dev)
  ops.replay_errors_into(of, oe, torch.from_numpy(preds).to(dev), ld, T, heads)
  f2, e2 = of.cpu().numpy(), oe.cpu().numpy()
  want_nan = np.zeros_like(f2, dtype=bool)
  want_nan[bad_t, 0] = True
  if koff is not None and T > 1:
    want_nan[T - 1, [h for h, hd in enumerate(heads) if hd[2] == 1][0]] = True
  np.testing.assert_array_equal(np.isnan(f2), want_nan)
  np.testing.assert_array_equal(f2[~want_nan], frame[~want_nan])
  np.testing.assert_array_equal(np.isnan(e2), want_nan.any(axis=0))


# ---- the whole path -----------------------------------------------------------------------------------------------------------
MODELS = [(False, dict()), (True, dict(proc_obs='sequence', proc_tgt='constant')), (True, dict(proc_obs='sequence', proc_tgt='residual'))]
K_PATH = 3
T_PATH = 2 * K_PATH + 3


def _episode(cfg, T, u8, seed):
  r = np.random.default_rng(seed)
  rgb = r.integers(0, 256, (T, S, S, 3), dtype=np.uint8)
  goal = r.integers(0, 256, (S, S, 3), dtype=np.uint8)
  if not u8:
    rgb, goal = rgb.astype(np.float32) / np.float32(255), goal.astype(np.float32) / np.float32(255)
  ep = {'rgb': rgb, 'jnt_state': r.standard_normal((T, cfg.dim_jnt_state)).astype(np.float32),
        'cmd': np.concatenate([0.3 * r.standard_normal((T, 3)), r.integers(-1, 2, (T, 1))], 1).astype(np.float32),
        'ee_state': r.random((T, 7)).astype(np.float32), 'obj_state': r.random((T, 7)).astype(np.float32)}
  return ep, goal


def _as_float(a):
  return a.astype(np.float32) / np.float32(255) if a.dtype == np.uint8 else a


def replay_against_oracle_and_stepped(dev, path, goal, extra, u8):
  """One case of the whole path; returns the measured agreement with the stepped predictor (tests/golden/replay_achieved.json)."""
  from geeco_amd import replay as rp
  from geeco_amd.predictor import E2EVMCPredictor, GoalE2EVMCPredictor
  K, T = K_PATH, T_PATH
  kw = dict(window_size=K, img_height=S, img_width=S, **extra)
  cfg, P = _model_dir(path, goal, kw)
  ep, goal_frame = _episode(cfg, T, u8, 11 + 2 * len(extra) + u8)
  chunked = rp.EpisodeReplay(path, device=dev, max_frames=16, chunk_frames=4)
  assert chunked.goal == goal and chunked.chunk_frames == 4 and -(-(T + goal) // 4) == 3 and (T + goal) % 4      # three chunks, the last ragged
  assert chunked.enc.Nf == 4 and chunked.decoder.N == 16 and chunked.decoder.T == K
  out = chunked.replay(ep, goal_frame=goal_frame if goal else None)
  heads = chunked.heads
  assert set(out) == {k for k, _, _ in heads} | {'errors', 'episode_errors'}
  for k, _, size in heads:
    assert out[k].shape == (T, size) and out[k].dtype == np.float32
  assert out['errors'].shape == (T, len(heads)) and set(out['episode_errors']) == {k for k, _, _ in heads}
  # (a) the float64 oracle on the explicitly built windows
  idx = R.window_index(T, K)
  f = _as_float(ep['rgb'])
  feats = {'rgb': torch.tensor(f[idx], dtype=torch.float64), 'jnt_state': torch.tensor(ep['jnt_state'][idx], dtype=torch.float64)}
  if goal:
    feats['target_rgb'] = torch.tensor(np.broadcast_to(_as_float(goal_frame), (T, S, S, 3)).copy(), dtype=torch.float64)
  ref, _ = O.model_forward(feats, {k: torch.tensor(v, dtype=torch.float64) for k, v in P.items()}, O.make_config(batch_size=T, **kw), goal)
  for k, _, _ in heads:
    np.testing.assert_allclose(out[k], ref[k].numpy(), rtol=RTOL, atol=ATOL, err_msg='%s vs oracle' % k)
  # (b) the batch-1 incremental predictor stepped through the same frames after reset()
  pred = (GoalE2EVMCPredictor if goal else E2EVMCPredictor)(path, memcap=None, device=dev, incremental=True)
  if goal:
    pred.set_goal(_as_float(goal_frame))
  pred.reset()
  worst, largest, bitwise = 0.0, 0.0, True
  for t in range(T):
    o = pred.predict(f[t], ep['jnt_state'][t])
    step = {k: v[0].cpu().numpy() for k, v in pred._model.predictions().items()}
    assert set(step) == {k for k, _, _ in heads}
    for k in step:
      worst = max(worst, float(np.abs(out[k][t] - step[k]).max()))
      largest = max(largest, float(np.abs(step[k]).max()))
      bitwise = bitwise and np.array_equal(out[k][t], step[k])
      # measured bitwise in all six cases (tests/golden/replay_achieved.json): at these shapes the encoder's launches at 4 frames
      # and at 1 frame sum in the same order, so equality is asserted rather than the tolerance of (a)
      np.testing.assert_array_equal(out[k][t], step[k], err_msg='%s vs stepped, frame %d' % (k, t))
    np.testing.assert_array_equal(o['cmd_grp'], step['logits_cmd_grp'].argmax()[None] - 1.0)
  print('replay vs stepped: max |diff| %.3g (largest value %.3g, bitwise %s)' % (worst, largest, bitwise))
  # the chunked pass equals the pass in one chunk, bit for bit
  whole = rp.EpisodeReplay(path, device=dev, max_frames=16)
  assert whole.chunk_frames >= T + goal
  out1 = whole.replay(ep, goal_frame=goal_frame if goal else None)
  for k in out:
    if k != 'episode_errors':
      np.testing.assert_array_equal(out[k], out1[k], err_msg='%s chunked vs one chunk' % k)
  assert out['episode_errors'] == out1['episode_errors']
  # the errors are the reduction of these predictions against the recorded values
  lab = rp.recorded_labels(cfg, ep, T)
  preds = np.concatenate([out[k] for k, _, _ in heads], axis=1)
  want_f, _ = R.errors_ref(preds, lab, rp.error_heads(cfg))
  np.testing.assert_allclose(out['errors'], want_f, rtol=8 * U, atol=0)
  for h, (k, _, _) in enumerate(heads):
    assert np.float32(out['episode_errors'][k]) == R.episode_sum_order(out['errors'][:, h])
  # resident frames: a device tensor and the DeviceWindows of the episode give the dense array's result
  if u8:
    from geeco_amd.device_windows import DeviceWindows
    res = torch.from_numpy(ep['rgb'].reshape(T, -1)).to(dev)
    dw = DeviceWindows(K, (S, S, 3), 255.0)
    dw.add(res, np.arange(T - K + 1))
    for form in (res.view(T, S, S, 3), dw):
      out2 = chunked.replay(dict(ep, rgb=form), goal_frame=goal_frame if goal else None)
      for k, _, _ in heads:
        np.testing.assert_array_equal(out[k], out2[k], err_msg=k)
  return dict(goal=goal, proc_tgt=extra.get('proc_tgt'), frames='uint8' if u8 else 'float32', max_abs_diff=worst, max_abs_value=largest,
              bitwise=bitwise)


@pytest.mark.parametrize('u8', [True, False])
@pytest.mark.parametrize('goal,extra', MODELS)
def test_replay_whole_path(dev, tmp_path, goal, extra, u8):
  replay_against_oracle_and_stepped(dev, str(tmp_path), goal, extra, u8)


def test_replay_episode_lengths(dev, tmp_path):
  """T = 1 and T < K work and give the first rows of the longer episode bit for bit (a window looks back only); an episode longer
  than max_frames raises; labels=False computes no errors; a goal model asks for its goal."""
  from geeco_amd import replay as rp
  K = 4
  kw = dict(window_size=K, img_height=S, img_width=S, proc_obs='sequence', proc_tgt='residual')
  cfg, _ = _model_dir(str(tmp_path), True, kw)
  ep, goal = _episode(cfg, 10, True, 3)
  r = rp.EpisodeReplay(str(tmp_path), device=dev, max_frames=9, chunk_frames=3)
  full = r.replay({k: v[:9] for k, v in ep.items()}, goal_frame=goal)
  for T in (1, 2, K - 1, K):
    part = r.replay({k: v[:T] for k, v in ep.items()}, goal_frame=goal, labels=False)
    assert 'errors' not in part and 'episode_errors' not in part
    for k, _, size in r.heads:
      assert part[k].shape == (T, size)
      np.testing.assert_array_equal(part[k], full[k][:T], err_msg='%s T=%d' % (k, T))
  with pytest.raises(ValueError, match='holds 10 frames.*max_frames=9'):
    r.replay(ep, goal_frame=goal)
  with pytest.raises(ValueError, match='goal_frame'):
    r.replay({k: v[:3] for k, v in ep.items()})
  with pytest.raises(ValueError, match='jnt_state must be'):
    r.replay(dict(ep, rgb=ep['rgb'][:3]), goal_frame=goal)
  bad = ep['rgb'][:2].astype(np.float32)      # 0..255 as floats
  with pytest.raises(ValueError, match='exceed range'):
    r.replay({'rgb': bad, 'jnt_state': ep['jnt_state'][:2]}, goal_frame=goal, labels=False)
  _model_dir(str(tmp_path / 'f'), True, dict(kw, proc_obs='dynimg', proc_tgt='dyndiff'))
  with pytest.raises(ValueError, match='a dynamic image'):
    rp.EpisodeReplay(str(tmp_path / 'f'), device=dev)


# ---- Estimator.replay and the script ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
  from geeco_amd.synthetic import write_synthetic_dataset
  root = str(tmp_path_factory.mktemp('replay_data'))
  write_synthetic_dataset(root, 2, episode_length=8, img_hw=(S, S), seed=2)
  return root


def test_estimator_replay(dev, tmp_path, dataset):
  from geeco_amd import estimator as est
  from geeco_amd import replay as rp
  cfg, _ = _model_dir(str(tmp_path), False, dict(window_size=3, img_height=S, img_width=S))
  e = est.Estimator(est.e2evmc_model_fn, str(tmp_path), est.RunConfig(device=dev), {'e2evmc_config': cfg})
  episodes = list(rp.dataset_episodes(dataset, 'default', 'eval', dev))
  assert len(episodes) == 2 and episodes[0]['rgb'].dtype == torch.uint8 and tuple(episodes[0]['rgb'].shape) == (7, S, S, 3)
  gen = e.replay(lambda: iter(episodes), max_frames=8, chunk_frames=4)
  outs = list(gen)
  assert len(outs) == 2
  direct = rp.EpisodeReplay(str(tmp_path), device=dev, max_frames=8, chunk_frames=4)
  for ep, out in zip(episodes, outs):
    assert set(out) == {'cmd_ee', 'logits_cmd_grp', 'pos_ee', 'pos_obj', 'errors', 'episode_errors'}
    assert out['cmd_ee'].shape == (7, 3) and out['logits_cmd_grp'].shape == (7, 3) and out['errors'].shape == (7, 4)
    want = direct.replay(ep)
    for k in out:
      if k != 'episode_errors':
        np.testing.assert_array_equal(out[k], want[k], err_msg=k)
    # the gripper column is the hit of the recorded class
    hit = (out['logits_cmd_grp'].argmax(1) == np.rint(ep['cmd'][:, 3]) + 1).astype(np.float32)
    np.testing.assert_array_equal(out['errors'][:, 1], hit)
  assert not np.array_equal(outs[0]['cmd_ee'], outs[1]['cmd_ee'])
  outs2 = list(e.replay(episodes[:1], checkpoint_path=str(tmp_path), max_frames=8))      # the episodes themselves; a model_dir as the checkpoint
  np.testing.assert_allclose(outs2[0]['cmd_ee'], outs[0]['cmd_ee'], rtol=RTOL, atol=ATOL)


def test_replay_episodes_script(dev, tmp_path, dataset, capsys):
  spec = importlib.util.spec_from_file_location('replay_episodes', os.path.join(ROOT, 'scripts', 'replay_episodes.py'))
  script = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(script)
  _model_dir(str(tmp_path), True, dict(window_size=3, img_height=S, img_width=S, proc_obs='sequence', proc_tgt='constant'))
  out = str(tmp_path / 'replay.npz')
  with torch.cuda.device(dev):
    script.main(['--model_dir', str(tmp_path), '--dataset_dir', dataset, '--split', 'val', '--max_frames', '8', '--chunk_frames', '3', '--out', out])
  z = np.load(out)
  heads = ['cmd_ee', 'logits_cmd_grp', 'pos_ee', 'pos_obj']
  assert set(z.files) == set(heads) | {'errors', 'episode_errors', 'episode_lengths', 'episode_names', 'heads'}
  assert z['heads'].tolist() == heads and z['episode_lengths'].tolist() == [7, 7]
  assert z['episode_names'].tolist() == ['ep00000.tfrecord.zlib', 'ep00001.tfrecord.zlib']
  for k in heads:
    assert z[k].shape == (14, 3) and z[k].dtype == np.float32 and np.isfinite(z[k]).all()
  assert z['errors'].shape == (14, 4) and z['episode_errors'].shape == (2, 4)
  np.testing.assert_allclose(z['episode_errors'][1], z['errors'][7:].mean(axis=0), rtol=1e-6)
  text = capsys.readouterr().out
  assert 'ep00000.tfrecord.zlib: 7 frames' in text and 'all 2 episodes, 14 frames' in text and text.count('logits_cmd_grp') == 3
