"""Dynamic-image replay on the GPU: geeco_replay_images bitwise against the goal model's input stage on explicitly
gathered windows, geeco_replay_states_pair bitwise against its host model, and the whole path -- geeco-f and 'sequence' x 'dyndiff',
K = 3 and 4, uint8 and float32 frames -- against the float64 oracle, the stepped non-incremental predictor, itself in one chunk and
on a prefix, ``Estimator.replay`` and scripts/replay_episodes.py."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import _replay_dynimg_ref as D
import _replay_ref as R
from oracle import geeco_oracle as O
from test_batched_predictor_gpu import _model_dir

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = 1e-4, 2e-5      # tests/test_predictor_gpu.py: predictions against the oracle
S = 136
U = 2.0 ** -24
HW_BLOCKS = 4 * (2 * 256 + 40)      # 2208 pixels: three blocks of 256 four-pixel units per window, the last one ragged (40 units)


# ---- geeco_replay_images ----------------------------------------------------------------------------------------------------
def _planted_episode(T, HW, seed):
  """uint8 frames [T][HW][3] and a goal [HW][3].  One block per window (HW = 64): full-range random bytes.  Several blocks: a narrow
  random band with four planted pixels, so that for every window t >= 1 the buffer image has its maximum in the FIRST block (a pixel
  rising over the episode) and its minimum in the LAST (a falling pixel), and the pair image its maximum in the first (goal 255 under
  frames of 0) and its minimum in the last (goal 0 under frames of 255): a reduction that misses a block gives another image."""
  r = np.random.default_rng(seed)
  if HW == 64:
    return r.integers(0, 256, (T, HW, 3), dtype=np.uint8), r.integers(0, 256, (HW, 3), dtype=np.uint8)
  frames = r.integers(124, 132, (T, HW, 3), dtype=np.uint8)
  goal = r.integers(124, 132, (HW, 3), dtype=np.uint8)
  ramp = np.round(np.linspace(0, 255, T)).astype(np.uint8) if T > 1 else np.asarray([128], np.uint8)
  frames[:, 5], frames[:, HW - 3] = ramp[:, None], ramp[::-1, None]      # buffer image: rising in block 0, falling in the last block
  goal[5] = goal[HW - 3] = 128
  frames[:, 9], goal[9] = 0, 255                                          # pair image: maximum in block 0
  frames[:, HW - 7], goal[HW - 7] = 255, 0                                # ... minimum in the last block
  return frames, goal


def _check_planted(frames, goal, K):
  """The planted extrema are where the docstring says, for every window t >= 1 (float64, raw images)."""
  T, HW = frames.shape[:2]
  f, g = frames.astype(np.float64) / 255, goal.astype(np.float64) / 255
  a, a2 = D.alpha(K).astype(np.float64), D.alpha(2).astype(np.float64)
  idx = R.window_index(T, K)
  block = lambda i: (i // 3) // 1024
  last = (HW - 1) // 1024
  for t in range(1, T):
    pair = a2[0] * f[t] + a2[1] * g
    assert block(pair.argmax()) == 0 and block(pair.argmin()) == last
    if K > 1:
      buf = np.tensordot(a, f[idx[t]], axes=1)
      assert block(buf.argmax()) == 0 and block(buf.argmin()) == last, (t, K)


@pytest.mark.parametrize('u8', [True, False])
@pytest.mark.parametrize('K', [1, 3, 4, 16])
@pytest.mark.parametrize('HW', [64, HW_BLOCKS])
def test_replay_images_are_the_goal_input_stage_bitwise(dev, HW, K, u8):
  """T = 1, K - 1 and 9; the ranges [0, T), [2, 5) and [T - 1, T); with and without the buffer image.  Reference: the one-pass goal
  input stage (float32: goal_dynimgs_into on the gathered dense windows; uint8: goal_dynimgs_u8_into on gathered uint8 windows) and
  dynimg_into for the two-frame image.  Two runs are bitwise equal; the row behind the range keeps -7; the inputs keep their bytes."""
  from geeco_amd import ops
  for T in sorted({1, max(K - 1, 1), 9}):
    fr, gl = _planted_episode(T, HW, 100 * K + T)
    if HW != 64 and T == 9:
      _check_planted(fr, gl, K)
    # the float32 form of the bytes, divided on the host (IEEE): what the two-frame reference reads in both cases
    frames_f, goal_f = (torch.from_numpy(a.astype(np.float32) / np.float32(255)).to(dev) for a in (fr, gl))
    frames, goal = (torch.from_numpy(fr).to(dev), torch.from_numpy(gl).to(dev)) if u8 else (frames_f, goal_f)
    keep_f, keep_g = frames.clone(), goal.clone()
    addr = torch.from_numpy(frames.data_ptr() + np.arange(T, dtype=np.int64) * HW * 3 * frames.element_size()).to(dev)
    idx = torch.from_numpy(R.window_index(T, K)).to(dev)
    for t0, t1 in sorted({(0, T), (T - 1, T)} | ({(2, 5)} if T >= 5 else set())):
      n = t1 - t0
      # the reference: explicitly gathered windows through the goal model's input stage
      win = frames[idx[t0:t1]].contiguous()                      # [n][K][HW][3]
      tgt = goal[None].expand(n, HW, 3).contiguous()
      want = [torch.zeros(n, HW, 4, device=dev) for _ in range(3)]
      gws = ops.goal_dynimgs_ws(n, HW, dev)
      if u8:
        wp = torch.from_numpy(win.data_ptr() + np.arange(n, dtype=np.int64) * K * HW * 3).to(dev)
        tp = torch.from_numpy(tgt.data_ptr() + np.arange(n, dtype=np.int64) * HW * 3).to(dev)
        ops.goal_dynimgs_u8_into(want[0], want[1], want[2], wp, tp, K, n, HW, gws)
        cur_f, tgt_f = frames_f[t0:t1], goal_f[None].expand(n, HW, 3)
      else:
        ops.goal_dynimgs_into(want[0], want[1], want[2], win, tgt, K, n, HW, gws, K * HW * 3, HW * 3)
        cur_f, tgt_f = frames[t0:t1].contiguous(), tgt
      assert ops.goal_dynimgs_timeouts(gws, n) == 0
      pair = torch.zeros(n, HW, 4, device=dev)
      ops.dynimg_into(pair, cur_f.contiguous(), 2, n, HW, 3, 4, ops.dynimg_ws(n, HW * 3, dev), HW * 3, 0, frames2=tgt_f.contiguous())
      assert torch.equal(pair, want[2])
      ws = ops.replay_images_ws(n, HW, dev)
      for with_buf in (True, False):
        runs = []
        for _ in range(2):
          ws.fill_(float('nan'))      # no zero-fill contract: whatever the workspace holds
          got = [torch.full((n + 1, HW, 4), -7.0, device=dev) for _ in range(3)]
          ops.replay_images_into(got[0], got[1] if with_buf else None, got[2], addr, goal, T, t0, t1, K, HW, ws)
          runs.append(got)
        what = 'T=%d [%d, %d) buf=%s' % (T, t0, t1, with_buf)
        for i, name in enumerate(('cur', 'buf', 'diff')):
          assert torch.equal(runs[0][i], runs[1][i]), '%s: %s differs between two runs' % (what, name)
          if name == 'buf' and not with_buf:
            assert (runs[0][i] == -7.0).all(), what
            continue
          assert torch.equal(runs[0][i][:n], want[i]), '%s: %s' % (what, name)
          assert (runs[0][i][n] == -7.0).all(), what
    assert torch.equal(frames, keep_f) and torch.equal(goal, keep_g)


# ---- geeco_replay_states_pair -------------------------------------------------------------------------------------------------
# (ch, ch_t, J, pad): 16-byte loads and stores / 16-byte loads, one-float stores (J = 7, odd stride) / one float everywhere / mixed: the
# first table could take 16-byte loads, the second (ch_t = 3) cannot, so the whole call takes one float everywhere
PAIR_LAYOUTS = [(8, 4, 8, 4), (8, 4, 7, 5), (6, 3, 7, 3), (8, 3, 8, 4)]


@pytest.mark.parametrize('K', [1, 4])
@pytest.mark.parametrize('ch,ch_t,J,pad', PAIR_LAYOUTS)
def test_replay_states_pair_matches_host_model_bitwise(dev, K, ch, ch_t, J, pad):
  """ch != ch_t, J = 7 and 8, the vectorised and the scalar forms; T = 1, K + 1 and 37; the whole episode and a ragged range; more
  rows per step than windows and a row pitch wider than the row: everything outside the written cells keeps -7."""
  from geeco_amd import ops
  cells = 4
  Dw = cells * (ch + J + ch_t)
  r = np.random.default_rng(10 * K + ch + J)
  for T in (1, K + 1, 37):
    feat = r.standard_normal((T, cells, ch)).astype(np.float32)
    tgt = r.standard_normal((T, cells, ch_t)).astype(np.float32)
    jnt = r.standard_normal((T, J)).astype(np.float32)
    fd, td, jd = (torch.from_numpy(a).to(dev) for a in (feat, tgt, jnt))
    for t0, t1 in [(0, T)] + ([(T // 3, T - 1)] if T - 1 > T // 3 else []):
      n = t1 - t0
      states = torch.full((K, n + 2, Dw + pad), -7.0, device=dev)
      ops.replay_states_pair_into(states, fd, td, jd, T, t0, t1, K, cells, ch, ch_t, J)
      got = states.cpu().numpy()
      np.testing.assert_array_equal(got[:, :n, :Dw], D.states_pair_ref(feat, tgt, jnt, K, t0, t1), err_msg='T=%d [%d, %d)' % (T, t0, t1))
      assert (got[:, n:] == -7.0).all() and (got[:, :, Dw:] == -7.0).all()


@pytest.mark.parametrize('which', ['feat', 'tgt'])
def test_replay_states_pair_from_a_table_that_is_not_16_byte_aligned(dev, which):
  """ch % 4 == 0 and ch_t % 4 == 0, but one table starts 4 bytes past a 16-byte boundary: the call takes the one-float form and equals
  the host model bit for bit; the guard cells keep -7."""
  from geeco_amd import ops
  from test_replay_gpu import _view_4_bytes_in
  T, K, cells, ch, ch_t, J, pad = 5, 4, 4, 8, 4, 8, 4
  Dw = cells * (ch + J + ch_t)
  r = np.random.default_rng(78)
  feat = r.standard_normal((T, cells, ch)).astype(np.float32)
  tgt = r.standard_normal((T, cells, ch_t)).astype(np.float32)
  jnt = r.standard_normal((T, J)).astype(np.float32)
  fd, td = (_view_4_bytes_in(a, dev) if which == name else torch.from_numpy(a).to(dev) for name, a in (('feat', feat), ('tgt', tgt)))
  states = torch.full((K, T + 2, Dw + pad), -7.0, device=dev)
  ops.replay_states_pair_into(states, fd, td, torch.from_numpy(jnt).to(dev), T, 0, T, K, cells, ch, ch_t, J)
  got = states.cpu().numpy()
  np.testing.assert_array_equal(got[:, :T, :Dw], D.states_pair_ref(feat, tgt, jnt, K, 0, T))
  assert (got[:, T:] == -7.0).all() and (got[:, :, Dw:] == -7.0).all()


def test_replay_states_pair_columns_are_the_dense_models_concat(dev):
  """Slot k of window t equals, bit for bit, what state_concat_fwd_into writes for the features of frame max(0, t - K + 1 + k) with
  jnt_pos = 1 -- the launch the dense 'sequence' x 'dyndiff' model makes per step (graph.py: _concat_states)."""
  from geeco_amd import ops
  T, K, cells, ch, ch_t, J = 7, 3, 4, 64, 32, 7
  r = np.random.default_rng(4)
  feat = torch.from_numpy(r.standard_normal((T, cells, ch)).astype(np.float32)).to(dev)
  tgt = torch.from_numpy(r.standard_normal((T, cells, ch_t)).astype(np.float32)).to(dev)
  jnt = torch.from_numpy(r.standard_normal((T, J)).astype(np.float32)).to(dev)
  Dw = cells * (ch + J + ch_t)
  got = torch.zeros(K, T, Dw, device=dev)
  ops.replay_states_pair_into(got, feat, tgt, jnt, T, 0, T, K, cells, ch, ch_t, J)
  idx = torch.from_numpy(R.window_index(T, K)).to(dev)
  for k in range(K):
    want = torch.zeros(T, Dw, device=dev)
    ops.state_concat_fwd_into(want, [feat[idx[:, k]].contiguous(), tgt[idx[:, k]].contiguous()], [ch, ch_t], 1, jnt[idx[:, k]].contiguous(), J, J, T,
                              cells, Dw)
    assert torch.equal(got[k], want), k


# ---- the whole path -----------------------------------------------------------------------------------------------------------
MODELS = {'geeco_f': dict(proc_obs='dynimg', proc_tgt='dyndiff'), 'seq_dyndiff': dict(proc_obs='sequence', proc_tgt='dyndiff')}
T_PATH = 9
# The one frame left out of the oracle comparison for the proc_obs='dynimg' models: after a reset the buffer holds K copies of frame 0
# and the coefficients sum to zero, so the raw buffer image is float32 rounding residue divided by its own range -- the reference's
# behaviour, but nothing a float64 model predicts.  It is asserted finite and pinned by the bitwise image test above and
# by the stepped predictor below, whose images come from the same arithmetic.
ILL_CONDITIONED_FRAME = 0


def _episode(cfg, T, u8, seed):
  """Random frames and a random goal: no two frames are equal, so every window t >= 1 and every pair image has an O(1) range."""
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


def replay_against_oracle_and_stepped(dev, path, model, K, u8):
  """One case of the whole path; returns the measured agreement with the stepped predictor (tests/golden/replay_dynimg_achieved.json)."""
  from geeco_amd import replay as rp
  from geeco_amd import replay_dynimg as rd
  from geeco_amd.batched_predictor import BatchedGoalE2EVMCPredictor
  T, extra = T_PATH, MODELS[model]
  geeco_f = model == 'geeco_f'
  kw = dict(window_size=K, img_height=S, img_width=S, **extra)
  cfg, P = _model_dir(path, True, kw)
  ep, goal_frame = _episode(cfg, T, u8, 31 + 2 * K + u8)
  chunked = rd.open_replay(path, device=dev, max_frames=16, chunk_frames=4)
  assert isinstance(chunked, rd.DynamicImageReplay) and chunked.kind == ('dynimg' if geeco_f else 'seq_dyndiff')
  assert chunked.chunk_frames == 4 and -(-T // 4) == 3 and T % 4      # three chunks, the last ragged
  assert len(chunked.encs) == (3 if geeco_f else 2) and all(e.Nf == 4 and e.G == 1 for e in chunked.encs)
  assert chunked.decoder.N == 16 and chunked.decoder.T == (1 if geeco_f else K)
  out = chunked.replay(ep, goal_frame=goal_frame, return_images=True)
  heads = chunked.heads
  image_keys = {'dynbuff', 'dyndiff'} if geeco_f else {'dyndiff'}
  assert set(out) == {k for k, _, _ in heads} | {'errors', 'episode_errors'} | image_keys
  for k, _, size in heads:
    assert out[k].shape == (T, size) and out[k].dtype == np.float32 and np.isfinite(out[k]).all()
  for k in image_keys:
    assert out[k].shape == (T, S, S, 3) and out[k].dtype == np.float32
  plain = chunked.replay(ep, goal_frame=goal_frame)
  assert set(plain) == set(out) - image_keys
  for k in plain:
    if k != 'episode_errors':
      np.testing.assert_array_equal(plain[k], out[k])
  # (a) the float64 oracle on the explicitly built windows, every frame but the ill-conditioned one
  idx = R.window_index(T, K)
  f = _as_float(ep['rgb'])
  feats = {'rgb': torch.tensor(f[idx], dtype=torch.float64), 'jnt_state': torch.tensor(ep['jnt_state'][idx], dtype=torch.float64),
           'target_rgb': torch.tensor(np.broadcast_to(_as_float(goal_frame), (T, S, S, 3)).copy(), dtype=torch.float64)}
  ref, _ = O.model_forward(feats, {k: torch.tensor(v, dtype=torch.float64) for k, v in P.items()}, O.make_config(batch_size=T, **kw), True)
  rows = [t for t in range(T) if not (geeco_f and t == ILL_CONDITIONED_FRAME)]
  for k, _, _ in heads:
    np.testing.assert_allclose(out[k][rows], ref[k].numpy()[rows], rtol=RTOL, atol=ATOL, err_msg='%s vs oracle' % k)
  # (b) the non-incremental predictor stepped through the same frames after reset(): EVERY frame, frame 0 included
  pred = BatchedGoalE2EVMCPredictor(path, 1, memcap=None, device=dev, frame_dtype='uint8' if u8 else 'float32', debug_images=True)
  pred.set_goal(goal_frame[None])
  pred.reset()
  worst, largest, bitwise = 0.0, 0.0, True
  for t in range(T):
    o = pred.predict(ep['rgb'][t][None], ep['jnt_state'][t][None])
    step = {k: v[0].cpu().numpy() for k, v in pred._model.predictions().items()}
    assert set(step) == {k for k, _, _ in heads}
    for k in step:
      worst = max(worst, float(np.abs(out[k][t] - step[k]).max()))
      largest = max(largest, float(np.abs(step[k]).max()))
      bitwise = bitwise and np.array_equal(out[k][t], step[k])
      np.testing.assert_allclose(out[k][t], step[k], rtol=RTOL, atol=ATOL, err_msg='%s vs stepped, frame %d' % (k, t))
      # measured bitwise in all eight cases (tests/golden/replay_dynimg_achieved.json): a property of these shapes (the encoders at 4
      # frames against 1), not of the design, so it is asserted behind the tolerance, as DESIGN 5.27 does
      np.testing.assert_array_equal(out[k][t], step[k], err_msg='%s vs stepped, frame %d' % (k, t))
    for k in image_keys:      # the images the model saw: the predictor's debug_images, bit for bit
      np.testing.assert_array_equal(out[k][t], o[k][0], err_msg='%s, frame %d' % (k, t))
  print('replay vs stepped: max |diff| %.3g (largest value %.3g, bitwise %s)' % (worst, largest, bitwise))
  # the chunked pass against the pass in one chunk (the encoders at another frame count: the rule of DESIGN 5.27)
  whole = rd.DynamicImageReplay(path, device=dev, max_frames=16)
  assert whole.chunk_frames == 16
  out1 = whole.replay(ep, goal_frame=goal_frame)
  chunk_bitwise = all(np.array_equal(out[k], out1[k]) for k, _, _ in heads)
  for k, _, _ in heads:
    np.testing.assert_allclose(out[k], out1[k], rtol=RTOL, atol=ATOL, err_msg='%s chunked vs one chunk' % k)
    np.testing.assert_array_equal(out[k], out1[k], err_msg='%s chunked vs one chunk' % k)      # (measured so at these shapes: same file)
  # a prefix gives the first rows bit for bit (a window looks back only), T < K included
  for Tp in (1, K - 1, K + 1):
    part = chunked.replay({k: v[:Tp] for k, v in ep.items()}, goal_frame=goal_frame, labels=False)
    assert 'errors' not in part and 'episode_errors' not in part
    for k, _, _ in heads:
      np.testing.assert_array_equal(part[k], out[k][:Tp], err_msg='%s prefix %d' % (k, Tp))
  # the errors are the reduction of these predictions against the recorded values, in the order of tests/_replay_ref.py
  lab = rp.recorded_labels(cfg, ep, T)
  preds = np.concatenate([out[k] for k, _, _ in heads], axis=1)
  want_f, _ = R.errors_ref(preds, lab, rp.error_heads(cfg))
  np.testing.assert_allclose(out['errors'], want_f, rtol=8 * U, atol=0)
  for h, (k, _, _) in enumerate(heads):
    assert np.float32(out['episode_errors'][k]) == R.episode_sum_order(out['errors'][:, h])
  # resident frames: a device tensor gives the dense array's result
  res = torch.from_numpy(np.ascontiguousarray(ep['rgb'])).to(dev)
  out2 = chunked.replay(dict(ep, rgb=res), goal_frame=goal_frame)
  for k, _, _ in heads:
    np.testing.assert_array_equal(out[k], out2[k], err_msg=k)
  return dict(model=model, K=K, frames='uint8' if u8 else 'float32', max_abs_diff=worst, max_abs_value=largest, bitwise=bitwise,
              chunked_bitwise=chunk_bitwise)


@pytest.mark.parametrize('u8', [True, False])
@pytest.mark.parametrize('K', [3, 4])
@pytest.mark.parametrize('model', sorted(MODELS))
def test_replay_whole_path(dev, tmp_path, model, K, u8):
  replay_against_oracle_and_stepped(dev, str(tmp_path), model, K, u8)


def test_replay_argument_errors(dev, tmp_path):
  from geeco_amd import replay_dynimg as rd
  kw = dict(window_size=4, img_height=S, img_width=S, proc_obs='dynimg', proc_tgt='dyndiff')
  cfg, _ = _model_dir(str(tmp_path), True, kw)
  ep, goal = _episode(cfg, 10, True, 3)
  r = rd.DynamicImageReplay(str(tmp_path), device=dev, max_frames=9, chunk_frames=3, chunk_windows=4)
  with pytest.raises(ValueError, match='holds 10 frames.*max_frames=9'):
    r.replay(ep, goal_frame=goal)
  with pytest.raises(ValueError, match='goal_frame'):
    r.replay({k: v[:3] for k, v in ep.items()})
  with pytest.raises(ValueError, match='jnt_state must be'):
    r.replay(dict(ep, rgb=ep['rgb'][:3]), goal_frame=goal)
  with pytest.raises(ValueError, match='one kind'):
    r.replay({k: v[:3] for k, v in ep.items()}, goal_frame=goal.astype(np.float32) / 255)
  full = r.replay({k: v[:9] for k, v in ep.items()}, goal_frame=goal)      # three decoder launches of 4, the last ragged
  assert full['cmd_ee'].shape == (9, 3) and np.isfinite(full['errors']).all()


# ---- Estimator.replay and the script, on a geeco-f run directory ----------------------------------------------------------------
@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
  from geeco_amd.synthetic import write_synthetic_dataset
  root = str(tmp_path_factory.mktemp('replay_dynimg_data'))
  write_synthetic_dataset(root, 2, episode_length=8, img_hw=(S, S), seed=2)
  return root


def test_estimator_replay_and_script_on_a_geeco_f_run(dev, tmp_path, dataset, capsys):
  from geeco_amd import estimator as est
  from geeco_amd import replay as rp
  from geeco_amd import replay_dynimg as rd
  cfg, _ = _model_dir(str(tmp_path), True, dict(window_size=3, img_height=S, img_width=S, proc_obs='dynimg', proc_tgt='dyndiff'))
  with pytest.raises(ValueError, match='a dynamic image'):      # the per-frame class still refuses this run directory
    rp.EpisodeReplay(str(tmp_path), device=dev)
  e = est.Estimator(est.goal_e2evmc_model_fn, str(tmp_path), est.RunConfig(device=dev), {'e2evmc_config': cfg})
  episodes = list(rp.dataset_episodes(dataset, 'default', 'eval', dev, fetch_target=True))
  assert len(episodes) == 2 and 'target_rgb' in episodes[0]
  outs = list(e.replay(lambda: iter(episodes), max_frames=8, chunk_frames=4))
  direct = rd.DynamicImageReplay(str(tmp_path), device=dev, max_frames=8, chunk_frames=4)
  for ep, out in zip(episodes, outs):
    assert set(out) == {'cmd_ee', 'logits_cmd_grp', 'pos_ee', 'pos_obj', 'errors', 'episode_errors'}
    assert out['cmd_ee'].shape == (7, 3) and out['errors'].shape == (7, 4)
    want = direct.replay(ep)
    for k in out:
      if k != 'episode_errors':
        np.testing.assert_array_equal(out[k], want[k], err_msg=k)
    hit = (out['logits_cmd_grp'].argmax(1) == np.rint(ep['cmd'][:, 3]) + 1).astype(np.float32)
    np.testing.assert_array_equal(out['errors'][:, 1], hit)
  assert not np.array_equal(outs[0]['cmd_ee'], outs[1]['cmd_ee'])
  spec = importlib.util.spec_from_file_location('replay_episodes', os.path.join(ROOT, 'scripts', 'replay_episodes.py'))
  script = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(script)
  path = str(tmp_path / 'replay.npz')
  with torch.cuda.device(dev):
    script.main(['--model_dir', str(tmp_path), '--dataset_dir', dataset, '--split', 'val', '--max_frames', '8', '--chunk_frames', '4', '--out', path])
  z = np.load(path)
  assert z['episode_lengths'].tolist() == [7, 7] and z['errors'].shape == (14, 4)
  np.testing.assert_array_equal(z['cmd_ee'], np.concatenate([o['cmd_ee'] for o in outs]))
  assert 'all 2 episodes, 14 frames' in capsys.readouterr().out
