"""Episode replay, host side (no GPU): the window index rule against a literal simulation of the reference predictor's buffer, the
host models against each other, the recorded-label pairing against the input pipeline's own, the refusals of ``ops`` and of the
model check, and the new entry points in the header and the library."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import _replay_ref as R

import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('K', [1, 4])
def test_index_rule_is_the_reference_buffer(K):
  from geeco_amd.replay import window_frames
  for T in sorted({1, 2, max(K - 1, 1), K, K + 1, 3 * K + 1}):
    sim = R.deque_simulation(T, K)
    np.testing.assert_array_equal(R.window_index(T, K), sim, err_msg='T=%d' % T)
    np.testing.assert_array_equal(window_frames(T, K), sim, err_msg='T=%d' % T)
    assert (sim[:, -1] == np.arange(T)).all() and (sim[0] == 0).all()      # newest slot = the frame itself; frame 0 pads


@pytest.mark.parametrize('mode', ['plain', 'constant', 'residual'])
def test_states_ref_is_the_feature_ring_model(mode):
  """The replay layout model equals the incremental predictor's ring model (test_incremental_predictor_cpu.FeatureRingModel)
  stepped through the episode after a reset: one spec, written twice."""
  from test_incremental_predictor_cpu import FeatureRingModel
  T, K, cells, ch, J = 9, 4, 4, 6, 7
  r = np.random.default_rng(3)
  feat = r.standard_normal((T, cells, ch)).astype(np.float32)
  jnt = r.standard_normal((T, J)).astype(np.float32)
  tgt = r.standard_normal((cells, ch)).astype(np.float32)
  want = R.states_ref(feat, jnt, tgt, mode, K, 0, T)
  rm = FeatureRingModel(1, K, cells, ch, J, mode)
  for t in range(T):
    got = rm.push(feat[t][None], jnt[t][None], np.asarray([t == 0]), tgt[None])      # [K][1][D]
    np.testing.assert_array_equal(got[:, 0], want[:, t], err_msg='frame %d' % t)
  np.testing.assert_array_equal(R.states_ref(feat, jnt, tgt, mode, K, 3, 7), want[:, 3:7])


def test_errors_ref_and_sum_order():
  heads = [(0, 3, 0), (3, 3, 1), (6, 2, 0)]
  p = np.asarray([[1, 2, 3, 0.5, 0.5, 0.1, 1, 1], [0, 0, 0, 0.1, 0.9, 0.9, 2, 0], [0, 0, 0, np.nan, 1, 0, 0, 0]], np.float32)
  l = np.asarray([[1, 2, 5, 0, 0, 0, 0, 0], [1, 1, 1, 1, 0, 0, 0, 0], [0, 0, 0, 1, 0, 0, 0, 0]], np.float32)
  frame, ep = R.errors_ref(p, l, heads)
  np.testing.assert_allclose(frame[:, 0], [4 / 3, 1.0, 0.0])
  assert frame[0, 1] == 1.0 and frame[1, 1] == 1.0 and np.isnan(frame[2, 1])      # ties: the first maximum
  np.testing.assert_allclose(frame[:, 2], [1.0, 2.0, 0.0])
  assert np.isnan(ep[1]) and ep[2] == 1.0
  v = np.random.default_rng(0).random(700).astype(np.float32)
  assert abs(float(R.episode_sum_order(v)) - v.astype(np.float64).mean()) <= 12 * 2.0 ** -24 * v.astype(np.float64).mean()


@pytest.mark.parametrize('mode', ['cartesian', 'velocity'])
def test_recorded_labels_are_the_input_pipelines_pairing(mode):
  """recorded_labels()[t] holds what episode_windows pairs with the window ENDING at t, read as build_targets reads it."""
  from geeco_amd import replay as rp
  from geeco_amd.input_fn import _finish_episode, episode_windows
  from geeco_amd.params import create_e2evmc_config
  from oracle import geeco_oracle as O
  K, T0 = 3, 8
  r = np.random.default_rng(5)
  ex = {'step': np.arange(T0), 'ts': r.random(T0).astype(np.float32), 'rgb': np.zeros((T0, 2, 2, 3), np.float32),
        'depth': np.zeros((T0, 2, 2, 1), np.float32), 'ctrl': r.standard_normal((T0, 2)).astype(np.float32)}
  for k in ('jnt_state', 'vel_state', 'ee_state', 'goal_state', 'obj_state'):
    ex[k] = r.standard_normal((T0, 7)).astype(np.float32)
  ex['grp_state'] = r.standard_normal((T0, 2)).astype(np.float32)
  ex['cmd'] = np.concatenate([r.standard_normal((T0, 3)), r.integers(-1, 2, (T0, 1))], 1).astype(np.float32)
  ex = _finish_episode(ex, False)
  T = T0 - 1
  cfg = create_e2evmc_config(dict(control_mode=mode, window_size=K))
  lab = rp.recorded_labels(cfg, ex, T)
  starts = np.arange(T - K + 1)
  feats, labels = episode_windows(ex, K, starts)
  tg = O.build_targets({k: torch.tensor(v) for k, v in feats.items() if k in ('ee_state', 'obj_state')},
                       {k: torch.tensor(v) for k, v in labels.items()}, O.make_config(control_mode=mode, window_size=K))
  off = 0
  for _, key, size, kind, _ in rp.head_table(cfg):
    want = tg[key.replace('logits_', '')].numpy()
    got = lab[K - 1:, off:off + (1 if kind == 1 else size)]
    np.testing.assert_array_equal(got, want.reshape(len(starts), -1), err_msg=key)
    off += size
  assert rp.error_heads(cfg) == ([(0, 3, 0), (3, 3, 1), (6, 3, 0), (9, 3, 0)] if mode == 'cartesian' else
                                 [(0, 7, 0), (7, 3, 0), (10, 2, 0), (12, 3, 0), (15, 3, 0)])
  with pytest.raises(ValueError, match="'ee_state'"):
    rp.recorded_labels(cfg, {k: v for k, v in ex.items() if k != 'ee_state'}, T)


def test_dynamic_image_and_rgbd_configs_are_refused():
  """Before any allocation, with the config fields and the reason in the message."""
  from geeco_amd.params import create_e2evmc_config
  from geeco_amd.replay import check_replay_config, default_chunk_frames
  for extra in (dict(proc_obs='dynimg', proc_tgt='dyndiff'), dict(proc_obs='sequence', proc_tgt='dyndiff'),
                dict(proc_obs='dynimg', proc_tgt='constant')):
    cfg = create_e2evmc_config(extra)
    with pytest.raises(ValueError) as e:
      check_replay_config(cfg, True)
    msg = str(e.value)
    assert "proc_obs='%s'" % cfg.proc_obs in msg and "proc_tgt='%s'" % cfg.proc_tgt in msg
    assert 'a dynamic image' in msg and 'belongs to its window, so nothing is shared between windows' in msg and 'Estimator.predict' in msg
  with pytest.raises(ValueError, match='img_channels=4'):
    check_replay_config(create_e2evmc_config(dict(img_channels=4)), False)
  assert check_replay_config(create_e2evmc_config(dict(proc_obs='dynimg', proc_tgt='dyndiff')), False) == ('VMC', 256, 'plain')
  assert check_replay_config(create_e2evmc_config(dict(proc_tgt='residual', dim_s_obs=64)), True) == ('GoalVMC', 64, 'residual')
  cfg = create_e2evmc_config({})
  assert default_chunk_frames(cfg, 256, 100) == 101 and default_chunk_frames(cfg, 256, 100, budget=1) == 1
  assert 100 <= default_chunk_frames(cfg, 256, 10 ** 6) <= 200      # 2 GiB of 256 x 256 activations (about 14 MB per frame)


def test_ops_refusals_need_no_gpu():
  """Bad arguments raise ValueError in ``ops`` before a pointer is taken (host tensors stand in for device memory here)."""
  from geeco_amd import ops
  cells, ch, J, K, T = 4, 8, 7, 4, 10
  feat, jnt, tgt = torch.zeros(T, cells, ch), torch.zeros(T, J), torch.zeros(cells, ch)
  states = torch.zeros(K, T, cells * (ch + J))
  for msg, call in (
      ('K=65', lambda: ops.replay_states_into(torch.zeros(65, T, 60), feat, jnt, 'plain', T, 0, T, 65, cells, ch, J)),
      ('K=0', lambda: ops.replay_states_into(states, feat, jnt, 'plain', T, 0, T, 0, cells, ch, J)),
      ('mode', lambda: ops.replay_states_into(states, feat, jnt, 'dyndiff', T, 0, T, K, cells, ch, J)),
      (r'windows \[3, 3\)', lambda: ops.replay_states_into(states, feat, jnt, 'plain', T, 3, 3, K, cells, ch, J)),
      (r'windows \[0, 11\)', lambda: ops.replay_states_into(states, feat, jnt, 'plain', T, 0, 11, K, cells, ch, J)),
      (r'windows \[-1, 4\)', lambda: ops.replay_states_into(states, feat, jnt, 'plain', T, -1, 4, K, cells, ch, J)),
      ('tgt_feat', lambda: ops.replay_states_into(states, feat, jnt, 'residual', T, 0, T, K, cells, ch, J)),
      ('tgt_feat', lambda: ops.replay_states_into(states, feat, jnt, 'plain', T, 0, T, K, cells, ch, J, tgt_feat=tgt)),
      ('states of shape', lambda: ops.replay_states_into(states, feat, jnt, 'constant', T, 0, T, K, cells, ch, J, tgt_feat=tgt)),
      ('states of shape', lambda: ops.replay_states_into(states[:, :5], feat, jnt, 'plain', T, 0, T, K, cells, ch, J)),
      ('feat / jnt', lambda: ops.replay_states_into(states, feat[:5], jnt, 'plain', T, 0, T, K, cells, ch, J)),
  ):
    with pytest.raises(ValueError, match=msg):
      call()
  preds, labels = torch.zeros(T, 12), torch.zeros(T, 12)
  of, oe = torch.zeros(T, 2), torch.zeros(2)
  for msg, heads, kw in (
      ('0 heads', [], {}), ('9 heads', [(0, 1, 0)] * 9, {}), (r'head 1 \[10, \+3\)', [(0, 3, 0), (10, 3, 0)], {}),
      (r'head 0 \[0, \+0\)', [(0, 0, 0)], {}), ('kind=2', [(0, 3, 2)], {}), ('T=11', [(0, 3, 0)], dict(T=11)), ('T=0', [(0, 3, 0)], dict(T=0)),
      ('outputs of', [(0, 3, 0), (3, 3, 1), (6, 3, 0)], {}), ('one width', [(0, 3, 0)], dict(labels=torch.zeros(T, 11))),
  ):
    with pytest.raises(ValueError, match=msg):
      ops.replay_errors_into(of, oe, preds, kw.get('labels', labels), kw.get('T', T), heads)


def test_library_refuses_bad_arguments_before_any_launch():
  """The C boundary itself: GEECO_EINVAL and a message, no GPU needed."""
  from geeco_amd import _native
  lib = _native.load()
  one = ctypes.c_void_p(16)
  st = lambda *a: lib.geeco_replay_states(*a)
  assert st(None, one, None, 0, 10, 0, 10, 10, 4, 4, 8, 7, one, 60, None) == -1 and b'null pointer' in lib.geeco_last_error()
  assert st(one, one, None, 1, 10, 0, 10, 10, 4, 4, 8, 7, one, 92, None) == -1 and b'tgt_feat' in lib.geeco_last_error()
  assert st(one, one, None, 0, 10, 0, 10, 10, 65, 4, 8, 7, one, 60, None) == -1 and b'K=65' in lib.geeco_last_error()
  assert st(one, one, None, 0, 10, 0, 10, 10, 0, 4, 8, 7, one, 60, None) == -1 and b'K=0' in lib.geeco_last_error()
  assert st(one, one, None, 0, 10, 4, 11, 10, 4, 4, 8, 7, one, 60, None) == -1 and b'windows [4, 11)' in lib.geeco_last_error()
  assert st(one, one, None, 0, 10, 5, 5, 10, 4, 4, 8, 7, one, 60, None) == -1 and b'windows [5, 5)' in lib.geeco_last_error()
  assert st(one, one, None, 0, 10, 0, 10, 9, 4, 4, 8, 7, one, 60, None) == -1 and b'N=9' in lib.geeco_last_error()
  assert st(one, one, None, 0, 10, 0, 10, 10, 4, 4, 8, 7, one, 59, None) == -1 and b'state_stride=59' in lib.geeco_last_error()
  assert st(one, one, None, 3, 10, 0, 10, 10, 4, 4, 8, 7, one, 60, None) == -1 and b'mode=3' in lib.geeco_last_error()
  arr = lambda *v: (ctypes.c_int * len(v))(*v)
  er = lambda *a: lib.geeco_replay_errors(*a)
  assert er(one, None, 5, 12, 1, arr(0), arr(3), arr(0), one, one, None) == -1 and b'null pointer' in lib.geeco_last_error()
  assert er(one, one, 0, 12, 1, arr(0), arr(3), arr(0), one, one, None) == -1 and b'T=0' in lib.geeco_last_error()
  assert er(one, one, 5, 12, 9, arr(0), arr(3), arr(0), one, one, None) == -1 and b'nheads=9' in lib.geeco_last_error()
  assert er(one, one, 5, 12, 2, arr(0, 10), arr(3, 3), arr(0, 0), one, one, None) == -1 and b'head 1 [10, +3)' in lib.geeco_last_error()
  assert er(one, one, 5, 12, 1, arr(0), arr(3), arr(2), one, one, None) == -1 and b'kind=2' in lib.geeco_last_error()


def test_header_declares_and_library_exports_the_new_entries():
  from geeco_amd import _native
  lib = ctypes.CDLL(_native.LIB_PATH)
  listed = _abi.added_within(7)
  for name in ('geeco_replay_states', 'geeco_replay_errors'):
    assert _abi.functions()[name][0] == 'int', name
    assert name in listed and name in _native.SIGNATURES and hasattr(lib, name), name
  assert _abi.define('GEECO_ABI_VERSION') == 7 == _native.ABI_VERSION
  assert _abi.define('GEECO_REPLAY_MAXHEADS') == _native.REPLAY_MAXHEADS
  src = open(os.path.join(ROOT, 'geeco_amd', 'csrc', 'sources.sh')).read()
  assert re.search(r'HIP_SOURCES="[^"]*\breplay\b', src)


def test_package_surface():
  import inspect
  import geeco_amd
  from geeco_amd import estimator as est
  from geeco_amd.replay import EpisodeReplay
  assert geeco_amd.EpisodeReplay is EpisodeReplay
  sig = inspect.signature(EpisodeReplay.__init__)
  assert list(sig.parameters)[:7] == ['self', 'model_dir', 'checkpoint_name', 'use_ema', 'device', 'max_frames', 'chunk_frames']
  assert list(inspect.signature(EpisodeReplay.replay).parameters) == ['self', 'episode', 'goal_frame', 'labels']
  assert list(inspect.signature(est.Estimator.replay).parameters)[:3] == ['self', 'input_fn_or_episodes', 'checkpoint_path']
  assert inspect.isgeneratorfunction(est.Estimator.replay)
  assert os.path.exists(os.path.join(ROOT, 'scripts', 'replay_episodes.py'))


def test_recorded_agreement_with_the_stepped_predictor():
  """tests/golden/replay_achieved.json: the largest difference between replay and the batch-1 incremental predictor stepped through the
  same frames, as measured on the GPU (test_replay_gpu.py asserts it on every run); inside the predictors' tolerance."""
  rec = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'replay_achieved.json')))
  assert rec['rtol'] == 1e-4 and rec['atol'] == 2e-5
  assert len(rec['cases']) == 6
  for case in rec['cases']:
    assert case['max_abs_diff'] <= rec['atol'] + rec['rtol'] * case['max_abs_value'], case
