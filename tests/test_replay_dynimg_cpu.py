"""Dynamic-image replay, host side (no GPU): which configs the new class takes and which it sends to EpisodeReplay, the
class ``open_replay`` picks from a checkpoint, the image-stage model against a literal simulation of the reference predictor's
buffer, the state-pair columns against the oracle's concat, the chunk default, every refusal of the ``ops`` wrappers and of the C
boundary, and the new entry points in the header and the library."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import _replay_dynimg_ref as D
import _replay_ref as R

import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(**kw):
  from geeco_amd.params import create_e2evmc_config
  return create_e2evmc_config(kw)


def test_config_check_accepts_and_refuses_exactly_the_documented_sets():
  from geeco_amd.replay_dynimg import check_dynimg_replay_config, serves_dynamic_images
  root = 'GoalVMC/'
  for tgt in ('constant', 'residual', 'dyndiff'):      # the dense model's 'dynimg' branch ignores proc_tgt
    cfg = _cfg(proc_obs='dynimg', proc_tgt=tgt, dim_s_obs=64, dim_s_dyn=32, dim_s_diff=16)
    assert check_dynimg_replay_config(cfg, True) == ('dynimg', [root + 'ConvEncoder', root + 'DynBuffEncoder', root + 'DynDiffEncoder'], [64, 32, 16])
    assert serves_dynamic_images(cfg, True) and not serves_dynamic_images(cfg, False)
  cfg = _cfg(proc_obs='sequence', proc_tgt='dyndiff', dim_s_obs=64, dim_s_diff=16)
  assert check_dynimg_replay_config(cfg, True) == ('seq_dyndiff', [root + 'ConvEncoder', root + 'DynDiffEncoder'], [64, 16])
  assert serves_dynamic_images(cfg, True)
  for tgt in ('constant', 'residual'):                 # the per-frame configs: the message points at EpisodeReplay
    cfg = _cfg(proc_obs='sequence', proc_tgt=tgt)
    with pytest.raises(ValueError, match="proc_tgt='%s'.*EpisodeReplay" % tgt):
      check_dynimg_replay_config(cfg, True)
    assert not serves_dynamic_images(cfg, True)
  with pytest.raises(ValueError, match='e2e_vmc.*EpisodeReplay'):
    check_dynimg_replay_config(_cfg(proc_obs='dynimg', proc_tgt='dyndiff'), False)
  with pytest.raises(ValueError, match='img_channels=4'):
    check_dynimg_replay_config(_cfg(proc_obs='dynimg', proc_tgt='dyndiff', img_channels=4), True)
  assert not serves_dynamic_images(_cfg(proc_obs='dynimg', proc_tgt='dyndiff', img_channels=4), True)
  with pytest.raises(ValueError, match='frame buffer'):
    check_dynimg_replay_config(_cfg(proc_obs='other'), True)


@pytest.mark.parametrize('goal,extra,want', [
    (False, dict(), 'EpisodeReplay'), (True, dict(proc_obs='sequence', proc_tgt='residual'), 'EpisodeReplay'),
    (True, dict(proc_obs='dynimg', proc_tgt='dyndiff'), 'DynamicImageReplay'), (True, dict(proc_obs='sequence', proc_tgt='dyndiff'), 'DynamicImageReplay')])
def test_open_replay_picks_the_class_from_the_checkpoint(tmp_path, monkeypatch, goal, extra, want):
  """The config comes from the run directory and goal / no goal from the checkpoint's variable names; the classes are stand-ins that
  record how they were called (the real ones need the GPU)."""
  from geeco_amd import replay_dynimg as rd
  from test_batched_predictor_gpu import _model_dir
  _model_dir(str(tmp_path), goal, dict(window_size=3, **extra))
  calls = []
  for name in ('EpisodeReplay', 'DynamicImageReplay'):
    monkeypatch.setattr(rd, name, lambda *a, _n=name, **kw: calls.append((_n, a, kw)) or _n)
  assert rd.open_replay(str(tmp_path), max_frames=7, chunk_frames=2) == want
  (name, args, kw), = calls
  assert name == want and args == (str(tmp_path), None) and kw['goal'] == goal and kw['cfg'].window_size == 3
  assert kw['max_frames'] == 7 and kw['chunk_frames'] == 2


@pytest.mark.parametrize('K', [1, 3, 4, 16])
def test_image_model_is_the_reference_buffer(K):
  """The index-rule model of geeco_replay_images equals, bit for bit, the images formed from a literal simulation of the reference
  predictor's buffer (reset at frame 0, then t pushes): T below, at and above K; the whole episode and a range; the per-frame form
  without the buffer image."""
  r = np.random.default_rng(K)
  HW = 8
  goal = (r.integers(0, 256, (HW, 3)) / np.float32(255)).astype(np.float32)
  for T in sorted({1, max(K - 1, 1), K + 2, 9}):
    frames = (r.integers(0, 256, (T, HW, 3)) / np.float32(255)).astype(np.float32)
    sim = D.images_by_buffer_simulation(frames, goal, K)
    got = D.images_ref(frames, goal, K, 0, T)
    for a, b, what in zip(got, sim, ('cur', 'buf', 'diff')):
      np.testing.assert_array_equal(a, b, err_msg='%s T=%d' % (what, T))
    assert (got[0][..., 3] == 0).all() and (got[1][..., 3] == 0).all() and (got[2][..., 3] == 0).all()
    np.testing.assert_array_equal(got[0][..., :3], frames)
    if T > 2:
      part = D.images_ref(frames, goal, K, 1, T - 1)
      for a, b in zip(part, got):
        np.testing.assert_array_equal(a, b[1:T - 1])
    cur, none, diff = D.images_ref(frames, goal, K, 0, T, buf=False)
    sim2 = D.images_by_buffer_simulation(frames, goal, K, buf=False)
    assert none is None and sim2[1] is None
    np.testing.assert_array_equal(cur, got[0])
    np.testing.assert_array_equal(diff, got[2])
    np.testing.assert_array_equal(diff, sim2[2])


def test_alpha_model_is_the_librarys_and_the_oracles():
  from geeco_amd import ops
  from oracle import geeco_oracle as O
  for K in (1, 2, 3, 4, 16, 64):
    np.testing.assert_array_equal(D.alpha(K), np.asarray(ops.dynimg_alpha(K), np.float32))
    np.testing.assert_array_equal(D.alpha(K), O.dynimg_alpha(K))
    a = D.alpha(K).astype(np.float64)      # the coefficients sum to zero up to their float32 rounding: frame 0's buffer image
    assert abs(a.sum()) <= 1e-5 * np.abs(a).sum()


def test_first_window_is_rounding_residue():
  """DESIGN 5.29's frame-0 note: K copies of one frame leave, with the float32 coefficients, a raw image whose range is rounding
  residue (at most 1e-4 here, K = 3, 4, 16) where exact coefficients leave 1e-12 or less; divided by range + 1e-6 the two normalised
  images differ by O(0.1 .. 1): a float64 model says nothing about the first window."""
  r = np.random.default_rng(0)
  x = (r.integers(0, 256, (4096, 3)) / np.float32(255)).astype(np.float32)

  def exact_alpha(K):
    H = lambda t: sum(1.0 / i for i in range(1, t + 1))
    return np.asarray([2 * (K - t + 1) - (K + 1) * (H(K) - H(t - 1)) for t in range(1, K + 1)], np.float64)
  norm = lambda d, one: (d - d.min()) / (d.max() - d.min() + one(1e-6))
  for K in (3, 4, 16):
    a32, a64 = D.alpha(K), exact_alpha(K)
    d32, d64 = np.zeros_like(x), np.zeros(x.shape, np.float64)
    for k in range(K):
      d32, d64 = d32 + a32[k] * x, d64 + a64[k] * x.astype(np.float64)
    r32, r64 = float(d32.max() - d32.min()), float(d64.max() - d64.min())
    worst = float(np.abs(norm(d32, np.float32) - norm(d64, np.float64)).max())
    print('K=%d: float32 range %.3g, float64 range %.3g, normalised images differ by up to %.3g' % (K, r32, r64, worst))
    assert r32 <= 1e-4 and r64 <= 1e-12 and worst > 0.05


def test_state_pair_columns_are_the_oracles_concat():
  """Slot k of window t of the host model = representation_concatenation(feat, tgt, jnt) (graph.py:146-167: [obs | jnt | tgt] per cell)
  of frame max(0, t - K + 1 + k)."""
  from oracle import geeco_oracle as O
  T, K, cells, ch, ch_t, J = 6, 4, 4, 6, 3, 7
  r = np.random.default_rng(2)
  feat = r.standard_normal((T, cells, ch)).astype(np.float32)
  tgt = r.standard_normal((T, cells, ch_t)).astype(np.float32)
  jnt = r.standard_normal((T, J)).astype(np.float32)
  got = D.states_pair_ref(feat, tgt, jnt, K, 0, T)
  rows = O.representation_concatenation(torch.from_numpy(feat).view(T, 2, 2, ch), torch.from_numpy(tgt).view(T, 2, 2, ch_t), torch.from_numpy(jnt)).numpy()
  idx = R.window_index(T, K)
  for k in range(K):
    np.testing.assert_array_equal(got[k], rows[idx[:, k]])
  np.testing.assert_array_equal(D.states_pair_ref(feat, tgt, jnt, K, 2, 5), got[:, 2:5])


def test_default_chunk_divides_the_budget_by_the_stacks():
  from geeco_amd import replay as rp
  from geeco_amd.replay_dynimg import default_chunk_frames
  cfg = _cfg()
  per = rp.activation_bytes_per_frame(cfg, 256)
  for stacks in (2, 3):
    dims = [256] * stacks
    assert default_chunk_frames(cfg, dims, 10 ** 6) == rp.ACTIVATION_BUDGET // stacks // per
    assert default_chunk_frames(cfg, dims, 10 ** 6, budget=stacks * 5 * per) == 5
    assert default_chunk_frames(cfg, dims, 3) == 3 and default_chunk_frames(cfg, dims, 100, budget=1) == 1
  one = rp.default_chunk_frames(cfg, 256, 10 ** 6)
  assert one // 3 - 1 <= default_chunk_frames(cfg, [256] * 3, 10 ** 6) <= one // 3


def test_ops_refusals_need_no_gpu():
  """Every GEECO_EINVAL case of the two entry points is refused with ValueError in ``ops`` before a pointer is taken (host tensors stand
  in for device memory)."""
  from geeco_amd import ops
  T, K, HW = 5, 3, 16
  img = lambda n=T: torch.zeros(n, HW, 4)
  addr, goal, ws = torch.zeros(T, dtype=torch.int64), torch.zeros(HW, 3), torch.zeros(64)
  mis = torch.zeros(T * HW * 4 + 1)[1:]      # 4 bytes past a 16-byte boundary
  call = lambda **kw: ops.replay_images_into(kw.get('cur', img()), kw.get('buf', img()), kw.get('diff', img()), kw.get('addr', addr),
                                             kw.get('goal', goal), kw.get('T', T), kw.get('t0', 0), kw.get('t1', T), kw.get('K', K),
                                             kw.get('HW', HW), kw.get('ws', ws))
  for msg, kw in (('K=0', dict(K=0)), ('K=65', dict(K=65)), ('HW=18', dict(HW=18)), ('HW=0', dict(HW=0)),
                  (r'windows \[0, 6\)', dict(t1=6)), (r'windows \[-1, 3\)', dict(t0=-1, t1=3)), (r'windows \[2, 2\)', dict(t0=2, t1=2)),
                  ('cur_out and diff_out', dict(cur=None)), ('cur_out and diff_out', dict(diff=None)),
                  ('cur_out is misaligned', dict(cur=mis)), ('buf_out is misaligned', dict(buf=mis)), ('diff_out is misaligned', dict(diff=mis)),
                  ('buf_out must be', dict(buf=img(2))), ('goal must be', dict(goal=torch.zeros(HW, 4))),
                  ('frame_addr', dict(addr=addr[:3])), ('frame_addr', dict(addr=addr.to(torch.int32))), ('ws of', dict(ws=torch.zeros(4)))):
    with pytest.raises(ValueError, match=msg):
      call(**kw)
  cells, ch, ch_t, J = 4, 8, 4, 7
  feat, tgt, jnt = torch.zeros(T, cells, ch), torch.zeros(T, cells, ch_t), torch.zeros(T, J)
  states = torch.zeros(K, T, cells * (ch + J + ch_t))
  pair = lambda st=states, f=feat, t=tgt, j=jnt, T=T, t0=0, t1=T, K=K: ops.replay_states_pair_into(st, f, t, j, T, t0, t1, K, cells, ch, ch_t, J)
  for msg, kw in (('K=0', dict(K=0)), ('K=65', dict(K=65)), (r'windows \[0, 6\)', dict(t1=6)), (r'windows \[3, 3\)', dict(t0=3, t1=3)),
                  ('states of shape', dict(st=states[:, :4])), ('states of shape', dict(st=torch.zeros(K, T, 10))),
                  ('feat / tgt_feat / jnt', dict(t=tgt[:4])), ('feat / tgt_feat / jnt', dict(f=feat[:2]))):
    with pytest.raises(ValueError, match=msg):
      pair(**kw)


def test_library_refuses_bad_arguments_before_any_launch():
  """The C boundary itself: GEECO_EINVAL and a message, no GPU needed."""
  from geeco_amd import _native
  lib = _native.load()
  one, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
  a = (ctypes.c_float * 64)()
  al = ctypes.cast(a, ctypes.c_void_p)
  im = lambda *v: lib.geeco_replay_images(*v)
  ok = dict(addr=one, goal=one, u8=0, T=9, t0=0, t1=9, K=4, HW=64, cur=one, buf=one, diff=one, ws=one)
  def images(**kw):
    v = dict(ok, **kw)
    return im(v['addr'], v['goal'], v['u8'], al, al, v['T'], v['t0'], v['t1'], v['K'], v['HW'], v['cur'], v['buf'], v['diff'], v['ws'], None)
  for msg, kw in ((b'K=0', dict(K=0)), (b'K=65', dict(K=65)), (b'HW=66', dict(HW=66)), (b'windows [0, 10)', dict(t1=10)),
                  (b'windows [4, 4)', dict(t0=4, t1=4)), (b'windows [-1, 2)', dict(t0=-1, t1=2)), (b'null pointer', dict(cur=None)),
                  (b'null pointer', dict(diff=None)), (b'null pointer', dict(ws=None)), (b'null pointer', dict(addr=None)),
                  (b'16-byte aligned', dict(cur=odd)), (b'16-byte aligned', dict(buf=odd)), (b'16-byte aligned', dict(diff=odd)),
                  (b'misaligned goal', dict(goal=odd)), (b'misaligned goal', dict(goal=ctypes.c_void_p(4097), u8=1))):
    assert images(**kw) == -1 and msg in lib.geeco_last_error(), (msg, lib.geeco_last_error())
  assert lib.geeco_replay_images_ws_bytes(3, 64) == 3 * 16 and lib.geeco_replay_images_ws_bytes(2, 4 * 257) == 2 * 2 * 16
  assert lib.geeco_replay_images_ws_bytes(0, 64) == 0
  sp = lambda *v: lib.geeco_replay_states_pair(*v)
  assert sp(one, None, one, 9, 0, 9, 9, 4, 4, 8, 4, 7, one, 76, None) == -1 and b'null pointer' in lib.geeco_last_error()
  assert sp(one, one, one, 9, 0, 9, 9, 65, 4, 8, 4, 7, one, 76, None) == -1 and b'K=65' in lib.geeco_last_error()
  assert sp(one, one, one, 9, 3, 10, 9, 4, 4, 8, 4, 7, one, 76, None) == -1 and b'windows [3, 10)' in lib.geeco_last_error()
  assert sp(one, one, one, 9, 0, 9, 8, 4, 4, 8, 4, 7, one, 76, None) == -1 and b'N=8' in lib.geeco_last_error()
  assert sp(one, one, one, 9, 0, 9, 9, 4, 4, 8, 4, 7, one, 75, None) == -1 and b'state_stride=75' in lib.geeco_last_error()
  assert sp(one, one, one, 9, 0, 9, 9, 4, 4, 8, 0, 7, one, 76, None) == -1 and b'ch_t=0' in lib.geeco_last_error()


def test_header_declares_and_library_exports_the_new_entries():
  from geeco_amd import _native
  lib = ctypes.CDLL(_native.LIB_PATH)
  listed = _abi.added_within(7)
  for name in ('geeco_replay_images', 'geeco_replay_states_pair', 'geeco_replay_images_ws_bytes'):
    assert _abi.functions()[name][0] in ('int', 'int64_t'), name
    assert name in listed and name in _native.SIGNATURES and hasattr(lib, name), name
  assert _abi.define('GEECO_ABI_VERSION') == 7 == _native.ABI_VERSION
  src = open(os.path.join(ROOT, 'geeco_amd', 'csrc', 'sources.sh')).read()
  assert re.search(r'HIP_SOURCES="[^"]*\breplay_dynimg\b', src)


def test_package_surface():
  import geeco_amd
  from geeco_amd import replay_dynimg as rd
  from geeco_amd.replay import EpisodeReplay
  assert geeco_amd.DynamicImageReplay is rd.DynamicImageReplay and geeco_amd.open_replay is rd.open_replay
  assert geeco_amd.EpisodeReplay is EpisodeReplay
  sig = inspect.signature(rd.DynamicImageReplay.__init__)
  assert list(sig.parameters)[:8] == ['self', 'model_dir', 'checkpoint_name', 'use_ema', 'device', 'max_frames', 'chunk_frames', 'chunk_windows']
  assert list(sig.parameters) == list(inspect.signature(EpisodeReplay.__init__).parameters)
  assert list(inspect.signature(rd.DynamicImageReplay.replay).parameters) == ['self', 'episode', 'goal_frame', 'labels', 'return_images']
  from geeco_amd import estimator as est
  assert 'open_replay(' in inspect.getsource(est.Estimator.replay)
  script = open(os.path.join(ROOT, 'scripts', 'replay_episodes.py')).read()
  assert 'open_replay(' in script and 'EpisodeReplay(' not in script


def test_recorded_agreement_with_the_stepped_predictor():
  """tests/golden/replay_dynimg_achieved.json: the largest difference between replay and the stepped non-incremental predictor over
  every frame, frame 0 included, as measured on the GPU (test_replay_dynimg_gpu.py asserts the tolerance on every run)."""
  rec = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'replay_dynimg_achieved.json')))
  assert rec['rtol'] == 1e-4 and rec['atol'] == 2e-5
  assert len(rec['cases']) == 8      # two models x K = 3, 4 x uint8, float32
  for case in rec['cases']:
    assert case['max_abs_diff'] <= rec['atol'] + rec['rtol'] * case['max_abs_value'], case
    assert case['bitwise'] is True and case['chunked_bitwise'] is True      # what test_replay_dynimg_gpu.py asserts on every run
