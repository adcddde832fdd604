"""Window-level shuffle on the GPU: geeco_gather_windows_by_address bitwise against geeco_gather_windows run per
window on the same resident tensors, the Estimator's post-flush fill of dense windows from shuffled batches, the goal model's
K = 1 target stream through the same launch, geeco-f's address form on shuffled batches, and the refusal of shared frames.

Tolerances.  The kernel moves values (uint8 / 255 with the IEEE division, float32 copied): bitwise.  A model fed the same
float32 windows by another route computes the same step: the loss trajectories are held to the 1e-4 relative bound of
test_shared_frames_gpu.py::test_estimator_trains_on_shared_frames (equality is expected); geeco-f's address form against its
dense form is bitwise, as in test_estimator_gpu.py::test_u8_window_addresses_equal_dense_windows."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T_EP = 8
# (episode, start) per window: non-monotone over three episodes, window 2 repeats window 0, windows 1 and 3 overlap
PICKS = {1: [(1, 3)], 5: [(2, 4), (0, 1), (2, 4), (0, 2), (1, 0)]}
KINDS = {'uint8': (True, True, True), 'float32': (False, False, False), 'mixed': (True, False, True)}

_EPISODES = {}


def _episodes(dev, shape, kinds):
  """Three resident episodes [T_EP][frame_elems] (uint8 0..255, or float32 in [0, 1)), built once per case and left unchanged."""
  key = (shape, kinds)
  if key not in _EPISODES:
    fe = int(np.prod(shape))
    r = np.random.default_rng(fe + sum(kinds))
    _EPISODES[key] = [torch.from_numpy(r.integers(0, 256, [T_EP, fe]).astype(np.uint8) if u8 else r.random([T_EP, fe], dtype=np.float32)).to(dev)
                      for u8 in kinds]
  return _EPISODES[key]


def _reference(dev, eps, picks, K, fe):
  """geeco_gather_windows, one launch per window, each with its episode's own divisor"""
  from geeco_amd import ops
  want = torch.full((len(picks), K, fe), float('nan'), device=dev)
  for n, (e, st) in enumerate(picks):
    ops.gather_windows_into(want[n:n + 1], eps[e], torch.tensor([st], dtype=torch.int32, device=dev), 1, K, fe,
                            255.0 if eps[e].dtype == torch.uint8 else 1.0)
  return want


def _by_address(dev, eps, picks, K, fe):
  """The tables sit at a non-zero offset of larger buffers; the output starts as NaN."""
  from geeco_amd import ops
  N = len(picks)
  addr = [eps[e].data_ptr() + st * fe * eps[e].element_size() for e, st in picks]
  kind = [0 if eps[e].dtype == torch.uint8 else 1 for e, _ in picks]
  big_a = torch.full((N + 7,), -1, dtype=torch.int64, device=dev)
  big_k = torch.full((N + 9,), 7, dtype=torch.int32, device=dev)
  big_a[3:3 + N] = torch.tensor(addr, dtype=torch.int64)
  big_k[5:5 + N] = torch.tensor(kind, dtype=torch.int32)
  got = torch.full((N, K, fe), float('nan'), device=dev)
  ops.gather_windows_by_address_into(got, big_a[3:3 + N], big_k[5:5 + N], N, K, fe)
  return got


def _same_bits(got, want):
  torch.cuda.synchronize()
  assert not torch.isnan(want).any() and not torch.isnan(got).any()        # the poisoned output was overwritten everywhere
  assert torch.equal(got.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize('kinds', list(KINDS))
@pytest.mark.parametrize('N', [1, 5])
@pytest.mark.parametrize('K', [1, 3])
@pytest.mark.parametrize('shape', [(8, 12, 3), (6, 10, 3), (6, 10, 1)], ids=['8x12x3', '6x10x3', '6x10x1'])
def test_gather_by_address_is_the_per_window_gather(dev, shape, K, N, kinds):
  fe = int(np.prod(shape))
  eps = _episodes(dev, shape, KINDS[kinds])
  assert all(st + K <= T_EP for _, st in PICKS[N])
  _same_bits(_by_address(dev, eps, PICKS[N], K, fe), _reference(dev, eps, PICKS[N], K, fe))


@pytest.mark.parametrize('u8', [True, False], ids=['uint8', 'float32'])
def test_gather_by_address_unaligned_windows(dev, u8):
  """Episode tensors that are one-ELEMENT-offset views: a uint8 episode 1 byte off a 4-byte boundary, a float32 episode 4 bytes
  off a 16-byte boundary -> the per-element path, next to an aligned episode in the same launch."""
  shape, K = (6, 10, 3), 3
  fe = int(np.prod(shape))
  r = np.random.default_rng(11)
  host = r.integers(0, 256, [1 + T_EP * fe]).astype(np.uint8) if u8 else r.random([1 + T_EP * fe], dtype=np.float32)
  buf = torch.from_numpy(host).to(dev)
  odd = buf[1:].view(T_EP, fe)
  assert odd.data_ptr() % (4 if u8 else 16) == (1 if u8 else 4)
  eps = [odd, _episodes(dev, shape, KINDS['uint8' if u8 else 'float32'])[1], odd]
  _same_bits(_by_address(dev, eps, PICKS[5], K, fe), _reference(dev, eps, PICKS[5], K, fe))


def test_gather_by_address_more_than_one_block_per_frame(dev):
  """1024 elements per block: a frame of 1028 takes two, the second with one active thread"""
  fe, K = 1028, 2
  eps = _episodes(dev, (fe,), KINDS['mixed'])
  _same_bits(_by_address(dev, eps, PICKS[5], K, fe), _reference(dev, eps, PICKS[5], K, fe))


def test_gather_by_address_refusals(dev):
  """Bad arguments return GEECO_EINVAL before anything is launched (the output keeps its poison) and raise through ops."""
  from geeco_amd import _native, ops
  lib = _native.load()
  fe, K, N = 180, 3, 2
  ep = _episodes(dev, (6, 10, 3), KINDS['uint8'])[0]
  addr = torch.tensor([ep.data_ptr(), ep.data_ptr() + fe], dtype=torch.int64, device=dev)
  kind = torch.zeros(N, dtype=torch.int32, device=dev)
  out = torch.full((N, K, fe), float('nan'), device=dev)
  a, k, o = addr.data_ptr(), kind.data_ptr(), out.data_ptr()
  call = lib.geeco_gather_windows_by_address
  for args in ((None, k, N, K, fe, o), (a, None, N, K, fe, o), (a, k, N, K, fe, None), (a, k, 0, K, fe, o), (a, k, N, 0, fe, o),
               (a, k, N, K, 6, o), (a, k, N, K, 0, o), (a, k, N, K, fe, o + 4), (a, k, 65536, K, fe, o)):
    assert call(*args, None) == _native.GEECO_EINVAL, args
    assert lib.geeco_last_error()
  torch.cuda.synchronize()
  assert torch.isnan(out).all()
  with pytest.raises(_native.GeecoNativeError, match='frame_elems=6'):
    ops.gather_windows_by_address_into(out, addr, kind, N, K, 6)
  with pytest.raises(ValueError, match='tables'):
    ops.gather_windows_by_address_into(out, addr.to(torch.float32), kind, N, K, fe)
  with pytest.raises(ValueError, match='output of'):
    ops.gather_windows_by_address_into(out[:1], addr, kind, N, K, fe)
  assert call(a, k, N, K, fe, o, None) == 0                      # ... and the good call still runs
  torch.cuda.synchronize()
  assert not torch.isnan(out).any()


# ================================================================================================
# through the Estimator
# ================================================================================================
H = 136
K3 = 3


def _losses(model_dir):
  return [json.loads(l)['loss'] for l in open(os.path.join(model_dir, 'events.jsonl'))]


def _batches(root, device, **kw):
  """The batches of one shuffled epoch: ``device`` None = dense host arrays, 'cuda' = DeviceWindows of the same picks (the
  shuffle's generator depends on the seed alone)."""
  from geeco_amd import input_fn as I
  kw = dict(dict(window_size=K3, batch_size=4, num_threads=2, shuffle_windows=True, shuffle_buffer=8, seed=3), **kw)
  if device is not None:
    kw.update(device=device, device_keys=('rgb',), cache=False)
  return list(I.pickplace_input_fn(root, 'default', 'train', **kw))


def _same_picks(devb, host):
  assert len(devb) == len(host)
  for (fd, ld), (fh, lh) in zip(devb, host):
    for k in ('step', 'goal_state', 'jnt_state'):
      np.testing.assert_array_equal(fd[k], fh[k], err_msg=k)
    for k in lh:
      np.testing.assert_array_equal(ld[k], lh[k], err_msg=k)


def test_estimator_trains_on_shuffled_windows(dev, tmp_path, monkeypatch):
  """e2e_vmc, 2 episodes x 6 windows in three shuffled batches of 4: after every feed the model's 'rgb' input is, bitwise, the
  windows the host pipeline builds from the same picks (filled by ONE by-address launch queued behind the arena's copy: the
  per-segment gather is not reachable here); the loss trajectory is that of a run fed the same batches as dense host arrays."""
  from geeco_amd import estimator as est
  from geeco_amd import input_fn as I
  from geeco_amd.params import create_e2evmc_config
  root = str(tmp_path / 'ds')
  I.write_synthetic_dataset(root, 2, episode_length=9, img_hw=(H, H), seed=5)
  host, devb = _batches(root, None), _batches(root, 'cuda')
  _same_picks(devb, host)
  assert len(devb) == 3 and all(f['rgb'].scattered and len(f['rgb'].segments) > 1 for f, _ in devb)
  cfg = create_e2evmc_config(dict(window_size=K3, img_height=H, img_width=H, batch_size=4))
  params = {'e2evmc_config': cfg, 'log_steps': 1, 'debug': False}
  ev_kw = dict(window_size=K3, batch_size=4, num_threads=2, device='cuda', device_keys=('rgb',), cache=False)
  # dense host arrays
  e_host = est.Estimator(est.e2evmc_model_fn, str(tmp_path / 'host'), est.RunConfig(init_seed=4), params)
  e_host.train(input_fn=lambda: iter(host))
  ev_host = e_host.evaluate(input_fn=lambda: I.pickplace_input_fn(root, 'default', 'eval', **ev_kw))
  # shuffled DeviceWindows
  e = est.Estimator(est.e2evmc_model_fn, str(tmp_path / 'dev'), est.RunConfig(init_seed=4), params)
  with monkeypatch.context() as m:
    def unreachable(self, out):
      raise AssertionError('the per-segment gather ran for a shuffled batch')
    m.setattr(I.DeviceWindows, 'materialize_into', unreachable)
    e.train(input_fn=lambda: iter(devb))
    (spec, fbuf, lbuf), = [v for k, v in e._specs.items() if k[0] == est.ModeKeys.TRAIN]
    feed = fbuf['rgb']
    assert isinstance(feed, I.WindowFeed) and feed.scattered and feed.buffer is not None and feed.table is None
    assert feed.arena.has(feed.key + ('window_addr',)) and feed.arena.has(feed.key + ('window_kind',))
    assert spec.model.inputs['rgb'] is feed.buffer
    for (fd, ld), (fh, _) in zip(devb, host):
      e._feed_step(fbuf, lbuf, fd, ld)
      torch.cuda.synchronize()
      got = spec.model.inputs['rgb'].cpu().numpy()
      assert got.dtype == fh['rgb'].dtype and np.array_equal(got.view(np.uint32), fh['rgb'].view(np.uint32))
  ev = e.evaluate(input_fn=lambda: I.pickplace_input_fn(root, 'default', 'eval', **ev_kw))
  a, b = _losses(str(tmp_path / 'dev')), _losses(str(tmp_path / 'host'))
  print('loss trajectories: shuffled DeviceWindows %s, dense host arrays %s; eval %s / %s' % (a, b, ev['loss'], ev_host['loss']))
  assert len(a) == len(b) == 3 and ev['global_step'] == 3
  np.testing.assert_allclose(a, b, rtol=1e-4)
  np.testing.assert_allclose(ev['loss'], ev_host['loss'], rtol=1e-4)


def test_goal_model_target_stream_through_the_same_launch(dev, tmp_path):
  """'sequence' x 'residual' with fetch_target: 'rgb' (K = 3) and 'target_rgb' (K = 1, squeezed) are each filled by address;
  one shuffled step runs and both inputs are bitwise the host pipeline's arrays."""
  from geeco_amd import estimator as est
  from geeco_amd import input_fn as I
  from geeco_amd.params import create_e2evmc_config
  root = str(tmp_path / 'ds')
  I.write_synthetic_dataset(root, 2, episode_length=7, img_hw=(H, H), seed=6)
  host, devb = _batches(root, None, fetch_target=True), _batches(root, 'cuda', fetch_target=True)
  _same_picks(devb, host)
  assert devb[0][0]['target_rgb'].scattered and devb[0][0]['target_rgb'].squeeze_k
  cfg = create_e2evmc_config(dict(proc_obs='sequence', proc_tgt='residual', window_size=K3, img_height=H, img_width=H, batch_size=4))
  e = est.Estimator(est.goal_e2evmc_model_fn, str(tmp_path / 'm'), est.RunConfig(), {'e2evmc_config': cfg, 'log_steps': 1})
  e.train(input_fn=lambda: iter(devb[:1]))
  (spec, fbuf, lbuf), = e._specs.values()
  torch.cuda.synchronize()
  for k in ('rgb', 'target_rgb'):
    assert fbuf[k].scattered and spec.model.inputs[k] is fbuf[k].buffer
    got = spec.model.inputs[k].cpu().numpy()
    assert got.shape == host[0][0][k].shape and np.array_equal(got.view(np.uint32), host[0][0][k].view(np.uint32)), k
  loss, = _losses(str(tmp_path / 'm'))
  assert np.isfinite(loss) and int(e._store.global_step.item()) == 1


def test_geeco_f_follows_shuffled_window_addresses(dev, tmp_path, monkeypatch):
  """geeco-f on uint8 episodes takes ``pointers()``: ``addresses()`` serves any segment list, so shuffled batches need nothing
  new there.  Training and evaluation are BITWISE those of the same batches fed densely (a model that declares no
  u8_window_keys: its dense windows are filled by address)."""
  from geeco_amd import estimator as est, graph
  from geeco_amd import input_fn as I
  from geeco_amd.params import create_e2evmc_config
  root = str(tmp_path / 'ds')
  I.write_synthetic_dataset(root, 2, episode_length=7, img_hw=(H, H), seed=7)
  devb = _batches(root, 'cuda', fetch_target=True)
  assert len(devb) == 2 and all(f['rgb'].is_u8() and f['rgb'].scattered for f, _ in devb)
  params = {'e2evmc_config': create_e2evmc_config(dict(proc_obs='dynimg', proc_tgt='dyndiff', window_size=K3, img_height=H,
                                                       img_width=H, batch_size=4)), 'log_steps': 1000, 'debug': False}
  res = []
  for dense in (False, True):
    with monkeypatch.context() as m:
      if dense:
        init = graph.GoalE2EVMC.__init__

        def dense_init(self, *a, **k):
          init(self, *a, **k)
          self.u8_window_keys = ()
        m.setattr(graph.GoalE2EVMC, '__init__', dense_init)
      e = est.Estimator(est.goal_e2evmc_model_fn, None, est.RunConfig(init_seed=5), params)
      e.train(input_fn=lambda: iter(devb))
      ev = e.evaluate(input_fn=lambda: iter(devb))
    feeds = [f for (spec, fbuf, lbuf) in e._specs.values() for f in fbuf.values() if isinstance(f, I.WindowFeed)]
    took = {(f.table is not None, f.buffer is not None) for f in feeds}
    assert took == ({(False, True)} if dense else {(True, False)}), took
    res.append((ev, {n: e.get_variable_value(n) for n in e.get_variable_names()}))
  (ev_a, var_a), (ev_b, var_b) = res
  assert ev_a == ev_b and ev_a['global_step'] == 2, (ev_a, ev_b)
  for n in var_a:
    np.testing.assert_array_equal(var_a[n], var_b[n], err_msg=n)


def test_shared_frames_refuse_a_shuffling_input(dev, tmp_path):
  from geeco_amd import estimator as est
  from geeco_amd import input_fn as I
  from geeco_amd.params import create_e2evmc_config
  root = str(tmp_path / 'ds')
  I.write_synthetic_dataset(root, 2, episode_length=7, img_hw=(H, H), seed=8)
  cfg = create_e2evmc_config(dict(window_size=K3, img_height=H, img_width=H, batch_size=4))
  e = est.Estimator(est.e2evmc_model_fn, None, est.RunConfig(), {'e2evmc_config': cfg, 'shared_frames': True})
  with pytest.raises(ValueError, match='nothing to share'):
    e.train(input_fn=lambda: iter(_batches(root, 'cuda')), steps=1)
