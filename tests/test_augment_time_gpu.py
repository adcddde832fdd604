"""Time augmentation on the GPU: geeco_gather_windows_frames against its three siblings (bitwise, for a consecutive
table and for any table on windows unrolled into single frames), against the restatement of tests/_augment_time_ref.py, across
frame alignments, and through the feed and the Estimator.

Standards, those of tests/test_augment_gpu.py and tests/test_augment_scene_gpu.py for the siblings.  Plain windows and pure
shifts: bitwise numpy's float32 division (a copy for float32 frames), moved.  Tint against float64: atol 1e-6.  Occluders: exact.
Noise against float64: |err| <= 1e-6 + 3e-6 sigma.  Against a sibling entry point: bitwise."""
import numpy as np
import pytest
import torch

from _augment_ref import moved
from _augment_scene_ref import paint
from _augment_time_ref import slot_frame_indices, time_values, time_windows

pytestmark = pytest.mark.gpu

T_EP, N, K = 8, 3, 4
PICKS = [(2, 3), (0, 1), (1, 0)]                  # (episode, start) per window
KINDS = (True, False, True)                       # uint8, float32, uint8 episodes: every launch mixes the kinds
SHAPES = [(6, 8), (5, 5)]                         # W * C % 4 == 0 for C = 3 and 1; the one-element path (75 / 25 elements per frame)
CONSECUTIVE = np.tile(np.arange(K, dtype=np.int32), (N, 1))
# lag 2 with drops at slots 2 and 3; lag 3 from start 1 (frames 0, 0, 0, 1); lag 3 with a drop from start 0 (frame 0 four times)
LAGGED = np.asarray([[-2, -1, -1, -1], [-3, -2, -1, 0], [-3, -2, -2, 0]], np.int32)
DROPPED = np.asarray([[0, 0, 2, 2], [0, 1, 1, 1], [0, 1, 2, 3]], np.int32)      # drops alone, chained in window 1
TABLES = {'lagged': LAGGED, 'dropped': DROPPED}
KEY = np.asarray([0x243f6a88, 0x85a308d3], np.uint32)
SHIFT = np.asarray([(1, -1), (0, 3), (-2, 0)], np.int32)
IDS = dict(ids=lambda hw: '%dx%d' % hw)

_EPISODES = {}


def bound(sigma):
  return 1e-6 + 3e-6 * sigma


def _episodes(dev, fe):
  """(host arrays, device tensors): [T_EP][fe] uint8 or float32 per KINDS, built once per frame size and left unchanged."""
  if fe not in _EPISODES:
    r = np.random.default_rng(fe)
    host = [r.integers(0, 256, [T_EP, fe]).astype(np.uint8) if u8 else r.random([T_EP, fe], dtype=np.float32) for u8 in KINDS]
    _EPISODES[fe] = (host, [torch.from_numpy(h).to(dev) for h in host])
  return _EPISODES[fe]


def _up(dev, a, dt):
  return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)


def _colour(C, seed=0):
  r = np.random.default_rng(seed)
  return np.concatenate([r.uniform(0.5, 1.5, (N, C)), r.uniform(-0.3, 0.3, (N, C))], axis=1).astype(np.float32)


def _rects(H, W):
  rect = np.zeros((N, 4, 4), np.int32)
  rect[0] = [(1, 1, 3, 4), (0, 0, 0, 5), (2, 3, 3, W), (0, 0, H, 1)]
  rect[2] = [(H - 1, -3, 1, W + 9), (-2, W - 1, H + 9, 1), (0, 0, -1, 5), (H, W, 4, 4)]
  return rect, np.random.default_rng(5).random((N, 4, 3), dtype=np.float32)


def _frame_table(eps, src, fe, picks=PICKS):
  """(int64 [n][K] addresses, int32 [n] kinds) on the host: every index checked against T_EP here, before anything is queued."""
  idx = slot_frame_indices([st for _, st in picks], src)
  assert idx.min() >= 0 and idx.max() < T_EP
  addr = np.stack([eps[e].data_ptr() + idx[n] * fe * eps[e].element_size() for n, (e, _) in enumerate(picks)])
  return addr.astype(np.int64), np.asarray([0 if eps[e].dtype == torch.uint8 else 1 for e, _ in picks], np.int32)


def _frames(dev, addr, kind, H, W, C, shift=None, colour=None, occ_rect=None, occ_colour=None, key=None, sigma=0.0, tag=0):
  """One launch of the entry point under test; the output starts as NaN."""
  from geeco_amd import ops
  n, k = addr.shape
  got = torch.full((n, k, H, W, C), float('nan'), device=dev)
  ops.gather_windows_frames_into(got, _up(dev, addr, np.int64), _up(dev, kind, np.int32), _up(dev, shift, np.int32),
                                 _up(dev, colour, np.float32), _up(dev, occ_rect, np.int32), _up(dev, occ_colour, np.float32),
                                 None if key is None else _up(dev, np.asarray(key, np.uint32).view(np.int32), np.int32), sigma, tag,
                                 n, k, H, W, C)
  torch.cuda.synchronize()
  got = got.cpu().numpy()
  assert not np.isnan(got).any()                  # the poisoned output was overwritten everywhere
  return got


def _sibling(dev, addr, kind, k, H, W, C, shift=None, colour=None, occ_rect=None, occ_colour=None, key=None, sigma=0.0, tag=0):
  """The same arguments through the entry point that takes one address per WINDOW: the scene builder with extras, the augmented
  one with a shift, else the by-address one."""
  from geeco_amd import ops
  n = len(addr)
  got = torch.full((n, k, H, W, C), float('nan'), device=dev)
  a, kd = _up(dev, addr, np.int64), _up(dev, kind, np.int32)
  if occ_rect is not None or key is not None:
    ops.gather_windows_scene_into(got, a, kd, _up(dev, shift, np.int32), _up(dev, colour, np.float32), _up(dev, occ_rect, np.int32),
                                  _up(dev, occ_colour, np.float32), None if key is None else _up(dev, np.asarray(key, np.uint32).view(np.int32), np.int32),
                                  sigma, tag, n, k, H, W, C)
  elif shift is not None:
    ops.gather_windows_augmented_into(got, a, kd, _up(dev, shift, np.int32), _up(dev, colour, np.float32), n, k, H, W, C)
  else:
    ops.gather_windows_by_address_into(got, a, kd, n, k, H * W * C)
  torch.cuda.synchronize()
  return got.cpu().numpy()


def _bits(a):
  return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ================================================================================================
# a consecutive table is the sibling, bitwise
# ================================================================================================
@pytest.mark.parametrize('C', [3, 1])
@pytest.mark.parametrize('hw', SHAPES, **IDS)
def test_consecutive_table_is_bitwise_the_siblings(dev, hw, C):
  H, W = hw
  fe = H * W * C
  eps = _episodes(dev, fe)[1]
  addr, kind = _frame_table(eps, CONSECUTIVE, fe)
  zero = np.zeros((N, 2), np.int32)
  if fe % 4 == 0:                                 # (the by-address builder takes no other frames)
    want = _sibling(dev, addr[:, 0], kind, K, H, W, C)
    assert np.array_equal(_bits(_frames(dev, addr, kind, H, W, C)), _bits(want))
    assert np.array_equal(_bits(_frames(dev, addr, kind, H, W, C, zero)), _bits(want))
  for shift, colour in ((zero, None), (SHIFT, None), (SHIFT, _colour(C))):
    want = _sibling(dev, addr[:, 0], kind, K, H, W, C, shift, colour)
    assert np.array_equal(_bits(_frames(dev, addr, kind, H, W, C, shift, colour)), _bits(want)), (shift.tolist(), colour is None)
  assert np.array_equal(_bits(_frames(dev, addr, kind, H, W, C, None, _colour(C))), _bits(_sibling(dev, addr[:, 0], kind, K, H, W, C, zero, _colour(C))))
  if C == 3:
    rect, col = _rects(H, W)
    for extras in ((rect, col, None, 0.0, 0), (None, None, KEY, 0.25, 1), (rect, col, KEY, 0.25, 0)):
      want = _sibling(dev, addr[:, 0], kind, K, H, W, C, SHIFT, _colour(C), *extras)
      assert np.array_equal(_bits(_frames(dev, addr, kind, H, W, C, SHIFT, _colour(C), *extras)), _bits(want)), extras[3:]


# ================================================================================================
# lagged and dropped tables
# ================================================================================================
@pytest.mark.parametrize('table', list(TABLES))
@pytest.mark.parametrize('C', [3, 1])
@pytest.mark.parametrize('hw', SHAPES, **IDS)
def test_plain_and_shifted_slots_are_bitwise_the_frames_they_show(dev, hw, C, table):
  """No tint: every slot is, bitwise, the converted frame it points at (moved under a shift) -- clamped rows included."""
  H, W = hw
  fe = H * W * C
  host, eps = _episodes(dev, fe)
  src = TABLES[table]
  addr, kind = _frame_table(eps, src, fe)
  _, v32 = time_values(host, PICKS, src, (H, W, C))
  got = _frames(dev, addr, kind, H, W, C)
  assert np.array_equal(_bits(got), _bits(v32))
  if table == 'lagged':                           # start 1 and start 0 under lag 3: frame 0 repeats
    assert np.array_equal(got[1, 0], got[1, 2]) and np.array_equal(got[2, 0], got[2, 3]) and not np.array_equal(got[1, 2], got[1, 3])
  got = _frames(dev, addr, kind, H, W, C, SHIFT)
  want = np.stack([moved(v32[n], *SHIFT[n]) for n in range(N)])
  assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize('table', list(TABLES))
@pytest.mark.parametrize('C', [3, 1])
@pytest.mark.parametrize('hw', SHAPES, **IDS)
def test_shift_and_tint_against_float64_and_the_unrolled_sibling(dev, hw, C, table):
  H, W = hw
  fe = H * W * C
  host, eps = _episodes(dev, fe)
  src = TABLES[table]
  addr, kind = _frame_table(eps, src, fe)
  v64, _ = time_values(host, PICKS, src, (H, W, C))
  colour = _colour(C)
  got = _frames(dev, addr, kind, H, W, C, SHIFT, colour)
  err = np.abs(got.astype(np.float64) - time_windows(v64, SHIFT, colour)).max()
  print('%s %dx%dx%d: worst |err| %.3g' % (table, H, W, C, err))
  assert err <= 1e-6
  # ... and bitwise the augmented builder on N * K windows of one frame each
  rep = lambda a: np.repeat(a, K, axis=0)
  want = _sibling(dev, addr.reshape(-1), rep(kind), 1, H, W, C, rep(SHIFT), rep(colour))
  assert np.array_equal(_bits(got), _bits(want.reshape(got.shape)))


@pytest.mark.parametrize('table', list(TABLES))
@pytest.mark.parametrize('hw', SHAPES, **IDS)
def test_occluders_and_noise(dev, hw, table):
  H, W = hw
  fe = H * W * 3
  host, eps = _episodes(dev, fe)
  src = TABLES[table]
  addr, kind = _frame_table(eps, src, fe)
  v64, _ = time_values(host, PICKS, src, (H, W, 3))
  rect, col = _rects(H, W)
  colour = _colour(3)
  # occluders: exact -- the tinted windows with the colours copied in
  base = _frames(dev, addr, kind, H, W, 3, SHIFT, colour)
  got = _frames(dev, addr, kind, H, W, 3, SHIFT, colour, rect, col)
  want, covered = paint(base, rect, col)
  assert np.array_equal(_bits(got), _bits(want)) and covered[0].any() and not covered[0].all()
  # noise, alone and over the rectangles: the float64 restatement with the OUTPUT slot in the counter
  for extras in ((None, None), (rect, col)):
    for sigma, tag in ((0.05, 0), (0.5, 1)):
      got = _frames(dev, addr, kind, H, W, 3, SHIFT, colour, *extras, KEY, sigma, tag)
      err = np.abs(got.astype(np.float64) - time_windows(v64, SHIFT, colour, *extras, KEY, sigma, tag)).max()
      print('%s %dx%d sigma %g tag %d occluded %s: worst |err| %.3g, bound %.3g' % (table, H, W, sigma, tag, extras[0] is not None, err, bound(sigma)))
      assert err <= bound(sigma)


# ================================================================================================
# alignment is a property of the frame
# ================================================================================================
def test_uint8_frames_of_75_bytes_at_all_four_residues(dev):
  """5 x 5 x 3 uint8 frames: consecutive frames lie 75 bytes apart.  One window from start 1 under lag 1 with a drop shows frames
  0, 1, 2, 2, 3 -- residues 0, 3, 2, 2, 1 of the episode's base -- next to a float32 window."""
  H, W, C = 5, 5, 3
  host, eps = _episodes(dev, 75)
  picks, src = [(0, 1), (1, 2)], np.asarray([[-1, 0, 1, 1, 2], [-2, -2, 0, 0, 3]], np.int32)
  addr, kind = _frame_table(eps, src, 75, picks)
  assert sorted(set((addr[0] % 4).tolist())) == [0, 1, 2, 3]
  _, v32 = time_values(host, picks, src, (H, W, C))
  assert np.array_equal(_bits(_frames(dev, addr, kind, H, W, C)), _bits(v32))
  shift = np.asarray([(0, 1), (-1, 2)], np.int32)
  want = np.stack([moved(v32[n], *shift[n]) for n in range(2)])
  assert np.array_equal(_bits(_frames(dev, addr, kind, H, W, C, shift)), _bits(want))


@pytest.mark.parametrize('u8', [True, False], ids=['uint8', 'float32'])
def test_slots_of_one_window_at_different_alignments_on_the_vector_path(dev, u8):
  """6 x 8 x 3 frames (rows of 24 elements: the vector path).  The table points the slots of ONE window at copies of an episode
  that sit 0, 1, 2 and 3 elements off an aligned address, slot 0 at the aligned one: were its alignment taken for the window's,
  the other slots would be read with misaligned vector loads.  A shift by one pixel (3 elements) then breaks the 16-byte
  alignment of the float32 sources in some slots only."""
  H, W, C = 6, 8, 3
  fe = H * W * C
  host = _episodes(dev, fe)[0][0 if u8 else 1]
  flat = torch.from_numpy(host).flatten()
  bufs = [torch.cat([flat[:off], flat]).to(dev) for off in range(4)]            # kept alive to the end of the test
  views = [b[off:].view(T_EP, fe) for off, b in enumerate(bufs)]
  size = views[0].element_size()
  assert [v.data_ptr() % (4 * size) for v in views] == [0, size, 2 * size, 3 * size]
  frames = [[0, 1, 1, 3], [2, 2, 3, 4]]                                        # lagged / dropped rows, frame index per slot
  order = [[0, 1, 2, 3], [3, 0, 2, 1]]                                         # which copy each slot reads
  addr = np.asarray([[views[order[n][k]].data_ptr() + frames[n][k] * fe * size for k in range(4)] for n in range(2)], np.int64)
  kind = np.full(2, 0 if u8 else 1, np.int32)
  v32 = np.stack([host[frames[n]] for n in range(2)]).reshape(2, 4, H, W, C)
  v32 = v32.astype(np.float32) / np.float32(255.0) if u8 else v32
  assert np.array_equal(_bits(_frames(dev, addr, kind, H, W, C)), _bits(v32))
  for shift in ([(0, 1), (1, -1)], [(0, 4), (-1, 0)]):
    shift = np.asarray(shift, np.int32)
    want = np.stack([moved(v32[n], *shift[n]) for n in range(2)])
    assert np.array_equal(_bits(_frames(dev, addr, kind, H, W, C, shift)), _bits(want)), shift.tolist()


# ================================================================================================
# a repeated frame gets fresh noise
# ================================================================================================
def test_two_slots_that_show_one_frame_differ_under_noise_only(dev):
  H, W = 6, 8
  fe = H * W * 3
  eps = _episodes(dev, fe)[1]
  addr, kind = _frame_table(eps, DROPPED, fe)
  quiet = _frames(dev, addr, kind, H, W, 3, None, None, None, None, KEY, 0.0, 0)
  assert np.array_equal(quiet[0, 0], quiet[0, 1]) and np.array_equal(quiet[1, 1], quiet[1, 3])
  noisy = _frames(dev, addr, kind, H, W, 3, None, None, None, None, KEY, 0.1, 0)
  assert (noisy[0, 0] != noisy[0, 1]).mean() > 0.9 and (noisy[1, 1] != noisy[1, 3]).mean() > 0.9


# ================================================================================================
# argument checks
# ================================================================================================
def test_argument_checks(dev):
  from geeco_amd import _native, ops
  lib = _native.load()
  H, W = 6, 8
  fe = H * W * 3
  eps = _episodes(dev, fe)[1]
  addr, kind = _frame_table(eps, LAGGED, fe)
  a, kd = _up(dev, addr, np.int64), _up(dev, kind, np.int32)
  out = torch.full((N, K, H, W, 3), float('nan'), device=dev)
  rect, col = (_up(dev, t, dt) for t, dt in zip(_rects(H, W), (np.int32, np.float32)))
  key = _up(dev, KEY.view(np.int32), np.int32)
  call = lib.geeco_gather_windows_frames
  good = (a.data_ptr(), kd.data_ptr(), None, None, rect.data_ptr(), col.data_ptr(), key.data_ptr(), 0.5, 0, N, K, H, W, 3, out.data_ptr())
  bad = [good[:i] + (v,) + good[i + 1:] for i, v in ((0, None), (1, None), (14, None), (4, None), (5, None), (6, None), (7, 1.0),
                                                     (7, float('nan')), (8, 2), (9, 0), (10, 0), (10, 65536), (11, 0), (13, 4),
                                                     (13, 1), (14, out.data_ptr() + 4), (0, a.data_ptr() + 4))]
  for args in bad:
    assert call(*args, None) == _native.GEECO_EINVAL, args
    assert lib.geeco_last_error()
  torch.cuda.synchronize()
  assert torch.isnan(out).all()                   # nothing was launched
  with pytest.raises(ValueError, match='shift only'):
    ops.gather_windows_frames_into(out, a, kd, None, None, rect, col, None, 0.0, 0, N, K, H, W, 1)
  with pytest.raises(ValueError, match='tables'):                     # a table of window addresses is too short
    ops.gather_windows_frames_into(out, a[:, 0].contiguous(), kd, None, None, None, None, None, 0.0, 0, N, K, H, W, 3)
  with pytest.raises(ValueError, match='come together'):
    ops.gather_windows_frames_into(out, a, kd, None, None, rect, None, None, 0.0, 0, N, K, H, W, 3)
  with pytest.raises(ValueError, match='output of'):
    ops.gather_windows_frames_into(out[:1], a, kd, None, None, None, None, None, 0.0, 0, N, K, H, W, 3)
  assert call(*good, None) == 0
  torch.cuda.synchronize()
  assert not torch.isnan(out).any()


# ================================================================================================
# through DeviceWindows, the feed and the Estimator
# ================================================================================================
def test_materialize_into_and_the_feed_give_one_result(dev):
  from geeco_amd import feed
  from geeco_amd.input_fn import DeviceWindows, WindowAugment
  H, W = 6, 8
  rect, col = _rects(H, W)
  draws = WindowAugment(SHIFT, _colour(3), rect, col, KEY, 0.25, frame_src=LAGGED)
  streams = {}
  for name, C in (('rgb', 3), ('depth', 1)):
    host, eps = _episodes(dev, H * W * C)
    dw = DeviceWindows(K, (H, W, C), 255.0)
    for e, st in PICKS:
      dw.add(eps[e], np.asarray([st], np.int32), 255.0 if eps[e].dtype == torch.uint8 else 1.0)
    dw.augment, dw.timed = draws, True
    streams[name] = dw
  feats = dict(streams, step=np.zeros((N, 1), np.float32))
  fbuf, lbuf = feed.build_slots(dev, feats, None)
  bufs = {k: fbuf[k].dense() for k in streams}
  assert all(fbuf[k].form == 'dense_frames' for k in streams) and fbuf['rgb'].scene == 'occlude+noise' and fbuf['depth'].scene is None
  fbuf, lbuf = feed.adopted_slots(fbuf, lbuf, {})
  feed.feed_step(fbuf, lbuf, feats, None)
  torch.cuda.synchronize()
  for name, dw in streams.items():
    C = dw.frame_shape[-1]
    got = bufs[name].cpu().numpy()
    assert np.array_equal(_bits(got), _bits(dw.numpy())), name
    addr, kind = dw.frame_addresses(dev)
    assert np.array_equal(addr, _frame_table(_episodes(dev, H * W * C)[1], LAGGED, H * W * C)[0])
    direct = _frames(dev, addr, kind, H, W, C, SHIFT, *((_colour(3), rect, col, KEY, 0.25, 0) if C == 3 else ()))
    assert np.array_equal(_bits(got), _bits(direct)), name


HH, K3, BATCH = 136, 3, 4
TIME = dict(frame_drop=0.5, frame_lag=2, shift=1)
MODELS = {'e2e_vmc': (False, dict()), 'geeco_f': (True, dict(proc_obs='dynimg', proc_tgt='dyndiff'))}


@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
  """2 episodes x 8 windows of K = 3 at 136 x 136: four full batches of 4."""
  from geeco_amd import input_fn as I
  root = str(tmp_path_factory.mktemp('augment_time_ds'))
  I.write_synthetic_dataset(root, 2, episode_length=11, img_hw=(HH, HH), seed=9)
  return root


def _values_of(dw, src):
  """float64 [n][K][H][W][3]: the frames the slots of a DeviceWindows show, as real numbers, from its resident segments."""
  out, off = [], 0
  for frames, starts, div in dw.segments:
    fr = frames.cpu().numpy().astype(np.float64) / div
    idx = slot_frame_indices(starts, src[off:off + len(starts)])
    out += [fr[i] for i in idx]
    off += len(starts)
  return np.stack(out).reshape((dw.n, dw.K) + dw.frame_shape)


@pytest.mark.parametrize('name', list(MODELS))
def test_estimator_trains_on_time_augmented_windows(dev, dataset, name, monkeypatch):
  """Steps under dict(frame_drop=0.5, frame_lag=2, shift=1), the last two replays of the captured step: after every feed the
  model's image inputs are the restatement of THAT batch's draws, and a step queues the gathers a shift-only step queues."""
  from geeco_amd import estimator as est, input_fn as I, ops
  from geeco_amd.params import create_e2evmc_config
  goal, kw = MODELS[name]
  launches = []
  for fn in ('gather_windows_frames_into', 'gather_windows_scene_into', 'gather_windows_augmented_into', 'gather_windows_by_address_into',
             'gather_windows_into'):
    monkeypatch.setattr(ops, fn, lambda *a, fn=fn, real=getattr(ops, fn): (launches.append(fn), real(*a))[1])
  batches = list(I.pickplace_input_fn(dataset, 'default', 'train', window_size=K3, batch_size=BATCH, num_threads=2, seed=3, device='cuda',
                                      device_keys=('rgb',), cache=False, fetch_target=goal, augment=TIME))
  assert len(batches) == 4 and all(f['rgb'].frame_src is not None for f, _ in batches)
  src_all = np.concatenate([f['rgb'].frame_src for f, _ in batches])
  assert (src_all[:, 1:] == src_all[:, :-1]).any() and (src_all[:, 0] < 0).any()      # drops and lags were drawn
  cfg = create_e2evmc_config(dict(kw, window_size=K3, img_height=HH, img_width=HH, batch_size=BATCH))
  e = est.Estimator(est.goal_e2evmc_model_fn if goal else est.e2evmc_model_fn, None, est.RunConfig(init_seed=4, use_hipgraph=True),
                    {'e2evmc_config': cfg, 'log_steps': 10 ** 9})
  per_step = []
  for fd, ld in batches:
    spec, fbuf, lbuf = e._get_spec(est.ModeKeys.TRAIN, fd, ld, BATCH)
    del launches[:]
    e._feed_step(fbuf, lbuf, fd, ld)
    per_step.append(list(launches))
    torch.cuda.synchronize()
    draws = fd['rgb'].augment
    assert fbuf['rgb'].form == 'dense_frames' and spec.model.inputs['rgb'] is fbuf['rgb'].buffer
    got = spec.model.inputs['rgb'].cpu().numpy()
    want = time_windows(_values_of(fd['rgb'], draws.frame_src), draws.shift, draws.colour)
    assert np.abs(got.astype(np.float64) - want.reshape(got.shape)).max() <= 1e-6
    if goal:                                      # the target frame is not touched by the time keys
      assert fbuf['target_rgb'].form == 'dense_augmented' and not fd['target_rgb'].timed
      got = spec.model.inputs['target_rgb'].cpu().numpy()
      want = time_windows(_values_of(fd['target_rgb'], np.zeros((BATCH, 1), np.int32)), draws.shift, draws.colour)
      assert np.abs(got.astype(np.float64) - want.reshape(got.shape)).max() <= 1e-6
    spec.train_op()
    torch.cuda.synchronize()
    assert np.isfinite(float(spec.model.loss))
  # ONE model, ONE captured step, and per step the launches of a shift-only step: one gather per image stream
  want = ['gather_windows_frames_into'] + (['gather_windows_augmented_into'] if goal else [])
  assert all(sorted(p) == sorted(want) for p in per_step), per_step
  assert len(e._specs) == 1 and next(iter(e._specs))[-2:] == ('augmented', 'frames')
  runner = spec.train_op.__self__
  assert runner._graphs is not None and runner._calls == 4          # steps 3 and 4 were replays
  assert int(e._store.global_step.item()) == 4
  spec.model.check_device_errors()
