"""Scene augmentation on the GPU: geeco_gather_windows_scene against the merged augmented gather (bitwise, wherever
occluders and noise leave an element alone), against the float64 restatement of tests/_augment_scene_ref.py, across its load
paths (bitwise: an element depends on (key, tag, n, k, e) alone), and through the feed and the Estimator for e2e_vmc and geeco-f.

Tolerances.  Occluders: exact (a colour is copied).  Noise against float64: |err| <= 1e-6 + 3e-6 sigma -- 1e-6 is the standing
bound of test_augment_gpu.py on the value under the noise (it also covers the rounding of the final multiply-add of values
below 2), and 3e-6 bounds the error of z itself: 8 float32 roundings (2^-24 each: the logarithm, its correction, the scaling by
-2, the square root, cos / sin at up to 2 ulp, the product) at |z| <= 5.89, i.e. 8 * 6e-8 * 5.89 = 2.8e-6."""
import numpy as np
import pytest
import torch

from _augment_scene_ref import noise_field, paint, scene_windows

pytestmark = pytest.mark.gpu

T_EP, N, K = 6, 3, 2
PICKS = [(2, 3), (0, 1), (1, 0)]                  # (episode, start) per window
KINDS = (True, False, True)                       # uint8, float32, uint8 episodes: every launch mixes the kinds
SHAPES = [(8, 8), (6, 5), (12, 16)]               # W * C % 4 == 0; the one-element path (W * C = 15); rows of 48 elements
KEY = np.asarray([0x243f6a88, 0x85a308d3], np.uint32)
I32 = np.iinfo(np.int32)
IDS = dict(ids=lambda hw: '%dx%d' % hw)


def bound(sigma):
  return 1e-6 + 3e-6 * sigma


_EPISODES = {}


def _episodes(dev, fe, fill='random'):
  """(aligned episodes, one-element-offset views of copies of them, the buffers behind the views): [T_EP][fe] uint8 or float32 per
  KINDS, random or mid-grey; built once per case and left unchanged."""
  if (fe, fill) not in _EPISODES:
    r = np.random.default_rng(fe)
    host = []
    for u8 in KINDS:
      if fill == 'grey':
        host.append(np.full([T_EP, fe], 128, np.uint8) if u8 else np.full([T_EP, fe], 0.5, np.float32))
      else:
        host.append(r.integers(0, 256, [T_EP, fe]).astype(np.uint8) if u8 else r.random([T_EP, fe], dtype=np.float32))
    aligned = [torch.from_numpy(h).to(dev) for h in host]
    bufs = [torch.cat([a.flatten()[:1], a.flatten()]) for a in aligned]
    odd = [b[1:].view(T_EP, fe) for b in bufs]
    assert all(o.data_ptr() % (4 if o.dtype == torch.uint8 else 16) != 0 for o in odd)
    _EPISODES[fe, fill] = (aligned, odd, bufs)
  return _EPISODES[fe, fill]


def _plain_values(eps, k, fe):
  out = np.empty((N, k, fe), np.float64)
  for n, (e, st) in enumerate(PICKS):
    fr = eps[e][st:st + k].cpu().numpy()
    out[n] = fr.astype(np.float64) / 255.0 if fr.dtype == np.uint8 else fr.astype(np.float64)
  return out


def _tables(dev, eps, fe, shift, colour):
  t = lambda a, dt: torch.tensor(a, dtype=dt, device=dev)
  addr = t([eps[e].data_ptr() + st * fe * eps[e].element_size() for e, st in PICKS], torch.int64)
  kind = t([0 if eps[e].dtype == torch.uint8 else 1 for e, _ in PICKS], torch.int32)
  return addr, kind, torch.from_numpy(np.ascontiguousarray(shift, np.int32)).to(dev), \
      None if colour is None else torch.from_numpy(np.ascontiguousarray(colour, np.float32)).to(dev)


def _sibling(dev, eps, k, H, W, shift, colour):
  from geeco_amd import ops
  got = torch.full((N, k, H, W, 3), float('nan'), device=dev)
  ops.gather_windows_augmented_into(got, *_tables(dev, eps, H * W * 3, shift, colour), N, k, H, W, 3)
  torch.cuda.synchronize()
  return got.cpu().numpy()


def _scene(dev, eps, k, H, W, shift, colour, occ_rect=None, occ_colour=None, key=None, sigma=0.0, tag=0):
  """One launch; the output starts as NaN."""
  from geeco_amd import ops
  up = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
  got = torch.full((N, k, H, W, 3), float('nan'), device=dev)
  ops.gather_windows_scene_into(got, *_tables(dev, eps, H * W * 3, shift, colour), up(occ_rect, np.int32), up(occ_colour, np.float32),
                                None if key is None else up(np.asarray(key, np.uint32).view(np.int32), np.int32), sigma, tag, N, k, H, W, 3)
  torch.cuda.synchronize()
  got = got.cpu().numpy()
  assert not np.isnan(got).any()                  # the poisoned output was overwritten everywhere
  return got


def _shifts(H, W):
  """[launches][N][2]: no shift, shifts that cross each of the four edges, both at once, and a window moved out of view."""
  return np.asarray([[(0, 0), (2, 0), (-2, 0)], [(0, 3), (0, -3), (1, -1)], [(-1, 2), (H, 0), (0, -W)]], np.int32)


def _colour(seed=0):
  """gain in [0.5, 1.5] and bias in [-0.3, 0.3] per window and channel: both clamps of the tint act."""
  r = np.random.default_rng(seed)
  return np.concatenate([r.uniform(0.5, 1.5, (N, 3)), r.uniform(-0.3, 0.3, (N, 3))], axis=1).astype(np.float32)


def _rects(H, W):
  """[N][4][4] and colours [N][4][3].  Window 0: two overlapping rectangles (the later one wins), an empty slot between them
  and one on the border that a shift moves in; window 1: int32 extremes -- a rectangle ending just before the frame (y0 + h = -1
  needs 33 bits), one reaching from outside over the whole frame, one starting at INT32_MAX, negative sizes; window 2: the whole frame's last row and column as
  one-pixel-wide rectangles, partly outside the frame."""
  rect = np.zeros((N, 4, 4), np.int64)
  rect[0] = [(1, 1, 3, 4), (0, 0, 0, 5), (2, 3, 3, W), (0, 0, H, 2)]
  rect[1] = [(I32.min, I32.min, I32.max, I32.max), (-5, -7, I32.max, I32.max), (I32.max, 0, I32.max, I32.max), (1, 1, I32.min, -1)]
  rect[2] = [(H - 1, -3, 1, W + 9), (-2, W - 1, H + 9, 1), (0, 0, -1, 5), (H, W, 4, 4)]
  colour = np.random.default_rng(5).random((N, 4, 3), dtype=np.float32)
  colour[0, 2] = [0.0, 1.0, 0.5]
  return rect.astype(np.int32), colour


# ================================================================================================
# against the merged augmented gather, bitwise
# ================================================================================================
@pytest.mark.parametrize('unaligned', [False, True], ids=['aligned', 'unaligned'])
@pytest.mark.parametrize('hw', SHAPES, **IDS)
def test_without_extras_it_is_bitwise_the_augmented_gather(dev, hw, unaligned):
  H, W = hw
  eps = _episodes(dev, H * W * 3)[1 if unaligned else 0]
  for colour in (None, _colour()):
    for shift in _shifts(H, W):
      want = _sibling(dev, eps, K, H, W, shift, colour)
      got = _scene(dev, eps, K, H, W, shift, colour)
      assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (shift.tolist(), colour is None)
      # ... also with a key and a tag that sigma == 0 leaves unused, and with four empty slots
      got = _scene(dev, eps, K, H, W, shift, colour, np.zeros((N, 4, 4)), np.ones((N, 4, 3)), KEY, 0.0, 1)
      assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), shift.tolist()


@pytest.mark.parametrize('unaligned', [False, True], ids=['aligned', 'unaligned'])
@pytest.mark.parametrize('hw', SHAPES, **IDS)
def test_occluders_paint_their_colour_and_leave_the_rest(dev, hw, unaligned):
  H, W = hw
  eps = _episodes(dev, H * W * 3)[1 if unaligned else 0]
  rect, col = _rects(H, W)
  colour = _colour()
  for shift in _shifts(H, W):
    base = _sibling(dev, eps, K, H, W, shift, colour)
    got = _scene(dev, eps, K, H, W, shift, colour, rect, col)
    want, covered = paint(base, rect, col)                              # (keeps float32: the colours are copied)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), shift.tolist()
    for n in range(N):                                                  # stated apart: outside bitwise the sibling, inside the colour
      assert np.array_equal(got[n][:, ~covered[n]].view(np.uint32), base[n][:, ~covered[n]].view(np.uint32))
    assert covered[0].any() and not covered[0].all() and covered[1].all() and covered[2][H - 1].all() and covered[2][:, W - 1].all()
    assert (got[0][:, 2:min(5, H), 3:W] == col[0, 2]).all()             # the later of two overlapping rectangles
    assert (got[0][:, :, :2] == col[0, 3]).all()                        # ... and the border a shift moved in is painted over
    assert (got[1] == col[1, 1]).all()                                  # (-5, -7, INT32_MAX, INT32_MAX) covers the frame, its neighbours nothing
  assert (_scene(dev, eps, K, H, W, _shifts(H, W)[2], None, rect, col)[1] == col[1, 1]).all()      # a window moved out of view


# ================================================================================================
# the noise against float64
# ================================================================================================
def _check_noise(dev, eps, H, W, shift, colour, rect, col, sigma, tag, what):
  fe = H * W * 3
  values = _plain_values(eps, K, fe).reshape(N, K, H, W, 3)
  got = _scene(dev, eps, K, H, W, shift, colour, rect, col, KEY, sigma, tag)
  want = scene_windows(values, shift, colour, rect, col, KEY, sigma, tag)
  err = np.abs(got.astype(np.float64) - want)
  worst = np.unravel_index(err.argmax(), err.shape)
  print('%s %dx%d sigma %g tag %d: worst |err| %.3g at (n, k, y, x, c) = %s: got %.9g, float64 %.9g, bound %.3g' %
        (what, H, W, sigma, tag, err.max(), worst, got[worst], want[worst], bound(sigma)))
  assert err.max() <= bound(sigma), (what, worst, float(err.max()))
  return got, want


@pytest.mark.parametrize('unaligned', [False, True], ids=['aligned', 'unaligned'])
@pytest.mark.parametrize('hw', SHAPES, **IDS)
def test_small_noise_on_mid_grey_exposes_the_normals(dev, hw, unaligned):
  """sigma = 0.05 on frames of 128 / 255 and 0.5: nothing clips (0.5 +- 0.05 * 5.89), so (out - v) / sigma is z itself."""
  H, W = hw
  fe = H * W * 3
  eps = _episodes(dev, fe, 'grey')[1 if unaligned else 0]
  zero = np.zeros((N, 2), np.int32)
  for tag in (0, 1):
    got, want = _check_noise(dev, eps, H, W, zero, None, None, None, 0.05, tag, 'grey')
    assert got.min() > 0 and got.max() < 1
    v = _plain_values(eps, K, fe).reshape(got.shape)
    z = noise_field(KEY, tag, N, K, fe).reshape(got.shape)
    assert np.abs((got.astype(np.float64) - v) / 0.05 - z).max() <= bound(0.05) / 0.05
  # with a shift the border is noise around 0: the negative half clips to exactly 0
  got, _ = _check_noise(dev, eps, H, W, _shifts(H, W)[1], None, None, None, 0.05, 0, 'grey, shifted')
  assert (got[0][:, :, :3] == 0).any() and (got[0][:, :, :3] > 0).any()


@pytest.mark.parametrize('unaligned', [False, True], ids=['aligned', 'unaligned'])
@pytest.mark.parametrize('hw', SHAPES, **IDS)
def test_large_noise_on_random_frames_clips_both_ways(dev, hw, unaligned):
  H, W = hw
  eps = _episodes(dev, H * W * 3)[1 if unaligned else 0]
  rect, col = _rects(H, W)
  for shift in _shifts(H, W):
    got, want = _check_noise(dev, eps, H, W, shift, _colour(), None, None, 0.5, 0, 'random')
    assert (got == 0).any() and (got == 1).any() and (want == 0).any() and (want == 1).any()
  # shift, tint, occluders and noise together: the noise lies over the rectangles too
  got, _ = _check_noise(dev, eps, H, W, _shifts(H, W)[0], _colour(), rect, col, 0.5, 1, 'random, occluded')
  assert len(np.unique(got[1])) > 8


# ================================================================================================
# an element depends on (key, tag, n, k, e) alone
# ================================================================================================
@pytest.mark.parametrize('hw', SHAPES, **IDS)
def test_load_paths_tags_frames_and_runs(dev, hw):
  H, W = hw
  aligned, odd, _ = _episodes(dev, H * W * 3)
  rect, col = _rects(H, W)
  shift, colour = _shifts(H, W)[1], _colour()
  args = (K, H, W, shift, colour, rect, col, KEY, 0.25)
  a = _scene(dev, aligned, *args, 0)
  assert np.array_equal(a.view(np.uint32), _scene(dev, odd, *args, 0).view(np.uint32))          # aligned loads vs narrow ones
  assert np.array_equal(a.view(np.uint32), _scene(dev, aligned, *args, 0).view(np.uint32))      # two runs with one key
  b = _scene(dev, aligned, *args, 1)
  assert not np.array_equal(a, b) and (a != b).mean() > 0.5                                      # the tag
  other = _scene(dev, aligned, K, H, W, shift, colour, rect, col, KEY + np.uint32(1), 0.25, 0)
  assert (a != other).mean() > 0.5                                                               # the key
  grey = _episodes(dev, H * W * 3, 'grey')[0]
  g = _scene(dev, grey, K, H, W, np.zeros((N, 2), np.int32), None, None, None, KEY, 0.05, 0)
  assert (g[0, 0] != g[0, 1]).mean() > 0.9 and (g[0, 0] != g[2, 0]).mean() > 0.9                # frame k vs k + 1, window n vs n + 2


def test_materialize_into_and_the_feed_give_one_result(dev):
  """The same draws through DeviceWindows.materialize_into (tables uploaded one by one) and through the feed (tables in the
  arena's block, the launch in after_flush()): bitwise equal, and the restatement within the bound."""
  from geeco_amd import feed
  from geeco_amd.input_fn import DeviceWindows, WindowAugment
  H, W = 12, 16
  fe = H * W * 3
  eps = _episodes(dev, fe)[0]
  rect, col = _rects(H, W)
  streams = {}
  for name, k, tag in (('rgb', K, 0), ('target_rgb', 1, 1)):
    dw = DeviceWindows(k, (H, W, 3), 255.0, squeeze_k=(k == 1))
    for e, st in PICKS:
      dw.add(eps[e], np.asarray([st], np.int32), 255.0 if eps[e].dtype == torch.uint8 else 1.0)
    dw.scene_tag = tag
    streams[name] = dw
  draws = WindowAugment(_shifts(H, W)[1], _colour(), rect, col, KEY, 0.25)
  for dw in streams.values():
    dw.augment = draws
  feats = dict(streams, step=np.zeros((N, 1), np.float32))
  fbuf, lbuf = feed.build_slots(dev, feats, None)
  bufs = {k: fbuf[k].dense() for k in streams}
  assert all(fbuf[k].form == 'dense_augmented' and fbuf[k].scene == 'occlude+noise' for k in streams)
  fbuf, lbuf = feed.adopted_slots(fbuf, lbuf, {})
  feed.feed_step(fbuf, lbuf, feats, None)
  torch.cuda.synchronize()
  for name, dw in streams.items():
    got = bufs[name].cpu().numpy()
    assert np.array_equal(got.view(np.uint32), dw.numpy().view(np.uint32)), name
    want = scene_windows(_plain_values(eps, dw.K, fe).reshape(N, dw.K, H, W, 3), draws.shift, draws.colour, rect, col, KEY, 0.25,
                         dw.scene_tag)
    assert np.abs(got.reshape(want.shape).astype(np.float64) - want).max() <= bound(0.25), name
  direct = _scene(dev, eps, K, H, W, draws.shift, draws.colour, rect, col, KEY, 0.25, 0)
  assert np.array_equal(bufs['rgb'].cpu().numpy().view(np.uint32), direct.view(np.uint32))


def test_argument_checks_return_the_error_code(dev):
  from geeco_amd import _native, ops
  lib = _native.load()
  H, W = 6, 4
  fe = H * W * 3
  ep = _episodes(dev, fe)[0][0]
  addr = torch.tensor([ep.data_ptr(), ep.data_ptr() + fe], dtype=torch.int64, device=dev)
  kind = torch.zeros(2, dtype=torch.int32, device=dev)
  shift = torch.zeros((2, 2), dtype=torch.int32, device=dev)
  col = torch.ones((2, 6), device=dev)
  rect = torch.zeros((2, 4, 4), dtype=torch.int32, device=dev)
  rcol = torch.zeros((2, 4, 3), device=dev)
  key = torch.zeros(2, dtype=torch.int32, device=dev)
  out = torch.full((2, K, H, W, 3), float('nan'), device=dev)
  a, k, s, c, r, rc, ky, o = (t.data_ptr() for t in (addr, kind, shift, col, rect, rcol, key, out))
  call = lib.geeco_gather_windows_scene
  good = (a, k, s, c, r, rc, ky, 0.5, 0, 2, K, H, W, 3, o)
  bad = {0: None, 1: None, 2: None, 14: None}                           # the sibling's null checks
  cases = [good[:i] + (v,) + good[i + 1:] for i, v in bad.items()]
  cases += [good[:13] + (1, o), good[:13] + (4, o),                     # C must be 3
            good[:4] + (None, rc) + good[6:], good[:4] + (r, None) + good[6:],      # the occluder tables come together
            good[:6] + (None,) + good[7:],                              # sigma > 0 without a key
            good[:7] + (1.0,) + good[8:], good[:7] + (-0.5,) + good[8:], good[:7] + (float('nan'),) + good[8:],
            good[:8] + (2,) + good[9:],                                 # tag
            good[:9] + (0,) + good[10:], good[:9] + (65536,) + good[10:], good[:10] + (0,) + good[11:],
            good[:11] + (0,) + good[12:], good[:12] + (0,) + good[13:], good[:14] + (o + 4,),
            good[:4] + (r + 2,) + good[5:], good[:6] + (ky + 1,) + good[7:]]
  for args in cases:
    assert call(*args, None) == _native.GEECO_EINVAL, args
    assert lib.geeco_last_error()
  assert call(*(good[:13] + (1, o)), None) == _native.GEECO_EINVAL and b'C=1' in lib.geeco_last_error()
  torch.cuda.synchronize()
  assert torch.isnan(out).all()                   # nothing was launched
  with pytest.raises(_native.GeecoNativeError, match='C=1'):
    ops.gather_windows_scene_into(out, addr, kind, shift, None, None, None, None, 0.0, 0, 2, K, H, W, 1)
  with pytest.raises(ValueError, match='tables'):
    ops.gather_windows_scene_into(out, addr, kind, shift, col, rect[:1], rcol, key, 0.5, 0, 2, K, H, W, 3)
  with pytest.raises(ValueError, match='come together'):
    ops.gather_windows_scene_into(out, addr, kind, shift, col, rect, None, key, 0.5, 0, 2, K, H, W, 3)
  with pytest.raises(ValueError, match='output of'):
    ops.gather_windows_scene_into(out[:1], addr, kind, shift, col, rect, rcol, key, 0.5, 0, 2, K, H, W, 3)
  assert call(*good, None) == 0 and call(a, k, s, None, None, None, None, 0.0, 1, 2, K, H, W, 3, o, None) == 0
  torch.cuda.synchronize()
  assert not torch.isnan(out).any()


# ================================================================================================
# through the Estimator
# ================================================================================================
HH, K3, BATCH = 136, 3, 4
SCENE = dict(shift=1, noise=0.02, occlude=2)
MODELS = {'e2e_vmc': (False, dict()), 'geeco_f': (True, dict(proc_obs='dynimg', proc_tgt='dyndiff'))}


@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
  from geeco_amd import input_fn as I
  root = str(tmp_path_factory.mktemp('augment_scene_ds'))
  I.write_synthetic_dataset(root, 1, episode_length=11, img_hw=(HH, HH), seed=9)
  return root


def _batches(root, goal, augment):
  from geeco_amd import input_fn as I
  return list(I.pickplace_input_fn(root, 'default', 'train', window_size=K3, batch_size=BATCH, num_threads=2, seed=3, device='cuda',
                                   device_keys=('rgb',), cache=False, fetch_target=goal, augment=augment))[:2]


def _values_of(dw):
  """float64 [n][K][H][W][3]: the plain windows of a DeviceWindows as real numbers, from its resident segments."""
  out = []
  for frames, starts, div in dw.segments:
    fr = frames.cpu().numpy().astype(np.float64) / div
    out += [fr[s:s + dw.K] for s in starts]
  return np.stack(out).reshape((dw.n, dw.K) + dw.frame_shape)


def _train(name, batches):
  from geeco_amd import estimator as est
  from geeco_amd.params import create_e2evmc_config
  goal, kw = MODELS[name]
  cfg = create_e2evmc_config(dict(kw, window_size=K3, img_height=HH, img_width=HH, batch_size=BATCH))
  e = est.Estimator(est.goal_e2evmc_model_fn if goal else est.e2evmc_model_fn, None, est.RunConfig(init_seed=4),
                    {'e2evmc_config': cfg, 'log_steps': 10 ** 9})
  e.train(input_fn=lambda: iter(batches))
  torch.cuda.synchronize()
  (key, (spec, fbuf, lbuf)), = e._specs.items()
  assert int(e._store.global_step.item()) == len(batches) and np.isfinite(float(spec.model.loss))
  return key, spec, fbuf


@pytest.mark.parametrize('name', list(MODELS))
def test_estimator_trains_on_scene_augmented_windows(dev, dataset, name):
  """Two steps under dict(shift=1, noise=0.02, occlude=2): a finite loss, and the image inputs the second step read are the
  restatement of the second batch's draws."""
  goal = MODELS[name][0]
  batches = _batches(dataset, goal, SCENE)
  assert len(batches) == 2 and all(f['rgb'].augment.scene == 'occlude+noise' for f, _ in batches)
  key, spec, fbuf = _train(name, batches)
  assert key[-2:] == ('augmented', 'scene:occlude+noise')
  feats = batches[-1][0]
  draws = feats['rgb'].augment
  assert (draws.occ_rect[..., 2] > 0).any()
  for k, tag in (('rgb', 0), ('target_rgb', 1)) if goal else (('rgb', 0),):
    assert fbuf[k].form == 'dense_augmented' and fbuf[k].scene == 'occlude+noise'
    got = spec.model.inputs[k].cpu().numpy()
    want = scene_windows(_values_of(feats[k]), draws.shift, draws.colour, draws.occ_rect, draws.occ_colour, draws.noise_key,
                         draws.sigma, tag).reshape(got.shape)
    err = np.abs(got.astype(np.float64) - want).max()
    print('%s %s: worst |err| %.3g' % (name, k, err))
    assert err <= bound(draws.sigma), (k, err)
  spec.model.check_device_errors()


@pytest.mark.parametrize('name', list(MODELS))
def test_with_the_new_keys_off_the_fed_buffer_is_the_merged_gather(dev, dataset, name):
  from geeco_amd import ops
  goal = MODELS[name][0]
  batches = _batches(dataset, goal, dict(shift=1, noise=0.0, occlude=0))
  key, spec, fbuf = _train(name, batches)
  assert key[-1] == 'augmented'
  feats = batches[-1][0]
  for k in ('rgb', 'target_rgb') if goal else ('rgb',):
    dw = feats[k]
    assert fbuf[k].scene is None and dw.scene_tables() is None and dw.augment.scene is None
    addr, kinds = dw.window_table(dev)
    shift, colour = dw.augment_tables()
    want = torch.full((dw.n, dw.K) + dw.frame_shape, float('nan'), device=dev)
    up = lambda a: torch.from_numpy(a).to(dev)
    ops.gather_windows_augmented_into(want, up(addr), up(kinds), up(shift), up(colour), dw.n, dw.K, *dw.frame_shape)
    torch.cuda.synchronize()
    got = spec.model.inputs[k].cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.cpu().numpy().reshape(got.shape).view(np.uint32)), k
