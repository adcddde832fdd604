"""Time augmentation, host side: the validator and the draws of pickplace_input_fn(augment=dict(frame_drop=,
frame_lag=)), what the keys leave alone, DeviceWindows.frame_addresses with its clamp and its bounds check, and the feed slot's
'dense_frames' form against a recording arena.  No GPU: the device path runs with device='cpu'."""
import numpy as np
import pytest
import torch

from _augment_time_ref import compose, slot_frame_indices
from _fake_frames import FE, FakeFrames, RecordingArena
from geeco_amd import input_fn as I
from geeco_amd.input_fn import DeviceWindows, WindowAugment, WindowFeed

EPISODES, EP_LEN, K, BATCH, HW = 3, 8, 3, 4, 16
AUG = dict(shift=3, gain=0.25, bias=0.125)
SCENE = dict(noise=0.05, occlude=3, occlude_size=0.5)
TIME = dict(frame_drop=0.5, frame_lag=2)
STATES = ('step', 'goal_state', 'jnt_state')


@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
  root = str(tmp_path_factory.mktemp('augment_time_ds'))
  I.write_synthetic_dataset(root, EPISODES, episode_length=EP_LEN, img_hw=(HW, HW), seed=2)
  return root


def _run(root, mode='train', **kw):
  kw = dict(dict(window_size=K, batch_size=BATCH, seed=3, num_threads=2, fetch_target=True, device='cpu', cache=False), **kw)
  return list(I.pickplace_input_fn(root, 'default', mode, **kw))


def _same_windows(a, b):
  assert len(a) == len(b)
  for (fa, la), (fb, lb) in zip(a, b):
    for k in fa:
      if isinstance(fa[k], DeviceWindows):
        assert len(fa[k].segments) == len(fb[k].segments) and fa[k].scattered == fb[k].scattered
        for (ta, sa, da), (tb, sb, db) in zip(fa[k].segments, fb[k].segments):
          assert torch.equal(ta, tb) and np.array_equal(sa, sb) and da == db, k
      else:
        assert np.array_equal(fa[k], fb[k]), k
    for k in la:
      assert np.array_equal(la[k], lb[k]), k


# ================================================================================================
# the validator
# ================================================================================================
def test_validator_accepts():
  assert I.check_augment_time(None) is None and I.check_augment_time({}) is None
  assert I.check_augment_time(dict(frame_lag=0, frame_drop=0.0)) is None
  assert I.check_augment_time(dict(shift=2, noise=0.1)) is None                       # the other keys are not its business
  assert I.check_augment_time(dict(frame_lag=2)) == (2, 0.0)
  assert I.check_augment_time(dict(frame_drop=0.25)) == (0, 0.25)
  assert I.check_augment_time(dict(frame_lag=np.int64(3), frame_drop=np.float32(0.5)), K=4) == (3, 0.5)
  assert I.check_augment_time(dict(frame_drop=0)) is None
  # K == 1: nothing to drop -- accepted, a no-op; the lag still applies
  assert I.check_augment_time(dict(frame_drop=0.5), K=1) is None
  assert I.check_augment_time(dict(frame_drop=0.5, frame_lag=2), K=1) == (2, 0.0)


@pytest.mark.parametrize('bad,key', [
    (dict(frame_lag=-1), 'frame_lag'), (dict(frame_lag=True), 'frame_lag'), (dict(frame_lag=1.0), 'frame_lag'),
    (dict(frame_lag=float('nan')), 'frame_lag'), (dict(frame_lag='2'), 'frame_lag'),
    (dict(frame_drop=-0.1), 'frame_drop'), (dict(frame_drop=1.0), 'frame_drop'), (dict(frame_drop=1), 'frame_drop'),
    (dict(frame_drop=True), 'frame_drop'), (dict(frame_drop=float('nan')), 'frame_drop'), (dict(frame_drop='0.5'), 'frame_drop')],
    ids=lambda v: repr(v) if isinstance(v, dict) else v)
def test_bad_values_are_refused_by_name(dataset, bad, key):
  with pytest.raises(ValueError, match=r"augment\['%s'\]" % key):
    I.check_augment_time(bad)
  with pytest.raises(ValueError, match=r"augment\['%s'\]" % key):
    I.pickplace_input_fn(dataset, 'default', 'train', window_size=K, batch_size=BATCH, seed=3, device='cpu', cache=False, augment=bad)


def test_unknown_key_message_names_the_new_keys():
  assert I.check_augment(dict(frame_drop=0.5, frame_lag=1)) is None                   # known to it, and not shift / gain / bias
  assert I.check_augment_scene(dict(frame_drop=0.5, frame_lag=1)) is None
  with pytest.raises(ValueError, match="'frame_drop' and 'frame_lag'"):
    I.check_augment(dict(frame_skip=1))
  with pytest.raises(ValueError, match='unknown key'):
    I.check_augment_scene(dict(frame_lags=1))


# ================================================================================================
# the draws
# ================================================================================================
def test_draw_shape_dtype_and_documented_order():
  n, K8, L, p = 64, 8, 3, 0.5
  src = I.draw_augment_time(np.random.default_rng(7), n, K8, L, p)
  assert src.shape == (n, K8) and src.dtype == np.int32
  r = np.random.default_rng(7)
  d = r.integers(0, L + 1, size=n)                                    # first the n lags ...
  drop = r.random((n, K8 - 1)) < p                                    # ... then the [n][K - 1] block of uniforms
  want = np.asarray([compose(K8, d[i], {k + 1 for k in np.flatnonzero(drop[i])}) for i in range(n)])
  assert np.array_equal(src, want)
  assert np.array_equal(src[:, 0], -d)
  assert (np.diff(src, axis=1) >= 0).all()
  assert (src <= np.arange(K8)[None, :]).all() and (src >= -L).all()


def test_draws_that_are_off_give_consecutive_frames():
  for n, k in ((1, 1), (5, 4), (3, 8)):
    assert np.array_equal(I.draw_augment_time(np.random.default_rng(0), n, k, 0, 0.0), np.tile(np.arange(k), (n, 1)))
  assert I.draw_augment_time(np.random.default_rng(0), 4, 1, 2, 0.0).shape == (4, 1)      # K == 1: the lag alone


def test_composition_on_a_hand_written_case():
  """Lag 2 with drops at slots 2 and 3: the lagged sequence -2, -1, 0, 1, 2, 3 with slots 2 and 3 repeating slot 1."""
  assert compose(6, 2, {2, 3}) == [-2, -1, -1, -1, 2, 3]

  class Fixed:       # a generator that hands out exactly these draws, in the documented order
    def integers(self, lo, hi, size):
      assert (lo, hi, size) == (0, 3, 1)
      return np.asarray([2])

    def random(self, shape):
      assert shape == (1, 5)
      return np.asarray([[0.9, 0.1, 0.2, 0.8, 0.7]])      # < 0.5 at slots 2 and 3

  assert I.draw_augment_time(Fixed(), 1, 6, 2, 0.5).tolist() == [[-2, -1, -1, -1, 2, 3]]


def test_the_draw_fires():
  """A fixed seed at p = 0.5, K = 8, n = 64: both stale and fresh slots, in about equal numbers (448 Bernoulli(0.5) draws: the
  count of stale slots lies within 5 standard deviations, 224 +- 53)."""
  src = I.draw_augment_time(np.random.default_rng(11), 64, 8, 0, 0.5)
  stale = int((src[:, 1:] == src[:, :-1]).sum())
  fresh = int((src[:, 1:] == np.arange(1, 8)[None, :]).sum())
  assert stale + fresh == 64 * 7 and 171 <= stale <= 277, (stale, fresh)
  lag = -I.draw_augment_time(np.random.default_rng(11), 64, 8, 2, 0.0)[:, 0]
  assert sorted(set(lag.tolist())) == [0, 1, 2]


# ================================================================================================
# what the keys leave alone
# ================================================================================================
@pytest.fixture(scope='module')
def time_batches(dataset):
  return _run(dataset, augment=dict(AUG, **SCENE, **TIME))


def test_every_other_draw_the_file_order_and_the_picks_are_those_without_the_keys(dataset, time_batches):
  old = _run(dataset, augment=dict(AUG, **SCENE))
  _same_windows(old, time_batches)                                    # file order, starts, states, labels
  for (fa, _), (fb, _) in zip(old, time_batches):
    a, b = fa['rgb'].augment, fb['rgb'].augment
    for k in ('shift', 'colour', 'occ_rect', 'occ_colour', 'noise_key'):
      assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.frame_src is None and b.frame_src is not None and b.frame_src.shape == (len(fb['step']), K)
    assert fa['rgb'].frame_src is None
  a = _run(dataset, shuffle_windows=True, shuffle_buffer=8, augment=AUG)
  b = _run(dataset, shuffle_windows=True, shuffle_buffer=8, augment=dict(AUG, **TIME))
  _same_windows(a, b)                                                 # the shuffle's picks
  assert all(np.array_equal(fa['rgb'].augment.shift, fb['rgb'].augment.shift) and
             np.array_equal(fa['rgb'].augment.colour, fb['rgb'].augment.colour) for (fa, _), (fb, _) in zip(a, b))
  _same_windows(_run(dataset), time_batches)
  assert any((f['rgb'].frame_src != np.arange(K)[None, :]).any() for f, _ in time_batches)


def test_only_the_camera_streams_of_the_observation_follow_the_sources(dataset, time_batches):
  plain = _run(dataset)
  for (f, l), (fp, lp) in zip(time_batches, plain):
    src = f['rgb'].augment.frame_src
    assert f['rgb'].timed and f['depth'].timed and f['rgb'].frame_src is src and f['depth'].frame_src is src
    for k in ('target_rgb', 'target_depth'):
      assert f[k].augment is f['rgb'].augment and not f[k].timed and f[k].frame_src is None
      addr, _ = f[k].frame_addresses('cpu')                           # ... and their table is the consecutive one
      assert np.array_equal(addr[:, 0], f[k].window_table('cpu')[0])
    for k in STATES:                                                  # proprioception stays fresh
      assert np.array_equal(f[k], fp[k]), k
    for k in l:
      assert np.array_equal(l[k], lp[k]), k
    # the rgb table follows the sources, clamped at the episode's first frame
    addr, kinds = f['rgb'].frame_addresses('cpu')
    first, _ = f['rgb'].window_table('cpu')
    starts = np.concatenate([s for _, s, _ in f['rgb'].segments])
    fe = int(np.prod(f['rgb'].frame_shape))
    assert np.array_equal(addr, (first - starts * fe)[:, None] + slot_frame_indices(starts, src) * fe) and not kinds.any()


def test_a_single_key_is_enough_and_the_draws_are_reproducible(dataset, time_batches):
  for one in (dict(frame_lag=1), dict(frame_drop=0.5)):
    b = _run(dataset, augment=one)
    aug = b[0][0]['rgb'].augment
    assert aug.frame_src is not None and not aug.shift.any() and aug.scene is None
    assert np.array_equal(aug.colour, np.tile([1, 1, 1, 0, 0, 0], (len(aug), 1)))      # the neutral row
  again = _run(dataset, augment=dict(AUG, **SCENE, **TIME))
  assert all(np.array_equal(fa['rgb'].frame_src, fb['rgb'].frame_src) for (fa, _), (fb, _) in zip(time_batches, again))
  other = _run(dataset, augment=dict(AUG, **SCENE, **TIME), seed=4)
  assert not all(np.array_equal(fa['rgb'].frame_src, fb['rgb'].frame_src) for (fa, _), (fb, _) in zip(time_batches, other))


def test_the_host_path_is_refused_and_other_modes_ignore_the_keys(dataset):
  for aug in (TIME, dict(frame_lag=1), dict(frame_drop=0.5)):
    with pytest.raises(ValueError, match='device='):
      _run(dataset, device=None, augment=aug)
  assert isinstance(_run(dataset, device=None, augment=dict(frame_lag=0, frame_drop=0.0))[0][0]['rgb'], np.ndarray)
  assert isinstance(_run(dataset, mode='eval', device=None, augment=TIME)[0][0]['rgb'], np.ndarray)
  ev = _run(dataset, mode='eval', augment=TIME)
  assert all(f['rgb'].augment is None and f['rgb'].frame_src is None for f, _ in ev)


def test_a_window_of_one_frame_takes_the_lag_alone(dataset):
  b = _run(dataset, window_size=1, augment=dict(frame_drop=0.5))
  assert all(f['rgb'].augment is None for f, _ in b)                  # nothing to drop: off
  b = _run(dataset, window_size=1, augment=TIME)
  src = np.concatenate([f['rgb'].frame_src for f, _ in b])
  assert src.shape[1] == 1 and src.min() == -2 and src.max() == 0


# ================================================================================================
# DeviceWindows.frame_addresses
# ================================================================================================
def _fake(src, starts=(0, 4, 1), T=9, dtype=torch.uint8, div=255.0, base=1 << 20, timed=True):
  dw = DeviceWindows(3, (4, 6, 3), div)
  dw.add(FakeFrames(base, T, dtype, device='cpu'), np.asarray(starts, np.int32))
  n = len(starts)
  dw.augment = WindowAugment(np.zeros((n, 2)), np.tile([1, 1, 1, 0, 0, 0], (n, 1)), frame_src=src)
  dw.timed = timed
  return dw


def test_frame_addresses_follow_the_sources_and_clamp_at_frame_zero():
  src = np.asarray([[-2, -1, -1], [-3, -3, 2], [0, 0, 0]], np.int32)
  addr, kinds = _fake(src).frame_addresses('cpu')
  assert addr.dtype == np.int64 and addr.shape == (3, 3) and kinds.dtype == np.int32 and kinds.tolist() == [0, 0, 0]
  want = [[0, 0, 0], [1, 1, 6], [1, 1, 1]]                            # max(start + src, 0)
  assert np.array_equal(addr, (1 << 20) + np.asarray(want) * FE)
  addr, kinds = _fake(src, dtype=torch.float32, div=1.0).frame_addresses('cpu')
  assert np.array_equal(addr, (1 << 20) + np.asarray(want) * FE * 4) and kinds.tolist() == [1, 1, 1]
  # without sources, and for a stream that does not follow them: the consecutive table
  for dw in (_fake(None), _fake(src, timed=False)):
    assert dw.frame_src is None
    addr, _ = dw.frame_addresses('cpu')
    assert np.array_equal(addr, (1 << 20) + (np.asarray([0, 4, 1])[:, None] + np.arange(3)[None, :]) * FE)


def test_frame_addresses_check_every_frame_on_the_host():
  with pytest.raises(IndexError, match='outside the 7 resident frames'):
    _fake(np.asarray([[0, 1, 2], [0, 1, 3], [0, 0, 0]]), T=7).frame_addresses('cpu')      # 4 + 3 = frame 7 of 7
  _fake(np.asarray([[0, 1, 2], [0, 1, 2], [0, 0, 0]]), T=7).frame_addresses('cpu')        # frame 6: the last one
  with pytest.raises(IndexError):
    _fake(np.asarray([[0, 1, 2 ** 31 - 1], [0, 0, 0], [0, 0, 0]])).frame_addresses('cpu')  # no int32 wrap-around in the sum
  with pytest.raises(ValueError, match='frame_src of shape'):
    _fake(np.zeros((3, 2), np.int32)).frame_addresses('cpu')
  with pytest.raises(ValueError, match='frame_src of shape'):
    WindowAugment(np.zeros((3, 2)), np.zeros((3, 6)), frame_src=np.zeros((2, 3)))
  with pytest.raises(ValueError, match='multiple of 4'):
    _fake(None, dtype=torch.float32, div=1.0, base=(1 << 20) + 2).frame_addresses('cpu')
  with pytest.raises(ValueError, match='neither'):
    _fake(None, dtype=torch.float32, div=255.0).frame_addresses('cpu')
  dw = _fake(np.zeros((3, 3), np.int32))
  with pytest.raises(ValueError, match='augmented windows'):          # --shared_frames stays excluded
    dw.frame_table(8, device='cpu')
  with pytest.raises(ValueError, match='augmented windows'):
    dw.addresses('cpu')


# ================================================================================================
# the feed slot and materialize_into
# ================================================================================================
OCC = dict(occ_rect=np.arange(48).reshape(3, 4, 4), occ_colour=np.arange(36).reshape(3, 4, 3) / 36.0)
NOISE = dict(sigma=0.25, noise_key=[0xdeadbeef, 7])
SRC = np.asarray([[0, 0, 1], [-1, 0, 0], [-2, -1, 0]], np.int32)


def _fake_stream(extras, C=3, src=SRC):
  dw = DeviceWindows(3, (4, 6, C), 255.0)
  dw.add(FakeFrames(1 << 20, 9, device='cpu'), np.asarray([0, 4, 1], np.int32))
  dw.augment = WindowAugment([[1, -2], [0, 0], [-3, 5]], np.arange(18, dtype=np.float32).reshape(3, 6), frame_src=src, **extras)
  dw.timed = True
  return dw


@pytest.mark.parametrize('extras', [{}, OCC, dict(OCC, **NOISE)], ids=['plain', 'occlude', 'both'])
@pytest.mark.parametrize('C', [3, 1])
def test_feed_slot_takes_the_dense_frames_form(monkeypatch, extras, C):
  from geeco_amd import ops
  calls = []
  for name in ('gather_windows_frames_into', 'gather_windows_scene_into', 'gather_windows_augmented_into', 'gather_windows_by_address_into'):
    monkeypatch.setattr(ops, name, lambda *a, name=name: calls.append((name,) + a))
  dw = _fake_stream(extras, C)
  log, key = [], ('features', 'rgb' if C == 3 else 'depth')
  arena = RecordingArena(log)
  slot = WindowFeed(dw, arena, key)
  assert slot.frames and slot.augmented and not slot.u8
  extras = extras if C == 3 else {}                                   # a one-channel stream: shift only
  want = ['window_addr', 'window_kind', 'aug_shift'] + (['aug_colour'] if C == 3 else []) + \
      (['aug_occ_rect', 'aug_occ_colour'] if 'occ_rect' in extras else []) + (['aug_noise_key'] if 'sigma' in extras else [])
  assert [k[-1] for k in arena.layout] == want
  assert arena.layout[key + ('window_addr',)] == ((3, 3), np.dtype(np.int64))       # one address per FRAME, in the step's one block
  slot.form, slot.buffer = 'dense_frames', 'buffer'
  slot.feed(dw)
  assert [e[1] for e in log if e[0] == 'write'] == want and slot._gather_pending and not calls
  assert np.array_equal(arena.values[key + ('window_addr',)], dw.frame_addresses('cpu')[0])
  arena.seal()
  slot.after_flush()
  assert len(calls) == 1 and not slot._gather_pending                 # ONE launch per stream, as 'dense_augmented'
  view = lambda name: ('view',) + key + (name,)
  assert calls[0] == ('gather_windows_frames_into', 'buffer', view('window_addr'), view('window_kind'), view('aug_shift'),
                      view('aug_colour') if C == 3 else None, view('aug_occ_rect') if 'occ_rect' in extras else None,
                      view('aug_occ_colour') if 'occ_rect' in extras else None, view('aug_noise_key') if 'sigma' in extras else None,
                      extras.get('sigma', 0.0), 0, 3, 3, 4, 6, C)
  # a batch without sources in this slot sends the consecutive table
  plain = _fake_stream(extras, C, src=None)
  slot.feed(plain)
  assert np.array_equal(arena.values[key + ('window_addr',)], (1 << 20) + (np.asarray([0, 4, 1])[:, None] + np.arange(3)) * 4 * 6 * C)


def test_a_batch_with_sources_in_a_slot_built_without_them_is_an_error():
  arena = RecordingArena([])
  slot = WindowFeed(_fake_stream({}, src=None), arena, ('features', 'rgb'))
  assert not slot.frames and arena.layout[('features', 'rgb', 'window_addr')] == ((3,), np.dtype(np.int64))
  slot.form, slot.buffer = 'dense_augmented', 'buffer'
  with pytest.raises(RuntimeError, match='frame sources'):
    slot.feed(_fake_stream({}))


@pytest.mark.parametrize('extras', [{}, dict(OCC, **NOISE)], ids=['plain', 'both'])
def test_materialize_into_takes_the_new_launch(monkeypatch, extras):
  from geeco_amd import ops
  calls = []
  for name in ('gather_windows_frames_into', 'gather_windows_scene_into', 'gather_windows_augmented_into'):
    monkeypatch.setattr(ops, name, lambda *a, name=name: calls.append((name, a)))
  dw = _fake_stream(extras)
  dw.segments = [(torch.zeros((9, 72), dtype=torch.uint8), dw.segments[0][1], 255.0)]
  out = torch.empty((3, 3, 4, 6, 3))
  dw.materialize_into(out)
  (name, a), = calls
  assert name == 'gather_windows_frames_into' and a[0] is out
  assert np.array_equal(a[1].numpy(), dw.frame_addresses('cpu')[0]) and a[1].shape == (3, 3)
  assert np.array_equal(a[3].numpy(), dw.augment.shift) and a[9:] == (0, 3, 3, 4, 6, 3)
  assert (a[5] is None) == ('occ_rect' not in extras) and a[8] == extras.get('sigma', 0.0)
