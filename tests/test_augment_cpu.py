"""Window augmentation, host side: the draws of pickplace_input_fn(augment=...), what the option leaves alone, its
refusals, the feed slot's 'dense_augmented' form against a recording arena, and the known answers of tests/_augment_ref.py.
No GPU: the device path runs with device='cpu' (resident frames as host tensors; nothing is gathered here)."""
import numpy as np
import pytest
import torch

from _augment_ref import augment_windows, in_view, moved
from _fake_frames import FakeFrames, RecordingArena, windows as fake_windows
from geeco_amd import input_fn as I
from geeco_amd.input_fn import DeviceWindows, WindowAugment, WindowFeed

EPISODES, EP_LEN, K, BATCH, HW = 3, 8, 3, 4, 16
NWIN = EP_LEN - 1 - K + 1
AUG = dict(shift=3, gain=0.25, bias=0.125)
STREAMS = ('rgb', 'target_rgb', 'depth', 'target_depth')


@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
  root = str(tmp_path_factory.mktemp('augment_ds'))
  I.write_synthetic_dataset(root, EPISODES, episode_length=EP_LEN, img_hw=(HW, HW), seed=2)
  return root


def _run(root, mode='train', **kw):
  kw = dict(dict(window_size=K, batch_size=BATCH, seed=3, num_threads=2, fetch_target=True, device='cpu', cache=False), **kw)
  return list(I.pickplace_input_fn(root, 'default', mode, **kw))


@pytest.fixture(scope='module')
def plain(dataset):
  return _run(dataset)


@pytest.fixture(scope='module')
def augmented(dataset):
  return _run(dataset, augment=AUG)


def _draws(batches):
  return [f['rgb'].augment for f, _ in batches]


def _same_batches(a, b):
  """States, labels and the windows' (frames, starts, divisor) segments, bitwise."""
  assert len(a) == len(b)
  for (fa, la), (fb, lb) in zip(a, b):
    assert set(fa) == set(fb) and set(la) == set(lb)
    for k in fa:
      if isinstance(fa[k], DeviceWindows):
        assert (fa[k].K, fa[k].frame_shape, fa[k].squeeze_k, fa[k].scattered, len(fa[k].segments)) == \
            (fb[k].K, fb[k].frame_shape, fb[k].squeeze_k, fb[k].scattered, len(fb[k].segments)), k
        for (ta, sa, da), (tb, sb, db) in zip(fa[k].segments, fb[k].segments):
          assert torch.equal(ta, tb) and ta.dtype == tb.dtype and np.array_equal(sa, sb) and da == db, k
      else:
        assert fa[k].dtype == fb[k].dtype and np.array_equal(fa[k], fb[k]), k
    for k in la:
      assert la[k].dtype == lb[k].dtype and np.array_equal(la[k], lb[k]), k


# ================================================================================================
# the draws
# ================================================================================================
def test_every_stream_of_a_batch_references_one_draw_object(augmented):
  assert len(augmented) == -(-EPISODES * NWIN // BATCH)
  for f, _ in augmented:
    aug = f['rgb'].augment
    assert isinstance(aug, WindowAugment) and all(f[k].augment is aug and f[k].augmented for k in STREAMS)
    n = len(f['step'])
    assert aug.shift.shape == (n, 2) and aug.shift.dtype == np.int32 and aug.colour.shape == (n, 6) and aug.colour.dtype == np.float32
    # RGB streams take the colour, one-channel streams only the shift
    assert f['rgb'].augment_tables()[1] is aug.colour and f['target_rgb'].augment_tables()[1] is aug.colour
    assert f['depth'].augment_tables() == (aug.shift, None) and f['target_depth'].augment_tables() == (aug.shift, None)
  assert len({id(a) for a in _draws(augmented)}) == len(augmented)        # a batch has its own


def test_draws_lie_in_their_ranges_and_use_them(augmented):
  shift = np.concatenate([a.shift for a in _draws(augmented)])
  colour = np.concatenate([a.colour for a in _draws(augmented)])
  S, g, b = AUG['shift'], AUG['gain'], AUG['bias']
  assert shift.min() >= -S and shift.max() <= S and len(np.unique(shift)) > 3
  gain, bias = colour[:, :3], colour[:, 3:]
  assert gain.min() >= 1 - g and gain.max() <= 1 + g and bias.min() >= -b and bias.max() <= b
  assert gain.max() - gain.min() > g / 2 and bias.max() - bias.min() > b / 2
  assert not np.array_equal(gain[:, 0], gain[:, 1])                       # per channel


def test_draws_are_reproducible_and_differ_between_ranks_and_seeds(dataset, augmented):
  again = _run(dataset, augment=AUG)
  for a, b in zip(_draws(augmented), _draws(again)):
    assert np.array_equal(a.shift, b.shift) and np.array_equal(a.colour, b.colour)
  other = _run(dataset, augment=AUG, seed=4)
  assert not np.array_equal(_draws(augmented)[0].colour, _draws(other)[0].colour)
  per_rank = []
  for r in range(2):
    a = _run(dataset, augment=AUG, shard=(r, 2))
    b = _run(dataset, augment=AUG, shard=(r, 2))
    assert all(np.array_equal(x.shift, y.shift) and np.array_equal(x.colour, y.colour) for x, y in zip(_draws(a), _draws(b)))
    per_rank.append(_draws(a)[0])
  assert not np.array_equal(per_rank[0].colour, per_rank[1].colour)
  # rank 0 of a sharded run draws from the stream of an unsharded run (the generator is default_rng([seed, rank, constant]))
  assert np.array_equal(per_rank[0].colour, _draws(augmented)[0].colour)
  want = I.draw_augment(np.random.default_rng([3, 0, I.AUGMENT_STREAM]), BATCH, AUG['shift'], AUG['gain'], AUG['bias'])
  assert np.array_equal(want.shift, _draws(augmented)[0].shift) and np.array_equal(want.colour, _draws(augmented)[0].colour)


def test_a_single_option_is_enough(dataset):
  for aug in (dict(shift=2), dict(gain=0.5), dict(bias=0.25), dict(shift=0, gain=0.0, bias=0.5)):
    draws = _draws(_run(dataset, augment=aug))
    assert all(d is not None for d in draws)
    shift, colour = np.concatenate([d.shift for d in draws]), np.concatenate([d.colour for d in draws])
    assert (shift != 0).any() == bool(aug.get('shift'))
    assert (colour[:, :3] != 1).any() == bool(aug.get('gain')) and (colour[:, 3:] != 0).any() == bool(aug.get('bias'))


# ================================================================================================
# what the option leaves alone
# ================================================================================================
def test_file_order_states_and_labels_are_those_without_the_option(plain, augmented):
  _same_batches(plain, augmented)
  assert all(f[k].augment is None and not f[k].augmented for f, _ in plain for k in STREAMS)


def test_shuffle_picks_are_those_without_the_option(dataset):
  a = _run(dataset, shuffle_windows=True, shuffle_buffer=8)
  b = _run(dataset, shuffle_windows=True, shuffle_buffer=8, augment=AUG)
  _same_batches(a, b)
  assert all(f['rgb'].scattered and f['rgb'].augmented for f, _ in b)
  # ... and the draws are those of the unshuffled run: one stream, drawn per emitted batch
  for x, y in zip(_draws(b), _draws(_run(dataset, augment=AUG))):
    assert np.array_equal(x.shift, y.shift) and np.array_equal(x.colour, y.colour)


@pytest.mark.parametrize('off', [None, dict(shift=0, gain=0.0, bias=0.0), dict(shift=0), {}], ids=['none', 'zeros', 'shift0', 'empty'])
def test_off_is_bitwise_today(dataset, plain, off):
  got = _run(dataset, augment=off)
  _same_batches(plain, got)
  assert all(f[k].augment is None for f, _ in got for k in STREAMS)


def test_other_modes_ignore_the_option(dataset):
  a, b = _run(dataset, mode='eval'), _run(dataset, mode='eval', augment=AUG)
  _same_batches(a, b)
  assert all(f[k].augment is None for f, _ in b for k in STREAMS)
  # ... also on the host path, where 'train' refuses it
  host = _run(dataset, mode='eval', device=None, augment=AUG)
  assert isinstance(host[0][0]['rgb'], np.ndarray)


def test_synthetic_inputs_ignore_the_option():
  a = list(I.pickplace_input_fn('synthetic:2:16x16', None, 'train', window_size=K, batch_size=2, seed=1))
  b = list(I.pickplace_input_fn('synthetic:2:16x16', None, 'train', window_size=K, batch_size=2, seed=1, augment=AUG))
  assert len(a) == len(b) == 2
  for (f, _), (fp, _) in zip(b, a):
    assert np.array_equal(f['rgb'], fp['rgb'])


# ================================================================================================
# refusals
# ================================================================================================
@pytest.mark.parametrize('bad,key', [
    (dict(shift=-1), 'shift'), (dict(shift=1.5), 'shift'), (dict(shift=HW), 'shift'), (dict(shift=True), 'shift'),
    (dict(gain=1.0), 'gain'), (dict(gain=-0.1), 'gain'), (dict(gain=float('nan')), 'gain'), (dict(gain='0.1'), 'gain'),
    (dict(bias=-0.5), 'bias'), (dict(bias=float('inf')), 'bias'), (dict(bias=None), 'bias'),
    (dict(shift=1, rotate=3), 'rotate'), (3, 'dict')])
def test_bad_values_are_refused_by_name(dataset, bad, key):
  with pytest.raises(ValueError, match=key):
    I.pickplace_input_fn(dataset, 'default', 'train', window_size=K, batch_size=BATCH, seed=3, device='cpu', cache=False, augment=bad)


def test_the_largest_shift_is_one_short_of_the_frame(dataset):
  assert I.check_augment(dict(shift=HW - 1), (HW, HW)) == (HW - 1, 0.0, 0.0)
  assert I.check_augment(dict(shift=np.int64(2), gain=np.float32(0.5)), (HW, 2 * HW)) == (2, 0.5, 0.0)
  with pytest.raises(ValueError, match='shift'):
    I.check_augment(dict(shift=HW), (2 * HW, HW))


def test_the_host_path_is_refused(dataset):
  with pytest.raises(ValueError, match='device='):
    I.pickplace_input_fn(dataset, 'default', 'train', window_size=K, batch_size=BATCH, seed=3, augment=AUG)
  # off: nothing to refuse
  assert len(list(I.pickplace_input_fn(dataset, 'default', 'train', window_size=K, batch_size=BATCH, seed=3, num_threads=2,
                                       augment=dict(shift=0)))) == -(-EPISODES * NWIN // BATCH)


def test_augmented_windows_offer_neither_addresses_nor_shared_frames():
  dw = fake_windows([(FakeFrames(1 << 20, 9), [0, 1], 255.0)])
  dw.augment = WindowAugment(np.zeros((2, 2)), np.tile([1, 1, 1, 0, 0, 0], (2, 1)))
  with pytest.raises(ValueError, match='augmented'):
    dw.addresses('cuda:0')
  with pytest.raises(ValueError, match='augmented'):
    dw.frame_table(8, device='cuda:0')
  with pytest.raises(ValueError, match='augmented'):
    DeviceWindows.concat(dw, dw)
  dw.augment = WindowAugment(np.zeros((3, 2)), np.zeros((3, 6)))
  with pytest.raises(ValueError, match='3 windows'):
    dw.augment_tables()
  with pytest.raises(ValueError, match='shifts'):
    WindowAugment(np.zeros((3, 2)), np.zeros((2, 6)))


# ================================================================================================
# the feed slot (feed.WindowFeed 'dense_augmented') against a recording arena
# ================================================================================================
def _augmented_fake(scattered=False):
  from _fake_frames import FE, SHAPE
  a, b = FakeFrames(1 << 20, 9, device='cpu'), FakeFrames(1 << 22, 9, dtype=torch.float32, device='cpu')
  dw = fake_windows([(a, [0, 4], 255.0), (b, [2], 1.0)])
  dw.scattered = scattered
  dw.augment = WindowAugment([[1, -2], [0, 0], [-3, 5]], np.arange(18, dtype=np.float32).reshape(3, 6))
  return dw, [(1 << 20), (1 << 20) + 4 * FE, (1 << 22) + 2 * FE * 4]


@pytest.mark.parametrize('scattered', [False, True])
def test_feed_slot_takes_the_dense_augmented_form(scattered):
  dw, addr = _augmented_fake(scattered=scattered)
  assert dw.is_u8() is False          # (mixed kinds) ... and a uint8-only batch is not offered as addresses either:
  u8 = fake_windows([(FakeFrames(1 << 20, 9, device='cpu'), [0, 1, 2], 255.0)])
  assert u8.is_u8()
  u8.augment = dw.augment
  log = []
  arena = RecordingArena(log)
  slot = WindowFeed(u8, arena, ('features', 'rgb'))
  assert slot.augmented and not slot.u8 and not arena.has(('features', 'rgb'))
  with pytest.raises(RuntimeError, match='not uint8'):
    slot.pointers()
  arena = RecordingArena(log)
  slot = WindowFeed(dw, arena, ('features', 'rgb'))
  key = ('features', 'rgb')
  assert arena.layout == {key + ('window_addr',): ((3,), np.dtype(np.int64)), key + ('window_kind',): ((3,), np.dtype(np.int32)),
                          key + ('aug_shift',): ((3, 2), np.dtype(np.int32)), key + ('aug_colour',): ((3, 6), np.dtype(np.float32))}
  slot.form = 'dense_augmented'       # (dense() allocates a device buffer: chosen by hand here)
  slot.feed(dw)
  assert [e for e in log if e[0] == 'write'] == [('write', 'window_addr'), ('write', 'window_kind'), ('write', 'aug_shift'),
                                                 ('write', 'aug_colour')]
  assert arena.values[key + ('window_addr',)].tolist() == addr and arena.values[key + ('window_kind',)].tolist() == [0, 0, 1]
  assert arena.values[key + ('aug_shift',)].tolist() == [[1, -2], [0, 0], [-3, 5]]
  assert np.array_equal(arena.values[key + ('aug_colour',)], dw.augment.colour)
  assert slot._gather_pending                                            # the launch itself waits for after_flush()
  # a plain batch in this slot (or an augmented one in a plain slot) is an error, not a silently different transform
  plain = fake_windows([(FakeFrames(1 << 20, 9, device='cpu'), [0, 1, 2], 255.0)])
  with pytest.raises(RuntimeError, match='plain windows in a slot built for augmented'):
    slot.feed(plain)
  other = WindowFeed(plain, RecordingArena([]), key)
  other.form = 'dense'
  with pytest.raises(RuntimeError, match='augmented windows in a slot built for plain'):
    other.feed(dw)


def test_one_channel_streams_reserve_no_colour():
  dw = DeviceWindows(1, (4, 6, 1), 1.0, squeeze_k=True)
  dw.add(FakeFrames(1 << 20, 1, dtype=torch.float32, device='cpu'), np.zeros(2, np.int32))
  dw.augment = WindowAugment([[1, 1], [2, 2]], np.ones((2, 6)))
  arena = RecordingArena([])
  slot = WindowFeed(dw, arena, ('features', 'target_depth'))
  assert slot.augmented and arena.has(slot.key + ('aug_shift',)) and not arena.has(slot.key + ('aug_colour',))
  bad = DeviceWindows(1, (4, 6, 4), 1.0)
  bad.add(FakeFrames(1 << 20, 1, dtype=torch.float32, device='cpu'), np.zeros(2, np.int32))
  bad.augment = dw.augment
  with pytest.raises(ValueError, match=r'\[H, W, 3\]'):
    WindowFeed(bad, RecordingArena([]), ('features', 'rgb'))


# ================================================================================================
# the reference helper's own known answers
# ================================================================================================
def _counting(H=3, W=4, C=1):
  return np.arange(1, H * W * C + 1, dtype=np.float64).reshape(H, W, C)


def test_helper_shift_down_by_one_row():
  got = moved(_counting(), 1, 0)[..., 0]
  assert got.tolist() == [[0, 0, 0, 0], [1, 2, 3, 4], [5, 6, 7, 8]]


def test_helper_shift_left_by_two_columns():
  got = moved(_counting(), 0, -2)[..., 0]
  assert got.tolist() == [[3, 4, 0, 0], [7, 8, 0, 0], [11, 12, 0, 0]]
  rgb = moved(_counting(C=3), 0, -2)
  assert rgb[0, 0].tolist() == [7, 8, 9] and rgb[0, 1].tolist() == [10, 11, 12] and not rgb[:, 2:].any()      # channels stay together


def test_helper_mixed_signs_and_dtype():
  img = _counting().astype(np.uint8)
  got = moved(img, -1, 1)
  assert got.dtype == np.uint8 and got[..., 0].tolist() == [[0, 5, 6, 7], [0, 9, 10, 11], [0, 0, 0, 0]]
  assert in_view(3, 4, -1, 1).tolist() == (got[..., 0] != 0).tolist()


@pytest.mark.parametrize('dy,dx', [(3, 0), (-3, 0), (0, 4), (0, -4), (5, 1), (-1, -9)])
def test_helper_out_of_frame_shifts_give_zeros(dy, dx):
  assert not moved(_counting(), dy, dx).any() and not in_view(3, 4, dy, dx).any()
  out = augment_windows(np.ones((1, 2, 3, 4, 3)), [[dy, dx]], [[1, 1, 1, 0.5, 0.5, 0.5]])
  assert out.shape == (1, 2, 3, 4, 3) and not out.any()          # zeros are moved in, not tinted (a bias would show)


def test_helper_colour_clamps_and_leaves_the_fill_alone():
  v = np.full((2, 1, 2, 2, 3), 0.5)
  out = augment_windows(v, [[0, 1], [0, 0]], [[1.5, 1.0, 0.5, 0.3, -0.6, 0.0], [2.0, 1, 1, 0.5, 0, 0]])
  assert out[0, 0, :, 0].tolist() == [[0, 0, 0], [0, 0, 0]]                         # moved in
  np.testing.assert_allclose(out[0, 0, :, 1], [[1.0, 0.0, 0.25]] * 2, rtol=0, atol=1e-15)      # 1.05 -> 1, -0.1 -> 0
  np.testing.assert_allclose(out[1, 0, 0, 0], [1.0, 0.5, 0.5], rtol=0, atol=1e-15)
  assert out.dtype == np.float64
  same = augment_windows(v, [[0, 0], [0, 0]])
  assert np.array_equal(same, v)
