"""Scene augmentation, host side: the generator of tests/_augment_scene_ref.py against published known answers and
its moments, the draws of pickplace_input_fn(augment=dict(noise=, occlude=)), what the keys leave alone, their refusals, and
which entry point the feed slot and materialize_into call.  No GPU: the device path runs with device='cpu'."""
import numpy as np
import pytest
import torch

from _augment_scene_ref import noise_field, normals_of_words, paint, philox4x32_10
from _fake_frames import FakeFrames, RecordingArena, windows as fake_windows
from geeco_amd import input_fn as I
from geeco_amd.input_fn import DeviceWindows, WindowAugment, WindowFeed

EPISODES, EP_LEN, K, BATCH, HW = 3, 8, 3, 4, 16
NWIN = EP_LEN - 1 - K + 1
AUG = dict(shift=3, gain=0.25, bias=0.125)
SCENE = dict(noise=0.05, occlude=3, occlude_size=0.5)
STREAMS = ('rgb', 'target_rgb', 'depth', 'target_depth')


@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
  root = str(tmp_path_factory.mktemp('augment_scene_ds'))
  I.write_synthetic_dataset(root, EPISODES, episode_length=EP_LEN, img_hw=(HW, HW), seed=2)
  return root


def _run(root, mode='train', **kw):
  kw = dict(dict(window_size=K, batch_size=BATCH, seed=3, num_threads=2, fetch_target=True, device='cpu', cache=False), **kw)
  return list(I.pickplace_input_fn(root, 'default', mode, **kw))


def _draws(batches):
  return [f['rgb'].augment for f, _ in batches]


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


def _same_draws(a, b):
  return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ('shift', 'colour', 'occ_rect', 'occ_colour', 'noise_key')) \
      and a.sigma == b.sigma


# ================================================================================================
# the generator
# ================================================================================================
@pytest.mark.parametrize('counter,key,want', [
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])])
def test_philox_known_answers(counter, key, want):
  """The three philox4x32-10 vectors of Random123's kat_vectors."""
  assert philox4x32_10(np.asarray(counter, np.uint64), np.asarray(key, np.uint64)).tolist() == want


def test_philox_is_vectorised_over_counters():
  ctr = np.asarray([[0, 0, 0, 0], [0xffffffff] * 4], np.uint64)
  got = philox4x32_10(ctr, np.asarray([0, 0], np.uint64))
  assert got.shape == (2, 4) and got[0].tolist() == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
  assert got[1].tolist() != [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]      # (that answer belongs to the all-ones KEY)


def test_normals_have_the_moments_of_a_standard_normal():
  """65 536 normals of one fixed key: |mean| <= 0.02 = 5 / sqrt(65536) and |variance - 1| <= 0.03 ~ 5 sqrt(2 / 65536)."""
  z = noise_field([0x12345678, 0x9abcdef0], 0, 2, 2, 16384)
  assert z.shape == (2, 2, 16384) and np.isfinite(z).all() and np.abs(z).max() <= 5.89
  print('mean %.5f variance %.5f' % (z.mean(), z.var()))
  assert abs(z.mean()) <= 0.02 and abs(z.var() - 1.0) <= 0.03
  # the four normals of a group come from its four words: an element depends on (key, tag, n, k, e) alone
  assert np.array_equal(noise_field([0x12345678, 0x9abcdef0], 0, 2, 2, 10), z[:, :, :10])
  assert not np.array_equal(noise_field([0x12345678, 0x9abcdef0], 1, 2, 2, 10), z[:, :, :10])
  assert not np.array_equal(z[0, 0], z[0, 1]) and not np.array_equal(z[0, 0], z[1, 0])


def test_box_muller_extremes():
  """ua is never 0 or 1: the smallest word gives the longest radius, sqrt(2 ln 2^25) = 5.887, the largest a radius above 0."""
  z = normals_of_words(np.asarray([[0, 0, 0xffffffff, 0]], np.uint32))
  assert abs(z[0, 0] - np.sqrt(2 * 25 * np.log(2))) < 1e-12 and z[0, 1] == 0
  assert abs(z[0, 2] - np.sqrt(-2 * np.log1p(-2.0 ** -25))) < 1e-12 and z[0, 2] > 2e-4


# ================================================================================================
# the draws
# ================================================================================================
@pytest.fixture(scope='module')
def scene_batches(dataset):
  return _run(dataset, augment=dict(AUG, **SCENE))


def test_shift_colour_draws_file_order_and_picks_are_those_without_the_keys(dataset, scene_batches):
  old = _run(dataset, augment=AUG)
  _same_windows(old, scene_batches)
  for a, b in zip(_draws(old), _draws(scene_batches)):
    assert np.array_equal(a.shift, b.shift) and np.array_equal(a.colour, b.colour)
    assert a.scene is None and a.occ_rect is None and a.noise_key is None and b.scene == 'occlude+noise'
  a = _run(dataset, shuffle_windows=True, shuffle_buffer=8, augment=AUG)
  b = _run(dataset, shuffle_windows=True, shuffle_buffer=8, augment=dict(AUG, **SCENE))
  _same_windows(a, b)
  assert all(np.array_equal(x.shift, y.shift) and np.array_equal(x.colour, y.colour) for x, y in zip(_draws(a), _draws(b)))
  _same_windows(_run(dataset), scene_batches)


def test_scene_draws_are_reproducible_and_differ_between_ranks(dataset, scene_batches):
  again = _run(dataset, augment=dict(AUG, **SCENE))
  assert all(_same_draws(a, b) for a, b in zip(_draws(scene_batches), _draws(again)))
  keys = [tuple(d.noise_key.tolist()) for d in _draws(scene_batches)]
  assert len(set(keys)) == len(keys)                                   # a key per emitted batch
  per_rank = []
  for r in range(2):
    a, b = (_run(dataset, augment=dict(AUG, **SCENE), shard=(r, 2)) for _ in range(2))
    assert all(_same_draws(x, y) for x, y in zip(_draws(a), _draws(b)))
    per_rank.append(_draws(a)[0])
  assert not np.array_equal(per_rank[0].noise_key, per_rank[1].noise_key)
  assert not np.array_equal(per_rank[0].occ_colour, per_rank[1].occ_colour)
  # rank 0 of a sharded run draws from the stream of an unsharded run (the generator is default_rng([seed, rank, constant]))
  assert np.array_equal(per_rank[0].noise_key, _draws(scene_batches)[0].noise_key)
  want = I.draw_augment_scene(np.random.default_rng([3, 0, I.AUGMENT_SCENE_STREAM]), BATCH, HW, HW, 0.05, 3, 0.5)
  first = _draws(scene_batches)[0]
  assert np.array_equal(want['noise_key'], first.noise_key) and np.array_equal(want['occ_rect'], first.occ_rect) and \
      np.array_equal(want['occ_colour'], first.occ_colour) and first.sigma == 0.05
  assert I.AUGMENT_SCENE_STREAM != I.AUGMENT_STREAM


def test_rectangles_lie_inside_the_frame(scene_batches):
  rect = np.concatenate([d.occ_rect for d in _draws(scene_batches)])
  colour = np.concatenate([d.occ_colour for d in _draws(scene_batches)])
  assert rect.dtype == np.int32 and rect.shape[1:] == (4, 4) and colour.dtype == np.float32 and colour.shape[1:] == (4, 3)
  used = rect[..., 2] > 0
  counts = used.sum(axis=1)
  assert counts.max() <= SCENE['occlude'] and len(set(counts.tolist())) > 1
  assert all(used[i, :c].all() and not used[i, c:].any() for i, c in enumerate(counts))      # slots fill from 0
  assert not rect[~used].any() and not colour[~used].any()             # unused slots are all zero
  y0, x0, h, w = (rect[used][:, i] for i in range(4))
  lim = max(1, int(SCENE['occlude_size'] * HW))
  assert (y0 >= 0).all() and (x0 >= 0).all() and (h >= 1).all() and (w >= 1).all() and h.max() <= lim and w.max() <= lim
  assert (y0 + h <= HW).all() and (x0 + w <= HW).all()
  assert colour[used].min() >= 0 and colour[used].max() < 1 and len(np.unique(h)) > 1


def test_draw_sizes_at_the_edges():
  one = I.draw_augment_scene(np.random.default_rng(0), 6, 5, 7, 0.0, 4, 0.01)      # floor(f H) = 0: one-pixel rectangles
  assert set(one) == {'occ_rect', 'occ_colour'}
  used = one['occ_rect'][..., 2] > 0
  assert used.any() and (one['occ_rect'][used][:, 2:] == 1).all()
  full = I.draw_augment_scene(np.random.default_rng(0), 64, 5, 7, 0.0, 1, 1.0)
  r = full['occ_rect'][full['occ_rect'][..., 2] > 0]
  assert r[:, 2].max() == 5 and r[:, 3].max() == 7 and (r[:, 0] + r[:, 2] <= 5).all() and (r[:, 1] + r[:, 3] <= 7).all()
  only_noise = I.draw_augment_scene(np.random.default_rng(0), 3, 5, 7, 0.25, 0, 0.25)
  assert set(only_noise) == {'noise_key', 'sigma'} and only_noise['noise_key'].dtype == np.uint32


def test_a_single_new_key_is_enough(dataset):
  for aug, scene in ((dict(noise=0.1), 'noise'), (dict(occlude=1), 'occlude'), (dict(noise=0.1, occlude=2), 'occlude+noise')):
    batches = _run(dataset, augment=aug)
    for f, _ in batches:
      d = f['rgb'].augment
      assert isinstance(d, WindowAugment) and d.scene == scene and all(f[k].augment is d for k in STREAMS)
      assert not d.shift.any() and (d.colour[:, :3] == 1).all() and not d.colour[:, 3:].any()      # identity shift and tint
      assert f['rgb'].scene_tables()[4] == 0 and f['target_rgb'].scene_tables()[4] == 1            # the streams' tags
      assert f['depth'].scene_tables() is None and f['target_depth'].scene_tables() is None        # depth: shift only
      assert f['depth'].augment_tables() == (d.shift, None)


@pytest.mark.parametrize('off', [dict(noise=0), dict(noise=0.0, occlude=0), dict(occlude=0, occlude_size=0.5),
                                 dict(shift=0, gain=0.0, bias=0.0, noise=0.0, occlude=0), dict(occlude_size=1.0)])
def test_off_in_every_spelling(dataset, off):
  assert I.check_augment_scene(off) is None and I.check_augment(off) is None
  got = _run(dataset, augment=off)
  _same_windows(_run(dataset), got)
  assert all(f[k].augment is None for f, _ in got for k in STREAMS)
  # ... and on the host path there is nothing to refuse
  assert isinstance(_run(dataset, device=None, augment=off)[0][0]['rgb'], np.ndarray)


def test_validators():
  assert I.check_augment_scene(None) is None and I.check_augment_scene({}) is None
  assert I.check_augment_scene(dict(noise=np.float32(0.5), occlude=np.int64(4))) == (0.5, 4, 0.25)
  assert I.check_augment_scene(dict(shift=2, occlude=1, occlude_size=1)) == (0.0, 1, 1.0)
  # check_augment stays the validator of the three old keys, with its pinned return value, and accepts the new names
  assert I.check_augment(dict(shift=2, noise=0.5, occlude=2, occlude_size=0.5), (HW, HW)) == (2, 0.0, 0.0)
  assert I.check_augment(dict(noise=0.5)) is None


@pytest.mark.parametrize('bad,key', [
    (dict(noise=1.0), 'noise'), (dict(noise=-0.1), 'noise'), (dict(noise=float('nan')), 'noise'), (dict(noise='0.1'), 'noise'),
    (dict(noise=True), 'noise'), (dict(occlude=5), 'occlude'), (dict(occlude=-1), 'occlude'), (dict(occlude=1.0), 'occlude'),
    (dict(occlude=True), 'occlude'), (dict(occlude='2'), 'occlude'), (dict(occlude=1, occlude_size=0), 'occlude_size'),
    (dict(occlude=1, occlude_size=-0.5), 'occlude_size'), (dict(occlude_size=1.5), 'occlude_size'),
    (dict(occlude_size=float('nan')), 'occlude_size'), (dict(occlude_size=True), 'occlude_size'),
    (dict(noise=0.1, rotate=3), 'rotate'), (dict(noise=0.1, shift=-1), 'shift')])
def test_bad_values_are_refused_by_name(dataset, bad, key):
  with pytest.raises(ValueError, match=key):
    I.pickplace_input_fn(dataset, 'default', 'train', window_size=K, batch_size=BATCH, seed=3, device='cpu', cache=False, augment=bad)
  with pytest.raises(ValueError, match=key):
    I.check_augment_scene(bad)


def test_the_host_path_is_refused(dataset):
  for aug in (dict(noise=0.1), dict(occlude=1)):
    with pytest.raises(ValueError, match='device='):
      I.pickplace_input_fn(dataset, 'default', 'train', window_size=K, batch_size=BATCH, seed=3, augment=aug)


def test_other_modes_and_synthetic_inputs_ignore_the_keys(dataset):
  a, b = _run(dataset, mode='eval'), _run(dataset, mode='eval', augment=dict(AUG, **SCENE))
  _same_windows(a, b)
  assert all(f[k].augment is None for f, _ in b for k in STREAMS)
  assert isinstance(_run(dataset, mode='eval', device=None, augment=SCENE)[0][0]['rgb'], np.ndarray)
  kw = dict(window_size=K, batch_size=2, seed=1)
  a = list(I.pickplace_input_fn('synthetic:2:16x16', None, 'train', **kw))
  b = list(I.pickplace_input_fn('synthetic:2:16x16', None, 'train', augment=SCENE, **kw))
  assert len(a) == len(b) == 2 and all(np.array_equal(f['rgb'], fp['rgb']) for (f, _), (fp, _) in zip(b, a))


def test_window_augment_checks_its_extras():
  z2, c6 = np.zeros((2, 2)), np.tile([1, 1, 1, 0, 0, 0], (2, 1))
  with pytest.raises(ValueError, match='come together'):
    WindowAugment(z2, c6, occ_rect=np.zeros((2, 4, 4)))
  with pytest.raises(ValueError, match='occluder rows'):
    WindowAugment(z2, c6, occ_rect=np.zeros((3, 4, 4)), occ_colour=np.zeros((3, 4, 3)))
  with pytest.raises(ValueError, match='noise key'):
    WindowAugment(z2, c6, sigma=0.5)
  with pytest.raises(ValueError, match='sigma'):
    WindowAugment(z2, c6, sigma=1.0, noise_key=[1, 2])
  a = WindowAugment(z2, c6, sigma=0.5, noise_key=[1, 0xffffffff])
  assert a.scene == 'noise' and a.noise_key.dtype == np.uint32 and a.noise_key.tolist() == [1, 0xffffffff]
  assert WindowAugment(z2, c6, sigma=0.0, noise_key=[1, 2]).scene is None      # sigma 0: no noise, whatever the key


def test_all_existing_refusals_stand_with_extras():
  dw = fake_windows([(FakeFrames(1 << 20, 9), [0, 1], 255.0)])
  dw.augment = WindowAugment(np.zeros((2, 2)), np.tile([1, 1, 1, 0, 0, 0], (2, 1)), sigma=0.1, noise_key=[1, 2])
  for call in (lambda: dw.addresses('cuda:0'), lambda: dw.frame_table(8, device='cuda:0'), lambda: DeviceWindows.concat(dw, dw)):
    with pytest.raises(ValueError, match='augmented'):
      call()


# ================================================================================================
# which entry point runs
# ================================================================================================
def _fake(extras, C=3):
  shape = (4, 6, C)
  dw = DeviceWindows(3, shape, 255.0)
  dw.add(FakeFrames(1 << 20, 9, device='cpu'), np.asarray([0, 4, 1], np.int32))
  dw.augment = WindowAugment([[1, -2], [0, 0], [-3, 5]], np.arange(18, dtype=np.float32).reshape(3, 6), **extras)
  return dw


OCC = dict(occ_rect=np.arange(48).reshape(3, 4, 4), occ_colour=np.arange(36).reshape(3, 4, 3) / 36.0)
NOISE = dict(sigma=0.25, noise_key=[0xdeadbeef, 7])


@pytest.mark.parametrize('extras,scene', [({}, None), (OCC, 'occlude'), (NOISE, 'noise'), (dict(OCC, **NOISE), 'occlude+noise')],
                         ids=['plain', 'occlude', 'noise', 'both'])
def test_feed_slot_reserves_writes_and_launches_by_the_extras(monkeypatch, extras, scene):
  from geeco_amd import ops
  calls = []
  monkeypatch.setattr(ops, 'gather_windows_scene_into', lambda *a: calls.append(('scene',) + a))
  monkeypatch.setattr(ops, 'gather_windows_augmented_into', lambda *a: calls.append(('augmented',) + a))
  dw = _fake(extras)
  dw.scene_tag = 1
  log, key = [], ('features', 'target_rgb')
  arena = RecordingArena(log)
  slot = WindowFeed(dw, arena, key)
  assert slot.scene == scene
  want = ['window_addr', 'window_kind', 'aug_shift', 'aug_colour'] + (['aug_occ_rect', 'aug_occ_colour'] if 'occ_rect' in extras else []) + \
      (['aug_noise_key'] if 'sigma' in extras else [])
  assert [k[-1] for k in arena.layout] == want
  slot.form, slot.buffer = 'dense_augmented', 'buffer'
  slot.feed(dw)
  assert [e[1] for e in log if e[0] == 'write'] == want and slot._gather_pending and not calls
  if 'occ_rect' in extras:
    assert arena.layout[key + ('aug_occ_rect',)] == ((3, 4, 4), np.dtype(np.int32))
    assert arena.layout[key + ('aug_occ_colour',)] == ((3, 4, 3), np.dtype(np.float32))
    assert np.array_equal(arena.values[key + ('aug_occ_rect',)], dw.augment.occ_rect)
  if 'sigma' in extras:
    assert arena.values[key + ('aug_noise_key',)].view(np.uint32).tolist() == [0xdeadbeef, 7]
  arena.seal()
  slot.after_flush()
  assert len(calls) == 1 and not slot._gather_pending                   # ONE launch per stream
  view = lambda name: ('view',) + key + (name,)
  head = ('buffer', view('window_addr'), view('window_kind'), view('aug_shift'), view('aug_colour'))
  if scene is None:                                                      # extras absent: the scene op is never called
    assert calls[0] == ('augmented',) + head + (3, 3, 4, 6, 3)
  else:
    assert calls[0] == ('scene',) + head + (view('aug_occ_rect') if 'occ_rect' in extras else None,
                                            view('aug_occ_colour') if 'occ_rect' in extras else None,
                                            view('aug_noise_key') if 'sigma' in extras else None,
                                            extras.get('sigma', 0.0), 1, 3, 3, 4, 6, 3)
  # a batch with other extras in this slot is an error, not a silently different transform
  other = _fake(dict(NOISE) if scene != 'noise' else dict(OCC))
  slot.form = 'dense_augmented'
  with pytest.raises(RuntimeError, match='scene extras'):
    slot.feed(other)


def test_one_channel_streams_keep_the_merged_entry(monkeypatch):
  from geeco_amd import ops
  calls = []
  monkeypatch.setattr(ops, 'gather_windows_scene_into', lambda *a: calls.append('scene'))
  monkeypatch.setattr(ops, 'gather_windows_augmented_into', lambda *a: calls.append('augmented'))
  dw = _fake(dict(OCC, **NOISE), C=1)
  assert dw.scene_tables() is None
  arena = RecordingArena([])
  slot = WindowFeed(dw, arena, ('features', 'depth'))
  assert slot.scene is None and [k[-1] for k in arena.layout] == ['window_addr', 'window_kind', 'aug_shift']
  slot.form, slot.buffer = 'dense_augmented', 'buffer'
  slot.feed(dw)
  arena.seal()
  slot.after_flush()
  assert calls == ['augmented']


@pytest.mark.parametrize('extras,want', [({}, 'augmented'), (OCC, 'scene'), (NOISE, 'scene')], ids=['plain', 'occlude', 'noise'])
def test_materialize_into_picks_the_entry_point(monkeypatch, extras, want):
  from geeco_amd import ops
  calls = []
  monkeypatch.setattr(ops, 'gather_windows_scene_into', lambda *a: calls.append(('scene', a)))
  monkeypatch.setattr(ops, 'gather_windows_augmented_into', lambda *a: calls.append(('augmented', a)))
  dw = _fake(extras)
  out = torch.empty((3, 3, 4, 6, 3))
  dw.materialize_into(out)
  assert [c[0] for c in calls] == [want]
  if want == 'scene':
    args = calls[0][1]
    assert args[8:] == (extras.get('sigma', 0.0), 0, 3, 3, 4, 6, 3)
    assert (args[5] is None) == ('occ_rect' not in extras) and (args[7] is None) == ('sigma' not in extras)
    if 'sigma' in extras:
      assert args[7].dtype == torch.int32 and args[7].numpy().view(np.uint32).tolist() == [0xdeadbeef, 7]


# ================================================================================================
# the reference helper's own known answers
# ================================================================================================
def test_helper_paints_in_slot_order_and_clips_to_the_frame():
  v = np.zeros((1, 2, 4, 5, 3))
  i32 = np.iinfo(np.int32)
  rect = np.asarray([[[1, 1, 2, 3], [2, 2, 5, 9], [0, 0, 0, 4], [i32.min, 3, i32.max, 1]]], np.int64)
  col = np.asarray([[[.1, .2, .3], [.4, .5, .6], [.7, .8, .9], [1, 1, 1]]])
  got, covered = paint(v, rect, col)
  assert covered[0].astype(int).tolist() == [[0, 0, 0, 0, 0], [0, 1, 1, 1, 0], [0, 1, 1, 1, 1], [0, 0, 1, 1, 1]]
  assert got[0, 1, 1, 1].tolist() == [.1, .2, .3] and got[0, 0, 2, 2].tolist() == [.4, .5, .6]      # the later slot wins
  assert not got[0, :, 0].any()                      # the empty slot and the one ending above the frame paint nothing
  rect[0, 3] = [-5, 4, i32.max, 1]
  assert paint(v, rect, col)[1][0][:, 4].all()
