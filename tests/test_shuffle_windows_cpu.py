"""Window-level shuffle, host side (no GPU): the shuffle-buffer generator, ``pickplace_input_fn(shuffle_windows=True)`` on the
host path against the unshuffled pipeline's own arrays, the data-parallel schedule, and ``DeviceWindows.window_table`` on fake
resident episodes."""
import collections

import numpy as np
import pytest
import torch

from _fake_frames import FE, SHAPE, FakeFrames, RecordingArena as _RecordingArena, windows as _windows
from geeco_amd import input_fn as I
from geeco_amd.input_fn import DeviceWindows, shuffle_stream

K = 3
BATCH = 4
EPISODES, EP_LEN = 3, 9
NWIN = (EP_LEN - 1) - K + 1          # windows of an episode (the last frame only supplies targets)


# ================================================================================================
# shuffle_stream
# ================================================================================================
def _order(n, B, seed):
  return list(shuffle_stream(range(n), B, np.random.default_rng(seed)))


def test_shuffle_stream_is_a_permutation():
  for n, B in ((50, 4), (5, 4), (4, 4), (0, 3), (1, 1)):
    assert sorted(_order(n, B, 0)) == list(range(n)), (n, B)


def test_shuffle_stream_buffer_of_one_is_the_identity():
  assert _order(50, 1, 0) == list(range(50))


def test_shuffle_stream_displacement_bound():
  """input position i never leaves before output position i - (B - 1): it enters the buffer only when output i - B is emitted"""
  B, moved = 4, 0
  for seed in range(8):
    out = _order(50, B, seed)
    for pos, item in enumerate(out):
      assert pos >= item - (B - 1), (seed, pos, item)
    moved += out != list(range(50))
  assert moved == 8


def test_shuffle_stream_full_buffer_and_seeds():
  a = _order(20, 64, 1)
  assert sorted(a) == list(range(20)) and a != list(range(20))
  assert a == _order(20, 64, 1)
  assert a != _order(20, 64, 2)
  assert _order(50, 4, 1) == _order(50, 4, 1) and _order(50, 4, 1) != _order(50, 4, 2)


def test_shuffle_stream_is_lazy_and_refuses_an_empty_buffer():
  seen = []

  def items():
    for i in range(10):
      seen.append(i)
      yield i
  g = shuffle_stream(items(), 3, np.random.default_rng(0))
  next(g)
  assert seen == [0, 1, 2, 3]          # the buffer and the one item that displaced the first pick; nothing read ahead
  with pytest.raises(ValueError, match='buffer_size'):
    list(shuffle_stream(range(3), 0, np.random.default_rng(0)))


# ================================================================================================
# pickplace_input_fn, host path
# ================================================================================================
@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
  root = str(tmp_path_factory.mktemp('shuffle_ds'))
  I.write_synthetic_dataset(root, EPISODES, episode_length=EP_LEN, img_hw=(16, 16))
  return root


def _run(root, mode='train', **kw):
  kw = dict(dict(window_size=K, batch_size=BATCH, seed=3, num_threads=2), **kw)
  return list(I.pickplace_input_fn(root, 'default', mode, **kw))


def _by_window(batches):
  """window id -> (features, labels) rows of the unshuffled pipeline.  'ts' is the same in every episode, so the id takes the
  episode from the per-episode random states."""
  table = {}
  for f, l in batches:
    for n in range(len(f['step'])):
      key = (f['goal_state'][n].tobytes(), int(f['step'][n, 0]))
      assert key not in table
      table[key] = ({k: v[n] for k, v in f.items()}, {k: v[n] for k, v in l.items()})
  return table


def _keys(batches):
  return [(f['goal_state'][n].tobytes(), int(f['step'][n, 0])) for f, _ in batches for n in range(len(f['step']))]


@pytest.fixture(scope='module')
def plain(dataset):
  return _run(dataset)


@pytest.fixture(scope='module')
def shuffled(dataset):
  return _run(dataset, shuffle_windows=True, shuffle_buffer=8)


def test_one_epoch_holds_every_window_once(plain, shuffled):
  assert len(_keys(plain)) == EPISODES * NWIN == len(set(_keys(plain)))
  assert collections.Counter(_keys(shuffled)) == collections.Counter(_keys(plain))
  assert _keys(shuffled) != _keys(plain)
  assert [len(f['step']) for f, _ in shuffled] == [len(f['step']) for f, _ in plain]        # ragged final batch as before


def test_batches_hold_the_unshuffled_pipelines_arrays(plain, shuffled):
  table = _by_window(plain)
  checked = 0
  for f, l in shuffled:
    for n in range(len(f['step'])):
      fw, lw = table[(f['goal_state'][n].tobytes(), int(f['step'][n, 0]))]
      for k in ('rgb', 'jnt_state', 'depth', 'step', 'cmd'):
        assert f[k][n].dtype == fw[k].dtype and np.array_equal(f[k][n], fw[k]), k
      for k in lw:
        assert np.array_equal(l[k][n], lw[k]), k
      checked += 1
  assert checked == EPISODES * NWIN
  assert set(shuffled[0][0]) == set(plain[0][0]) and set(shuffled[0][1]) == set(plain[0][1])


def test_target_frames_follow_their_windows(dataset):
  a = _run(dataset, fetch_target=True)
  b = _run(dataset, fetch_target=True, shuffle_windows=True, shuffle_buffer=8)
  table = _by_window(a)
  for f, _ in b:
    for n in range(len(f['step'])):
      fw, _l = table[(f['goal_state'][n].tobytes(), int(f['step'][n, 0]))]
      assert np.array_equal(f['target_rgb'][n], fw['target_rgb']) and np.array_equal(f['target_depth'][n], fw['target_depth'])


def test_buffer_of_one_reproduces_the_unshuffled_batches(dataset, plain):
  got = _run(dataset, shuffle_windows=True, shuffle_buffer=1)
  assert len(got) == len(plain)
  for (f, l), (fp, lp) in zip(got, plain):
    assert set(f) == set(fp) and set(l) == set(lp)
    for k in f:
      assert f[k].dtype == fp[k].dtype and np.array_equal(f[k], fp[k]), k
    for k in l:
      assert np.array_equal(l[k], lp[k]), k


def test_epochs_do_not_mix(dataset, plain):
  got = _keys(_run(dataset, shuffle_windows=True, shuffle_buffer=8, num_epochs=2))
  n = EPISODES * NWIN
  assert len(got) == 2 * n
  every = collections.Counter(_keys(plain))
  assert collections.Counter(got[:n]) == every and collections.Counter(got[n:]) == every
  assert got[:n] != got[n:]                                   # one generator runs on: the second epoch is shuffled afresh


def test_same_seed_same_batches_other_seed_other_batches(dataset, shuffled):
  assert _keys(_run(dataset, shuffle_windows=True, shuffle_buffer=8)) == _keys(shuffled)
  other = _run(dataset, shuffle_windows=True, shuffle_buffer=8, seed=4)
  assert collections.Counter(_keys(other)) == collections.Counter(_keys(shuffled)) and _keys(other) != _keys(shuffled)


def test_eval_ignores_the_option(dataset):
  a = _run(dataset, mode='eval')
  b = _run(dataset, mode='eval', shuffle_windows=True, shuffle_buffer=8)
  assert len(a) == len(b)
  for (f, l), (fp, lp) in zip(b, a):
    for k in f:
      assert np.array_equal(f[k], fp[k]), k
    for k in l:
      assert np.array_equal(l[k], lp[k]), k


def test_empty_buffer_is_refused(dataset):
  with pytest.raises(ValueError, match='shuffle_buffer'):
    I.pickplace_input_fn(dataset, 'default', 'train', window_size=K, batch_size=BATCH, seed=3, shuffle_windows=True, shuffle_buffer=0)
  # without the option the argument stays unused, as before
  assert len(_run(dataset, shuffle_buffer=0)) == -(-EPISODES * NWIN // BATCH)


def test_sharded_ranks_keep_their_schedule_and_their_windows(dataset, plain):
  seen = collections.Counter()
  for r in range(2):
    base = I.pickplace_input_fn(dataset, 'default', 'train', window_size=K, batch_size=BATCH, seed=3, num_threads=2, shard=(r, 2))
    shuf = I.pickplace_input_fn(dataset, 'default', 'train', window_size=K, batch_size=BATCH, seed=3, num_threads=2, shard=(r, 2),
                                shuffle_windows=True, shuffle_buffer=8)
    assert shuf.dp_schedule == base.dp_schedule and base.dp_schedule
    kb, ks = _keys(list(base)), _keys(list(shuf))
    assert collections.Counter(ks) == collections.Counter(kb)
    assert [len(f['step']) for f, _ in I.pickplace_input_fn(dataset, 'default', 'train', window_size=K, batch_size=BATCH, seed=3,
                                                            num_threads=2, shard=(r, 2), shuffle_windows=True, shuffle_buffer=8)] \
        == [c[r] for c in base.dp_schedule if c[r]]
    seen.update(ks)
  assert seen == collections.Counter(_keys(plain))            # disjoint (every count 1) and complete


def test_synthetic_inputs_ignore_the_option():
  a = list(I.pickplace_input_fn('synthetic:2:16x16', None, 'train', window_size=K, batch_size=2, seed=1))
  b = list(I.pickplace_input_fn('synthetic:2:16x16', None, 'train', window_size=K, batch_size=2, seed=1, shuffle_windows=True))
  assert len(a) == len(b) == 2
  for (f, _), (fp, _) in zip(b, a):
    assert np.array_equal(f['rgb'], fp['rgb'])


# ================================================================================================
# DeviceWindows.window_table
# ================================================================================================
def _expect(segments):
  """(address, kind) of every window, straight from the definition"""
  addr, kind = [], []
  for frames, starts, _ in segments:
    u8 = frames.dtype == torch.uint8
    for s in starts:
      addr.append(frames.base + s * FE * (1 if u8 else 4))
      kind.append(0 if u8 else 1)
  return np.asarray(addr, np.int64), np.asarray(kind, np.int32)


def _table_cases():
  a, b, c = FakeFrames(1 << 20, 9), FakeFrames(1 << 22, 9), FakeFrames(1 << 24, 9, torch.float32)
  return {
      'scattered': [(b, [4], 255.0), (a, [0], 255.0), (b, [1], 255.0), (a, [6], 255.0)],
      'repeats and overlaps': [(a, [3, 3], 255.0), (b, [2], 255.0), (a, [4], 255.0)],
      'uint8 + float32': [(a, [5], 255.0), (c, [0, 2], 1.0), (a, [1], 255.0), (c, [6], 1.0)],
  }


@pytest.mark.parametrize('name', list(_table_cases()))
def test_window_table_from_the_definition(name):
  segs = _table_cases()[name]
  addr, kind = _windows(segs).window_table('cuda:0')
  want_a, want_k = _expect(segs)
  assert addr.dtype == np.int64 and kind.dtype == np.int32
  np.testing.assert_array_equal(addr, want_a)
  np.testing.assert_array_equal(kind, want_k)


def test_window_table_of_squeezed_single_frames():
  ta, tb = FakeFrames(1 << 26, 1), FakeFrames(1 << 27, 1, torch.float32)
  segs = [(ta, [0], 255.0), (tb, [0, 0], 1.0), (ta, [0], 255.0)]
  dw = _windows(segs, k=1, squeeze=True)
  assert dw.shape == (4,) + SHAPE
  addr, kind = dw.window_table('cuda:0')
  assert addr.tolist() == [1 << 26, 1 << 27, 1 << 27, 1 << 26] and kind.tolist() == [0, 1, 1, 0]


def test_window_table_starts_with_the_addresses_of_the_pointer_form():
  segs = _table_cases()['scattered']
  dw = _windows(segs)
  addr, kind = dw.window_table('cuda:0')
  np.testing.assert_array_equal(addr[:dw.n], dw.addresses('cuda:0'))
  assert not kind.any()


def test_window_table_refusals():
  with pytest.raises(IndexError, match='outside the 9 resident frames'):
    _windows([(FakeFrames(1 << 20, 9), [7], 255.0)]).window_table('cuda:0')
  with pytest.raises(RuntimeError, match='each rank must upload'):
    _windows(_table_cases()['scattered']).window_table('cuda:1')
  with pytest.raises(ValueError, match='neither the uint8'):
    _windows([(FakeFrames(1 << 20, 9), [0], 2.0)]).window_table('cuda:0')
  with pytest.raises(ValueError, match='neither the uint8'):
    _windows([(FakeFrames(1 << 20, 9, torch.float32), [0], 255.0)]).window_table('cuda:0')
  with pytest.raises(RuntimeError, match='not uploaded'):
    _windows([(None, [0], 255.0)]).window_table('cuda:0')


def test_concat_keeps_the_mark():
  a = _windows(_table_cases()['scattered'])
  b = _windows(_table_cases()['scattered'])
  assert not a.scattered
  b.scattered = True
  assert DeviceWindows.concat(a, b).scattered and not DeviceWindows.concat(a, a).scattered


def test_assembler_builds_segments_from_runs_and_marks_them():
  """Picks in pick order; consecutive picks of one episode share a segment; states and labels are ex[k][idx] per pick."""
  T = 8
  eps = []
  for e in range(2):
    r = np.random.default_rng(e)
    ex = {k: r.random([T, 2]).astype(np.float32) for k in I._FEATURE_KEYS + I._LABEL_KEYS if k not in ('rgb', 'depth', 'step')}
    ex['step'] = np.arange(T, dtype=np.int64)
    ex['_hw'] = SHAPE[:2]
    eps.append((ex, {'rgb': FakeFrames((e + 1) << 20, T), 'rgb_div': 255.0}))
  picks = [(eps[0], 2), (eps[0], 5), (eps[1], 0), (eps[1], 1), (eps[0], 2)]
  f, l = I._assemble_picks(picks, K)
  rgb = f['rgb']
  assert rgb.scattered and f['depth'].scattered and rgb.n == 5 and rgb.shape == (5, K) + SHAPE
  assert [(fr.base, st.tolist()) for fr, st, _ in rgb.segments] == [(1 << 20, [2, 5]), (2 << 20, [0, 1]), (1 << 20, [2])]
  addr, kind = rgb.window_table('cuda:0')
  assert addr.tolist() == [(e + 1 << 20) + st * FE for e, st in ((0, 2), (0, 5), (1, 0), (1, 1), (0, 2))] and not kind.any()
  for n, (ep, st) in enumerate(picks):
    np.testing.assert_array_equal(f['jnt_state'][n], ep[0]['jnt_state'][st:st + K])
    np.testing.assert_array_equal(l['cmd'][n], ep[0]['cmd'][st + K - 1])
  assert f['step'][:, 0].tolist() == [2, 5, 0, 1, 2]


# ================================================================================================
# WindowFeed: the by-address fill is queued behind the arena's copy
# ================================================================================================
def test_window_feed_writes_the_table_then_gathers_after_the_flush(monkeypatch):
  from geeco_amd import ops
  log = []
  monkeypatch.setattr(ops, 'gather_windows_by_address_into', lambda out, addr, kind, N, Kw, fe: log.append(('gather', addr, kind, N, Kw, fe)))
  monkeypatch.setattr(DeviceWindows, 'materialize_into', lambda self, out: log.append(('per-segment',)))
  cpu = lambda segs: [(FakeFrames(f.base, f.shape[0], f.dtype, 'cpu'), st, d) for f, st, d in segs]
  first, second = _windows(cpu(_table_cases()['uint8 + float32'][:3])), _windows(cpu(_table_cases()['scattered']))       # 4 windows each
  first.scattered = second.scattered = True
  key = ('features', 'rgb')
  arena = _RecordingArena(log)
  feed = I.WindowFeed(first, arena, key)
  assert feed.scattered and arena.has(key + ('window_addr',)) and arena.has(key + ('window_kind',))
  arena.seal()
  feed.after_flush()                                   # nothing pending, nothing queued
  assert feed.dense().shape == (4, K) + SHAPE and log == []
  for dw in (first, second):
    del log[:]
    feed.feed(dw)
    arena.flush()
    feed.after_flush()
    feed.after_flush()                                 # once per feed
    assert log == [('write', 'window_addr'), ('write', 'window_kind'), ('flush',),
                   ('gather', ('view',) + key + ('window_addr',), ('view',) + key + ('window_kind',), 4, K, FE)]
    addr, kind = dw.window_table('cpu')
    np.testing.assert_array_equal(arena.values[key + ('window_addr',)], addr)
    np.testing.assert_array_equal(arena.values[key + ('window_kind',)], kind)
    assert feed._live[-1] is dw                        # the frames stay referenced while the launch is queued
  # a slot whose first batch was not marked keeps the per-segment path, whatever comes later
  del log[:]
  plain = _windows(cpu(_table_cases()['scattered']))
  arena2 = _RecordingArena(log)
  feed2 = I.WindowFeed(plain, arena2, key)
  assert not feed2.scattered and not arena2.has(key + ('window_addr',))
  feed2.dense()
  feed2.feed(second)
  arena2.flush()
  feed2.after_flush()
  assert log == [('per-segment',), ('flush',)]
