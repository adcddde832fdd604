"""The host side of the device feed after its split into modules (no GPU): ``DeviceWindows``' one walk over the segments, the
feature concatenation, ``WindowFeed``'s four forms against a recording arena, the slots ``feed.py`` builds and prunes for the
Estimator, and ``input_fn``'s import surface."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from _fake_frames import FE, K, SHAPE, FakeFrames, RecordingArena, windows
from geeco_amd import device_windows, feed, input_fn, ops, synthetic
from geeco_amd.device_windows import DeviceWindows
from geeco_amd.feed import WindowFeed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = ('features', 'rgb')


def _on(device, segments):
  return [(f if f is None else FakeFrames(f.base, f.shape[0], f.dtype, device), st, d) for f, st, d in segments]


def _u8_segments():
  """three segments from two episodes, with repeats (3, 3) and overlaps (3 / 4, 4 / 4)"""
  a, b = FakeFrames(1 << 20, 9), FakeFrames(1 << 22, 9)
  return [(a, [3, 3, 4], 255.0), (b, [2], 255.0), (a, [4, 0], 255.0)]


def _mixed_segments():
  a, c = FakeFrames(1 << 20, 9), FakeFrames(1 << 24, 9, torch.float32)
  return [(a, [5], 255.0), (c, [0, 2], 1.0), (a, [1], 255.0), (c, [6], 1.0)]


# ================================================================================================
# 1. the address forms agree
# ================================================================================================
def test_the_address_forms_agree():
  dw = windows(_u8_segments())
  want = np.asarray([f.base + s * FE for f, starts, _ in _u8_segments() for s in starts], np.int64)
  addr = dw.addresses('cuda:0')
  table, kinds = dw.window_table('cuda:0')
  frames, index, _, used = dw.frame_table(dw.n + 2 * (K - 1) + 4)
  assert addr.dtype == table.dtype == np.int64 and not kinds.any() and used == 7 + 3       # frames 0..6 of a, 2..4 of b
  np.testing.assert_array_equal(addr, want)
  np.testing.assert_array_equal(table, want)
  np.testing.assert_array_equal(frames[index[:, 0]], want)


def test_mixed_kinds_have_byte_strides_and_no_pointer_form():
  dw = windows(_mixed_segments())
  table, kinds = dw.window_table('cuda:0')
  np.testing.assert_array_equal(table, [f.base + s * FE * (1 if f.dtype == torch.uint8 else 4) for f, st, _ in _mixed_segments() for s in st])
  assert kinds.tolist() == [0, 1, 1, 0, 1]
  with pytest.raises(ValueError, match='float32 frames'):
    dw.addresses('cuda:0')
  with pytest.raises(ValueError, match='neither the uint8'):        # what the pointer form returned element-scaled addresses for
    windows([(FakeFrames(1 << 20, 9), [0], 2.0)]).addresses('cuda:0')


# ================================================================================================
# 2. materialize_into refuses before launching
# ================================================================================================
def test_materialize_into_refuses_before_launching(monkeypatch):
  calls = []
  monkeypatch.setattr(ops, 'gather_windows_into', lambda out, src, st, n, Kw, fe, div: calls.append((out, src, st, n, Kw, fe, div)))
  out = torch.zeros((6, K) + SHAPE)
  good = _on('cpu', _u8_segments())
  with pytest.raises(IndexError, match='outside the 9 resident frames'):      # the LAST segment is out of range: nothing is queued
    windows(good[:2] + [(good[2][0], [4, 7], 255.0)]).materialize_into(out)
  with pytest.raises(IndexError, match='outside the 9 resident frames'):
    windows([(good[0][0], [-1], 255.0)]).materialize_into(out)
  with pytest.raises(RuntimeError, match='not uploaded'):
    windows(good[:1] + [(None, [0], 255.0)]).materialize_into(out)
  with pytest.raises(RuntimeError, match='each rank must upload'):
    windows(good[:1] + _u8_segments()[1:]).materialize_into(out)            # (those live on cuda:0)
  assert calls == []
  segs = good[:2] + [(FakeFrames(1 << 24, 9, torch.float32, 'cpu'), [4, 0], 1.0)]
  windows(segs).materialize_into(out)
  assert len(calls) == 3
  off = 0
  for (frames, starts, div), (o, src, st, n, Kw, fe, d) in zip(segs, calls):
    assert src is frames and (n, Kw, fe, d) == (len(starts), K, FE, div)
    assert o.data_ptr() == out[off:off + n].data_ptr() and o.shape == (n, K) + SHAPE
    assert st.dtype == torch.int32 and st.tolist() == starts
    off += n


# ================================================================================================
# 3. input_fn still exports everything
# ================================================================================================
MOVED = {
    device_windows: ['resolve_device', 'DeviceWindows', '_PinnedPool', '_PINNED', 'EpisodeCache', 'EPISODE_CACHE', 'episode_to_device'],
    feed: ['FeedArena', 'WindowFeed'],
    synthetic: ['synthetic_batches', 'synthetic_from_spec', 'write_episode', 'synthetic_scene_frames', 'write_synthetic_dataset'],
}
KEPT = ['get_meta_v4', 'collect_tfrecords', 'load_target_frame', 'load_keyframes', 'load_target_frames', 'load_episode', 'load_episode_py',
        'episode_windows', 'shuffle_stream', '_assemble_picks', '_concat_feature', '_Prefetcher', '_EpisodeSource', '_buffer_limit',
        'usable_host_cores', 'default_reader_threads', 'pickplace_input_fn', '_Omitted', '_FEATURE_KEYS', '_LABEL_KEYS', '_IMAGE_KEYS',
        '_ARM_JOINTS', '_FINGER_JOINTS', 'PickAndPlaceMetaV4']


def test_input_fn_exports_what_moved_as_the_same_objects():
  for module, names in MOVED.items():
    for name in names:
      assert getattr(input_fn, name) is getattr(module, name), name
  for name in KEPT:
    assert hasattr(input_fn, name), name


@pytest.mark.parametrize('module', ['geeco_amd.feed', 'geeco_amd.device_windows'])
def test_feed_and_device_windows_do_not_import_input_fn(module):
  code = "import sys, %s; sys.exit(int('geeco_amd.input_fn' in sys.modules))" % module
  assert subprocess.run([sys.executable, '-c', code], cwd=ROOT).returncode == 0


# ================================================================================================
# 4. the concatenation
# ================================================================================================
def test_concat_of_three_device_windows():
  a, b, c = windows(_u8_segments()), windows(_mixed_segments()), windows(_u8_segments()[:1])
  b.scattered = True
  for got in (DeviceWindows.concat(a, b, c), input_fn._concat_feature([a, b, c])):
    assert got.n == 6 + 5 + 3 and got.shape == (14, K) + SHAPE and got.scattered
    assert len(got.segments) == 8 and all(x is y for x, y in zip(got.segments, a.segments + b.segments + c.segments))
  assert not DeviceWindows.concat(a, c, a).scattered and a.n == 6 and len(a.segments) == 3      # (the parts are left alone)
  assert input_fn._concat_feature([a]) is a
  with pytest.raises(ValueError, match='different shapes'):
    DeviceWindows.concat(a, c, windows(_u8_segments(), k=1, squeeze=True))


def test_concat_of_three_omitted_streams_and_arrays():
  parts = [input_fn._Omitted((n, K) + SHAPE, 'depth') for n in (2, 1, 4)]
  got = input_fn._concat_feature(parts)
  assert isinstance(got, input_fn._Omitted) and got.shape == (7, K) + SHAPE and got.key == 'depth'
  with pytest.raises(RuntimeError, match='not decoded'):
    np.asarray(got)
  r = np.random.default_rng(0)
  arrays = [r.random([n, K, 2]).astype(np.float32) for n in (2, 1, 4)]
  np.testing.assert_array_equal(input_fn._concat_feature(arrays), np.concatenate(arrays, axis=0))


# ================================================================================================
# 5. WindowFeed: one form per slot
# ================================================================================================
class _ArrayArena(RecordingArena):
  """``view`` as a host array of the reserved shape (the frame-table form slices its view)."""

  def view(self, key):
    return np.zeros(*self.layout[key])


def _batches(scattered):
  """two successive batches of 4 windows on the host device; with a target stream"""
  a, b = FakeFrames(1 << 20, 9, device='cpu'), FakeFrames(1 << 22, 9, device='cpu')
  ta, tb = FakeFrames(1 << 26, 1, device='cpu'), FakeFrames(1 << 27, 1, device='cpu')
  out = []
  for segs, tsegs in (([(a, [0, 1], 255.0), (b, [4, 5], 255.0)], [(ta, [0, 0], 255.0), (tb, [0, 0], 255.0)]),
                      ([(b, [2, 3, 4, 5], 255.0)], [(tb, [0, 0, 0, 0], 255.0)])):
    batch = {'rgb': windows(segs), 'target_rgb': windows(tsegs, k=1, squeeze=True)}
    batch['rgb'].scattered = batch['target_rgb'].scattered = scattered
    out.append(batch)
  return out


GATHER = ('gather', ('view',) + KEY + ('window_addr',), ('view',) + KEY + ('window_kind',), 4, K, FE)
FORMS = {       # form: (scattered first batch, shared_frames, what the model calls, arena keys reserved, calls per batch)
    'pointers': (False, None, lambda f: f.pointers(), {KEY}, [('write', 'rgb'), ('flush',)]),
    'dense': (False, None, lambda f: f.dense(), {KEY}, [('per-segment',), ('flush',)]),
    'dense_by_address': (True, None, lambda f: f.dense(), {KEY, KEY + ('window_addr',), KEY + ('window_kind',)},
                         [('write', 'window_addr'), ('write', 'window_kind'), ('flush',), GATHER]),
    'frame_table': (False, 12, lambda f: f.frame_table(10), {KEY, KEY + ('frame_table',), KEY + ('frame_index',), KEY + ('target_index',)},
                    [('write', 'frame_table'), ('write', 'frame_index'), ('write', 'target_index'), ('flush',)]),
}


@pytest.mark.parametrize('form', list(FORMS))
def test_window_feed_form_selection(form, monkeypatch):
  scattered, shared, choose, reserved, per_batch = FORMS[form]
  log = []
  monkeypatch.setattr(ops, 'gather_windows_by_address_into', lambda out, addr, kind, N, Kw, fe: log.append(('gather', addr, kind, N, Kw, fe)))
  monkeypatch.setattr(DeviceWindows, 'materialize_into', lambda self, out: log.append(('per-segment',)))
  batches = _batches(scattered)
  arena = (_ArrayArena if shared else RecordingArena)(log)
  slot = WindowFeed(batches[0]['rgb'], arena, KEY, **(dict(shared_frames=shared, shared_targets='target_rgb') if shared else {}))
  assert set(arena.layout) == reserved
  assert slot._with_targets is False and slot.shared == slot.shared_reserved == shared
  arena.seal()
  assert slot.form is None and not slot.adopted and not slot.feeds_frame_table
  slot.feed(batches[0]['rgb'], batches[0])                 # no model adopted the slot: nothing is fed
  arena.flush()
  slot.after_flush()
  assert log == [('flush',)] and len(slot._live) == 0
  choose(slot)
  assert slot.form == form and slot.adopted and slot.feeds_frame_table == (form == 'frame_table')
  assert (slot.table is not None) == (form == 'pointers') and (slot.buffer is not None) == form.startswith('dense')
  with pytest.raises(RuntimeError, match='already feeds'):
    (slot.pointers if form != 'pointers' else slot.dense)()
  for batch in batches:
    del log[:]
    slot.feed(batch['rgb'], batch)
    arena.flush()
    slot.after_flush()
    slot.after_flush()
    assert log == per_batch
    if form == 'pointers':
      np.testing.assert_array_equal(arena.values[KEY], batch['rgb'].addresses('cpu'))
    if form == 'frame_table':
      assert (slot.shared, slot.shared_reserved, slot._with_targets) == (10, 12, True)
      table, index, tindex, used = batch['rgb'].frame_table(10, batch['target_rgb'])
      got = arena.values[KEY + ('frame_table',)]
      assert got.shape == (12,) and not got[10:].any() and used <= 10           # the reserved tail is zero-padded
      np.testing.assert_array_equal(got[:10], table)
      np.testing.assert_array_equal(arena.values[KEY + ('frame_index',)], index)
      np.testing.assert_array_equal(arena.values[KEY + ('target_index',)], tindex)
      assert slot._live[-1] == (batch['rgb'], batch['target_rgb'])
    elif form != 'dense':
      assert slot._live[-1] is batch['rgb']


# ================================================================================================
# the slots of one model: what the model adopted is what the three-way id() expression selected
# ================================================================================================
class _TensorArena(RecordingArena):
  """Stands in for feed.FeedArena in build_slots (sealing the real one pins host memory, which needs a GPU)."""

  SLOTS = feed.FeedArena.SLOTS

  def __init__(self, device):
    super().__init__([])
    self.device = torch.device(device)

  def view(self, key):
    return torch.zeros(self.layout[key][0])

  def begin(self):
    pass


def _adopt(kind):
  """What estimator._model_fn does with the slots, for a dense model, a model that follows window addresses and a goal model
  built with shared_frames."""
  def model_inputs(fbuf, lbuf):
    inputs = {'jnt_state': fbuf['jnt_state'], 'cmd': lbuf['cmd']}
    if kind == 'dense':
      inputs['rgb'] = fbuf['rgb'].dense()
    elif kind == 'pointers':
      inputs.update({k: fbuf[k].pointers() for k in ('rgb', 'target_rgb')})
    else:
      inputs.update(fbuf['rgb'].frame_table(with_targets=True))
    return inputs
  return model_inputs


PRUNED = {'dense': ({'rgb', 'jnt_state'}, {'cmd'}), 'pointers': ({'rgb', 'target_rgb', 'jnt_state'}, {'cmd'}),
          'shared': ({'rgb', 'jnt_state'}, {'cmd'})}


@pytest.mark.parametrize('kind', list(PRUNED))
def test_adopted_slots_are_those_the_id_expression_selected(kind, monkeypatch):
  monkeypatch.setattr(feed, 'FeedArena', _TensorArena)
  monkeypatch.setattr(DeviceWindows, 'materialize_into', lambda self, out: None)
  batch = _batches(False)[0]
  feats = dict(batch, step=np.zeros([4, K], np.int64), jnt_state=np.ones([4, K, 7], np.float32), depth=windows([(None, [0, 1, 2, 3], 1.0)]),
               big=np.zeros([4, 1 << 17], np.float32))
  labels = {'cmd': np.ones([4, 4], np.float32), 'ctrl': np.ones([4, 2], np.float32)}
  fbuf, lbuf = feed.build_slots('cpu', feats, labels, (lambda Kw, goal: 4 + 2 * (Kw - 1) + 2 * goal) if kind == 'shared' else None)
  assert set(fbuf) == set(feats) and set(lbuf) == set(labels) and (fbuf.tag, lbuf.tag) == ('features', 'labels')
  assert isinstance(fbuf['rgb'], WindowFeed) and isinstance(fbuf['depth'], WindowFeed) and torch.is_tensor(fbuf['big'])
  assert not fbuf.arena.has(('features', 'big')) and fbuf.arena.has(('features', 'step')) and fbuf.arena.block
  assert fbuf['rgb'].shared == (4 + 2 * (K - 1) + 2 if kind == 'shared' else None)
  inputs = _adopt(kind)(fbuf, lbuf)
  used = {id(v) for v in inputs.values()}
  parent = lambda bufs: {k for k, v in bufs.items() if id(v) in used or (getattr(v, 'buffer', None) is not None and id(v.buffer) in used)
                         or getattr(v, 'feeds_frame_table', False)}
  f2, l2 = feed.adopted_slots(fbuf, lbuf, inputs)
  print('pruned slots, %s model: features %s, labels %s' % (kind, sorted(f2), sorted(l2)))
  assert (set(f2), set(l2)) == PRUNED[kind] == (parent(fbuf), parent(lbuf))
  assert f2.arena is fbuf.arena is l2.arena and (f2.tag, l2.tag) == ('features', 'labels')
  feed.feed_step(f2, l2, feats, labels)                    # one step through the pruned slots: begin, writes, ONE flush
  assert fbuf.arena.log.count(('flush',)) == 1 and fbuf.arena.log[-1] == ('flush',)
  assert ('write', 'jnt_state') in fbuf.arena.log and ('write', 'cmd') in fbuf.arena.log and ('write', 'step') not in fbuf.arena.log
