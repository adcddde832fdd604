"""Input pipelines: the GEECO pick&place dataset reader (encoding v4) and a synthetic generator.

Counterpart of the reference's ``src/data/geeco_gym.py`` live path: ``pickplace_input_fn`` (:234-279)
-> ``pickplace_input_fn_v4`` (:401-474) with ``_get_meta_v4`` (:283), ``_parse_v4`` (:291),
``_preprocess_states_v4`` (:317), ``_preprocess_targets_v3`` (:598), ``_window_v3`` (:615),
``_prepare_v4`` (:373) and ``_collect_tfrecords_v2`` (:780).  Same dataset directory layout, same
feature / label dictionaries (shapes and key names), same ordering semantics: record-level shuffle
in 'train' mode only, NO sample-level shuffle (it is commented out in the reference, :447-448), so
a batch holds consecutive windows of one episode; the final batch may be ragged (no drop_remainder).
``shuffle_windows=True`` opts into the sample-level shuffle of the reference's v1-v3 pipelines (:701-703), see ``shuffle_stream``.

Unlike the reference (which materialises every K-frame window on the host: 84 windows x 12.6 MB
for K = 16), an episode's frames are kept once and every batch is sliced from them; windows are
built per batch, not per episode.
"""
from __future__ import annotations

import collections
import json
import os
import queue
import threading

import numpy as np

from . import tfrecord
# what is not the reader keeps resolving from here (none of these modules imports this one when it loads)
from .device_windows import DeviceWindows, EPISODE_CACHE, EpisodeCache, SCENE_TAGS, TIMED_KEYS, WindowAugment, _PINNED, _PinnedPool, episode_to_device, resolve_device  # noqa: F401
from .feed import FeedArena, WindowFeed  # noqa: F401
from .synthetic import synthetic_batches, synthetic_from_spec, synthetic_scene_frames, write_episode, write_synthetic_dataset  # noqa: F401

PickAndPlaceMetaV4 = collections.namedtuple('PickAndPlaceMetaV4', [
    'episode_length', 'img_height', 'img_width', 'monitored_joints', 'actuated_joints', 'monitored_mocaps',
    'monitored_objects', 'dim_cmd', 'dim_ctrl'])

_ARM_JOINTS = ['shoulder_pan_joint', 'shoulder_lift_joint', 'upperarm_roll_joint', 'elbow_flex_joint',
               'forearm_roll_joint', 'wrist_flex_joint', 'wrist_roll_joint']          # geeco_gym.py:336-344
_FINGER_JOINTS = ['l_gripper_finger_joint', 'r_gripper_finger_joint']                # geeco_gym.py:364-367


def get_meta_v4(dataset_dir):
  """geeco_gym.py:283-289."""
  with open(os.path.join(dataset_dir, 'meta', 'meta_info.json'), 'r') as fp:
    return PickAndPlaceMetaV4(**json.load(fp))


def collect_tfrecords(dataset_dir, split_name, mode):
  """geeco_gym.py:780-793: record file names listed in splits/<split>/<mode>.txt (or all of data/)."""
  record_dir = os.path.join(dataset_dir, 'data')
  if split_name is None and mode is None:
    names = [fn for fn in os.listdir(record_dir) if fn.endswith('.tfrecord.zlib')]
  else:
    with open(os.path.join(dataset_dir, 'splits', split_name, '%s.txt' % (mode,))) as fp:
      names = fp.read().split('\n')
  return [os.path.join(record_dir, fn) for fn in names if fn.endswith('.tfrecord.zlib')]


# ---- target frames of an episode for the controller loop (the predictor's set_goal) ------------------------------------
def _episode_stem(tfrecord_name):
  return os.path.basename(tfrecord_name).split('.')[0]


def _read_rgb_png(path):
  from PIL import Image      # only the controller-side loaders need an image decoder
  with Image.open(path) as im:
    return np.array(im, dtype=np.float32) / 255.0


def load_target_frame(dataset_dir, tfrecord_name, load_depth=True):
  """geeco_gym.py:179-192: the episode's goal image ``images/targets/rgb/<stem>.png`` as float32 [H, W, 3] in [0, 1];
  with ``load_depth`` the raw depth map ``images/targets/depth/<stem>.npy`` becomes a 4th channel ([H, W, 4], the layout
  ``GoalE2EVMCPredictor.set_goal`` takes).  ``tfrecord_name`` may be a path; the stem is the name up to the first dot."""
  stem = _episode_stem(tfrecord_name)
  frame = _read_rgb_png(os.path.join(dataset_dir, 'images', 'targets', 'rgb', stem + '.png'))
  if load_depth:
    depth = np.load(os.path.join(dataset_dir, 'images', 'targets', 'depth', stem + '.npy'))
    frame = np.concatenate([frame, np.expand_dims(depth, axis=-1)], axis=-1)
  return frame


def load_keyframes(dataset_dir, tfrecord_name):
  """geeco_gym.py:194-211: every key frame of the episode (``images/keyframes/{rgb,depth}/<stem>*`` in sorted order,
  rgb and depth files paired by position) as RGB-D float32 [H, W, 4] arrays."""
  stem = _episode_stem(tfrecord_name)
  rgb_dir = os.path.join(dataset_dir, 'images', 'keyframes', 'rgb')
  depth_dir = os.path.join(dataset_dir, 'images', 'keyframes', 'depth')
  rgb_files = sorted(f for f in os.listdir(rgb_dir) if f.startswith(stem))
  depth_files = sorted(f for f in os.listdir(depth_dir) if f.startswith(stem))
  frames = []
  for rf, df in zip(rgb_files, depth_files):
    depth = np.load(os.path.join(depth_dir, df))
    frames.append(np.concatenate([_read_rgb_png(os.path.join(rgb_dir, rf)), np.expand_dims(depth, axis=-1)], axis=-1))
  return frames


def load_target_frames(dataset_dir, tfrecord_name, load_depth=True):
  """geeco_gym.py:165-177: the key frames when ``data/key_frames_<id>.json`` exists for the record (id = the first run of
  digits in the name), else the single goal image, as a list."""
  import re
  record_id = re.search(r'\d+', tfrecord_name).group(0)
  if os.path.exists(os.path.join(dataset_dir, 'data', 'key_frames_%s.json' % (record_id,))):
    return load_keyframes(dataset_dir, tfrecord_name)
  return [load_target_frame(dataset_dir, tfrecord_name, load_depth)]


def _finish_episode(ex, fetch_target):
  """_parse_v4's target (:313-315: LAST frame of the full episode) + _preprocess_targets_v3 (:598-613: next-frame
  states as targets, then the last frame is dropped) on per-frame arrays of the whole episode."""
  target = None
  if fetch_target:
    target = {'target_rgb': ex['rgb'][-1].copy(), 'target_depth': ex['depth'][-1].copy()}
  ex['vel_target'] = np.roll(ex['vel_state'], -1, axis=0)
  ex['ee_target'] = np.roll(ex['ee_state'], -1, axis=0)
  ex['grp_target'] = np.roll(ex['grp_state'], -1, axis=0)
  ex = {k: v[:-1] for k, v in ex.items()}
  if target:
    ex.update(target)
  return ex


def load_episode_py(path, meta, fetch_target, raw_rgb=False):
  """``load_episode`` through the pure-Python TFRecord / protobuf reader of tfrecord.py (one thread, holds the GIL):
  the independent restatement the native reader is tested against; not used by the pipeline."""
  H, W = meta.img_height, meta.img_width
  payload = next(iter(tfrecord.read_records(path, 'zlib')))
  _, fl = tfrecord.parse_sequence_example(payload)

  def stack(key, shape=None, dtype=np.float32):
    if key not in fl:
      raise KeyError("%s: feature list '%s' missing" % (path, key))
    arr = np.stack([np.asarray(f, dtype=dtype) for f in fl[key]], axis=0)
    return arr.reshape((arr.shape[0],) + tuple(shape)) if shape is not None else arr

  ex = {
      'step': stack('step', (), np.int64),
      'ts': stack('ts', ()),
      'rgb': stack('rgb', (H, W, 3)) / np.float32(1.0 if raw_rgb else 255.0),   # :312 RGB recorded as uint8 0..255
      'depth': stack('depth', (H, W, 1)),
      'cmd': stack('cmd', (meta.dim_cmd,)),
      'ctrl': stack('ctrl', (meta.dim_ctrl,)),
      'ee_state': stack('mocap_qpos-robot0:mocap', (7,)),
      'goal_state': stack('goal_qpos', (7,)),
      'obj_state': stack('obj_qpos', (7,)),
  }
  ex['jnt_state'] = np.stack([stack('joint_qpos-robot0:%s' % j, ()) for j in _ARM_JOINTS], axis=1)
  ex['vel_state'] = np.stack([stack('joint_qvel-robot0:%s' % j, ()) for j in _ARM_JOINTS], axis=1)
  ex['grp_state'] = np.stack([stack('joint_qpos-robot0:%s' % j, ()) for j in _FINGER_JOINTS], axis=1)
  return _finish_episode(ex, fetch_target)


def load_episode(path, meta, fetch_target, raw_rgb=False, image_keys=('rgb', 'depth'), alloc=None):
  """One episode -> dict of per-frame arrays after _parse_v4 + _preprocess_states_v4 + _preprocess_targets_v3 (i.e.
  the last frame already dropped: T = episode_length - 1), read by the native reader (inflate, CRC, SequenceExample
  scan and the float -> array copies run without the GIL: ``num_threads`` of these calls proceed side by side).

  ``raw_rgb``: 'rgb' / 'target_rgb' keep the recorded 0..255 values — as a uint8 array when every value is integral
  (the recorder stores uint8 frames as float lists, tfrecord.py:73-74; the test runs inside the conversion pass), else
  as float32; the device path divides by 255 on the GPU.  Otherwise float32 / 255 (:312).
  ``image_keys``: which of the image streams to decode (an RGB-only model never reads 'depth': 26 MB per episode).
  ``alloc(nbytes) -> uint8 array``: where the image arrays go (pinned staging memory of the device path)."""
  H, W = meta.img_height, meta.img_width
  with tfrecord.EpisodeReader(path, 'zlib') as rd:
    T = rd.frames('step')
    ex = {
        'step': rd.i64('step', 1).reshape(T),
        'ts': rd.f32('ts', 1).reshape(T),
        'cmd': rd.f32('cmd', meta.dim_cmd),
        'ctrl': rd.f32('ctrl', meta.dim_ctrl),
        'ee_state': rd.f32('mocap_qpos-robot0:mocap', 7),
        'goal_state': rd.f32('goal_qpos', 7),
        'obj_state': rd.f32('obj_qpos', 7),
        'jnt_state': np.concatenate([rd.f32('joint_qpos-robot0:%s' % j, 1) for j in _ARM_JOINTS], axis=1),
        'vel_state': np.concatenate([rd.f32('joint_qvel-robot0:%s' % j, 1) for j in _ARM_JOINTS], axis=1),
        'grp_state': np.concatenate([rd.f32('joint_qpos-robot0:%s' % j, 1) for j in _FINGER_JOINTS], axis=1),
    }
    new = (lambda n, dt: np.empty(n, dt)) if alloc is None else (lambda n, dt: alloc(n * np.dtype(dt).itemsize).view(dt))
    if 'rgb' in image_keys:
      n = H * W * 3
      rgb, exact = rd.u8('rgb', n, out=new(T * n, np.uint8))
      if not exact:
        rgb = rd.f32('rgb', n, out=new(T * n, np.float32))
      if not raw_rgb:
        rgb = rgb.astype(np.float32) / np.float32(255.0)
      ex['rgb'] = rgb.reshape(T, H, W, 3)
    else:
      rd.frames('rgb')
      ex['rgb'] = _Omitted((T, H, W, 3), 'rgb')
    if 'depth' in image_keys:
      ex['depth'] = rd.f32('depth', H * W, out=new(T * H * W, np.float32)).reshape(T, H, W, 1)
    else:
      rd.frames('depth')
      ex['depth'] = _Omitted((T, H, W, 1), 'depth')
  return _finish_episode(ex, fetch_target)


class _Omitted:
  """Stands in for an image stream the caller chose not to decode (``image_keys``): has the shape, indexes like the
  array would (frames, windows), refuses to produce values."""

  def __init__(self, shape, key):
    self.shape, self.key, self.dtype = tuple(shape), key, np.dtype(np.float32)

  def __len__(self):
    return self.shape[0]

  def __getitem__(self, idx):
    lead = np.empty(self.shape[:1], np.bool_)[idx].shape
    return _Omitted(lead + self.shape[1:], self.key)

  def copy(self):
    return self

  def __array__(self, *a, **k):
    raise RuntimeError("feature '%s' was not decoded (image_keys / device_keys excluded it)" % self.key)


_FEATURE_KEYS = ['step', 'ts', 'rgb', 'depth', 'jnt_state', 'vel_state', 'ee_state', 'grp_state', 'goal_state',
                 'obj_state', 'cmd', 'ctrl']
_LABEL_KEYS = ['cmd', 'ctrl', 'vel_target', 'ee_target', 'grp_target']
_IMAGE_KEYS = ('rgb', 'depth')


def _concat_feature(vals):
  """One feature of several runs of windows (a list, in order) as one: DeviceWindows, undecoded streams or host arrays."""
  if len(vals) == 1:
    return vals[0]
  if isinstance(vals[0], DeviceWindows):
    return DeviceWindows.concat(*vals)
  if isinstance(vals[0], _Omitted):
    return _Omitted((sum(v.shape[0] for v in vals),) + vals[0].shape[1:], vals[0].key)
  return np.concatenate(vals, axis=0)


def _check_episode_length(T, meta, shard):
  """Sharded input: the data-parallel batch schedule (``dp_schedule``) counts on episodes of the meta file's length."""
  if shard is not None and T != meta.episode_length - 1:
    raise ValueError('an episode holds %d frames, meta_info.json says %d: the data-parallel batch schedule assumes '
                     'fixed-length episodes' % (T + 1, meta.episode_length))


def episode_windows(ex, window_size, starts, dev=None):
  """(features, labels) for the windows beginning at ``starts`` (_window_v3 :615-631, _prepare_v4 :373-399).
  With ``dev`` (episode_to_device) the image features are DeviceWindows instead of host arrays and ``ex`` needs only
  the per-frame states."""
  K = window_size
  starts = np.asarray(starts)
  idx = starts[:, None] + np.arange(K)[None, :]
  last = starts + K - 1
  if dev is not None:
    feats = {k: ex[k][idx] for k in _FEATURE_KEYS if k not in _IMAGE_KEYS}
    H, W = ex['_hw'] if '_hw' in ex else ex['rgb'].shape[1:3]
    for key, shp in (('rgb', (H, W, 3)), ('depth', (H, W, 1))):
      dw = DeviceWindows(K, shp, dev.get(key + '_div', 1.0))
      dw.add(dev.get(key), starts)
      feats[key] = dw
    if 'target_rgb' in dev or 'target_depth' in dev:
      for key, shp in (('target_rgb', (H, W, 3)), ('target_depth', (H, W, 1))):
        dw = DeviceWindows(1, shp, dev.get(key + '_div', 1.0), squeeze_k=True)
        dw.add(dev.get(key), np.zeros(len(starts), np.int32))
        feats[key] = dw
    return feats, {k: ex[k][last] for k in _LABEL_KEYS}
  feats = {k: ex[k][idx] for k in _FEATURE_KEYS}
  if 'target_rgb' in ex:
    n = len(starts)
    for k in ('target_rgb', 'target_depth'):
      t = ex[k]
      feats[k] = _Omitted((n,) + t.shape, t.key) if isinstance(t, _Omitted) else np.broadcast_to(t, (n,) + t.shape).copy()
  labels = {k: ex[k][last] for k in _LABEL_KEYS}
  return feats, labels


def shuffle_stream(items, buffer_size, rng):
  """tf.data's shuffle-buffer algorithm (``dataset.shuffle(buffer_size)``, geeco_gym.py:701-703) as a lazy generator: the buffer
  fills with the first ``buffer_size`` items; from then on every incoming item takes the place of a uniformly chosen buffer
  element, which is emitted; at the end of the stream the buffer drains in uniformly random order.  The item at input position
  i therefore never leaves before output position i - (buffer_size - 1); ``buffer_size`` = 1 is the identity.  ``rng``: a
  numpy Generator (only the algorithm is TensorFlow's, not its random stream)."""
  if buffer_size < 1:
    raise ValueError('shuffle_stream: buffer_size must be >= 1, got %r' % (buffer_size,))
  buf = []
  for item in items:
    if len(buf) < buffer_size:
      buf.append(item)
      continue
    j = int(rng.integers(len(buf)))
    out, buf[j] = buf[j], item
    yield out
  while buf:
    j = int(rng.integers(len(buf)))
    out, buf[j] = buf[j], buf[-1]
    buf.pop()
    yield out


def _assemble_picks(picks, K):
  """(features, labels) of a shuffled batch: ``picks`` = ((ex, dev), start) per window, in pick order.  Runs of consecutive picks
  from one episode go through one ``episode_windows`` call (and share a DeviceWindows segment); the runs are concatenated.  The
  DeviceWindows are marked ``scattered``."""
  runs = []       # [(ex, dev), [starts]]
  for ep, start in picks:
    if runs and runs[-1][0][0] is ep[0]:
      runs[-1][1].append(start)
    else:
      runs.append([ep, [start]])
  parts = [episode_windows(ex, K, np.asarray(starts), dev) for (ex, dev), starts in runs]
  feats = {k: _concat_feature([f[k] for f, _ in parts]) for k in parts[0][0]}
  labels = {k: _concat_feature([l[k] for _, l in parts]) for k in parts[0][1]}
  for v in feats.values():
    if isinstance(v, DeviceWindows):
      v.scattered = True
  return feats, labels


AUGMENT_STREAM = 0x617567      # third word of the augmentation generator's seed: a stream apart from the file order's and the shuffle's
AUGMENT_SCENE_STREAM = 0x7363656e      # ... and of the scene draws' generator (occluders, noise key): the shift / colour draws stay put
AUGMENT_SCENE_KEYS = ('noise', 'occlude', 'occlude_size')      # validated by check_augment_scene
AUGMENT_TIME_STREAM = 0x74696d65      # ... and of the time draws' generator (frame lag, frame drops): every other draw stays put
AUGMENT_TIME_KEYS = ('frame_drop', 'frame_lag')      # validated by check_augment_time
OCCLUDE_MAX = 4      # rectangle slots per window (include/geeco_hip.h: geeco_gather_windows_scene)


def check_augment(augment, hw=None):
  """``pickplace_input_fn(augment=...)`` validated: None (off: ``augment`` is None or every value is 0) or (S, g, b).  ``hw`` =
  (H, W) of the frames, when known: the shift must leave a part of the image in view."""
  if augment is None:
    return None
  if not isinstance(augment, dict):
    raise ValueError('augment must be None or dict(shift=S, gain=g, bias=b), got %r' % (augment,))
  for k in augment:
    if k not in ('shift', 'gain', 'bias') + AUGMENT_SCENE_KEYS + AUGMENT_TIME_KEYS:
      raise ValueError("augment: unknown key %r (the keys are 'shift', 'gain', 'bias', 'noise', 'occlude', 'occlude_size', "
                       "'frame_drop' and 'frame_lag')" % (k,))
  S, g, b = augment.get('shift', 0), augment.get('gain', 0.0), augment.get('bias', 0.0)
  if isinstance(S, (bool, np.bool_)) or not isinstance(S, (int, np.integer)) or S < 0:
    raise ValueError("augment['shift'] must be an integer >= 0 (whole pixels), got %r" % (S,))
  if hw is not None and S >= min(hw):
    raise ValueError("augment['shift'] must be smaller than the frames (%d x %d), got %r" % (hw[0], hw[1], S))
  for k, v, hi in (('gain', g, 1.0), ('bias', b, float('inf'))):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0 <= v < hi:
      raise ValueError("augment[%r] must be a number in [0, %s), got %r" % (k, '1' if k == 'gain' else 'inf', v))
  return None if (S == 0 and g == 0 and b == 0) else (int(S), float(g), float(b))


def check_augment_scene(augment, hw=None):
  """The scene keys of ``pickplace_input_fn(augment=...)`` validated: None (off: no dict, or ``noise`` and
  ``occlude`` both 0) or (sigma, R, f) -- ``noise`` = sigma in [0, 1), ``occlude`` = R in 0..4 rectangles at most per window,
  ``occlude_size`` = f in (0, 1], their largest side as a fraction of the frame's (default 0.25).  The other keys are
  ``check_augment``'s, which also refuses unknown ones; ``hw`` is accepted for symmetry with it (no value depends on the frame)."""
  if augment is None:
    return None
  check_augment({k: v for k, v in augment.items() if k not in AUGMENT_SCENE_KEYS} if isinstance(augment, dict) else augment, hw)
  sigma, R, f = augment.get('noise', 0.0), augment.get('occlude', 0), augment.get('occlude_size', 0.25)
  number = lambda v: not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating))
  if not number(sigma) or not 0 <= sigma < 1:
    raise ValueError("augment['noise'] must be a number in [0, 1), got %r" % (sigma,))
  if isinstance(R, (bool, np.bool_)) or not isinstance(R, (int, np.integer)) or not 0 <= R <= OCCLUDE_MAX:
    raise ValueError("augment['occlude'] must be an integer in 0..%d (rectangles per window at most), got %r" % (OCCLUDE_MAX, R))
  if not number(f) or not 0 < f <= 1:
    raise ValueError("augment['occlude_size'] must be a number in (0, 1], got %r" % (f,))
  return None if (sigma == 0 and R == 0) else (float(sigma), int(R), float(f))


def check_augment_time(augment, K=None):
  """The time keys of ``pickplace_input_fn(augment=...)`` validated: None (off: no dict, or ``frame_lag`` and
  ``frame_drop`` both 0) or (L, p) -- ``frame_lag`` = L, an integer >= 0: the camera lags the encoders by d ~ U{0..L} frames per
  window; ``frame_drop`` = p, a number in [0, 1): the chance that a slot k >= 1 shows what slot k - 1 shows.  ``K`` = the window
  size, when known: with K == 1 there is no slot to drop, ``frame_drop`` is accepted and does nothing; ``frame_lag`` still
  applies.  The other keys are ``check_augment``'s and ``check_augment_scene``'s; unknown ones are refused there."""
  if augment is None:
    return None
  if not isinstance(augment, dict):
    raise ValueError('augment must be None or a dict, got %r' % (augment,))
  L, p = augment.get('frame_lag', 0), augment.get('frame_drop', 0.0)
  if isinstance(L, (bool, np.bool_)) or not isinstance(L, (int, np.integer)) or L < 0:
    raise ValueError("augment['frame_lag'] must be an integer >= 0 (frames), got %r" % (L,))
  if isinstance(p, (bool, np.bool_)) or not isinstance(p, (int, float, np.integer, np.floating)) or not 0 <= p < 1:      # (NaN fails both)
    raise ValueError("augment['frame_drop'] must be a number in [0, 1), got %r" % (p,))
  if K is not None and K == 1:
    p = 0.0
  return None if (L == 0 and p == 0) else (int(L), float(p))


def draw_augment_time(rng, n, K, L, p):
  """The time draws of one emitted batch of ``n`` windows of ``K`` slots, in this order: the n lags d ~ integers U{0..L}, then an
  [n][K - 1] block of uniforms u in [0, 1): slot k >= 1 is dropped when u[i][k - 1] < p (both blocks are drawn whatever L and p
  are).  Returns ``src`` int32 [n][K], the recorded frame each slot shows as an offset from the window's start: the lag first,
  src[i][k] = k - d[i], then the drops on the lagged sequence, a dropped slot showing what slot k - 1 shows (drops chain; slot 0 is
  never dropped).  So src[i][0] = -d[i], rows do not decrease, and src[i][k] <= k.  The clamp at the episode's first frame is
  ``DeviceWindows.frame_addresses``'s."""
  d = rng.integers(0, L + 1, size=n)
  drop = rng.random((n, K - 1)) < p
  src = np.arange(K, dtype=np.int64)[None, :] - d[:, None]
  for k in range(1, K):
    src[:, k] = np.where(drop[:, k - 1], src[:, k - 1], src[:, k])
  return src.astype(np.int32)


def draw_augment(rng, n, S, g, b):
  """The draws of one emitted batch of ``n`` windows, in this order: dy, dx ~ integers U[-S, S] ([n][2]), gain_c ~ U[1 - g, 1 + g]
  ([n][3]), bias_c ~ U[-b, b] ([n][3])."""
  shift = rng.integers(-S, S + 1, size=(n, 2))
  gain = rng.uniform(1.0 - g, 1.0 + g, size=(n, 3))
  bias = rng.uniform(-b, b, size=(n, 3))
  return WindowAugment(shift, np.concatenate([gain, bias], axis=1))


def draw_augment_scene(rng, n, H, W, sigma, R, f):
  """The scene draws of one emitted batch of ``n`` windows of H x W frames, in this order: the noise key, two uint32 words (drawn
  whatever sigma is, so the rectangles do not depend on it); per window a count r ~ U{0..R}; per slot j < r: h ~ U{1..max(1,
  floor(f H))}, w ~ U{1..max(1, floor(f W))}, y0 ~ U{0..H - h}, x0 ~ U{0..W - w} and a colour of three U[0, 1) values; slots
  j >= r stay zero (empty).  Returns the keyword arguments WindowAugment takes: noise_key and sigma when sigma > 0, occ_rect
  [n][4][4] and occ_colour [n][4][3] when R > 0."""
  key = rng.integers(0, 1 << 32, size=2, dtype=np.uint64).astype(np.uint32)
  out = dict(noise_key=key, sigma=sigma) if sigma > 0 else {}
  if R > 0:
    rect, colour = np.zeros((n, OCCLUDE_MAX, 4), np.int32), np.zeros((n, OCCLUDE_MAX, 3), np.float32)
    hmax, wmax = max(1, int(np.floor(f * H))), max(1, int(np.floor(f * W)))
    for i in range(n):
      for j in range(int(rng.integers(0, R + 1))):
        h, w = int(rng.integers(1, hmax + 1)), int(rng.integers(1, wmax + 1))
        rect[i, j] = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w
        colour[i, j] = rng.random(3).astype(np.float32)
    out.update(occ_rect=rect, occ_colour=colour)
  return out


def _augment_batch(feats, rng, aug, scene_rng=None, scene=None, hw=None, time_rng=None, time=None):
  """Marks every DeviceWindows stream of an emitted batch with ONE WindowAugment drawn for it (``scene``: with the scene extras,
  ``time``: with the frame sources, each from their own generator; the frame sources are followed by the TIMED_KEYS streams)."""
  n = len(feats['step'])
  extras = draw_augment_scene(scene_rng, n, hw[0], hw[1], *scene) if scene is not None else {}
  if time is not None:
    K = next(v.K for k, v in feats.items() if k in TIMED_KEYS and isinstance(v, DeviceWindows))
    extras['frame_src'] = draw_augment_time(time_rng, n, K, *time)
  draws = draw_augment(rng, n, *(aug or (0, 0.0, 0.0)))
  draws = WindowAugment(draws.shift, draws.colour, **extras)
  for k, v in feats.items():
    if isinstance(v, DeviceWindows):
      v.augment, v.scene_tag, v.timed = draws, SCENE_TAGS.get(k, 0), k in TIMED_KEYS
  return feats


def weigh_batch(fn, features, labels):
  """``pickplace_input_fn(sample_weight=fn)``: ``fn(features, labels)`` -> one weight per sample of the batch, checked ([n], finite,
  >= 0) and stored as labels['sample_weight'] (float32) of a NEW label dict; nothing else of the batch is touched."""
  n = len(features['step'])
  w = np.asarray(fn(features, labels))
  if w.shape != (n,) or w.dtype == np.bool_ or not (np.issubdtype(w.dtype, np.floating) or np.issubdtype(w.dtype, np.integer)):
    raise ValueError('sample_weight: the function must return one number per sample, shape (%d,); got shape %s, dtype %s'
                     % (n, w.shape, w.dtype))
  w = w.astype(np.float32)
  if not np.isfinite(w).all() or (w < 0).any():
    raise ValueError('sample_weight: weights must be finite and >= 0, got %r' % (w,))
  return features, dict(labels, sample_weight=w)


class _Prefetcher:
  """Runs an iterator factory in a background thread (tf.data's prefetch); the episode readers it draws from are a
  thread pool of their own (``_EpisodeSource``)."""

  def __init__(self, make_iter, depth, device=None):
    self._q = queue.Queue(maxsize=max(int(depth), 1))
    self._device = device
    self._stop = threading.Event()
    self._t = threading.Thread(target=self._run, args=(make_iter,), daemon=True)
    self._t.start()

  def _put(self, item):
    while not self._stop.is_set():
      try:
        self._q.put(item, timeout=0.2)
        return True
      except queue.Full:
        continue
    return False

  def _run(self, make_iter):
    try:
      if self._device is not None and self._device.type == 'cuda':
        import torch
        torch.cuda.set_device(self._device)     # thread-local: a new thread starts on device 0 whatever LOCAL_RANK is
      for item in make_iter():
        if not self._put(('item', item)):
          return
      self._put(('end', None))
    except BaseException as e:   # surfaced in the consumer
      self._put(('error', e))

  def close(self):
    """Stops the producer (a consumer that leaves the epoch early, e.g. Estimator.train(steps=...))."""
    self._stop.set()

  def __del__(self):
    self._stop.set()

  def __iter__(self):
    while True:
      kind, val = self._q.get()
      if kind == 'item':
        yield val
      elif kind == 'end':
        return
      else:
        raise val


class _EpisodeSource:
  """Episodes of ``paths`` in order, read ``num_threads`` at a time (tf.data's num_parallel_reads /
  num_parallel_calls, geeco_gym.py:442-473: parallel and order-preserving): a window of reads runs ahead of the
  consumer in a thread pool; the native reader holds no Python lock, so the threads really overlap.  On the device
  path a cached episode (EPISODE_CACHE) is never read again."""

  def __init__(self, paths, meta, fetch_target, num_threads, device, image_keys, cache):
    from concurrent.futures import ThreadPoolExecutor
    self.paths, self.meta, self.fetch_target = list(paths), meta, fetch_target
    self.device, self.image_keys, self.cache = device, tuple(image_keys), cache
    self.num_threads = max(int(num_threads or 1), 1)
    self._pool = ThreadPoolExecutor(max_workers=self.num_threads, thread_name_prefix='geeco-reader')
    self._reads = 0

  def _read(self, path):
    staged = []
    def alloc(nbytes):
      t = _PINNED.take(nbytes)
      staged.append(t)
      return t.numpy()
    pinned = self.device is not None and self.device.type == 'cuda'
    ex = load_episode(path, self.meta, self.fetch_target, raw_rgb=self.device is not None, image_keys=self.image_keys,
                      alloc=alloc if pinned else None)
    return ex, staged

  def __iter__(self):
    """Yields (states / ex, dev or None) per episode, in the order of ``paths``."""
    ahead = self.num_threads + 1
    pending = collections.deque()      # (path, key, cached entry or future)
    it = iter(self.paths)

    def submit():
      for path in it:
        key = entry = None
        if self.device is not None and self.cache is not None:
          key = self.cache.key(path, self.device, self.fetch_target, self.image_keys)
          entry = self.cache.get(key)
        if entry is None:
          if not self._reads:     # the reader keeps one mapped inflate buffer (~105 MB) per thread + 1 between episodes
            _buffer_limit(self, self.num_threads + 1)
          self._reads += 1
        pending.append((path, key, entry if entry is not None else self._pool.submit(self._read, path)))
        return

    try:
      for _ in range(ahead):
        submit()
      while pending:
        path, key, item = pending.popleft()
        submit()
        if isinstance(item, tuple):
          yield item
          continue
        ex, staged = item.result()
        if self.device is None:
          yield ex, None
          continue
        states, dev = episode_to_device(ex, self.device, self.image_keys)
        for t in staged:          # the copies above were synchronous: the staging blocks are free again
          _PINNED.give(t)
        if self.cache is not None:
          self.cache.put(key, states, dev, self.device)
        yield states, dev
    finally:
      for _, _, item in pending:
        if not isinstance(item, tuple) and not item.cancel():
          item.add_done_callback(_return_staging)      # a read already running: nobody will take its result
      # reads already running finish (they cannot be interrupted inside the native reader).  An epoch that read NOTHING (every
      # episode came out of the HBM cache) hands the reader's spare inflate buffers back to the OS: no reader will run again, and
      # under data parallelism every rank would otherwise hold its own pool (up to num_threads + 1 buffers of ~105 MB) for the
      # rest of training.  An epoch that did read keeps them for the next one (sixteen threads faulting fresh 105 MB mappings in
      # at once cost epoch 1 of the bench 0.13 s when the pool was emptied after every epoch).
      # (not waited for: an epoch left early -- Estimator.train(steps=...), an exception in the step -- returns at once)
      self._pool.shutdown(wait=False)
      _buffer_limit(self, None)
      if not self._reads:
        # off this thread: unmapping up to num_threads + 1 touched 105 MB buffers takes ~0.15 s (measured: the first fully cached
        # epoch of the bench ran 0.68 s instead of 0.53 s with the release inline); nothing waits for it
        threading.Thread(target=tfrecord._host().geeco_host_release_buffers, name='geeco-release', daemon=True).start()


def _return_staging(fut):
  """Done-callback of a read whose result nobody takes (the epoch was left early): its pinned staging blocks go back."""
  if fut.cancelled() or fut.exception() is not None:
    return
  for t in fut.result()[1]:
    _PINNED.give(t)


_LIMITS, _LIMITS_LOCK = {}, threading.Lock()


def _buffer_limit(source, n):
  """The native reader's spare-buffer limit is ONE number per process (geeco_host_set_buffer_limit): with several sources alive
  (a train and an eval pipeline with different thread counts) it is the MAX of what they asked for; ``n`` None = the source is done
  (the limit stays where it is while no source reads, so the next epoch finds the buffers of this one)."""
  with _LIMITS_LOCK:
    if n is None:
      _LIMITS.pop(id(source), None)
    else:
      _LIMITS[id(source)] = int(n)
    if _LIMITS:
      tfrecord._host().geeco_host_set_buffer_limit(max(_LIMITS.values()))


def usable_host_cores():
  """Host threads this process may use: the affinity mask capped by the cgroup CPU quota."""
  n = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
  try:
    with open('/sys/fs/cgroup/cpu.max') as f:
      quota, period = f.read().split()
    if quota != 'max':
      n = min(n, max(1, int(int(quota) / int(period))))
  except (OSError, ValueError):
    pass
  return max(1, n)


def default_reader_threads(world=1):
  """``num_threads=None``: this rank's share of the host, usable cores // ranks ON THIS NODE (LOCAL_WORLD_SIZE as torchrun exports
  it; ``world`` -- the global size -- only where that is absent, i.e. one node), within 4 (the reference's default,
  train_e2evmc.py:67) ... 32.  Reading an episode is 97 % inflate and scales with threads up to the cores a rank owns
  (profiles/r05/reader_scaling.json): one rank's GPU consumes ~119 episodes/s, one reader thread delivers ~9, so epoch 1 (before
  the HBM episode cache serves everything) is reader-bound below ~13 cores per rank."""
  try:
    local = int(os.environ.get('LOCAL_WORLD_SIZE', '') or world)
  except ValueError:
    local = world
  return max(4, min(32, usable_host_cores() // max(min(int(local), max(int(world), 1)), 1)))


def pickplace_input_fn(dataset_dir, split_name, mode, encoding='v4', window_size=4, fetch_target=False,
                       shuffle_buffer=128, batch_size=1, num_epochs=1, num_threads=4, prefetch_size=4, seed=None,
                       shard=None, device=None, device_keys=None, cache=True, shuffle_windows=False, augment=None, sample_weight=None):
  """Same signature as the reference's pickplace_input_fn (geeco_gym.py:234-279).  Returns an iterable of
  (features, labels) numpy batches.  ``num_threads`` episodes are read in parallel, in order (num_parallel_reads /
  num_parallel_calls of :442-473; None = ``default_reader_threads``: this rank's share of the host cores); ``prefetch_size`` batches are prepared ahead of the consumer (:473).
  Extensions: ``shard = (rank, world)`` makes each data-parallel rank read a disjoint, rank-strided subset of the
  episodes.  ``device`` (e.g. 'cuda'): upload every episode's frames once and hand out image features as DeviceWindows
  (windows are gathered in HBM); ``device_keys``: which image streams the model reads (default both; ('rgb',) for an
  RGB-only model skips decoding, uploading and caching 26 MB of depth per episode — the 'depth' features then refuse
  to materialise); ``cache``: keep uploaded episodes in HBM across epochs (EPISODE_CACHE; True, False or an
  EpisodeCache).
  ``shuffle_windows`` ('train' mode of an on-disk dataset only; off by default): the sample-level shuffle the reference's v1-v3
  pipelines run (``dataset.shuffle(buffer_size=shuffle_buffer, seed=seed)``, :701-703; commented out in v4, :446-448).  The
  window stream -- episodes in their shuffled file order, windows ascending -- passes through ``shuffle_stream`` with a buffer of
  ``shuffle_buffer`` windows, drained at every epoch boundary (shuffle(...).repeat(...)); the generator is
  ``default_rng([seed, rank])`` (rank 0 unless sharded; a fresh one for ``seed`` None).  The buffer holds (episode, start) pairs,
  never pixels: a batch is built from its picks when it is emitted, and on the ``device`` path an episode's resident frames stay
  referenced while one of its windows waits.  ``dp_schedule`` is the unshuffled one (it depends on counts only).  Without the
  option ``shuffle_buffer`` is accepted and unused, as before.
  ``augment`` = None | dict(shift=S, gain=g, bias=b) ('train' mode of an on-disk dataset on the ``device`` path only; off by
  default and when all three are 0; the reference has no augmentation): every emitted window is moved by a whole-pixel shift
  dy, dx ~ U{-S..S} (zeros move in; 0 <= S < min(H, W)) and its RGB channels become clip(v * gain_c + bias_c, 0, 1) with
  gain_c ~ U[1 - g, 1 + g] (0 <= g < 1) and bias_c ~ U[-b, b] (b >= 0).  One draw per window serves its K frames and its
  'target_rgb'; 'depth' / 'target_depth' take the same shift and no colour.  The host only draws (``draw_augment``, per emitted
  batch, generator ``default_rng([seed, rank, AUGMENT_STREAM])``: file order and shuffle picks are those without the option); the
  pixels are transformed on the device by the gather that builds the dense windows (DeviceWindows.augment).  Without
  ``device`` it raises; other modes and ``synthetic:`` inputs ignore it.
  Scene keys of the same dict (RGB streams only, depth keeps the shift alone; off by default, independent of the
  three above): ``noise=sigma`` in [0, 1) adds sigma * z, z ~ N(0, 1) independent per window, frame, pixel and channel (and between
  'rgb' and 'target_rgb'), then clips to [0, 1]; ``occlude=R`` in 0..4 paints up to R rectangles per window, one constant colour
  each, the same in its K frames and its 'target_rgb' (a static distractor), with sides up to ``occlude_size`` (default 0.25) of
  the frame's.  Order per element: shift / tint, rectangles, noise.  Their draws (``draw_augment_scene``) come from
  ``default_rng([seed, rank, AUGMENT_SCENE_STREAM])``, so file order, shuffle picks and the shift / colour draws are those without
  them.
  Time keys of the same dict (off by default, independent of the keys above): the deployed camera drops frames and
  lags the joint encoders, the recorded windows do neither.  ``frame_lag=L`` (integer >= 0): per window one lag d ~ U{0..L}, slot k
  of its 'rgb' and 'depth' shows recorded frame start + k - d, clamped at the episode's first frame (the scene is at rest there).
  ``frame_drop=p`` in [0, 1): per window and slot k >= 1 an independent chance p that the slot shows what slot k - 1 shows (drops
  chain; slot 0 is never dropped).  The lag is applied first, then the drops on the lagged sequence.  'rgb' and 'depth' take the
  same frame sources (the camera delivers both together).  'target_rgb', 'target_depth', every per-frame state feature and every
  label are NOT touched: proprioception and labels stay fresh, which is the point -- the images go stale against them.  Their
  draws (``draw_augment_time``) come from ``default_rng([seed, rank, AUGMENT_TIME_STREAM])``, so file order, shuffle picks, shift /
  colour draws and scene draws are those without them.
  ``sample_weight`` = None | fn(features, labels) -> [n] array (every mode, host and ``device`` path, ``synthetic:`` inputs too): the
  weight per sample that params['loss_shaping']['sample_weights'] reads.  Called on every emitted batch, the ragged
  last one included, behind the augmentation draws; its result is checked (shape, finite, >= 0: ``weigh_batch``) and stored as
  labels['sample_weight'].  Every other feature and label is what it is without the option."""
  if shuffle_windows and int(shuffle_buffer) < 1:
    raise ValueError('shuffle_windows needs shuffle_buffer >= 1, got %r' % (shuffle_buffer,))
  check_augment(augment)
  check_augment_scene(augment)
  check_augment_time(augment)
  if encoding != 'v4':
    # v1-v3 are dead code in the reference (undefined PickAndPlaceEncodingV1/2/3 -> NameError)
    raise KeyError(encoding)
  if num_threads is None:
    num_threads = default_reader_threads(shard[1] if shard is not None else 1)
  if sample_weight is not None and not callable(sample_weight):
    raise ValueError('sample_weight=%r: None or a function (features, labels) -> one weight per sample' % (sample_weight,))
  if dataset_dir.startswith('synthetic:'):
    it = synthetic_from_spec(dataset_dir, mode, window_size, fetch_target, batch_size, seed)
    return it if sample_weight is None else (weigh_batch(sample_weight, f, l) for f, l in it)
  meta = get_meta_v4(dataset_dir)
  paths = collect_tfrecords(dataset_dir, split_name, mode)
  if mode == 'train':   # record-level shuffle only (:436-437)
    if shard is not None and seed is None:
      raise ValueError('sharded training input needs one seed shared by all ranks (they must agree on the episode order)')
    np.random.default_rng(seed).shuffle(paths)
  shuffle_windows = bool(shuffle_windows) and mode == 'train'      # the reference's shuffles are train-only too (:436, :701)
  K = window_size
  dp_schedule = None
  if shard is not None:
    # every rank reads its own rank-strided subset of the episodes.  Episodes have the fixed length
    # of the meta file (pickplace.py:157), so each rank can work out how many windows EVERY rank contributes to
    # each step without talking to the others: dp_schedule[s][r] = windows of rank r in step s.
    rank, world = shard
    nwin = (meta.episode_length - 1) - K + 1
    per_rank = [len(paths[r::world]) * nwin * num_epochs for r in range(world)]
    steps = max(-(-w // batch_size) for w in per_rank) if per_rank else 0
    dp_schedule = [tuple(max(0, min(batch_size, w - s * batch_size)) for w in per_rank) for s in range(steps)]
    paths = paths[rank::world]
  aug = check_augment(augment, (meta.img_height, meta.img_width)) if mode == 'train' else None      # train-only, as the shuffles
  scene = check_augment_scene(augment, (meta.img_height, meta.img_width)) if mode == 'train' else None
  time = check_augment_time(augment, K) if mode == 'train' else None
  if (aug is not None or scene is not None or time is not None) and device is None:
    raise ValueError("augment needs device= (e.g. 'cuda'): the windows are transformed on the device, where the resident frames "
                     "are; the host path has no augmentation")
  if device is not None:
    device = resolve_device(device)
  image_keys = _IMAGE_KEYS if device_keys is None else tuple(device_keys)
  if not set(image_keys) <= set(_IMAGE_KEYS):
    raise ValueError('device_keys must be a subset of %s' % (_IMAGE_KEYS,))
  ep_cache = None
  if device is not None and device.type == 'cuda' and cache:
    ep_cache = cache if isinstance(cache, EpisodeCache) else EPISODE_CACHE
  print('[pickplace_input_fn_v4] #tfrecords: %d' % len(paths))

  def emitter():
    """What a finished batch passes through on its way out: the augmentation draws, in emission order, then the sample weights."""
    weigh = (lambda f, l: (f, l)) if sample_weight is None else (lambda f, l: weigh_batch(sample_weight, f, l))
    if aug is None and scene is None and time is None:
      return weigh
    stream = lambda word: np.random.default_rng(None if seed is None else [seed, shard[0] if shard is not None else 0, word])
    rng, scene_rng, time_rng = stream(AUGMENT_STREAM), stream(AUGMENT_SCENE_STREAM), stream(AUGMENT_TIME_STREAM)
    return lambda f, l: weigh(_augment_batch(f, rng, aug, scene_rng, scene, (meta.img_height, meta.img_width), time_rng, time), l)

  def shuffled_batches():
    import itertools
    rng = np.random.default_rng(None if seed is None else [seed, shard[0] if shard is not None else 0])
    source = iter(_EpisodeSource(paths * num_epochs, meta, fetch_target, num_threads, device, image_keys, ep_cache))

    def windows(episodes):
      for ep in episodes:
        T = ep[0]['step'].shape[0]
        _check_episode_length(T, meta, shard)
        for start in range(T - K + 1):
          yield ep, start

    picks = []      # the batch being filled; only the batch that straddles an epoch boundary mixes epochs, as without the shuffle
    emit = emitter()
    try:
      for _ in range(num_epochs):
        for pick in shuffle_stream(windows(itertools.islice(source, len(paths))), int(shuffle_buffer), rng):
          picks.append(pick)
          if len(picks) == batch_size:
            yield emit(*_assemble_picks(picks, K))
            picks = []
      if picks:     # ragged final batch
        yield emit(*_assemble_picks(picks, K))
    finally:
      source.close()    # (a generator: runs _EpisodeSource's clean-up now, not when it is collected)

  def batches():
    carry_f, carry_l = None, None   # windows left over from the previous episode (batch() spans episodes)
    emit = emitter()
    source = _EpisodeSource(paths * num_epochs, meta, fetch_target, num_threads, device, image_keys, ep_cache)
    for ex, dev in source:
      T = ex['step'].shape[0]
      _check_episode_length(T, meta, shard)
      nwin = T - K + 1
      pos = 0
      while pos < nwin:
        need = batch_size - (0 if carry_f is None else len(carry_f['step']))
        take = min(need, nwin - pos)
        f, l = episode_windows(ex, K, np.arange(pos, pos + take), dev)
        pos += take
        if carry_f is not None:
          f = {k: _concat_feature([carry_f[k], f[k]]) for k in f}
          l = {k: np.concatenate([carry_l[k], l[k]], axis=0) for k in l}
          carry_f = carry_l = None
        if len(f['step']) == batch_size:
          yield emit(f, l)
        else:
          carry_f, carry_l = f, l
    if carry_f is not None:   # ragged final batch (dataset.batch without drop_remainder, :471)
      yield emit(carry_f, carry_l)

  it = _Prefetcher(shuffled_batches if shuffle_windows else batches, prefetch_size, device)
  it.dp_schedule = dp_schedule
  return it
