"""Synthetic data and fixture writers: seeded random batches with the reader's feature / label dictionaries, and
episodes / dataset directories in the reference's on-disk format.  input_fn.py re-exports every name of this module."""
import collections
import json
import os

import numpy as np

from . import tfrecord


def synthetic_batches(batch_size, window_size, num_batches, img_hw=(256, 256), channels=3, fetch_target=True, seed=1234):
  """Seeded random batches with the feature / label dictionaries of _prepare_v4."""
  H, W = img_hw
  K = window_size

  def gen():
    r = np.random.default_rng(seed)
    for b in range(num_batches):
      N = batch_size
      f = {
          'step': (np.arange(K)[None, :] + r.integers(1, 80, size=[N, 1])).astype(np.int64),
          'ts': r.random([N, K], dtype=np.float32),
          'rgb': r.integers(0, 256, size=[N, K, H, W, 3]).astype(np.float32) / np.float32(255.0),
          'depth': (0.5 + 2.5 * r.random([N, K, H, W, 1], dtype=np.float32)),
          'jnt_state': r.standard_normal([N, K, 7]).astype(np.float32),
          'vel_state': r.standard_normal([N, K, 7]).astype(np.float32),
          'ee_state': 1.5 * r.random([N, K, 7], dtype=np.float32),
          'grp_state': 0.05 * r.random([N, K, 2], dtype=np.float32),
          'goal_state': 1.5 * r.random([N, K, 7], dtype=np.float32),
          'obj_state': 1.5 * r.random([N, K, 7], dtype=np.float32),
          'ctrl': r.standard_normal([N, K, 2]).astype(np.float32),
      }
      cmd = np.concatenate([0.3 * r.standard_normal([N, K, 3]), r.integers(-1, 2, size=[N, K, 1])], axis=2)
      f['cmd'] = cmd.astype(np.float32)
      if fetch_target:
        f['target_rgb'] = r.integers(0, 256, size=[N, H, W, 3]).astype(np.float32) / np.float32(255.0)
        f['target_depth'] = (0.5 + 2.5 * r.random([N, H, W, 1], dtype=np.float32))
      l = {'cmd': f['cmd'][:, -1], 'ctrl': f['ctrl'][:, -1], 'vel_target': r.standard_normal([N, 7]).astype(np.float32),
           'ee_target': r.random([N, 7], dtype=np.float32), 'grp_target': r.random([N, 2], dtype=np.float32)}
      yield f, l
  return gen


def synthetic_from_spec(spec, mode, window_size, fetch_target, batch_size, seed):
  """``--dataset_dir synthetic:<num_batches>[:<H>x<W>]`` (no dataset on disk; used by the benches and tests)."""
  parts = spec.split(':')
  nb = int(parts[1]) if len(parts) > 1 and parts[1] else 8
  hw = tuple(int(x) for x in parts[2].split('x')) if len(parts) > 2 else (256, 256)
  if mode != 'train':
    nb = max(1, nb // 4)
  base = 1234 if seed is None else seed
  return synthetic_batches(batch_size, window_size, nb, hw, 3, fetch_target, seed=base + (0 if mode == 'train' else 1))()


def write_episode(path, meta, frames_rgb_u8, depth, cmd, ctrl, joints_qpos, joints_qvel, mocap_qpos, obj_qpos,
                  goal_qpos, ts=None, task_goal='goal', task_object='object'):
  """Writes one episode in the reference's on-disk format (PickAndPlaceEncodingV4: geeco_gym.py:117-176,
  data_recorder.py:37-59,134-156).  Used to build fixtures and synthetic datasets, not by training."""
  T = frames_rgb_u8.shape[0]
  ctx = collections.OrderedDict([
      ('episode_length', np.array([meta.episode_length], np.int64)), ('img_height', np.array([meta.img_height], np.int64)),
      ('img_width', np.array([meta.img_width], np.int64)), ('monitored_joints', list(meta.monitored_joints)),
      ('actuated_joints', list(meta.actuated_joints)), ('monitored_mocaps', list(meta.monitored_mocaps)),
      ('monitored_objects', list(meta.monitored_objects)), ('dim_cmd', np.array([meta.dim_cmd], np.int64)),
      ('dim_ctrl', np.array([meta.dim_ctrl], np.int64)), ('task_goal', task_goal), ('task_object', task_object)])
  frames = []
  for t in range(T):
    fr = collections.OrderedDict()
    fr['step'] = np.array([t], np.int64)
    fr['ts'] = np.array([0.04 * t if ts is None else ts[t]], np.float32)
    fr['rgb'] = frames_rgb_u8[t]          # uint8 -> float list (tfrecord.py:73-74)
    fr['depth'] = depth[t].astype(np.float32)
    fr['cmd'] = cmd[t].astype(np.float32)
    fr['ctrl'] = ctrl[t].astype(np.float32)
    fr['goal_qpos'] = goal_qpos[t].astype(np.float32)
    fr['obj_qpos'] = obj_qpos[t].astype(np.float32)
    for j, name in enumerate(meta.monitored_joints):
      fr['joint_qpos-%s' % name] = np.array([joints_qpos[t, j]], np.float32)
      fr['joint_qvel-%s' % name] = np.array([joints_qvel[t, j]], np.float32)
    for name in meta.monitored_mocaps:
      fr['mocap_qpos-%s' % name] = mocap_qpos[t].astype(np.float32)
    for name in meta.monitored_objects:
      fr['object_qpos-%s' % name] = obj_qpos[t].astype(np.float32)
    frames.append(fr)
  tfrecord.write_records(path, [tfrecord.encode_sequence_example(ctx, frames)], 'zlib')


def synthetic_scene_frames(T, H, W, seed):
  """uint8 RGB frames [T, H, W, 3] + float32 depth [T, H, W, 1] of a toy table-top scene (shaded background, a textured
  table, a few boxes sliding between frames): flat and smooth regions with a little sensor-like noise, which is what
  makes a rendered frame compress — uniform noise (test fixtures) would not.  Generator of on-disk datasets for the
  input-pipeline benchmark; not part of training."""
  r = np.random.default_rng(seed)
  yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
  base = np.stack([90 + 60 * yy / H, 110 + 40 * xx / W, 140 - 50 * yy / H], axis=-1)            # wall gradient
  table = yy > 0.55 * H
  tex = r.integers(-6, 7, size=[H, W, 1]).astype(np.float32) * table[..., None]
  base = np.where(table[..., None], np.float32([150, 120, 90]) + tex, base)
  depth0 = (2.5 - 1.5 * yy / H + 0.02 * np.sin(xx / 9.0)).astype(np.float32)
  nbox = 4
  pos0, vel = r.random([nbox, 2]) * [0.4 * H, 0.8 * W] + [0.5 * H, 0.0], r.standard_normal([nbox, 2]) * 0.6
  size = r.integers(H // 16, H // 6, size=[nbox, 2])
  col = r.integers(20, 236, size=[nbox, 3]).astype(np.float32)
  rgb = np.empty([T, H, W, 3], np.uint8)
  depth = np.empty([T, H, W, 1], np.float32)
  for t in range(T):
    img, dep = base.copy(), depth0.copy()
    for b in range(nbox):
      y0, x0 = (pos0[b] + t * vel[b]).astype(int) % [H, W]
      y1, x1 = min(H, y0 + size[b, 0]), min(W, x0 + size[b, 1])
      shade = np.linspace(1.0, 0.8, max(x1 - x0, 1), dtype=np.float32)[None, :, None]
      img[y0:y1, x0:x1] = col[b] * shade
      dep[y0:y1, x0:x1] = 0.8 + 0.1 * b
    noise = r.integers(-1, 2, size=[H, W, 3]) * (r.random([H, W, 1]) < 0.15)                   # sparse +-1 sensor noise
    rgb[t] = np.clip(np.rint(img + noise), 0, 255).astype(np.uint8)
    depth[t, :, :, 0] = dep + (1e-3 * r.standard_normal([H, W])).astype(np.float32)
  return rgb, depth


def write_synthetic_dataset(root, num_episodes, episode_length=100, img_hw=(256, 256), seed=0, eval_episodes=None):
  """A dataset directory in the reference's layout (geeco_gym.py:249-264: meta/meta_info.json, data/*.tfrecord.zlib,
  splits/default/{train,eval}.txt) filled with ``synthetic_scene_frames`` episodes.  ``eval_episodes``: how many of
  the episodes the eval split lists (default: all).  Returns the meta tuple."""
  from .input_fn import _ARM_JOINTS, _FINGER_JOINTS, PickAndPlaceMetaV4      # (input_fn imports this module)
  H, W = img_hw
  joints = ['robot0:%s' % j for j in _ARM_JOINTS + _FINGER_JOINTS]
  meta = PickAndPlaceMetaV4(episode_length=episode_length, img_height=H, img_width=W, monitored_joints=joints,
                            actuated_joints=joints[:2], monitored_mocaps=['robot0:mocap'],
                            monitored_objects=['object0:joint'], dim_cmd=4, dim_ctrl=2)
  for sub in ('meta', 'data', os.path.join('splits', 'default')):
    os.makedirs(os.path.join(root, sub), exist_ok=True)
  with open(os.path.join(root, 'meta', 'meta_info.json'), 'w') as fp:
    json.dump(meta._asdict(), fp)
  names = []
  for e in range(num_episodes):
    r = np.random.default_rng([seed, e])
    T = episode_length
    rgb, depth = synthetic_scene_frames(T, H, W, seed=[seed, e, 1])
    cmd = np.concatenate([0.3 * r.standard_normal([T, 3]), r.integers(-1, 2, [T, 1])], 1).astype(np.float32)
    name = 'ep%05d.tfrecord.zlib' % e
    write_episode(os.path.join(root, 'data', name), meta, rgb, depth, cmd, r.standard_normal([T, 2]).astype(np.float32),
                  r.standard_normal([T, 9]).astype(np.float32), r.standard_normal([T, 9]).astype(np.float32),
                  (1.5 * r.random([T, 7])).astype(np.float32), (1.5 * r.random([T, 7])).astype(np.float32),
                  (1.5 * r.random([T, 7])).astype(np.float32))
    names.append(name)
  n_eval = num_episodes if eval_episodes is None else eval_episodes
  for mode, sel in (('train', names), ('eval', names[:n_eval])):
    with open(os.path.join(root, 'splits', 'default', mode + '.txt'), 'w') as fp:
      fp.write('\n'.join(sel) + '\n')
  return meta
