#!/usr/bin/env python
"""Replays a trained controller over the recorded episodes of a dataset split: what would it have commanded at every frame, and
how far is that from what was recorded?  The per-frame controllers go through EpisodeReplay, geeco-f (proc_obs 'dynimg') and
'sequence' x 'dyndiff' through DynamicImageReplay (geeco_amd.open_replay picks by the run's config).

  python scripts/replay_episodes.py --model_dir RUN --dataset_dir DATA --split val --out replay.npz

prints one per-head table per episode and one over all episodes, and writes (frames of all episodes along the leading axis):
  <head> [frames][size]          the prediction at every frame, per head ('cmd_ee', 'logits_cmd_grp', ... as Estimator.predict);
  errors [frames][heads]         per frame: mean squared error of a regression head, 1 / 0 gripper class hit for the logits;
  episode_errors [episodes][heads]   their means over each episode;
  episode_lengths / episode_names [episodes], heads [heads].
--split names the list of the split directory that is read ('train' / 'eval'; 'val' = 'eval'), --split_name the directory.
Goal models take each episode's last frame as the goal (the dataset's 'target_rgb').
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from geeco_amd import replay as rp      # noqa: E402
from geeco_amd.replay_dynimg import open_replay      # noqa: E402


def parse_args(argv=None):
  ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument('--model_dir', required=True, help='run directory (e2evmc_config.json + checkpoints)')
  ap.add_argument('--checkpoint_name', default=None)
  ap.add_argument('--use_ema', action='store_true')
  ap.add_argument('--dataset_dir', required=True)
  ap.add_argument('--split_name', default='default')
  ap.add_argument('--split', default='val', help="which list of the split: 'train', 'eval' or 'val' (= 'eval')")
  ap.add_argument('--max_frames', type=int, default=512)
  ap.add_argument('--chunk_frames', type=int, default=None)
  ap.add_argument('--out', required=True, help='OUT.npz')
  return ap.parse_args(argv)


def table(title, keys, values):
  lines = [title] + ['  %-16s %.6g' % (k, v) for k, v in zip(keys, values)]
  return '\n'.join(lines)


def main(argv=None):
  args = parse_args(argv)
  mode = 'eval' if args.split == 'val' else args.split
  r = open_replay(args.model_dir, args.checkpoint_name, use_ema=args.use_ema, max_frames=args.max_frames, chunk_frames=args.chunk_frames)
  keys = [k for k, _, _ in r.heads]
  outs, names = [], []
  for ep in rp.dataset_episodes(args.dataset_dir, args.split_name, mode, r.device, fetch_target=r.goal):
    out = r.replay(ep)
    outs.append(out)
    names.append(ep['name'])
    print(table('%s: %d frames' % (ep['name'], len(out['errors'])), keys, [out['episode_errors'][k] for k in keys]))
  if not outs:
    raise SystemExit('replay_episodes.py: the split lists no episode')
  arrays = {k: np.concatenate([o[k] for o in outs], axis=0) for k in keys + ['errors']}
  arrays['episode_errors'] = np.asarray([[o['episode_errors'][k] for k in keys] for o in outs], np.float32)
  arrays['episode_lengths'] = np.asarray([len(o['errors']) for o in outs], np.int64)
  arrays['episode_names'] = np.asarray(names)
  arrays['heads'] = np.asarray(keys)
  print(table('all %d episodes, %d frames (mean over frames)' % (len(outs), len(arrays['errors'])), keys,
              arrays['errors'].astype(np.float64).mean(axis=0)))
  np.savez(args.out, **arrays)
  print('replay_episodes.py: -> %s' % args.out)


if __name__ == '__main__':
  main()
