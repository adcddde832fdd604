#!/usr/bin/env python
"""Saliency maps of a trained controller: which pixels drive this command?

  python scripts/saliency.py --model_dir RUN --dataset_dir DATA --split default --num_windows 8 --heads cmd_ee --out sal.npz

writes, per window (leading axis = window):
  rgb / target_rgb / depth / target_depth   the frames the gradient was taken at, as the model has them;
  grad_rgb / grad_target_rgb / ...          the raw gradients d(loss)/d(frames), shaped like the frames (Estimator.input_gradients);
  saliency [n][K][H][W]                     max over the colour channels of |grad_rgb|, per frame;
  saliency_target [n][H][W]                 the same of the target frame (goal models);
  loss [batches]                            the loss that was differentiated, per batch.
--method integrated_gradients | smoothgrad (default gradient: the plain gradient above, same output as ever) puts the
attributions of Estimator.attributions in the grad_* arrays' place under attr_*, takes saliency / saliency_target from the device's
finish, and adds sample_sum and, for integrated gradients, completeness_gap per window and loss_baseline per batch; --steps, --noise_std and
--baseline black | FILE.npy (a [H][W][3] frame or an array shaped like a batch's rgb) go with it.
--method occlusion | rise (Estimator.perturbation_attributions: gradient-free, forwards only) writes instead of the
gradients saliency [n][H][W] (ONE map per window: the occluder is shared by its frames), coverage [n][H][W], scores [n][M] and, for
occlusion, patch_scores [n][Gy][Gx], and the same under *_target for goal models; --patch, --stride (occlusion), --grid, --keep_prob,
--steps (rise), --fill black | R,G,B | FILE.npy and --score prediction | loss go with them; --heads then picks the scored heads.
--heads picks the heads whose losses are summed (default: the training loss).  --synthetic runs on generated frames and random
initial weights when --model_dir holds no checkpoint (a smoke run of the whole path, no dataset needed).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from geeco_amd import estimator as est      # noqa: E402
from geeco_amd.estimator import e2evmc_model_fn, goal_e2evmc_model_fn      # noqa: E402
from geeco_amd.params import create_e2evmc_config      # noqa: E402
from geeco_amd.utils import load_model_config      # noqa: E402

IMAGE_KEYS = ('rgb', 'target_rgb', 'depth', 'target_depth')


def saliency_of(grad_rgb):
  """max_c |d rgb| over the colour axis (the last one)."""
  return np.abs(grad_rgb).max(axis=-1)


def parse_args(argv=None):
  ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument('--model_dir', default=None, help='run directory (e2evmc_config.json + checkpoints)')
  ap.add_argument('--goal_condition', default='target', choices=('none', 'target'))
  ap.add_argument('--dataset_dir', default=None)
  ap.add_argument('--split', default='default')
  ap.add_argument('--mode', default='eval', help='which list of the split to read (train / eval)')
  ap.add_argument('--num_windows', type=int, default=8)
  ap.add_argument('--batch_size', type=int, default=4)
  ap.add_argument('--heads', default=None, help='comma-separated head names, e.g. cmd_ee or cmd_grp; default: the training loss')
  ap.add_argument('--method', default='gradient', choices=('gradient', 'integrated_gradients', 'smoothgrad', 'occlusion', 'rise'))
  ap.add_argument('--steps', type=int, default=16, help='--method integrated_gradients / smoothgrad: path points / noise draws')
  ap.add_argument('--noise_std', type=float, default=0.1, help='--method smoothgrad: the noise\'s standard deviation')
  ap.add_argument('--baseline', default='black', help="--method integrated_gradients: 'black' or FILE.npy")
  ap.add_argument('--patch', type=int, default=None, help='--method occlusion: the square patch\'s side (default: a quarter of the image)')
  ap.add_argument('--stride', type=int, default=None, help='--method occlusion: the grid\'s stride (default: half the patch)')
  ap.add_argument('--grid', type=int, default=7, help='--method rise: the mask grid g, 2..31')
  ap.add_argument('--keep_prob', type=float, default=0.5, help='--method rise: the probability that a grid cell is kept')
  ap.add_argument('--fill', default='black', help="--method occlusion / rise: what a hidden pixel shows: 'black', R,G,B or FILE.npy")
  ap.add_argument('--score', default='prediction', choices=('prediction', 'loss'), help='--method occlusion / rise')
  ap.add_argument('--out', required=True, help='OUT.npz')
  ap.add_argument('--synthetic', action='store_true', help='generated frames instead of a dataset')
  ap.add_argument('--img_size', type=int, default=256, help='--synthetic: frame height and width')
  ap.add_argument('--window_size', type=int, default=4, help='without a saved config: the window length')
  ap.add_argument('--proc_obs', default='dynimg')
  ap.add_argument('--proc_tgt', default='dyndiff')
  return ap.parse_args(argv)


def main(argv=None):
  args = parse_args(argv)
  if not args.synthetic and not args.dataset_dir:
    raise SystemExit('saliency.py: --dataset_dir or --synthetic')
  if args.model_dir and os.path.exists(os.path.join(args.model_dir, 'e2evmc_config.json')):
    cfg = create_e2evmc_config(load_model_config(args.model_dir, 'e2evmc_config'))
  else:
    cfg = create_e2evmc_config(dict(window_size=args.window_size, proc_obs=args.proc_obs, proc_tgt=args.proc_tgt,
                                    batch_size=args.batch_size, img_height=args.img_size, img_width=args.img_size))
  goal = args.goal_condition == 'target'
  heads = tuple(h for h in args.heads.split(',') if h) if args.heads else None
  N = max(1, min(args.batch_size, args.num_windows))
  nb = -(-args.num_windows // N)
  if args.synthetic:
    from geeco_amd.synthetic import synthetic_batches
    source = synthetic_batches(N, cfg.window_size, nb, (cfg.img_height, cfg.img_width), 3, goal, seed=4321)
  else:
    from geeco_amd.input_fn import pickplace_input_fn
    source = lambda: pickplace_input_fn(args.dataset_dir, args.split, args.mode, window_size=cfg.window_size, fetch_target=goal,
                                        batch_size=N, num_epochs=1)

  def input_fn():
    for i, (f, l) in enumerate(source()):
      if i >= nb or int(f['rgb'].shape[0]) != N:      # (a ragged last batch would need a model of its own: left out)
        return
      kept.append({k: np.asarray(f[k]) for k in IMAGE_KEYS if k in f and (cfg.img_channels == 4 or 'depth' not in k)
                   and (goal or 'target' not in k)})
      yield f, l

  kept, outs = [], []
  e = est.Estimator(model_fn=goal_e2evmc_model_fn if goal else e2evmc_model_fn, model_dir=args.model_dir,
                    params={'e2evmc_config': cfg})
  perturbation = args.method in ('occlusion', 'rise')
  if args.method == 'gradient':
    passes = e.input_gradients(input_fn, heads=heads)
  elif perturbation:
    fill = None if args.fill == 'black' else (np.load(args.fill) if args.fill.endswith('.npy') else np.array(args.fill.split(','), np.float32))
    passes = e.perturbation_attributions(input_fn, method=args.method, patch=args.patch, stride=args.stride, grid=args.grid,
                                         keep_prob=args.keep_prob, steps=args.steps, fill=None if fill is None else fill.astype(np.float32),
                                         score=args.score, heads=heads)
  else:
    ig = args.method == 'integrated_gradients'
    baseline = None if (args.baseline == 'black' or not ig) else np.load(args.baseline).astype(np.float32)
    passes = e.attributions(input_fn, method=args.method, steps=args.steps, baseline=baseline, noise_std=0.0 if ig else args.noise_std,
                            heads=heads)
  for out in passes:
    outs.append(out)
  if not outs:
    raise SystemExit('saliency.py: the input produced no full batch of %d windows' % N)
  cat = lambda dicts, k: np.concatenate([d[k] for d in dicts], axis=0)[:args.num_windows]
  arrays = {k: cat(kept, k) for k in kept[0]}
  if args.method == 'gradient':
    arrays.update({'grad_' + k: cat(outs, k) for k in IMAGE_KEYS if k in outs[0]})
    arrays['saliency'] = saliency_of(arrays['grad_rgb'])
    if goal:
      arrays['saliency_target'] = saliency_of(arrays['grad_target_rgb'])
  elif perturbation:      # per window first: scores [M][N] -> [N][M], patch_scores [Gy][Gx][N] -> [N][Gy][Gx]
    for o in outs:
      o.update({k: np.moveaxis(v, -1, 0) for k, v in o.items() if k.startswith(('scores', 'patch_scores'))})
    arrays.update({k: cat(outs, k) for k in outs[0] if k.startswith(('saliency', 'coverage', 'scores', 'patch_scores'))})
  else:
    arrays.update({'attr_' + k: cat(outs, k) for k in IMAGE_KEYS if k in outs[0]})
    arrays.update({k: cat(outs, k) for k in ('saliency', 'saliency_target', 'sample_sum') if k in outs[0]})
    if 'completeness_gap' in outs[0]:      # per window; per batch for a decoder that keeps no per-sample loss terms
      arrays['completeness_gap'] = np.concatenate([np.atleast_1d(o['completeness_gap']) for o in outs]).astype(np.float64)[:args.num_windows]
      arrays['loss_baseline'] = np.asarray([o['loss_baseline'] for o in outs], np.float64)
  if not perturbation:
    arrays['loss'] = np.asarray([o['loss'] for o in outs], np.float32)
  np.savez(args.out, **arrays)
  print('saliency.py: %d windows, heads %s -> %s (%s)' % (arrays['saliency'].shape[0], heads or ('all' if perturbation else 'training loss'), args.out,
                                                           ', '.join('%s %s' % (k, v.shape) for k, v in sorted(arrays.items()))))


if __name__ == '__main__':
  main()
