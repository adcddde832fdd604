#!/usr/bin/env python
"""What following one address per frame costs the augmented window fill, one process, alternating.

Workload as scripts/augment_scene_step.py: ``--episodes`` synthetic uint8 episodes resident in HBM (256 x 256, K = 16, N = 32 at
the defaults), batches of N consecutive windows of one episode carrying the draws of ``augment=dict(shift=, gain=, bias=)``
and, per form, the frame sources of ``dict(frame_drop=, frame_lag=)``.

1. The dense fill alone, into one float32 [N][K][H][W][3] buffer through WindowFeed.feed + FeedArena.flush +
   WindowFeed.after_flush (the tables through the arena's one copy, then ONE launch):
     augmented: geeco_gather_windows_augmented, one address per window (the yardstick);
     frames_consecutive: geeco_gather_windows_frames following the consecutive [N][K] table -- the same frame bytes and values;
     frames_time: geeco_gather_windows_frames under frame drops and lags (repeated frames).
2. The e2e_vmc and geeco-f ('dynimg' x 'dyndiff') training steps through Estimator._feed_step + the captured step, fed
   augmented batches and time-augmented ones.

The forms alternate for ``--rounds`` rounds after ``--warmup`` calls each; the median block and all blocks are reported, and per
comparison whether the new form's median lies inside the min..max spread of the yardstick's own blocks.  Writes one JSON file
(default profiles/augment/time.json).  Needs the GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--size', type=int, default=256)
  ap.add_argument('--window_size', type=int, default=16)
  ap.add_argument('--batch_size', type=int, default=32)
  ap.add_argument('--episodes', type=int, default=8)
  ap.add_argument('--shift', type=int, default=16)
  ap.add_argument('--gain', type=float, default=0.2)
  ap.add_argument('--bias', type=float, default=0.1)
  ap.add_argument('--frame_drop', type=float, default=0.3)
  ap.add_argument('--frame_lag', type=int, default=2)
  ap.add_argument('--fills', type=int, default=50, help='fills per timed block')
  ap.add_argument('--steps', type=int, default=20, help='training steps per timed block')
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--warmup', type=int, default=6)
  ap.add_argument('--skip_step', action='store_true', help='time the fills only')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'augment', 'time.json'))
  args = ap.parse_args()

  import numpy as np
  import torch
  from geeco_amd import estimator as est
  from geeco_amd.input_fn import (DeviceWindows, FeedArena, WindowAugment, WindowFeed, draw_augment, draw_augment_time,
                                  synthetic_scene_frames)
  from geeco_amd.params import create_e2evmc_config
  from oracle import geeco_oracle as O

  if not torch.cuda.is_available():
    raise SystemExit('augment_time_step.py measures on the GPU; none is visible')
  dev = torch.device('cuda', torch.cuda.current_device())
  H, K, N, E = args.size, args.window_size, args.batch_size, args.episodes
  T = N + K - 1                                      # N consecutive windows
  base_rgb, _ = synthetic_scene_frames(T + 1, H, H, seed=[13, 0])
  resident, targets = [], []
  for e in range(E):                                 # the scene shifted per episode: distinct frames, one generator run
    ep = np.roll(base_rgb, 7 * e, axis=2)
    resident.append(torch.from_numpy(ep[:T].reshape(T, -1)).to(dev))
    targets.append(torch.from_numpy(ep[T:].reshape(1, -1)).to(dev))
  shape = (H, H, 3)
  r = np.random.default_rng(5)
  # (L, p) of the frame sources; None: no sources, the merged augmented fill
  FORMS = {'augmented': None, 'frames_consecutive': (0, 0.0), 'frames_time': (args.frame_lag, args.frame_drop)}

  def batch(form):
    """{'rgb', 'target_rgb'} of N consecutive windows of one episode under the draws of ``form``"""
    e = int(r.integers(0, E))
    base = draw_augment(r, N, args.shift, args.gain, args.bias)
    extras = dict(frame_src=draw_augment_time(r, N, K, *FORMS[form])) if FORMS[form] is not None else {}
    draws = WindowAugment(base.shift, base.colour, **extras)
    rgb, tgt = DeviceWindows(K, shape, 255.0), DeviceWindows(1, shape, 255.0, squeeze_k=True)
    rgb.add(resident[e], np.arange(N, dtype=np.int32))
    tgt.add(targets[e], np.zeros(N, np.int32))
    rgb.augment = tgt.augment = draws
    rgb.timed = True                                 # the observation follows the sources, the target frame does not
    return {'rgb': rgb, 'target_rgb': tgt}

  CYCLE = 4                                          # distinct batches per form, fed in turn (the tables really change)
  batches = {form: [batch(form) for _ in range(CYCLE)] for form in FORMS}

  def timed_block(call, n):
    """(host wall ms, device ms) per call of a block of n calls that ends in a synchronise"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for i in range(n):
      call(i)
    b.record()
    b.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n, a.elapsed_time(b) / n

  def alternate(forms, n):
    for call in forms.values():
      for i in range(args.warmup):
        call(i)
    torch.cuda.synchronize()
    blocks = {k: [] for k in forms}
    for _ in range(args.rounds):
      for k, call in forms.items():
        blocks[k].append(timed_block(call, n))
    out = {}
    for k, v in blocks.items():
      out[k] = {'wall_ms': round(statistics.median(x[0] for x in v), 4), 'device_ms': round(statistics.median(x[1] for x in v), 4),
                'wall_ms_blocks': [round(x[0], 4) for x in v], 'device_ms_blocks': [round(x[1], 4) for x in v]}
    return out

  def verdict(res, yardstick, new, what='device_ms'):
    """Whether the new form's median block lies inside the min..max spread of the yardstick's own blocks."""
    lo, hi = min(res[yardstick][what + '_blocks']), max(res[yardstick][what + '_blocks'])
    return {'yardstick': yardstick, 'new': new, 'clock': what, 'yardstick_min': lo, 'yardstick_max': hi, 'new_median': res[new][what],
            'new_over_yardstick_median': round(res[new][what] / res[yardstick][what], 4), 'inside_spread': bool(res[new][what] <= hi)}

  fill_written, fill_read = N * K * H * H * 3 * 4, N * K * H * H * 3
  results = {'shape': dict(size=H, window_size=K, batch_size=N, episodes=E, frames_per_episode=T, fill_bytes_written=fill_written,
                           fill_bytes_read=fill_read),
             'augment': dict(shift=args.shift, gain=args.gain, bias=args.bias, frame_drop=args.frame_drop, frame_lag=args.frame_lag),
             'timing': dict(fills_per_block=args.fills, steps_per_block=args.steps, rounds=args.rounds, warmup=args.warmup,
                            method='blocks of calls ending in a device synchronise, the forms alternating in one process; wall = host '
                                   'clock around the block, device = events around the block; median block and every block'),
             'device': torch.cuda.get_device_name(dev)}

  # ---- 1. the dense fill alone ----------------------------------------------------------------------------------------------
  def filler(form):
    arena = FeedArena(dev)
    feed = WindowFeed(batches[form][0]['rgb'], arena, ('features', 'rgb'))
    arena.seal()
    assert feed.dense().shape == (N, K) + shape and feed.form == ('dense_augmented' if form == 'augmented' else 'dense_frames'), feed.form

    def fill_with(windows):
      arena.begin()
      feed.feed(windows)
      arena.flush()
      feed.after_flush()
      return feed.buffer
    return fill_with

  fill_with = {form: filler(form) for form in FORMS}
  fills = {form: (lambda i, form=form: fill_with[form](batches[form][i % CYCLE]['rgb'])) for form in FORMS}
  results['fill'] = alternate(fills, args.fills)
  for k, v in results['fill'].items():               # bytes the algorithm moves over the device time of a fill (copy and launch)
    v['GBps_read_plus_written'] = round((fill_written + fill_read) / (v['device_ms'] * 1e-3) / 1e9, 1)
  results['fill']['verdicts'] = [verdict(results['fill'], 'augmented', 'frames_consecutive'),
                                 verdict(results['fill'], 'frames_consecutive', 'frames_time')]
  stale = np.mean([(b['rgb'].frame_src[:, 1:] == b['rgb'].frame_src[:, :-1]).mean() for b in batches['frames_time']])
  results['fill']['frames_time_stale_slot_fraction'] = round(float(stale), 4)
  print('fill', json.dumps(results['fill']), flush=True)

  # ---- 2. the training steps -------------------------------------------------------------------------------------------------
  if not args.skip_step:
    for name, goal, kw in (('e2e_vmc_step', False, {}), ('geeco_f_step', True, dict(proc_obs='dynimg', proc_tgt='dyndiff'))):
      kw = dict(kw, window_size=K, img_height=H, img_width=H, batch_size=N)
      feats, labels = O.synthetic_batch(O.make_config(**kw), goal, N, seed=3, H=8, W=8)   # states and labels only
      feats = {k: v for k, v in feats.items() if k not in ('rgb', 'depth', 'target_rgb', 'target_depth')}
      e = est.Estimator(est.goal_e2evmc_model_fn if goal else est.e2evmc_model_fn, None, est.RunConfig(),
                        {'e2evmc_config': create_e2evmc_config(kw), 'log_steps': 10 ** 9})

      def stepper(form):
        def step(i):
          b = batches[form][i % CYCLE]
          f = dict(feats, **(b if goal else {'rgb': b['rgb']}))
          spec, fbuf, lbuf = e._get_spec(est.ModeKeys.TRAIN, f, labels, N)
          e._feed_step(fbuf, lbuf, f, labels)
          spec.train_op()
        return step
      results[name] = alternate({k: stepper(k) for k in ('augmented', 'frames_time')}, args.steps)
      results[name]['verdicts'] = [verdict(results[name], 'augmented', 'frames_time', clock) for clock in ('device_ms', 'wall_ms')]
      results[name]['models_built'] = len(e._specs)
      for spec, _, _ in e._specs.values():
        spec.model.check_device_errors()
      print(name, json.dumps(results[name]), flush=True)
      del e
      torch.cuda.empty_cache()

  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as fp:
    json.dump(results, fp, indent=1, sort_keys=True)
    fp.write('\n')
  print('wrote', args.out)


if __name__ == '__main__':
  main()
