#!/usr/bin/env python
"""What a batch of SHUFFLED windows costs to feed, one process, alternating.

Workload: ``--episodes`` synthetic uint8 episodes resident in HBM (256 x 256, K = 16, N = 32 at the defaults) and batches that
take ONE window from each of N episodes -- what pickplace_input_fn(shuffle_windows=True) emits once the buffer holds more
windows than an episode has.

1. The dense fill alone, into one float32 [N][K][H][W][3] buffer:
     per_segment: DeviceWindows.materialize_into -- one geeco_gather_windows launch and one pageable H2D copy of ``starts`` per
                  segment, N segments (what a batch of this composition costs without the by-address form: the yardstick);
     by_address:  WindowFeed.feed + FeedArena.flush + WindowFeed.after_flush -- the window table through the arena's one copy,
                  then ONE geeco_gather_windows_by_address launch;
     consecutive: materialize_into of N consecutive windows of one episode (one segment: today's ordinary batch).
   Host wall clock around blocks of fills that end in a device synchronise (the per-segment form is bound by the host queueing
   its copies and launches, which device events alone would not show), and device events around the same blocks.
2. The e2e_vmc training step through Estimator._feed_step + the captured step, fed consecutive batches, shuffled batches by
   address, and shuffled batches per segment.  The three forms train the same variables in turn.

The forms alternate for ``--rounds`` rounds after ``--warmup`` calls each; the median block and all blocks are reported.  Writes
one JSON file (default profiles/shuffle_windows/feed.json).  Needs the GPU: there is no fallback.
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
  ap.add_argument('--episodes', type=int, default=32)
  ap.add_argument('--fills', type=int, default=50, help='fills per timed block')
  ap.add_argument('--steps', type=int, default=20, help='training steps per timed block')
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--warmup', type=int, default=6)
  ap.add_argument('--skip_step', action='store_true', help='time the fills only')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'shuffle_windows', 'feed.json'))
  args = ap.parse_args()

  import numpy as np
  import torch
  from geeco_amd import estimator as est
  from geeco_amd.input_fn import DeviceWindows, FeedArena, WindowFeed, synthetic_scene_frames
  from geeco_amd.params import create_e2evmc_config
  from oracle import geeco_oracle as O

  if not torch.cuda.is_available():
    raise SystemExit('shuffle_feed_step.py measures on the GPU; none is visible')
  dev = torch.device('cuda', torch.cuda.current_device())
  H, K, N, E = args.size, args.window_size, args.batch_size, args.episodes
  if E < N:
    raise SystemExit('--episodes must be >= --batch_size (one window from each of N episodes)')
  T = N + K - 1                                      # every episode can also supply the N consecutive windows of an ordinary batch
  base_rgb, _ = synthetic_scene_frames(T, H, H, seed=[13, 0])
  resident = []
  for e in range(E):                                 # the scene shifted per episode: distinct frames, one generator run
    resident.append(torch.from_numpy(np.roll(base_rgb, 7 * e, axis=2).reshape(T, -1)).to(dev))
  shape = (H, H, 3)
  r = np.random.default_rng(5)

  def shuffled_batch(scattered):
    dw = DeviceWindows(K, shape, 255.0)
    for e in r.permutation(E)[:N]:
      dw.add(resident[int(e)], np.asarray([int(r.integers(0, T - K + 1))], np.int32))
    dw.scattered = scattered
    return dw

  def consecutive_batch():
    dw = DeviceWindows(K, shape, 255.0)
    dw.add(resident[int(r.integers(0, E))], np.arange(N, dtype=np.int32))
    return dw

  CYCLE = 4                                          # distinct batches per form, fed in turn (the tables really change)
  batches = {'per_segment': [shuffled_batch(False) for _ in range(CYCLE)], 'by_address': [shuffled_batch(True) for _ in range(CYCLE)],
             'consecutive': [consecutive_batch() for _ in range(CYCLE)]}

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

  results = {'shape': dict(size=H, window_size=K, batch_size=N, episodes=E, frames_per_episode=T,
                           fill_bytes_written=N * K * H * H * 3 * 4, fill_bytes_read=N * K * H * H * 3),
             'timing': dict(fills_per_block=args.fills, steps_per_block=args.steps, rounds=args.rounds, warmup=args.warmup,
                            method='blocks of calls ending in a device synchronise, the forms alternating in one process; wall = host '
                                   'clock around the block, device = events around the block; median block and every block'),
             'device': torch.cuda.get_device_name(dev)}

  # ---- 1. the dense fill alone ----------------------------------------------------------------------------------------------
  out = torch.empty((N, K) + shape, dtype=torch.float32, device=dev)
  arena = FeedArena(dev)
  feed = WindowFeed(batches['by_address'][0], arena, ('features', 'rgb'))
  arena.seal()
  assert feed.scattered and feed.dense().shape == out.shape

  def fill_by_address(i):
    arena.begin()
    feed.feed(batches['by_address'][i % CYCLE])
    arena.flush()
    feed.after_flush()

  fills = {'per_segment': lambda i: batches['per_segment'][i % CYCLE].materialize_into(out), 'by_address': fill_by_address,
           'consecutive': lambda i: batches['consecutive'][i % CYCLE].materialize_into(out)}
  # same values first: the by-address fill of a batch against the per-segment fill of the same batch
  b0 = batches['by_address'][0]
  b0.materialize_into(out)
  arena.begin()
  feed.feed(b0)
  arena.flush()
  feed.after_flush()
  torch.cuda.synchronize()
  if not torch.equal(out.view(torch.int32), feed.dense().view(torch.int32)):
    raise SystemExit('the by-address fill differs from the per-segment fill of the same batch')
  results['fill'] = alternate(fills, args.fills)
  results['fill']['segments'] = {k: len(v[0].segments) for k, v in batches.items()}
  print('fill', json.dumps(results['fill']), flush=True)

  # ---- 2. the e2e_vmc training step ---------------------------------------------------------------------------------------------
  if not args.skip_step:
    kw = dict(window_size=K, img_height=H, img_width=H, batch_size=N)
    ocfg = O.make_config(**kw)
    feats, labels = O.synthetic_batch(ocfg, False, N, seed=3, H=8, W=8)          # states and labels only: the images come from the episodes
    feats = {k: v for k, v in feats.items() if k not in ('rgb', 'depth', 'target_rgb', 'target_depth')}
    e = est.Estimator(est.e2evmc_model_fn, None, est.RunConfig(), {'e2evmc_config': create_e2evmc_config(kw), 'log_steps': 10 ** 9})

    def stepper(form):
      def step(i):
        f = dict(feats, rgb=batches[form][i % CYCLE])
        spec, fbuf, lbuf = e._get_spec(est.ModeKeys.TRAIN, f, labels, N)
        e._feed_step(fbuf, lbuf, f, labels)
        spec.train_op()
      return step
    results['e2e_vmc_step'] = alternate({k: stepper(k) for k in ('consecutive', 'by_address', 'per_segment')}, args.steps)
    results['e2e_vmc_step']['models_built'] = len(e._specs)
    print('e2e_vmc_step', json.dumps(results['e2e_vmc_step']), flush=True)

  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as fp:
    json.dump(results, fp, indent=1, sort_keys=True)
    fp.write('\n')
  print('wrote', args.out)


if __name__ == '__main__':
  main()
