#!/usr/bin/env python
"""The training step with and without a learning-rate schedule (params['lr_schedule']), one process, alternating.

Workload: geeco-f at bench.py's shape (256 x 256, K = 16, N = 32), two training models that share nothing but their inputs:
  off: the captured step as it is without the option (the constant cfg.lr rides in the backward's last slab-sum launch);
  on:  the same step with a schedule (cosine behind a warm-up by default): the same launches, the block that does the prepare work
       evaluates lr(s) in double from the device's step counter.
Both go through runtime.TrainStepRunner (one hipGraph per step).  Timing: device events around blocks of ``--steps`` steps, the
two forms alternating for ``--rounds`` rounds after ``--warmup`` steps each; the median block and every block are reported, and
the spread of the 'off' blocks to judge the difference by.
Writes one JSON file (default profiles/lr_schedule/step.json).  Needs the GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--size', type=int, default=256)
  ap.add_argument('--window_size', type=int, default=16)
  ap.add_argument('--batch_size', type=int, default=32)
  ap.add_argument('--kind', default='cosine', choices=['constant', 'exponential', 'cosine', 'piecewise'])
  ap.add_argument('--steps', type=int, default=40, help='steps per timed block')
  ap.add_argument('--rounds', type=int, default=7)
  ap.add_argument('--warmup', type=int, default=6)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lr_schedule', 'step.json'))
  args = ap.parse_args()

  import torch
  from geeco_amd import graph, ops
  from geeco_amd.params import create_e2evmc_config
  from geeco_amd.runtime import TrainStepRunner
  from oracle import geeco_oracle as O

  if not torch.cuda.is_available():
    raise SystemExit('lr_schedule_step.py measures on the GPU; none is visible')
  dev = torch.device('cuda', torch.cuda.current_device())
  H, K, N = args.size, args.window_size, args.batch_size
  kw = dict(proc_obs='dynimg', proc_tgt='dyndiff', window_size=K, img_height=H, img_width=H, batch_size=N)
  ocfg = O.make_config(**kw)
  cfg = create_e2evmc_config(kw)
  P = O.init_params(O.model_param_shapes(ocfg, True), seed=0)
  feats, labels = O.synthetic_batch(ocfg, True, N, seed=3, H=H, W=H)
  feats = {k: torch.from_numpy(v) for k, v in feats.items()}
  labels = {k: torch.from_numpy(v) for k, v in labels.items()}
  total = args.warmup + args.rounds * args.steps
  schedule = {
      'constant': {'kind': 'constant', 'warmup_steps': 10},
      'exponential': {'kind': 'exponential', 'warmup_steps': 10, 'decay_steps': 50, 'decay_rate': 0.96},
      'cosine': {'kind': 'cosine', 'warmup_steps': 10, 'decay_steps': total, 'alpha': 0.1},
      'piecewise': {'kind': 'piecewise', 'warmup_steps': 10, 'boundaries': [20, 40, 80, 120, 160, 200, 240, 280],
                    'values': [cfg.lr * 0.8 ** i for i in range(9)]},
  }[args.kind]

  def timed_block(step, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
      step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n

  models, forms = {}, {}
  for name, sched in (('off', None), ('on', schedule)):
    m = graph.GoalE2EVMC(cfg, N, dev, training=True, lr_schedule=sched)
    m.store.load_numpy(P)
    m.load_batch(feats, labels)
    r = TrainStepRunner(m, use_graph=True)
    for _ in range(args.warmup):
      r.step()
    models[name], forms[name] = m, r.step
  torch.cuda.synchronize()
  assert models['on'].lr_schedule is not None and models['off'].lr_schedule is None
  blocks = {'off': [], 'on': []}
  for _ in range(args.rounds):
    for k in ('off', 'on'):
      blocks[k].append(timed_block(forms[k], args.steps))
  med = {k: statistics.median(v) for k, v in blocks.items()}
  # the rate the device holds after the last step against the host's evaluation of the same function at the same counter
  on = models['on']
  s = int(on.store.global_step.item()) - 1
  lr_dev, lr_host = float(on.scal[2]), ops.lr_schedule_eval(on.lr_schedule, s)
  results = {
      'shape': dict(size=H, window_size=K, batch_size=N, model='geeco-f', arena_floats=int(on.store.size)),
      'schedule': schedule,
      'timing': dict(steps_per_block=args.steps, rounds=args.rounds, warmup=args.warmup,
                     method='device events around blocks of steps, option off and on alternating in one process; medians of the blocks'),
      'device': torch.cuda.get_device_name(dev),
      'step_ms': {k: round(v, 4) for k, v in med.items()},
      'step_ms_blocks': {k: [round(x, 4) for x in v] for k, v in blocks.items()},
      'step_added_us': round((med['on'] - med['off']) * 1e3, 2),
      'off_spread_us': round((max(blocks['off']) - min(blocks['off'])) * 1e3, 2),
      'last_step': dict(completed_updates=s, lr_device=lr_dev, lr_host_float64=lr_host),
  }
  print(json.dumps(results), flush=True)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as fp:
    json.dump(results, fp, indent=1, sort_keys=True)
    fp.write('\n')
  print('wrote', args.out)


if __name__ == '__main__':
  main()
