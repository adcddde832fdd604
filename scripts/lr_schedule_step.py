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
import _step_ab as ab


def main():
  ap = ab.arguments('lr_schedule')
  ap.add_argument('--kind', default='cosine', choices=['constant', 'exponential', 'cosine', 'piecewise'])
  args = ap.parse_args()
  w = ab.workload(args, 'lr_schedule_step.py')

  import torch
  from geeco_amd import ops

  total = args.warmup + args.rounds * args.steps
  schedule = {
      'constant': {'kind': 'constant', 'warmup_steps': 10},
      'exponential': {'kind': 'exponential', 'warmup_steps': 10, 'decay_steps': 50, 'decay_rate': 0.96},
      'cosine': {'kind': 'cosine', 'warmup_steps': 10, 'decay_steps': total, 'alpha': 0.1},
      'piecewise': {'kind': 'piecewise', 'warmup_steps': 10, 'boundaries': [20, 40, 80, 120, 160, 200, 240, 280],
                    'values': [w.cfg.lr * 0.8 ** i for i in range(9)]},
  }[args.kind]
  models, forms = {}, {}
  for name, sched in (('off', None), ('on', schedule)):
    models[name], r = ab.build(w, args.warmup, lr_schedule=sched)
    forms[name] = r.step
  torch.cuda.synchronize()
  assert models['on'].lr_schedule is not None and models['off'].lr_schedule is None
  blocks = ab.alternate(forms, args.rounds, args.steps)
  med = ab.medians(blocks)
  # the rate the device holds after the last step against the host's evaluation of the same function at the same counter
  on = models['on']
  s = int(on.store.global_step.item()) - 1
  lr_dev, lr_host = float(on.scal[2]), ops.lr_schedule_eval(on.lr_schedule, s)
  ab.write({
      'shape': dict(size=w.H, window_size=w.K, batch_size=w.N, model='geeco-f', arena_floats=int(on.store.size)),
      'schedule': schedule,
      'timing': ab.timing(args, 'device events around blocks of steps, option off and on alternating in one process; medians of the blocks'),
      'device': torch.cuda.get_device_name(w.dev),
      'step_ms': {k: round(v, 4) for k, v in med.items()},
      'step_ms_blocks': ab.rounded(blocks, 4),
      'step_added_us': round((med['on'] - med['off']) * 1e3, 2),
      'off_spread_us': round((max(blocks['off']) - min(blocks['off'])) * 1e3, 2),
      'last_step': dict(completed_updates=s, lr_device=lr_dev, lr_host_float64=lr_host),
  }, args.out)


if __name__ == '__main__':
  main()
