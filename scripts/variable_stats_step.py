#!/usr/bin/env python
"""What the per-variable statistics (params['variable_stats']) cost, one process, two legs, alternating.

Workload: geeco-f at bench.py's shape (256 x 256, K = 16, N = 32).
  (a) the captured step (runtime.TrainStepRunner, one hipGraph) of a model built with the option off and of one built with it on.
      The option adds no launch to the step -- the statistics run on logging steps, outside it, and none falls inside the timed
      blocks -- so the two must agree within the spread of the option-off step measured in the same run, which is recorded.  If they
      do not, something leaked into the step: a defect, not a cost.
  (b) the statistics call alone (geeco_variable_stats: two launches over the parameter, Adam-m, Adam-v and gradient arenas of the
      model, 4 x 4 bytes per element read) against geeco_grad_sumsq_segments on the same arena (4 bytes per element read, l2 = 0), back
      to back with nothing beside them: time, achieved bytes per second of both, and their ratio.  Reported, not gated: the pass runs
      once per log_steps steps.
Timing: device events around blocks of ``--steps`` calls, the forms alternating for ``--rounds`` rounds after ``--warmup`` calls each;
the median block and every block are reported.  Writes one JSON file (default profiles/variable_stats/step.json).  Needs the GPU:
there is no fallback.
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
  ap.add_argument('--steps', type=int, default=40, help='calls per timed block')
  ap.add_argument('--rounds', type=int, default=7)
  ap.add_argument('--warmup', type=int, default=6)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'variable_stats', 'step.json'))
  args = ap.parse_args()

  import numpy as np
  import torch
  from geeco_amd import graph, ops
  from geeco_amd.params import create_e2evmc_config
  from geeco_amd.runtime import TrainStepRunner
  from oracle import geeco_oracle as O

  if not torch.cuda.is_available():
    raise SystemExit('variable_stats_step.py measures on the GPU; none is visible')
  dev = torch.device('cuda', torch.cuda.current_device())
  H, K, N = args.size, args.window_size, args.batch_size
  kw = dict(proc_obs='dynimg', proc_tgt='dyndiff', window_size=K, img_height=H, img_width=H, batch_size=N)
  ocfg = O.make_config(**kw)
  cfg = create_e2evmc_config(kw)
  P = O.init_params(O.model_param_shapes(ocfg, True), seed=0)
  feats, labels = O.synthetic_batch(ocfg, True, N, seed=3, H=H, W=H)
  feats = {k: torch.from_numpy(v) for k, v in feats.items()}
  labels = {k: torch.from_numpy(v) for k, v in labels.items()}

  def timed_block(step, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
      step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n

  def alternate(forms):
    blocks = {k: [] for k in forms}
    for _ in range(args.rounds):
      for name, step in forms.items():
        blocks[name].append(timed_block(step, args.steps))
    return blocks

  # ---- (a) the step ------------------------------------------------------------------------------
  models, forms = {}, {}
  for name, opt in (('off', {}), ('on', dict(variable_stats='histograms'))):
    m = graph.GoalE2EVMC(cfg, N, dev, training=True, **opt)
    m.store.load_numpy(P)
    m.load_batch(feats, labels)
    r = TrainStepRunner(m, use_graph=True)
    for _ in range(args.warmup):
      r.step()
    models[name], forms[name] = m, r.step
  torch.cuda.synchronize()
  assert models['off'].stats_plan is None and models['on'].stats_plan is not None
  blocks = alternate(forms)
  med = {k: statistics.median(v) for k, v in blocks.items()}
  spread = [min(blocks['off']), max(blocks['off'])]
  step = {'ms_per_step_median': med, 'ms_per_step_blocks': blocks, 'off_spread_ms': spread,
          'on_minus_off_us': 1e3 * (med['on'] - med['off']),
          'on_within_the_spread_of_off': spread[0] <= med['on'] <= spread[1]}

  # ---- (b) the statistics call alone ---------------------------------------------------------------
  m = models['on']
  s = m.store
  stats = m.variable_stats()      # (the records of the last replayed step: the call works behind a captured step)
  assert len(stats) == len(s.shapes) and all(np.isfinite(d['grad_norm']) for d in stats.values())
  elements = int(sum(int(np.prod(shp)) for shp in s.shapes.values()))
  partials = torch.zeros(ops.clip_ws_floats(s.size), dtype=torch.float32, device=dev)
  pieces = m.step_pieces
  alone = {
      'variable_stats': lambda: m.stats_plan.run(s.params, s.adam_m, s.adam_v, pieces, s.size),
      'grad_sumsq': lambda: ops.grad_sumsq_segments(partials, None, pieces, s.size),
  }
  for f in alone.values():
    for _ in range(args.warmup):
      f()
  torch.cuda.synchronize()
  ablocks = alternate(alone)
  amed = {k: statistics.median(v) for k, v in ablocks.items()}
  nbytes = {'variable_stats': 16 * elements, 'grad_sumsq': 4 * s.size}
  rate = {k: nbytes[k] / (amed[k] * 1e-3) for k in alone}
  call = {'us_per_call_median': {k: 1e3 * v for k, v in amed.items()}, 'us_per_call_blocks': {k: [1e3 * x for x in v] for k, v in ablocks.items()},
          'bytes_read': nbytes, 'bytes_per_second': rate, 'bandwidth_ratio_stats_over_sumsq': rate['variable_stats'] / rate['grad_sumsq'],
          'time_ratio_stats_over_sumsq': amed['variable_stats'] / amed['grad_sumsq'], 'pieces': len(pieces),
          'chunks': m.stats_plan.nchunks, 'variables': len(s.shapes), 'arena_floats': s.size, 'variable_floats': elements}

  results = {'workload': dict(kw, model='geeco-f'), 'steps_per_block': args.steps, 'rounds': args.rounds, 'warmup': args.warmup,
             'device': torch.cuda.get_device_name(dev), 'step': step, 'statistics_call': call}
  os.makedirs(os.path.dirname(args.out), exist_ok=True)
  with open(args.out, 'w') as fp:
    json.dump(results, fp, indent=1, sort_keys=True)
    fp.write('\n')
  print(json.dumps({'step': {k: step[k] for k in ('ms_per_step_median', 'off_spread_ms', 'on_minus_off_us', 'on_within_the_spread_of_off')},
                    'statistics_call': {k: call[k] for k in ('us_per_call_median', 'bytes_per_second', 'bandwidth_ratio_stats_over_sumsq')}}))


if __name__ == '__main__':
  main()
