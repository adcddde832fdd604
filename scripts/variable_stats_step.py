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
import _step_ab as ab


def main():
  args = ab.arguments('variable_stats', steps_help='calls per timed block').parse_args()
  w = ab.workload(args, 'variable_stats_step.py')

  import numpy as np
  import torch
  from geeco_amd import ops

  # ---- (a) the step ------------------------------------------------------------------------------
  models, forms = {}, {}
  for name, opt in (('off', {}), ('on', dict(variable_stats='histograms'))):
    models[name], r = ab.build(w, args.warmup, **opt)
    forms[name] = r.step
  torch.cuda.synchronize()
  assert models['off'].stats_plan is None and models['on'].stats_plan is not None
  blocks = ab.alternate(forms, args.rounds, args.steps)
  med = ab.medians(blocks)
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
  partials = torch.zeros(ops.clip_ws_floats(s.size), dtype=torch.float32, device=w.dev)
  pieces = m.step_pieces
  alone = {
      'variable_stats': lambda: m.stats_plan.run(s.params, s.adam_m, s.adam_v, pieces, s.size),
      'grad_sumsq': lambda: ops.grad_sumsq_segments(partials, None, pieces, s.size),
  }
  ablocks = ab.alternate(alone, args.rounds, args.steps, warm=args.warmup)
  amed = ab.medians(ablocks)
  nbytes = {'variable_stats': 16 * elements, 'grad_sumsq': 4 * s.size}
  rate = {k: nbytes[k] / (amed[k] * 1e-3) for k in alone}
  call = {'us_per_call_median': {k: 1e3 * v for k, v in amed.items()}, 'us_per_call_blocks': {k: [1e3 * x for x in v] for k, v in ablocks.items()},
          'bytes_read': nbytes, 'bytes_per_second': rate, 'bandwidth_ratio_stats_over_sumsq': rate['variable_stats'] / rate['grad_sumsq'],
          'time_ratio_stats_over_sumsq': amed['variable_stats'] / amed['grad_sumsq'], 'pieces': len(pieces),
          'chunks': m.stats_plan.nchunks, 'variables': len(s.shapes), 'arena_floats': s.size, 'variable_floats': elements}

  results = {'workload': dict(w.kw, model='geeco-f'), 'steps_per_block': args.steps, 'rounds': args.rounds, 'warmup': args.warmup,
             'device': torch.cuda.get_device_name(w.dev), 'step': step, 'statistics_call': call}
  ab.write(results, args.out, show={
      'step': {k: step[k] for k in ('ms_per_step_median', 'off_spread_ms', 'on_minus_off_us', 'on_within_the_spread_of_off')},
      'statistics_call': {k: call[k] for k in ('us_per_call_median', 'bytes_per_second', 'bandwidth_ratio_stats_over_sumsq')}})


if __name__ == '__main__':
  main()
