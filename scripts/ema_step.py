#!/usr/bin/env python
"""The training step with and without the averaged weights (params['ema_decay']), one process, alternating.

Workload: geeco-f at bench.py's shape (256 x 256, K = 16, N = 32), two training models that share nothing but their inputs:
  off: the captured step as it is without the option (geeco_adam_tf_segments beside and behind the fused encoder bottom);
  on:  the same step with ema_decay (geeco_adam_tf_segments_ema in the same two places: one more arena read and written).
Both go through runtime.TrainStepRunner (one hipGraph per step).  Timing: device events around blocks of ``--steps`` steps, the
two forms alternating for ``--rounds`` rounds after ``--warmup`` steps each; the median block and every block are reported.
The optimiser pass alone is timed the same way on the model's own arenas (geeco_adam_tf against geeco_adam_tf_ema, back-to-back
launches with nothing beside them), since inside the step most of it hides beside the fused bottom.
Writes one JSON file (default profiles/ema/step.json).  Needs the GPU: there is no fallback.
"""
import _step_ab as ab


def main():
  ap = ab.arguments('ema')
  ap.add_argument('--decay', type=float, default=0.999)
  args = ap.parse_args()
  w = ab.workload(args, 'ema_step.py')

  import torch
  from geeco_amd import ops

  models, forms = {}, {}
  for name, decay in (('off', None), ('on', args.decay)):
    models[name], r = ab.build(w, args.warmup, ema_decay=decay)
    forms[name] = r.step
  torch.cuda.synchronize()
  assert models['on'].store.ema is not None and models['off'].store.ema is None
  same = all(torch.equal(getattr(models['on'].store, a), getattr(models['off'].store, a)) for a in ('params', 'adam_m', 'adam_v'))
  blocks = ab.alternate(forms, args.rounds, args.steps)
  med = ab.medians(blocks)

  # the optimiser pass alone, on the 'on' model's arenas (lr_t and the step counter as the last step left them)
  m = models['on']
  s = m.store
  passes = {
      'adam_tf': lambda: ops.adam_tf(s.params, s.grads, s.adam_m, s.adam_v, s.size, m.scal),
      'adam_tf_ema': lambda: ops.adam_tf_ema(s.params, s.grads, s.adam_m, s.adam_v, s.ema, s.size, m.scal, s.global_step, args.decay),
  }
  pass_blocks = ab.alternate(passes, args.rounds, 200, warm=20, scale=1e3)
  pass_med = ab.medians(pass_blocks)
  arena_mb = 4 * s.size / 1e6
  ab.write({
      'shape': dict(size=w.H, window_size=w.K, batch_size=w.N, model='geeco-f', arena_floats=int(s.size), decay=args.decay),
      'timing': ab.timing(args, 'device events around blocks of steps (and of 200 back-to-back optimiser launches), option off and '
                                'on alternating in one process; medians of the blocks'),
      'device': torch.cuda.get_device_name(w.dev),
      'bitwise_same_params_and_slots_after_warmup': bool(same),
      'step_ms': {k: round(v, 4) for k, v in med.items()},
      'step_ms_blocks': ab.rounded(blocks, 4),
      'step_added_us': round((med['on'] - med['off']) * 1e3, 2),
      'optimiser_pass_us': {k: round(v, 2) for k, v in pass_med.items()},
      'optimiser_pass_us_blocks': ab.rounded(pass_blocks, 2),
      'optimiser_pass_added_us': round(pass_med['adam_tf_ema'] - pass_med['adam_tf'], 2),
      'optimiser_pass_tb_per_s': {'adam_tf': round(7 * arena_mb / pass_med['adam_tf'], 3),            # p g m v read, p m v written
                                  'adam_tf_ema': round(9 * arena_mb / pass_med['adam_tf_ema'], 3)},   # + the shadow arena read and written
  }, args.out)


if __name__ == '__main__':
  main()
