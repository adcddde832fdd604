#!/usr/bin/env python
"""The training step with and without global-norm gradient clipping (params['clip_norm']), one process, alternating.

Workload: geeco-f at bench.py's shape (256 x 256, K = 16, N = 32), two training models that share nothing but their inputs:
  off: the captured step as it is without the option (geeco_adam_tf_segments beside and behind the fused encoder bottom);
  on:  the same step with clip_norm: no piece is updated before the norm of the whole gradient is known, so the optimiser pass
       (sum of squares, scale, two clipped Adam launches) runs behind the fused bottom instead of beside it.
Both go through runtime.TrainStepRunner (one hipGraph per step).  Timing: device events around blocks of ``--steps`` steps, the
two forms alternating for ``--rounds`` rounds after ``--warmup`` steps each; the median block and every block are reported.
The optimiser pass alone is timed the same way on the model's own arenas: geeco_adam_tf against the three launches of the clipped
pass (and its sum-of-squares launch by itself), back to back with nothing beside them.
Writes one JSON file (default profiles/clip/step.json).  Needs the GPU: there is no fallback.
"""
import _step_ab as ab


def main():
  ap = ab.arguments('clip')
  ap.add_argument('--clip_norm', type=float, default=1.0)
  args = ap.parse_args()
  w = ab.workload(args, 'clip_step.py')

  import torch
  from geeco_amd import ops

  models, forms = {}, {}
  for name, clip in (('off', None), ('on', args.clip_norm)):
    models[name], r = ab.build(w, args.warmup, clip_norm=clip)
    forms[name] = r.step
  torch.cuda.synchronize()
  assert models['on'].clip_ws is not None and models['off'].clip_ws is None
  scale, norm = (float(x) for x in models['on'].clip_out.cpu())
  blocks = ab.alternate(forms, args.rounds, args.steps)
  med = ab.medians(blocks)

  # the optimiser pass alone, on the 'on' model's arenas (lr_t and the step counter as the last step left them)
  m = models['on']
  s = m.store
  whole = [(s.grads, 0, s.size)]

  def sumsq():
    ops.grad_sumsq_segments(m.clip_ws, s.params, whole, s.size)

  def clipped():
    sumsq()
    ops.clip_scale(m.clip_out, m.clip_ws, m.clip_ws.numel(), args.clip_norm)
    ops.adam_tf_segments_clip(s.params, s.adam_m, s.adam_v, whole, m.scal, m.clip_out)

  passes = {
      'adam_tf': lambda: ops.adam_tf(s.params, s.grads, s.adam_m, s.adam_v, s.size, m.scal),
      'clipped_three_launches': clipped,
      'grad_sumsq_segments': sumsq,
  }
  pass_blocks = ab.alternate(passes, args.rounds, 200, warm=20, scale=1e3)
  pass_med = ab.medians(pass_blocks)
  arena_mb = 4 * s.size / 1e6
  ab.write({
      'shape': dict(size=w.H, window_size=w.K, batch_size=w.N, model='geeco-f', arena_floats=int(s.size), clip_norm=args.clip_norm,
                    chunks=int(m.clip_ws.numel())),
      'timing': ab.timing(args, 'device events around blocks of steps (and of 200 back-to-back optimiser passes), option off and on '
                                'alternating in one process; medians of the blocks'),
      'device': torch.cuda.get_device_name(w.dev),
      'scale_and_norm_after_warmup': [scale, norm],
      'step_ms': {k: round(v, 4) for k, v in med.items()},
      'step_ms_blocks': ab.rounded(blocks, 4),
      'step_added_us': round((med['on'] - med['off']) * 1e3, 2),
      'step_added_percent': round(100.0 * (med['on'] - med['off']) / med['off'], 3),
      'optimiser_pass_us': {k: round(v, 2) for k, v in pass_med.items()},
      'optimiser_pass_us_blocks': ab.rounded(pass_blocks, 2),
      'optimiser_pass_added_us': round(pass_med['clipped_three_launches'] - pass_med['adam_tf'], 2),
      'grad_sumsq_tb_per_s': round(arena_mb / pass_med['grad_sumsq_segments'], 3),      # l2 = 0: the gradient arena read once
  }, args.out)


if __name__ == '__main__':
  main()
