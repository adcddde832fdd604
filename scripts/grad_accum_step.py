#!/usr/bin/env python
"""The training step with and without gradient accumulation (params['grad_accum_steps']), one process, alternating.

Workload: geeco-f at bench.py's shape (256 x 256, K = 16, N = 32), two training models that share nothing but their inputs:
  off:    the captured step as it is without the option (geeco_adam_tf_segments beside and behind the fused encoder bottom);
  first / middle / last: the three captured micro-steps of a model with grad_accum_steps = 3 -- the accumulate launch in overwrite
          mode / in add mode where Adam's pieces go and no optimiser step, and the accumulate launch in add mode with Adam behind it.
Every form is one hipGraph of runtime.TrainStepRunner, replayed by itself (a block of one form: the forms are timed apart, not as the
groups a training run replays).  Timing: device events around blocks of ``--steps`` steps, the forms alternating for ``--rounds``
rounds after ``--warmup`` steps each; the median block and every block are reported, and each form is judged against the min..max
of the option-off blocks of the same run.
The accumulate launch alone is timed the same way over the model's arena (overwrite and add), beside geeco_adam_tf, back to back
with nothing beside them.
Writes one JSON file (default profiles/grad_accum/step.json).  Needs the GPU: there is no fallback.
"""
import _step_ab as ab


def main():
  args = ab.arguments('grad_accum').parse_args()
  w = ab.workload(args, 'grad_accum_step.py')

  import torch
  from geeco_amd import ops

  def build(accum):
    m, r = ab.build(w, grad_accum_steps=accum)
    r.prepare()
    return m, r

  off, r_off = build(None)
  on, r_on = build(3)
  assert off.store.accum is None and on.store.accum is not None and r_off.beside_bottom and r_on.beside_bottom
  assert sorted(r_on._graphs) == ['first', 'last', 'middle']      # (replayed directly below: the store's count is not consulted)
  forms = {'off': r_off.step, 'first': r_on._graphs['first'], 'middle': r_on._graphs['middle'], 'last': r_on._graphs['last']}
  for fn in forms.values():
    for _ in range(args.warmup):
      fn()
  torch.cuda.synchronize()
  blocks = ab.alternate(forms, args.rounds, args.steps)
  med = ab.medians(blocks)
  lo, hi = min(blocks['off']), max(blocks['off'])

  # the accumulate launch alone over the model's arena, beside the Adam pass it takes the place of
  s = on.store
  whole = [(s.grads, 0, s.size)]
  passes = {
      'adam_tf': lambda: ops.adam_tf(s.params, s.grads, s.adam_m, s.adam_v, s.size, on.scal),
      'grad_accumulate_overwrite': lambda: ops.grad_accumulate_segments(s.accum, whole, s.size, True),
      'grad_accumulate_add': lambda: ops.grad_accumulate_segments(s.accum, whole, s.size, False),
  }
  pass_blocks = ab.alternate(passes, args.rounds, 200, warm=20, scale=1e3)
  pass_med = ab.medians(pass_blocks)
  arena_mb = 4 * s.size / 1e6
  ab.write({
      'shape': dict(size=w.H, window_size=w.K, batch_size=w.N, model='geeco-f', arena_floats=int(s.size), grad_accum_steps=3),
      'timing': ab.timing(args, 'device events around blocks of replays of one captured form (and of 200 back-to-back launches), the forms '
                                'alternating in one process; medians of the blocks'),
      'device': torch.cuda.get_device_name(w.dev),
      'step_ms': {k: round(v, 4) for k, v in med.items()},
      'step_ms_blocks': ab.rounded(blocks, 4),
      'off_blocks_min_max_ms': [round(lo, 4), round(hi, 4)],
      'step_added_us': {k: round((med[k] - med['off']) * 1e3, 2) for k in med if k != 'off'},
      'median_inside_off_spread': {k: bool(lo <= med[k] <= hi) for k in med if k != 'off'},
      'median_above_off_max': {k: bool(med[k] > hi) for k in med if k != 'off'},
      'launch_us': {k: round(v, 2) for k, v in pass_med.items()},
      'launch_us_blocks': ab.rounded(pass_blocks, 2),
      # bytes the launch must move: overwrite reads g and writes acc, add reads both and writes acc
      'launch_tb_per_s': {'grad_accumulate_overwrite': round(2 * arena_mb / pass_med['grad_accumulate_overwrite'], 3),
                          'grad_accumulate_add': round(3 * arena_mb / pass_med['grad_accumulate_add'], 3)},
  }, args.out)


if __name__ == '__main__':
  main()
