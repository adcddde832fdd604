#!/usr/bin/env python
"""The training step with and without skipping of non-finite optimiser steps (params['skip_nonfinite']), one process,
alternating.

Workload: geeco-f at bench.py's shape (256 x 256, K = 16, N = 32), training models that share nothing but their inputs:
  off:        the captured step as it is without any option (geeco_adam_tf_segments beside and behind the fused encoder bottom);
  clip:       the step with clip_norm alone: sum of squares, scale, two clipped Adam launches behind the fused bottom;
  skip:       the step with skip_nonfinite alone: sum of squares, decision, two guarded Adam launches behind the fused bottom;
  skip_clip:  both options: the same launches as ``skip``, the decision also forms the scale.
All go through runtime.TrainStepRunner (one hipGraph per step).  Timing: device events around blocks of ``--steps`` steps, the forms
alternating for ``--rounds`` rounds after ``--warmup`` steps each; the median block and every block are reported.  Then the ``skip``
model alone, its batch alternating between the clean one and one with a NaN label (every step of such a block is skipped: the Adam
launches write nothing).  The optimiser pass alone is timed the same way on the model's own arenas, back to back with nothing
beside it: geeco_adam_tf, the three launches of the clipped pass, the three of the guarded pass, and the decision kernel by itself.
Writes one JSON file (default profiles/skip_nonfinite/step.json).  Needs the GPU: there is no fallback.

``--merge_bench_ab FILE`` measures nothing: it adds to the JSON file already written the comparison of the option-off step with the
parent commit -- FILE holds one line {"tree": "parent" | "new", "run": i, "result": <bench.py's JSON line>} per run of
``bench.py --gpus 1 --steps 200`` in the two trees, alternating, in one session on one machine.
"""
import json

import _step_ab as ab


def merge_bench_ab(out, path):
  runs = [json.loads(l) for l in open(path) if l.strip()]
  ms = {t: [r['result']['ms_per_step'] for r in runs if r['tree'] == t] for t in ('parent', 'new')}
  with open(out) as fp:
    results = json.load(fp)
  results['option_off_against_parent'] = {
      'method': 'bench.py --gpus 1 --steps 200 --warmup 20 (headline leg only), parent tree and this tree alternating in one session on one machine',
      'order': [r['tree'] for r in runs],
      'ms_per_step': ms,
      'step_ms_median': {t: [r['result']['step_ms']['median'] for r in runs if r['tree'] == t] for t in ms},
      'parent_spread_ms': [min(ms['parent']), max(ms['parent'])],
      'new_not_slower_than_the_parents_slowest_run': max(ms['new']) <= max(ms['parent']),
  }
  with open(out, 'w') as fp:
    json.dump(results, fp, indent=1, sort_keys=True)
    fp.write('\n')
  print(json.dumps(results['option_off_against_parent']))


def main():
  ap = ab.arguments('skip_nonfinite')
  ap.add_argument('--clip_norm', type=float, default=1.0)
  ap.add_argument('--merge_bench_ab', default=None, help='measure nothing: add the bench.py runs of this file to --out (module docstring)')
  args = ap.parse_args()
  if args.merge_bench_ab:
    return merge_bench_ab(args.out, args.merge_bench_ab)
  w = ab.workload(args, 'skip_nonfinite_step.py')

  import torch
  from geeco_amd import ops

  feats, labels = w.feats, w.labels
  bad = {k: v.clone() for k, v in labels.items()}
  bad['cmd'][0, 0] = float('nan')
  options = {'off': {}, 'clip': dict(clip_norm=args.clip_norm), 'skip': dict(skip_nonfinite=True),
             'skip_clip': dict(skip_nonfinite=True, clip_norm=args.clip_norm)}
  models, forms = {}, {}
  for name, opt in options.items():
    models[name], r = ab.build(w, args.warmup, **opt)
    forms[name] = r.step
  torch.cuda.synchronize()
  assert models['off'].clip_ws is None and models['clip'].guard is None and models['skip'].guard is not None
  assert models['skip'].guard.tolist() == [1, 0, 0] and models['skip_clip'].guard.tolist() == [1, 0, 0]
  scale, norm = (float(x) for x in models['skip'].clip_out.cpu())
  blocks = ab.alternate(forms, args.rounds, args.steps)
  med = ab.medians(blocks)

  # applied against skipped steps: the ``skip`` model alone, the batch alternating
  m = models['skip']
  verdict_blocks = {'applied': [], 'skipped': []}
  for _ in range(args.rounds):
    for k, lab in (('applied', labels), ('skipped', bad)):
      m.load_batch(feats, lab)
      forms['skip']()      # (the first step on the new labels is outside the block)
      verdict_blocks[k].append(ab.timed_block(forms['skip'], args.steps))
      torch.cuda.synchronize()
      assert int(m.guard[0]) == (1 if k == 'applied' else 0), (k, m.guard.tolist())
  verdict_med = ab.medians(verdict_blocks)
  skipped_total = int(m.guard[1])
  assert bool(torch.isfinite(m.store.params).all())
  m.load_batch(feats, labels)

  # the optimiser pass alone, on the ``skip_clip`` model's arenas (lr_t and the step counter as the last step left them)
  m = models['skip_clip']
  s = m.store
  whole = [(s.grads, 0, s.size)]
  nch = m.clip_ws.numel()

  def sumsq():
    ops.grad_sumsq_segments(m.clip_ws, s.params, whole, s.size)

  def clipped():
    sumsq()
    ops.clip_scale(m.clip_out, m.clip_ws, nch, args.clip_norm)
    ops.adam_tf_segments_clip(s.params, s.adam_m, s.adam_v, whole, m.scal, m.clip_out)

  def guarded():
    sumsq()
    ops.guard_decide(m.clip_out, m.guard, m.clip_ws, nch, 0.0)
    ops.adam_tf_segments_guard(s.params, s.adam_m, s.adam_v, whole, m.scal, m.clip_out, m.guard)

  passes = {
      'adam_tf': lambda: ops.adam_tf(s.params, s.grads, s.adam_m, s.adam_v, s.size, m.scal),
      'clipped_three_launches': clipped,
      'guarded_three_launches': guarded,
      'guard_decide': lambda: ops.guard_decide(m.clip_out, m.guard, m.clip_ws, nch, 0.0),
      'clip_scale': lambda: ops.clip_scale(m.clip_out, m.clip_ws, nch, args.clip_norm),
  }
  pass_blocks = ab.alternate(passes, args.rounds, 200, warm=20, scale=1e3)
  pass_med = ab.medians(pass_blocks)
  us = lambda a, b: round((med[a] - med[b]) * 1e3, 2)
  ab.write({
      'shape': dict(size=w.H, window_size=w.K, batch_size=w.N, model='geeco-f', arena_floats=int(s.size), clip_norm=args.clip_norm, chunks=int(nch)),
      'timing': ab.timing(args, 'device events around blocks of steps (and of 200 back-to-back optimiser passes), the forms alternating in '
                                'one process; medians of the blocks'),
      'device': torch.cuda.get_device_name(w.dev),
      'scale_and_norm_after_warmup': [scale, norm],
      'step_ms': {k: round(v, 4) for k, v in med.items()},
      'step_ms_blocks': ab.rounded(blocks, 4),
      'step_added_us': {'clip_over_off': us('clip', 'off'), 'skip_over_off': us('skip', 'off'), 'skip_clip_over_off': us('skip_clip', 'off'),
                        'skip_over_clip': us('skip', 'clip'), 'skip_clip_over_clip': us('skip_clip', 'clip')},
      'step_added_percent': {k: round(100.0 * (med[k] - med['off']) / med['off'], 3) for k in ('clip', 'skip', 'skip_clip')},
      'skip_model_step_ms': {k: round(v, 4) for k, v in verdict_med.items()},
      'skip_model_step_ms_blocks': ab.rounded(verdict_blocks, 4),
      'skip_model_steps_skipped': skipped_total,
      'optimiser_pass_us': {k: round(v, 2) for k, v in pass_med.items()},
      'optimiser_pass_us_blocks': ab.rounded(pass_blocks, 2),
      'optimiser_pass_added_us': {'clipped_over_adam_tf': round(pass_med['clipped_three_launches'] - pass_med['adam_tf'], 2),
                                  'guarded_over_adam_tf': round(pass_med['guarded_three_launches'] - pass_med['adam_tf'], 2),
                                  'guarded_over_clipped': round(pass_med['guarded_three_launches'] - pass_med['clipped_three_launches'], 2)},
      'not_measured': ['the data-parallel forms', 'l2 != 0 (the sum of squares then reads the parameter arena too)', 'ema_decay together with the option',
                       'any model but geeco-f, any shape but this one'],
  }, args.out)


if __name__ == '__main__':
  main()
