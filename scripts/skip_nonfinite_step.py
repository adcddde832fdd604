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
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
  ap = argparse.ArgumentParser()
  ap.add_argument('--size', type=int, default=256)
  ap.add_argument('--window_size', type=int, default=16)
  ap.add_argument('--batch_size', type=int, default=32)
  ap.add_argument('--clip_norm', type=float, default=1.0)
  ap.add_argument('--steps', type=int, default=40, help='steps per timed block')
  ap.add_argument('--rounds', type=int, default=7)
  ap.add_argument('--warmup', type=int, default=6)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'skip_nonfinite', 'step.json'))
  ap.add_argument('--merge_bench_ab', default=None, help='measure nothing: add the bench.py runs of this file to --out (module docstring)')
  args = ap.parse_args()
  if args.merge_bench_ab:
    return merge_bench_ab(args.out, args.merge_bench_ab)

  import torch
  from geeco_amd import graph, ops
  from geeco_amd.params import create_e2evmc_config
  from geeco_amd.runtime import TrainStepRunner
  from oracle import geeco_oracle as O

  if not torch.cuda.is_available():
    raise SystemExit('skip_nonfinite_step.py measures on the GPU; none is visible')
  dev = torch.device('cuda', torch.cuda.current_device())
  H, K, N = args.size, args.window_size, args.batch_size
  kw = dict(proc_obs='dynimg', proc_tgt='dyndiff', window_size=K, img_height=H, img_width=H, batch_size=N)
  ocfg = O.make_config(**kw)
  cfg = create_e2evmc_config(kw)
  P = O.init_params(O.model_param_shapes(ocfg, True), seed=0)
  feats, labels = O.synthetic_batch(ocfg, True, N, seed=3, H=H, W=H)
  bad = {k: v.copy() for k, v in labels.items()}
  bad['cmd'][0, 0] = float('nan')
  feats = {k: torch.from_numpy(v) for k, v in feats.items()}
  labels = {k: torch.from_numpy(v) for k, v in labels.items()}
  bad = {k: torch.from_numpy(v) for k, v in bad.items()}

  def timed_block(step, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
      step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n

  options = {'off': {}, 'clip': dict(clip_norm=args.clip_norm), 'skip': dict(skip_nonfinite=True),
             'skip_clip': dict(skip_nonfinite=True, clip_norm=args.clip_norm)}
  models, forms = {}, {}
  for name, opt in options.items():
    m = graph.GoalE2EVMC(cfg, N, dev, training=True, **opt)
    m.store.load_numpy(P)
    m.load_batch(feats, labels)
    r = TrainStepRunner(m, use_graph=True)
    for _ in range(args.warmup):
      r.step()
    models[name], forms[name] = m, r.step
  torch.cuda.synchronize()
  assert models['off'].clip_ws is None and models['clip'].guard is None and models['skip'].guard is not None
  assert models['skip'].guard.tolist() == [1, 0, 0] and models['skip_clip'].guard.tolist() == [1, 0, 0]
  scale, norm = (float(x) for x in models['skip'].clip_out.cpu())
  blocks = {k: [] for k in options}
  for _ in range(args.rounds):
    for k in options:
      blocks[k].append(timed_block(forms[k], args.steps))
  med = {k: statistics.median(v) for k, v in blocks.items()}

  # applied against skipped steps: the ``skip`` model alone, the batch alternating
  m = models['skip']
  verdict_blocks = {'applied': [], 'skipped': []}
  for _ in range(args.rounds):
    for k, lab in (('applied', labels), ('skipped', bad)):
      m.load_batch(feats, lab)
      forms['skip']()      # (the first step on the new labels is outside the block)
      verdict_blocks[k].append(timed_block(forms['skip'], args.steps))
      torch.cuda.synchronize()
      assert int(m.guard[0]) == (1 if k == 'applied' else 0), (k, m.guard.tolist())
  verdict_med = {k: statistics.median(v) for k, v in verdict_blocks.items()}
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
  pass_blocks = {k: [] for k in passes}
  for k, fn in passes.items():
    timed_block(fn, 20)
  for _ in range(args.rounds):
    for k, fn in passes.items():
      pass_blocks[k].append(timed_block(fn, 200) * 1e3)
  pass_med = {k: statistics.median(v) for k, v in pass_blocks.items()}
  us = lambda a, b: round((med[a] - med[b]) * 1e3, 2)
  results = {
      'shape': dict(size=H, window_size=K, batch_size=N, model='geeco-f', arena_floats=int(s.size), clip_norm=args.clip_norm, chunks=int(nch)),
      'timing': dict(steps_per_block=args.steps, rounds=args.rounds, warmup=args.warmup,
                     method='device events around blocks of steps (and of 200 back-to-back optimiser passes), the forms alternating in '
                            'one process; medians of the blocks'),
      'device': torch.cuda.get_device_name(dev),
      'scale_and_norm_after_warmup': [scale, norm],
      'step_ms': {k: round(v, 4) for k, v in med.items()},
      'step_ms_blocks': {k: [round(x, 4) for x in v] for k, v in blocks.items()},
      'step_added_us': {'clip_over_off': us('clip', 'off'), 'skip_over_off': us('skip', 'off'), 'skip_clip_over_off': us('skip_clip', 'off'),
                        'skip_over_clip': us('skip', 'clip'), 'skip_clip_over_clip': us('skip_clip', 'clip')},
      'step_added_percent': {k: round(100.0 * (med[k] - med['off']) / med['off'], 3) for k in ('clip', 'skip', 'skip_clip')},
      'skip_model_step_ms': {k: round(v, 4) for k, v in verdict_med.items()},
      'skip_model_step_ms_blocks': {k: [round(x, 4) for x in v] for k, v in verdict_blocks.items()},
      'skip_model_steps_skipped': skipped_total,
      'optimiser_pass_us': {k: round(v, 2) for k, v in pass_med.items()},
      'optimiser_pass_us_blocks': {k: [round(x, 2) for x in v] for k, v in pass_blocks.items()},
      'optimiser_pass_added_us': {'clipped_over_adam_tf': round(pass_med['clipped_three_launches'] - pass_med['adam_tf'], 2),
                                  'guarded_over_adam_tf': round(pass_med['guarded_three_launches'] - pass_med['adam_tf'], 2),
                                  'guarded_over_clipped': round(pass_med['guarded_three_launches'] - pass_med['clipped_three_launches'], 2)},
      'not_measured': ['the data-parallel forms', 'l2 != 0 (the sum of squares then reads the parameter arena too)', 'ema_decay together with the option',
                       'any model but geeco-f, any shape but this one'],
  }
  print(json.dumps(results), flush=True)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as fp:
    json.dump(results, fp, indent=1, sort_keys=True)
    fp.write('\n')
  print('wrote', args.out)


if __name__ == '__main__':
  main()
