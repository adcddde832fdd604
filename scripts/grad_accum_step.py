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
  ap.add_argument('--steps', type=int, default=40, help='steps per timed block')
  ap.add_argument('--rounds', type=int, default=7)
  ap.add_argument('--warmup', type=int, default=6)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'grad_accum', 'step.json'))
  args = ap.parse_args()

  import torch
  from geeco_amd import graph, ops
  from geeco_amd.params import create_e2evmc_config
  from geeco_amd.runtime import TrainStepRunner
  from oracle import geeco_oracle as O

  if not torch.cuda.is_available():
    raise SystemExit('grad_accum_step.py measures on the GPU; none is visible')
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

  def build(accum):
    m = graph.GoalE2EVMC(cfg, N, dev, training=True, grad_accum_steps=accum)
    m.store.load_numpy(P)
    m.load_batch(feats, labels)
    r = TrainStepRunner(m, use_graph=True)
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
  blocks = {k: [] for k in forms}
  for _ in range(args.rounds):
    for k, fn in forms.items():
      blocks[k].append(timed_block(fn, args.steps))
  med = {k: statistics.median(v) for k, v in blocks.items()}
  lo, hi = min(blocks['off']), max(blocks['off'])

  # the accumulate launch alone over the model's arena, beside the Adam pass it takes the place of
  s = on.store
  whole = [(s.grads, 0, s.size)]
  passes = {
      'adam_tf': lambda: ops.adam_tf(s.params, s.grads, s.adam_m, s.adam_v, s.size, on.scal),
      'grad_accumulate_overwrite': lambda: ops.grad_accumulate_segments(s.accum, whole, s.size, True),
      'grad_accumulate_add': lambda: ops.grad_accumulate_segments(s.accum, whole, s.size, False),
  }
  pass_blocks = {k: [] for k in passes}
  for k, fn in passes.items():
    timed_block(fn, 20)
  for _ in range(args.rounds):
    for k, fn in passes.items():
      pass_blocks[k].append(timed_block(fn, 200) * 1e3)
  pass_med = {k: statistics.median(v) for k, v in pass_blocks.items()}
  arena_mb = 4 * s.size / 1e6
  results = {
      'shape': dict(size=H, window_size=K, batch_size=N, model='geeco-f', arena_floats=int(s.size), grad_accum_steps=3),
      'timing': dict(steps_per_block=args.steps, rounds=args.rounds, warmup=args.warmup,
                     method='device events around blocks of replays of one captured form (and of 200 back-to-back launches), the forms '
                            'alternating in one process; medians of the blocks'),
      'device': torch.cuda.get_device_name(dev),
      'step_ms': {k: round(v, 4) for k, v in med.items()},
      'step_ms_blocks': {k: [round(x, 4) for x in v] for k, v in blocks.items()},
      'off_blocks_min_max_ms': [round(lo, 4), round(hi, 4)],
      'step_added_us': {k: round((med[k] - med['off']) * 1e3, 2) for k in med if k != 'off'},
      'median_inside_off_spread': {k: bool(lo <= med[k] <= hi) for k in med if k != 'off'},
      'median_above_off_max': {k: bool(med[k] > hi) for k in med if k != 'off'},
      'launch_us': {k: round(v, 2) for k, v in pass_med.items()},
      'launch_us_blocks': {k: [round(x, 2) for x in v] for k, v in pass_blocks.items()},
      # bytes the launch must move: overwrite reads g and writes acc, add reads both and writes acc
      'launch_tb_per_s': {'grad_accumulate_overwrite': round(2 * arena_mb / pass_med['grad_accumulate_overwrite'], 3),
                          'grad_accumulate_add': round(3 * arena_mb / pass_med['grad_accumulate_add'], 3)},
  }
  print(json.dumps(results), flush=True)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as fp:
    json.dump(results, fp, indent=1, sort_keys=True)
    fp.write('\n')
  print('wrote', args.out)


if __name__ == '__main__':
  main()
