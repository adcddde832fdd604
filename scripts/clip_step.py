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
  ap.add_argument('--clip_norm', type=float, default=1.0)
  ap.add_argument('--steps', type=int, default=40, help='steps per timed block')
  ap.add_argument('--rounds', type=int, default=7)
  ap.add_argument('--warmup', type=int, default=6)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'clip', 'step.json'))
  args = ap.parse_args()

  import torch
  from geeco_amd import graph, ops
  from geeco_amd.params import create_e2evmc_config
  from geeco_amd.runtime import TrainStepRunner
  from oracle import geeco_oracle as O

  if not torch.cuda.is_available():
    raise SystemExit('clip_step.py measures on the GPU; none is visible')
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

  models, forms = {}, {}
  for name, clip in (('off', None), ('on', args.clip_norm)):
    m = graph.GoalE2EVMC(cfg, N, dev, training=True, clip_norm=clip)
    m.store.load_numpy(P)
    m.load_batch(feats, labels)
    r = TrainStepRunner(m, use_graph=True)
    for _ in range(args.warmup):
      r.step()
    models[name], forms[name] = m, r.step
  torch.cuda.synchronize()
  assert models['on'].clip_ws is not None and models['off'].clip_ws is None
  scale, norm = (float(x) for x in models['on'].clip_out.cpu())
  blocks = {'off': [], 'on': []}
  for _ in range(args.rounds):
    for k in ('off', 'on'):
      blocks[k].append(timed_block(forms[k], args.steps))
  med = {k: statistics.median(v) for k, v in blocks.items()}

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
  pass_blocks = {k: [] for k in passes}
  for k, fn in passes.items():
    timed_block(fn, 20)
  for _ in range(args.rounds):
    for k, fn in passes.items():
      pass_blocks[k].append(timed_block(fn, 200) * 1e3)
  pass_med = {k: statistics.median(v) for k, v in pass_blocks.items()}
  arena_mb = 4 * s.size / 1e6
  results = {
      'shape': dict(size=H, window_size=K, batch_size=N, model='geeco-f', arena_floats=int(s.size), clip_norm=args.clip_norm,
                    chunks=int(m.clip_ws.numel())),
      'timing': dict(steps_per_block=args.steps, rounds=args.rounds, warmup=args.warmup,
                     method='device events around blocks of steps (and of 200 back-to-back optimiser passes), option off and on '
                            'alternating in one process; medians of the blocks'),
      'device': torch.cuda.get_device_name(dev),
      'scale_and_norm_after_warmup': [scale, norm],
      'step_ms': {k: round(v, 4) for k, v in med.items()},
      'step_ms_blocks': {k: [round(x, 4) for x in v] for k, v in blocks.items()},
      'step_added_us': round((med['on'] - med['off']) * 1e3, 2),
      'step_added_percent': round(100.0 * (med['on'] - med['off']) / med['off'], 3),
      'optimiser_pass_us': {k: round(v, 2) for k, v in pass_med.items()},
      'optimiser_pass_us_blocks': {k: [round(x, 2) for x in v] for k, v in pass_blocks.items()},
      'optimiser_pass_added_us': round(pass_med['clipped_three_launches'] - pass_med['adam_tf'], 2),
      'grad_sumsq_tb_per_s': round(arena_mb / pass_med['grad_sumsq_segments'], 3),      # l2 = 0: the gradient arena read once
  }
  print(json.dumps(results), flush=True)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as fp:
    json.dump(results, fp, indent=1, sort_keys=True)
    fp.write('\n')
  print('wrote', args.out)


if __name__ == '__main__':
  main()
