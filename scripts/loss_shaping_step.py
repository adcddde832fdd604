#!/usr/bin/env python
"""The training step with and without loss shaping (params['loss_shaping']), one process, alternating.

Workload: geeco-f at bench.py's shape (256 x 256, K = 16, N = 32), two training models that share nothing but their inputs:
  off: the captured step as it is without the option (heads_sample_kernel<true>, the loss means in lstm_step_bwd_heads_kernel);
  on:  the same step with all four keys (sample weights from {0, 0.5, 1, 2}, gripper class weights, label smoothing, Huber on every
       regression head): heads_sample_kernel<true, shaped> in the same place.
Both go through runtime.TrainStepRunner (one hipGraph per step).  Timing: device events around blocks of ``--steps`` steps, the two
forms alternating for ``--rounds`` rounds after ``--warmup`` steps each; the median block and every block are reported, with the
launches of one eager step of each form (ops.kernel_trace).  The decoder tail alone (LSTMDecoder.forward(True) of the one-step decoder:
the gate GEMM and the per-sample launch; the batch sums ride in the backward's first grid and are not part of it) is captured into a
graph of its own on each model's buffers and timed the same way, 200 replays a block.
``--off_only``: the option-off step alone, through nothing this option added -- the form that also runs on the commit before it, to
show that an unshaped step did not move.
Writes one JSON file (default profiles/loss_shaping/step.json).  Needs the GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPING = {'sample_weights': True, 'grp_class_weights': [1.0, 0.25, 2.0], 'label_smoothing': 0.1, 'huber_delta': 0.5}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--size', type=int, default=256)
  ap.add_argument('--window_size', type=int, default=16)
  ap.add_argument('--batch_size', type=int, default=32)
  ap.add_argument('--steps', type=int, default=40, help='steps per timed block')
  ap.add_argument('--rounds', type=int, default=7)
  ap.add_argument('--warmup', type=int, default=6)
  ap.add_argument('--off_only', default=False, action='store_true')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'loss_shaping', 'step.json'))
  args = ap.parse_args()

  import torch
  from geeco_amd import graph, ops
  from geeco_amd.params import create_e2evmc_config
  from geeco_amd.runtime import TrainStepRunner
  from oracle import geeco_oracle as O

  if not torch.cuda.is_available():
    raise SystemExit('loss_shaping_step.py measures on the GPU; none is visible')
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

  names = ('off',) if args.off_only else ('off', 'on')
  models, forms, launches = {}, {}, {}
  for name in names:
    m = graph.GoalE2EVMC(cfg, N, dev, training=True, **({'loss_shaping': SHAPING} if name == 'on' else {}))
    m.store.load_numpy(P)
    m.load_batch(feats, labels)
    if name == 'on':
      m.inputs['sample_weight'].copy_(torch.tensor([0.0, 0.5, 1.0, 2.0]).repeat((N + 3) // 4)[:N])
    launches[name] = ops.kernel_trace(m.train_step)
    r = TrainStepRunner(m, use_graph=True)
    for _ in range(args.warmup):
      r.step()
    models[name], forms[name] = m, r.step
  torch.cuda.synchronize()
  blocks = {k: [] for k in names}
  for _ in range(args.rounds):
    for k in names:
      blocks[k].append(timed_block(forms[k], args.steps))
  med = {k: statistics.median(v) for k, v in blocks.items()}

  # the decoder tail alone: gate GEMM + the per-sample launch (the pending batch sums are dropped: they belong to the backward)
  def tail_of(m):
    d = m.decoder

    def run():
      d.forward(True)
      d.heads_pending = None
    return run
  eager = {k: tail_of(models[k]) for k in names}
  tail_launches = {k: ops.kernel_trace(fn) for k, fn in eager.items()}
  torch.cuda.synchronize()
  tails = {}
  for k, fn in eager.items():
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
      fn()
    tails[k] = g.replay
  tail_blocks = {k: [] for k in names}
  for fn in tails.values():
    timed_block(fn, 20)
  for _ in range(args.rounds):
    for k, fn in tails.items():
      tail_blocks[k].append(timed_block(fn, 200) * 1e3)
  tail_med = {k: statistics.median(v) for k, v in tail_blocks.items()}

  results = {
      'shape': dict(size=H, window_size=K, batch_size=N, model='geeco-f'),
      'timing': dict(steps_per_block=args.steps, rounds=args.rounds, warmup=args.warmup,
                     method='device events around blocks of captured steps (and of 200 replays of the captured decoder-tail forward), the '
                            'forms alternating in one process; medians, minima and maxima of the blocks'),
      'device': torch.cuda.get_device_name(dev),
      'step_ms': {k: round(v, 4) for k, v in med.items()},
      'step_ms_min_max': {k: [round(min(v), 4), round(max(v), 4)] for k, v in blocks.items()},
      'step_ms_blocks': {k: [round(x, 4) for x in v] for k, v in blocks.items()},
      'step_launches': {k: len(v) for k, v in launches.items()},
      'decoder_tail_us': {k: round(v, 2) for k, v in tail_med.items()},
      'decoder_tail_us_blocks': {k: [round(x, 2) for x in v] for k, v in tail_blocks.items()},
      'decoder_tail_launches': tail_launches,
  }
  if not args.off_only:
    results['loss_shaping'] = SHAPING
    results['step_added_us'] = round((med['on'] - med['off']) * 1e3, 2)
    results['on_inside_off_min_max'] = bool(min(blocks['off']) <= med['on'] <= max(blocks['off']))
    results['step_launch_names_that_differ'] = [[a, b] for a, b in zip(launches['off'], launches['on']) if a != b]      # (the trace buffer may cut the last name)
  print(json.dumps(results), flush=True)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as fp:
    json.dump(results, fp, indent=1, sort_keys=True)
    fp.write('\n')
  print('wrote', args.out)


if __name__ == '__main__':
  main()
