#!/usr/bin/env python
"""The training step under the fine-tuning option (lr_multipliers), one process, the variants alternating.

Workload: geeco-f at bench.py's shape (256 x 256, K = 16, N = 32), training models that share nothing but their inputs:
  off:             the captured step as it is without the option;
  enc_x0.1:        every encoder variable at 0.1, the decoder at 1: the full backward, the optimiser beside the fused bottom with
                   its two buckets cut at the runs (what TrainStepRunner picks);
  enc_x0.1_plain:  the same model through the plain path, backward(adam_prepare=True) + apply_gradients();
  bottom_frozen:   conv1 / conv2 of every encoder frozen: no encoder bottom;
  enc_frozen:      every encoder frozen: no encoder backward.
All go through runtime.TrainStepRunner (one hipGraph per step).  Timing: device events around blocks of ``--steps`` steps, the
variants alternating for ``--rounds`` rounds after ``--warmup`` steps each; the median block and every block are reported, the
spread of the 'off' blocks to judge differences by, and the library calls of one eager step of each variant.
The optimiser pass alone (the whole arena as one piece through geeco_adam_tf against the model's runs through
geeco_adam_tf_segments_scaled) is timed the same way.
Writes one JSON file (default profiles/finetune/step.json).  Needs the GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = [('off', None, None), ('enc_x0.1', {'Encoder/': 0.1}, None), ('enc_x0.1_plain', {'Encoder/': 0.1}, False),
            ('bottom_frozen', {'/conv[12]/': 0}, None), ('enc_frozen', {'Encoder/': 0}, None)]


class _Counting:
  def __init__(self, lib):
    self._lib, self.calls = lib, []

  def __getattr__(self, name):
    fn = getattr(self._lib, name)
    if not name.startswith('geeco_') or name in ('geeco_last_error', 'geeco_clip_ws_floats') or name.endswith('_bytes'):
      return fn

    def counted(*a):
      self.calls.append(name)
      return fn(*a)
    return counted


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--size', type=int, default=256)
  ap.add_argument('--window_size', type=int, default=16)
  ap.add_argument('--batch_size', type=int, default=32)
  ap.add_argument('--steps', type=int, default=40, help='steps per timed block')
  ap.add_argument('--rounds', type=int, default=7)
  ap.add_argument('--warmup', type=int, default=6)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'finetune', 'step.json'))
  args = ap.parse_args()

  import torch
  from geeco_amd import _native, graph, ops
  from geeco_amd.params import create_e2evmc_config
  from geeco_amd.runtime import TrainStepRunner
  from oracle import geeco_oracle as O

  if not torch.cuda.is_available():
    raise SystemExit('finetune_step.py measures on the GPU; none is visible')
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

  models, forms, launches, info = {}, {}, {}, {}
  lib = _native.load()
  for name, table, beside in VARIANTS:
    m = graph.GoalE2EVMC(cfg, N, dev, training=True, lr_multipliers=table)
    m.store.load_numpy(P)
    m.load_batch(feats, labels)
    r = TrainStepRunner(m, use_graph=True)
    if beside is not None:
      r.beside_bottom = beside
    counter = _Counting(lib)
    _native._lib = counter
    try:
      r._whole_step()      # one eager step, counted: the calls the captured step is made of
      torch.cuda.synchronize()
    finally:
      _native._lib = lib
    launches[name] = len(counter.calls)
    info[name] = dict(backward_cut=m.backward_cut, runs=len(m.lr_runs or []), beside_bottom=bool(r.beside_bottom), library_calls=len(counter.calls),
                      optimiser_calls=[c for c in counter.calls if 'adam_tf' in c])
    for _ in range(args.warmup):
      r.step()
    models[name], forms[name] = m, r.step
  torch.cuda.synchronize()
  blocks = {name: [] for name, _, _ in VARIANTS}
  for _ in range(args.rounds):
    for name, _, _ in VARIANTS:
      blocks[name].append(timed_block(forms[name], args.steps))
  med = {k: statistics.median(v) for k, v in blocks.items()}

  # the optimiser pass alone, on the models' own arenas (the gradients are what the last step left)
  off, on = models['off'], models['enc_x0.1']
  s = on.store
  pieces = [(s.grads[lo:lo + n], lo, n) for lo, n, _ in on.lr_runs]
  muls = [mul for _, _, mul in on.lr_runs]
  passes = {
      'adam_tf_whole_arena': lambda: ops.adam_tf(off.store.params, off.store.grads, off.store.adam_m, off.store.adam_v, off.store.size, off.scal),
      'adam_tf_segments_scaled_runs': lambda: ops.adam_tf_segments_scaled(s.params, s.adam_m, s.adam_v, pieces, muls, on.scal),
  }
  pass_blocks = {k: [] for k in passes}
  for fn in passes.values():
    for _ in range(args.warmup):
      fn()
  for _ in range(args.rounds):
    for k, fn in passes.items():
      pass_blocks[k].append(timed_block(fn, args.steps))
  pass_med = {k: statistics.median(v) for k, v in pass_blocks.items()}

  results = {
      'shape': dict(size=H, window_size=K, batch_size=N, model='geeco-f', arena_floats=int(s.size)),
      'timing': dict(steps_per_block=args.steps, rounds=args.rounds, warmup=args.warmup,
                     method='device events around blocks of steps, the variants alternating in one process; medians of the blocks'),
      'device': torch.cuda.get_device_name(dev),
      'variants': info,
      'step_ms': {k: round(v, 4) for k, v in med.items()},
      'step_ms_blocks': {k: [round(x, 4) for x in v] for k, v in blocks.items()},
      'step_minus_off_us': {k: round((v - med['off']) * 1e3, 2) for k, v in med.items()},
      'off_spread_us': round((max(blocks['off']) - min(blocks['off'])) * 1e3, 2),
      'optimiser_pass_us': {k: round(v * 1e3, 2) for k, v in pass_med.items()},
      'optimiser_pass_us_blocks': {k: [round(x * 1e3, 2) for x in v] for k, v in pass_blocks.items()},
  }
  print(json.dumps(results), flush=True)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as fp:
    json.dump(results, fp, indent=1, sort_keys=True)
    fp.write('\n')
  print('wrote', args.out)


if __name__ == '__main__':
  main()
