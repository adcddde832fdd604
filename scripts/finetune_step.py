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
import _step_ab as ab

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
  args = ab.arguments('finetune').parse_args()
  w = ab.workload(args, 'finetune_step.py')

  import torch
  from geeco_amd import _native, ops

  models, forms, info = {}, {}, {}
  lib = _native.load()
  for name, table, beside in VARIANTS:
    m, r = ab.build(w, lr_multipliers=table)
    if beside is not None:
      r.beside_bottom = beside
    counter = _Counting(lib)
    _native._lib = counter
    try:
      r._whole_step()      # one eager step, counted: the calls the captured step is made of
      torch.cuda.synchronize()
    finally:
      _native._lib = lib
    info[name] = dict(backward_cut=m.backward_cut, runs=len(m.lr_runs or []), beside_bottom=bool(r.beside_bottom), library_calls=len(counter.calls),
                      optimiser_calls=[c for c in counter.calls if 'adam_tf' in c])
    for _ in range(args.warmup):
      r.step()
    models[name], forms[name] = m, r.step
  torch.cuda.synchronize()
  blocks = ab.alternate(forms, args.rounds, args.steps)
  med = ab.medians(blocks)

  # the optimiser pass alone, on the models' own arenas (the gradients are what the last step left)
  off, on = models['off'], models['enc_x0.1']
  s = on.store
  pieces = [(s.grads[lo:lo + n], lo, n) for lo, n, _ in on.lr_runs]
  muls = [mul for _, _, mul in on.lr_runs]
  passes = {
      'adam_tf_whole_arena': lambda: ops.adam_tf(off.store.params, off.store.grads, off.store.adam_m, off.store.adam_v, off.store.size, off.scal),
      'adam_tf_segments_scaled_runs': lambda: ops.adam_tf_segments_scaled(s.params, s.adam_m, s.adam_v, pieces, muls, on.scal),
  }
  pass_blocks = ab.alternate(passes, args.rounds, args.steps, warm=args.warmup, scale=1e3)
  pass_med = ab.medians(pass_blocks)
  ab.write({
      'shape': dict(size=w.H, window_size=w.K, batch_size=w.N, model='geeco-f', arena_floats=int(s.size)),
      'timing': ab.timing(args, 'device events around blocks of steps, the variants alternating in one process; medians of the blocks'),
      'device': torch.cuda.get_device_name(w.dev),
      'variants': info,
      'step_ms': {k: round(v, 4) for k, v in med.items()},
      'step_ms_blocks': ab.rounded(blocks, 4),
      'step_minus_off_us': {k: round((v - med['off']) * 1e3, 2) for k, v in med.items()},
      'off_spread_us': round((max(blocks['off']) - min(blocks['off'])) * 1e3, 2),
      'optimiser_pass_us': {k: round(v, 2) for k, v in pass_med.items()},
      'optimiser_pass_us_blocks': ab.rounded(pass_blocks, 2),
  }, args.out)


if __name__ == '__main__':
  main()
