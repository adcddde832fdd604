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
import _step_ab as ab

SHAPING = {'sample_weights': True, 'grp_class_weights': [1.0, 0.25, 2.0], 'label_smoothing': 0.1, 'huber_delta': 0.5}


def main():
  ap = ab.arguments('loss_shaping')
  ap.add_argument('--off_only', default=False, action='store_true')
  args = ap.parse_args()
  w = ab.workload(args, 'loss_shaping_step.py')

  import torch
  from geeco_amd import ops

  names = ('off',) if args.off_only else ('off', 'on')
  models, forms, launches = {}, {}, {}

  def traced(name):
    def before_runner(m):
      if name == 'on':
        m.inputs['sample_weight'].copy_(torch.tensor([0.0, 0.5, 1.0, 2.0]).repeat((w.N + 3) // 4)[:w.N])
      launches[name] = ops.kernel_trace(m.train_step)
    return before_runner
  for name in names:
    models[name], r = ab.build(w, args.warmup, traced(name), **({'loss_shaping': SHAPING} if name == 'on' else {}))
    forms[name] = r.step
  torch.cuda.synchronize()
  blocks = ab.alternate(forms, args.rounds, args.steps)
  med = ab.medians(blocks)

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
  tail_blocks = ab.alternate(tails, args.rounds, 200, warm=20, scale=1e3)
  tail_med = ab.medians(tail_blocks)

  results = {
      'shape': dict(size=w.H, window_size=w.K, batch_size=w.N, model='geeco-f'),
      'timing': ab.timing(args, 'device events around blocks of captured steps (and of 200 replays of the captured decoder-tail forward), the '
                                'forms alternating in one process; medians, minima and maxima of the blocks'),
      'device': torch.cuda.get_device_name(w.dev),
      'step_ms': {k: round(v, 4) for k, v in med.items()},
      'step_ms_min_max': {k: [round(min(v), 4), round(max(v), 4)] for k, v in blocks.items()},
      'step_ms_blocks': ab.rounded(blocks, 4),
      'step_launches': {k: len(v) for k, v in launches.items()},
      'decoder_tail_us': {k: round(v, 2) for k, v in tail_med.items()},
      'decoder_tail_us_blocks': ab.rounded(tail_blocks, 2),
      'decoder_tail_launches': tail_launches,
  }
  if not args.off_only:
    results['loss_shaping'] = SHAPING
    results['step_added_us'] = round((med['on'] - med['off']) * 1e3, 2)
    results['on_inside_off_min_max'] = bool(min(blocks['off']) <= med['on'] <= max(blocks['off']))
    results['step_launch_names_that_differ'] = [[a, b] for a, b in zip(launches['off'], launches['on']) if a != b]      # (the trace buffer may cut the last name)
  ab.write(results, args.out)


if __name__ == '__main__':
  main()
