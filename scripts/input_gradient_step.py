#!/usr/bin/env python
"""What the input-gradient pass costs, and that the training step beside it is what it was.

One process, device events around blocks of calls, the forms alternating (scripts/_step_ab.py):
  conv1_dgrad:   geeco_conv1_dgrad alone at ``--chunk`` x size^2 frames, beside a plain device copy of the same bytes (dz1 read +
                 dx written) in the same process: the copy is the kernel's floor; the ratio is reported, no target is set;
  dynimg_bwd:    geeco_dynimg_bwd alone at N = batch_size, K = window_size (its two launches);
  pass:          ``model.input_gradients()`` on the geeco-f workload at bench.py's shape, after one forward + backward;
  step:          the captured training step of that model (``--off_only`` measures this alone: run it in the parent's tree and in this
                 one, alternating, to compare the trees -- no launch of the step changes, profiles/train_options/step_calls.py).
Writes one JSON file (default profiles/input_grad/step.json).  Needs the GPU: there is no fallback.
"""
import _step_ab as ab


def main():
  ap = ab.arguments('input_grad')
  ap.add_argument('--chunk', type=int, default=96, help='frames of the conv1_dgrad measurement and of the pass (chunk_frames)')
  ap.add_argument('--off_only', action='store_true', help='the training step alone (works in a tree without the pass)')
  args = ap.parse_args()
  w = ab.workload(args, 'input_gradient_step.py')

  import torch
  from geeco_amd import ops

  model, runner = ab.build(w, args.warmup)
  torch.cuda.synchronize()
  step_blocks = ab.alternate({'step': runner.step}, args.rounds, args.steps)
  results = {
      'shape': dict(size=w.H, window_size=w.K, batch_size=w.N, model='geeco-f', chunk_frames=args.chunk),
      'timing': ab.timing(args, 'device events around blocks of calls, the forms alternating in one process; medians of the blocks'),
      'device': torch.cuda.get_device_name(w.dev),
      'step_ms': round(ab.medians(step_blocks)['step'], 4),
      'step_ms_blocks': ab.rounded(step_blocks, 4)['step'],
  }
  if args.off_only:
    return ab.write(results, args.out)

  # conv1_dgrad alone against a copy of the same bytes
  F, H = args.chunk, w.H
  dz1 = torch.randn(F, H, H, 32, device=w.dev)
  dz1 *= (torch.rand_like(dz1) < 0.5)
  dx = torch.empty(F, H, H, 4, device=w.dev)
  w1 = model.enc._w(0, 0)
  nbytes = dz1.numel() * 4 + dx.numel() * 4
  src = torch.empty(nbytes // 8, device=w.dev)      # a copy reads and writes: half the bytes each way
  dst = torch.empty_like(src)
  forms = {'conv1_dgrad': lambda: ops.conv1_dgrad_into(dx, dz1, w1, 1, 0, 0, 0, F, H, H, 3),
           'copy_same_bytes': lambda: dst.copy_(src)}
  k_blocks = ab.alternate(forms, args.rounds, 50, warm=10, scale=1e3)
  k_med = ab.medians(k_blocks)
  del dz1, dx, src, dst

  # dynimg_bwd alone
  N, K, HW = w.N, w.K, H * H
  frames = model.inputs['rgb']
  g = torch.randn(N, HW, 4, device=w.dev)
  d_frames = torch.empty_like(frames)
  ws = ops.dynimg_bwd_ws(N, HW, 3, w.dev)
  d_blocks = ab.alternate({'dynimg_bwd': lambda: ops.dynimg_bwd_into(d_frames, g, frames, K, N, HW, 3, 4, ws, K * HW * 3, HW * 3,
                                                                      K * HW * 3, HW * 3)}, args.rounds, 20, warm=5, scale=1e3)
  del g, d_frames

  # the whole pass (its buffers are allocated by the first call)
  model.forward(backward_too=True)
  model.backward()
  model.input_gradients(args.chunk)
  torch.cuda.synchronize()
  p_blocks = ab.alternate({'pass': lambda: model.input_gradients(args.chunk)}, args.rounds, 5, warm=1)
  after = ab.alternate({'step': runner.step}, args.rounds, args.steps)

  results.update({
      'conv1_dgrad_us': {k: round(v, 2) for k, v in k_med.items()},
      'conv1_dgrad_us_blocks': ab.rounded(k_blocks, 2),
      'conv1_dgrad_bytes': nbytes,
      'conv1_dgrad_GBps': round(nbytes / k_med['conv1_dgrad'] / 1e3, 1),
      'conv1_dgrad_over_copy': round(k_med['conv1_dgrad'] / k_med['copy_same_bytes'], 3),
      'dynimg_bwd_us': round(ab.medians(d_blocks)['dynimg_bwd'], 2),
      'dynimg_bwd_us_blocks': ab.rounded(d_blocks, 2)['dynimg_bwd'],
      'dynimg_bwd_bytes': N * HW * 4 * (2 * K * 3 + 2 * 4 + K * 3),
      'pass_ms': round(ab.medians(p_blocks)['pass'], 4),
      'pass_ms_blocks': ab.rounded(p_blocks, 4)['pass'],
      'step_ms_after_the_pass': round(ab.medians(after)['step'], 4),
      'step_ms_after_the_pass_blocks': ab.rounded(after, 4)['step'],
      'not_measured': ['any model but geeco-f, any shape but this one', 'RGB-D', 'the pass beside other work on the device'],
  })
  ab.write(results, args.out)


if __name__ == '__main__':
  main()
