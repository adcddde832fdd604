#!/usr/bin/env python
"""What the attribution pass costs on the geeco-f workload at bench.py's shape.

One process, device events around blocks of calls, the forms alternating (scripts/_step_ab.py):
  pass:          ``model.attributions('integrated_gradients', M)`` (M = ``--points``) beside ``plain``: M x (forward + backward +
                 ``input_gradients()``), the work the pass cannot avoid (the form that also runs without this feature,
                 scripts/input_gradient_step.py), and beside ``python_loop``: the loop a user would write without the device-side
                 pass -- per step the path point made in numpy, a dense host batch through ``load_batch``, the plain pass, and the
                 gradient copied to the host and summed there;
  kernels:       each new kernel alone at the workload's rgb tensor, beside a device copy of the same bytes; the finish at its two
                 launches; and from ``pass`` and these an ESTIMATE of the share of the pass the three kernels take (their
                 stand-alone times summed over the launches the pass makes; not a measurement inside the pass).
Writes one JSON file (default profiles/attribution/step.json).  Needs the GPU: there is no fallback.
"""
import _step_ab as ab


def main():
  ap = ab.arguments('attribution', steps_help='(unused: a block is one pass; --warmup is unused too)')
  ap.add_argument('--points', type=int, default=16, help='M: path points of the pass')
  ap.add_argument('--python_rounds', type=int, default=2, help='rounds of the host-loop form (it takes seconds per pass)')
  args = ap.parse_args()
  w = ab.workload(args, 'attribution_step.py')

  import numpy as np
  import torch
  from geeco_amd import graph, ops

  M, N, K, H = args.points, w.N, w.K, w.H
  model = graph.GoalE2EVMC(w.cfg, N, w.dev, training=True)
  model.store.load_numpy(w.P)
  model.load_batch(w.feats, w.labels)

  def plain():
    for _ in range(M):
      model.forward(backward_too=True)
      model.backward()
      model.input_gradients()

  def device_pass():
    model.attributions('integrated_gradients', M)

  keys = ('rgb', 'target_rgb')
  host = {k: w.feats[k].numpy() for k in keys}

  def python_loop():
    total = {k: np.zeros(host[k].shape, np.float32) for k in keys}
    for m in range(M):
      alpha = np.float32((m + 0.5) / M)
      model.load_batch(dict(w.feats, **{k: torch.from_numpy(alpha * host[k]) for k in keys}), w.labels)
      model.forward(backward_too=True)
      model.backward()
      g = model.input_gradients()
      for k in keys:
        total[k] += g[k].cpu().numpy() / np.float32(M)
    model.load_batch(w.feats, w.labels)
    return {k: host[k] * total[k] for k in keys}

  plain()
  device_pass()
  torch.cuda.synchronize()
  p_blocks = ab.alternate({'pass': device_pass, 'plain': plain}, args.rounds, 1, warm=1)
  py_blocks = ab.alternate({'python_loop': python_loop}, args.python_rounds, 1)
  p_med = ab.medians(p_blocks)

  # each kernel alone on the rgb tensor, beside a copy of the bytes it moves
  x = model.inputs['rgb']
  n = x.numel()
  dst, acc, g = torch.empty_like(x), torch.zeros_like(x), torch.randn_like(x)
  sal, sums = torch.empty(x.shape[:-1], device=w.dev), torch.empty(N, device=w.dev)
  frame = torch.rand(H * H * 3, device=w.dev)

  def copy_of(nbytes):      # a copy reads and writes: half the bytes each way
    a, b = torch.empty(nbytes // 8, device=w.dev), torch.empty(nbytes // 8, device=w.dev)
    return lambda: b.copy_(a)

  nbytes = {'path_point': 8 * n, 'path_point_black': 8 * n, 'path_point_noise': 8 * n, 'accumulate': 12 * n, 'accumulate_overwrite': 8 * n,
            'finish': 4 * n * 4 + 4 * n // 3}      # acc + x read, attr written and read again by the sum; saliency written
  forms = {
      'path_point': lambda: ops.attr_path_point_into(dst, x, frame, 0.5),
      'path_point_black': lambda: ops.attr_path_point_into(dst, x, None, 0.5),      # the form the timed pass runs
      'path_point_noise': lambda: ops.attr_path_point_into(dst, x, None, 1.0, 0.1, 7, 3),
      'accumulate': lambda: ops.attr_accumulate_into(acc, g, 1.0 / M, False),
      'accumulate_overwrite': lambda: ops.attr_accumulate_into(acc, g, 1.0 / M, True),
      'finish': lambda: ops.attr_finish_into(dst, sal, sums, acc, x, frame, True, N, K, H * H, 3),
  }
  k_us, k_blocks = {}, {}
  for name, fn in forms.items():
    blocks = ab.alternate({name: fn, 'copy_same_bytes': copy_of(nbytes[name])}, args.rounds, 20, warm=5, scale=1e3)
    med = ab.medians(blocks)
    k_us[name] = dict(us=round(med[name], 2), copy_same_bytes_us=round(med['copy_same_bytes'], 2), bytes=nbytes[name],
                      GBps=round(nbytes[name] / med[name] / 1e3, 1), over_copy=round(med[name] / med['copy_same_bytes'], 3))
    k_blocks[name] = ab.rounded(blocks, 2)
  # An ESTIMATE of the share, not a measurement inside the pass: the stand-alone times of the launches the pass makes on 'rgb' (M + 1
  # path points from black, M accumulations of which the first overwrites, one finish), scaled by (K + 1) / K for 'target_rgb', which
  # is one frame per sample beside rgb's K
  us = lambda name: k_us[name]['us']
  in_pass_ms = ((M + 1) * us('path_point_black') + (M - 1) * us('accumulate') + us('accumulate_overwrite') + us('finish')) * (K + 1) / K / 1e3

  ab.write({
      'shape': dict(size=H, window_size=K, batch_size=N, model='geeco-f', points=M),
      'timing': dict(rounds=args.rounds, python_loop_rounds=args.python_rounds, pass_calls_per_block=1, pass_warm_calls=1,
                     kernel_calls_per_block=20, kernel_warm_calls=5,
                     method='device events around blocks of calls, the forms alternating in one process; medians of the blocks'),
      'device': torch.cuda.get_device_name(w.dev),
      'pass_ms': round(p_med['pass'], 3), 'plain_ms': round(p_med['plain'], 3), 'pass_over_plain': round(p_med['pass'] / p_med['plain'], 4),
      'pass_ms_blocks': ab.rounded(p_blocks, 3),
      'python_loop_ms': round(ab.medians(py_blocks)['python_loop'], 1), 'python_loop_ms_blocks': ab.rounded(py_blocks, 1)['python_loop'],
      'kernels': k_us, 'kernels_us_blocks': k_blocks,
      'new_kernels_ms_in_the_pass_estimate': round(in_pass_ms, 3), 'new_kernels_share_of_the_pass_estimate': round(in_pass_ms / p_med['pass'], 4),
      'estimate_from': 'the stand-alone kernel times on rgb x (K + 1) / K: (M + 1) path points from black, M accumulations, one finish',
      'the_pass_also_runs': 'two forwards (loss at the baseline and at the clean input), and copies of the clean inputs out and back',
      'not_measured': ['any model but geeco-f, any shape but this one', 'RGB-D', 'SmoothGrad as a whole pass (its path point alone is)'],
  }, args.out)


if __name__ == '__main__':
  main()
