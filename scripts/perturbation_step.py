#!/usr/bin/env python
"""What the perturbation pass costs on the geeco-f workload at bench.py's shape.

One process, device events around blocks of calls, the forms alternating (scripts/_step_ab.py):
  step:     the bare ``forward()`` beside one step of the pass on the observation frames -- apply + forward + score + accumulate --
            with the apply as a whole rewrite and in its incremental form (only the previous patch and the step's own);
  pass:     ``model.perturbation_attributions('occlusion', patch, stride)`` on the observation frames beside ``host_loop``: the
            loop a user would write without the device-side pass -- per position the occluded window made in numpy, a dense host
            batch through ``load_batch``, the forward, the predictions read back and scored on the host;
  kernels:  the apply on the rgb tensor, whole rewrite and incremental (alternating over the grid's steps, so every pair of
            neighbours and the row wraps are in it), the RISE apply, and the accumulate of both methods, each beside a device copy
            of the bytes the whole-tensor form moves.
Writes one JSON file (default profiles/perturbation/step.json).  Needs the GPU: there is no fallback.
"""
import _step_ab as ab


def main():
  ap = ab.arguments('perturbation', steps_help='(unused: a block is a fixed number of calls; --warmup is unused too)')
  ap.add_argument('--patch', type=int, default=64)
  ap.add_argument('--stride', type=int, default=64, help='the grid of the timed pass: (size - patch) / stride + 1 positions each way')
  ap.add_argument('--host_rounds', type=int, default=2, help='rounds of the host-loop form (it takes seconds per pass)')
  args = ap.parse_args()
  w = ab.workload(args, 'perturbation_step.py')

  import numpy as np
  import torch
  from geeco_amd import graph, ops

  N, K, H = w.N, w.K, w.H
  model = graph.GoalE2EVMC(w.cfg, N, w.dev, training=False)
  model.store.load_numpy(w.P)
  model.load_batch(w.feats, w.labels)
  occ = ops.perturb_desc('occlusion', H, H, patch=(args.patch, args.patch), stride=(args.stride, args.stride))
  rise = ops.perturb_desc('rise', H, H, grid=7, keep_prob=0.5, key=5)
  M = ops.perturb_steps(occ)
  x = model.inputs['rgb']
  clean = x.clone()
  d = model.decoder
  preds0, wgt, scores = torch.empty_like(d.preds), torch.ones(d.OT, device=w.dev), torch.zeros(M, N, device=w.dev)
  num, den = torch.zeros(N, H, H, device=w.dev), torch.zeros(N, H, H, device=w.dev)
  model.forward()
  preds0.copy_(d.preds)
  state = dict(m=0)

  def step_of(incremental):
    def step():
      m = state['m'] = (state['m'] + 1) % M
      ops.perturb_apply_into(x, clean, None, occ, m, prev_step=(m - 1) % M if incremental else -1)
      model.forward()
      ops.perturb_score_into(scores[m], d.preds, preds0, wgt)
      ops.perturb_accumulate_into(num, den, scores[m], occ, m, False)
    return step

  def prime():      # the buffer holds step state['m'] of the grid: what the incremental form starts from
    ops.perturb_apply_into(x, clean, None, occ, state['m'])

  prime()
  s_blocks = ab.alternate({'forward': model.forward, 'step_whole_rewrite': step_of(False), 'step_incremental': step_of(True)},
                          args.rounds, 16, warm=4)
  s_med = ab.medians(s_blocks)
  x.copy_(clean)

  def device_pass():
    model.perturbation_attributions('occlusion', patch=args.patch, stride=args.stride, inputs='rgb')

  host_rgb = w.feats['rgb'].numpy()
  rects = [ops.perturb_patch(occ, m)[2] for m in range(M)]

  def host_loop():
    model.load_batch(w.feats, w.labels)
    model.forward()
    p0 = d.preds.cpu().numpy()
    sums = np.zeros((2, N, H, H), np.float32)
    for y0, y1, x0, x1 in rects:
      hidden = host_rgb.copy()
      hidden[:, :, y0:y1, x0:x1] = 0
      model.load_batch(dict(w.feats, rgb=torch.from_numpy(hidden)), w.labels)
      model.forward()
      score = ((d.preds.cpu().numpy() - p0) ** 2).sum(1)
      sums[0, :, y0:y1, x0:x1] += score[:, None, None]
      sums[1, :, y0:y1, x0:x1] += 1
    model.load_batch(w.feats, w.labels)
    return sums[0] / np.maximum(sums[1], 1)

  device_pass()
  torch.cuda.synchronize()
  p_blocks = ab.alternate({'pass': device_pass}, args.rounds, 1, warm=1)
  h_blocks = ab.alternate({'host_loop': host_loop}, args.host_rounds, 1)
  p_med, h_med = ab.medians(p_blocks)['pass'], ab.medians(h_blocks)['host_loop']

  # the kernels alone on the rgb tensor, beside a copy of the bytes the whole-tensor form moves
  n = x.numel()

  def copy_of(nbytes):      # a copy reads and writes: half the bytes each way
    a, b = torch.empty(nbytes // 8, device=w.dev), torch.empty(nbytes // 8, device=w.dev)
    return lambda: b.copy_(a)

  dst = torch.empty_like(x)
  ops.perturb_apply_into(dst, clean, None, occ, 0)
  kstate = dict(m=0)

  def apply_of(incremental):
    def run():
      m = kstate['m'] = (kstate['m'] + 1) % M
      ops.perturb_apply_into(dst, clean, None, occ, m, prev_step=(m - 1) % M if incremental else -1)
    return run

  one = torch.ones(N, device=w.dev)
  patch_bytes = 2 * 2 * 4 * N * K * args.patch * args.patch * 3      # two patches, read and written
  forms = {
      'apply_whole_rewrite': (apply_of(False), 8 * n),
      'apply_incremental': (apply_of(True), 8 * n),
      'apply_rise': (lambda: ops.perturb_apply_into(dst, clean, None, rise, 3), 8 * n),
      'accumulate_occlusion': (lambda: ops.perturb_accumulate_into(num, den, one, occ, 1, False), 16 * N * H * H),
      'accumulate_rise': (lambda: ops.perturb_accumulate_into(num, den, one, rise, 3, False), 16 * N * H * H),
  }
  k_us, k_blocks = {}, {}
  for name, (fn, nbytes) in forms.items():
    if name == 'apply_incremental':      # (the buffer must hold the step before the first incremental call)
      ops.perturb_apply_into(dst, clean, None, occ, kstate['m'])
    blocks = ab.alternate({name: fn, 'copy_same_bytes': copy_of(nbytes)}, args.rounds, 16, warm=M, scale=1e3)
    med = ab.medians(blocks)
    k_us[name] = dict(us=round(med[name], 2), copy_same_bytes_us=round(med['copy_same_bytes'], 2), whole_tensor_bytes=nbytes,
                      over_copy=round(med[name] / med['copy_same_bytes'], 3))
    k_blocks[name] = ab.rounded(blocks, 2)
  k_us['apply_incremental']['bytes_touched'] = patch_bytes

  ab.write({
      'shape': dict(size=H, window_size=K, batch_size=N, model='geeco-f (training=False)', patch=args.patch, stride=args.stride, positions=M),
      'timing': dict(rounds=args.rounds, host_loop_rounds=args.host_rounds, step_calls_per_block=16, pass_calls_per_block=1,
                     kernel_calls_per_block=16,
                     method='device events around blocks of calls, the forms alternating in one process; medians of the blocks'),
      'device': torch.cuda.get_device_name(w.dev),
      'forward_ms': round(s_med['forward'], 3), 'step_whole_rewrite_ms': round(s_med['step_whole_rewrite'], 3),
      'step_incremental_ms': round(s_med['step_incremental'], 3), 'step_ms_blocks': ab.rounded(s_blocks, 3),
      'step_incremental_over_forward': round(s_med['step_incremental'] / s_med['forward'], 4),
      'pass_ms': round(p_med, 3), 'pass_ms_blocks': ab.rounded(p_blocks, 3)['pass'],
      'host_loop_ms': round(h_med, 1), 'host_loop_ms_blocks': ab.rounded(h_blocks, 1)['host_loop'], 'host_loop_over_pass': round(h_med / p_med, 2),
      'kernels': k_us, 'kernels_us_blocks': k_blocks,
      'the_pass_also_runs': 'two clean forwards (before and after), and copies of the clean frames out and back',
      'not_measured': ['any model but geeco-f, any shape but this one', 'RGB-D', "the target pass, RISE as a whole pass, score='loss'"],
  }, args.out)


if __name__ == '__main__':
  main()
