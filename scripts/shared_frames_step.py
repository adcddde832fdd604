#!/usr/bin/env python
"""Dense step vs shared-frame step of the per-frame controllers, one process, alternating.

Workload: N consecutive K-frame windows of ONE synthetic uint8 episode resident in HBM -- the batch Estimator.train feeds at
the defaults (256 x 256, K = 16, N = 32: 512 window positions, 47 distinct frames).  Per model (e2e_vmc; goal 'sequence' x
'residual') two training models share nothing but the inputs:
  dense:  geeco_gather_windows into the fp32 windows + the captured step on Nf = K N frames (what Estimator.train runs today);
  shared: the captured step on the frame table, Nf = F = N + 2 (K - 1) (+ 2 goal frames).
Both go through runtime.TrainStepRunner (hipGraph replays).  Timing: device events around blocks of ``--steps`` steps, the two
forms alternating for ``--rounds`` rounds after ``--warmup`` steps each; the median block and the spread of the blocks are
reported.  Peak memory: the rise of torch's allocator peak over what was allocated before the model was built, while it is
built, captured and warmed up (the shared model is built first and stays alive; the subtraction keeps it out of the dense figure).
Writes one JSON file (default profiles/shared_frames/step.json).  Needs the GPU: there is no fallback.
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
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--warmup', type=int, default=4)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'shared_frames', 'step.json'))
  args = ap.parse_args()

  import numpy as np
  import torch
  from geeco_amd import graph
  from geeco_amd.estimator import shared_frames_capacity
  from geeco_amd.input_fn import DeviceWindows, synthetic_scene_frames
  from geeco_amd.params import create_e2evmc_config
  from geeco_amd.runtime import TrainStepRunner
  from oracle import geeco_oracle as O

  if not torch.cuda.is_available():
    raise SystemExit('shared_frames_step.py measures on the GPU; none is visible')
  dev = torch.device('cuda', torch.cuda.current_device())
  H, K, N = args.size, args.window_size, args.batch_size
  T = N + K - 1
  rgb, _ = synthetic_scene_frames(T + 1, H, H, seed=[11, 0])
  resident = torch.from_numpy(rgb[:T].reshape(T, -1)).to(dev)
  goal_frame = torch.from_numpy(rgb[T:].reshape(1, -1)).to(dev)
  win = DeviceWindows(K, (H, H, 3), 255.0)
  win.add(resident, np.arange(N, dtype=np.int32))
  tgt = DeviceWindows(1, (H, H, 3), 255.0, squeeze_k=True)
  tgt.add(goal_frame, np.zeros(N, np.int32))

  def timed_block(step, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
      step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n

  results = {'shape': dict(size=H, window_size=K, batch_size=N, window_positions=N * K, distinct_frames=T),
             'timing': dict(steps_per_block=args.steps, rounds=args.rounds, warmup=args.warmup,
                            method='device events around blocks of steps, dense and shared alternating in one process; dense '
                                   'includes the window gather Estimator.train runs per step'),
             'device': torch.cuda.get_device_name(dev), 'models': {}}
  for name, goal, extra in (('e2e_vmc', False, {}), ('goal_sequence_residual', True, dict(proc_obs='sequence', proc_tgt='residual'))):
    kw = dict(window_size=K, img_height=H, img_width=H, batch_size=N, **extra)
    ocfg = O.make_config(**kw)
    cfg = create_e2evmc_config(kw)
    P = O.init_params(O.model_param_shapes(ocfg, goal), seed=0)
    feats, labels = O.synthetic_batch(ocfg, goal, N, seed=3, H=8, W=8)       # states and labels only: the images come from the episode
    small = {k: torch.from_numpy(v) for k, v in feats.items() if k not in ('rgb', 'target_rgb')}
    lab = {k: torch.from_numpy(v) for k, v in labels.items()}
    ctor = graph.GoalE2EVMC if goal else graph.E2EVMC
    forms, peak = {}, {}
    # -- shared ------------------------------------------------------------------------------------
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    F = shared_frames_capacity(True, N, K, goal)
    table, index, tindex, used = win.frame_table(F, tgt if goal else None, dev)
    ms = ctor(cfg, N, dev, training=True, shared_frames=F)
    ms.store.load_numpy(P)
    f = dict(small, frame_table=torch.from_numpy(table), frame_index=torch.from_numpy(index))
    if goal:
      f['target_index'] = torch.from_numpy(tindex)
    ms.load_batch(f, lab)
    rs = TrainStepRunner(ms, use_graph=True)
    forms['shared'] = rs.step
    for _ in range(args.warmup):
      rs.step()
    torch.cuda.synchronize()
    peak['shared'] = torch.cuda.max_memory_allocated(dev) - base
    # -- dense -------------------------------------------------------------------------------------
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    md = ctor(cfg, N, dev, training=True)
    md.store.load_numpy(P)
    for k, buf in md.inputs.items():
      if k in small:
        buf.copy_(small[k])
      elif k in lab:
        buf.copy_(lab[k])
    rd = TrainStepRunner(md, use_graph=True)

    def dense_step():
      win.materialize_into(md.inputs['rgb'])
      if goal:
        tgt.materialize_into(md.inputs['target_rgb'].view(N, 1, H, H, 3))
      rd.step()
    forms['dense'] = dense_step
    for _ in range(args.warmup):
      dense_step()
    torch.cuda.synchronize()
    peak['dense'] = torch.cuda.max_memory_allocated(dev) - base
    loss = {k: float(m.loss) for k, m in (('shared', ms), ('dense', md))}
    # -- alternate ---------------------------------------------------------------------------------
    blocks = {'dense': [], 'shared': []}
    for _ in range(args.rounds):
      for k in ('dense', 'shared'):
        blocks[k].append(timed_block(forms[k], args.steps))
    med = {k: statistics.median(v) for k, v in blocks.items()}
    results['models'][name] = {
        'F': F, 'slots_used': int(used), 'frames_encoded': {'dense': int(md.enc.Nf), 'shared': int(ms.enc.Nf)},
        'step_ms': {k: round(med[k], 4) for k in med},
        'step_ms_blocks': {k: [round(x, 4) for x in v] for k, v in blocks.items()},
        'speedup': round(med['dense'] / med['shared'], 3),
        'peak_memory_bytes': {k: int(v) for k, v in peak.items()},
        'loss_after_warmup': loss,
    }
    print(name, json.dumps(results['models'][name]), flush=True)
    del ms, md, rs, rd, forms
    torch.cuda.empty_cache()
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as fp:
    json.dump(results, fp, indent=1, sort_keys=True)
    fp.write('\n')
  print('wrote', args.out)


if __name__ == '__main__':
  main()
