"""Control steps per second: the batch-1 API (predictor.py: a one-env view of the batched predictor, with the host-side frame
check) vs B envs per call on the same engine (geeco_amd/batched_predictor.py).

Random-weight checkpoints as bench.py's inference leg builds them; geeco-f (dynimg + dyndiff, RGB) and e2e_vmc at 256^2,
K = 16; B in {1, 8, 32, 64}; float32 and uint8 frames from pinned host arrays.  Every timed call ends in the call's own
synchronise; host clock, after warm-up.  The per-frame models (e2e_vmc and goal_e2evmc 'sequence' x 'residual') also run in
incremental mode (``incremental=True``: encoder features cached on the device, B frames encoded per call instead of K * B): rows
``*_incremental`` beside the windowed rows of the same process, with ``speedup_vs_windowed`` and ``peak_mem_vs_windowed``.
Every row carries ``peak_mem_mb`` (torch.cuda.max_memory_allocated over the row's predictor).  Prints (and with --out writes)
one JSON document:
  python scripts/predictor_throughput.py [--calls 100] [--warmup 10] [--batches 1,8,32,64] [--models a,b] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from geeco_amd import estimator as est  # noqa: E402
from geeco_amd.batched_predictor import BatchedE2EVMCPredictor, BatchedGoalE2EVMCPredictor  # noqa: E402
from geeco_amd.graph import model_variable_shapes  # noqa: E402
from geeco_amd.params import create_e2evmc_config  # noqa: E402
from geeco_amd.predictor import E2EVMCPredictor, GoalE2EVMCPredictor  # noqa: E402
from geeco_amd.variables import VariableStore  # noqa: E402

MODELS = (('geeco-f', True, dict(proc_obs='dynimg', proc_tgt='dyndiff')), ('e2e_vmc', False, {}),
          ('goal_seq_residual', True, dict(proc_obs='sequence', proc_tgt='residual')))
INCREMENTAL = ('e2e_vmc', 'goal_seq_residual')       # the models whose observation path is per frame


def model_dir(root, name, goal, kw, K):
  md = os.path.join(root, name)
  os.makedirs(md, exist_ok=True)
  cfg = create_e2evmc_config(dict(window_size=K, **kw))
  with open(os.path.join(md, 'e2evmc_config.json'), 'w') as fp:
    json.dump(cfg._asdict(), fp)
  st = VariableStore(model_variable_shapes(cfg, goal), 'cpu')
  st.initialize(seed=0)
  est.save_checkpoint(st, md, keep_max=1)
  return md


def pinned(a):
  t = torch.empty(a.shape, dtype=torch.from_numpy(a[:0].copy()).dtype, pin_memory=True)
  t.numpy()[...] = a
  return t.numpy()


def timed(fn, calls, warmup):
  for i in range(warmup):
    fn(i)
  lat = []
  for i in range(calls):
    t = time.perf_counter()
    fn(i)
    lat.append((time.perf_counter() - t) * 1e3)
  lat.sort()
  return {'calls': calls, 'peak_mem_mb': round(torch.cuda.max_memory_allocated() / 2 ** 20, 1), 'p50_ms': round(float(np.percentile(lat, 50)), 4), 'p99_ms': round(float(np.percentile(lat, 99)), 4)}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--calls', type=int, default=100)
  ap.add_argument('--warmup', type=int, default=10)
  ap.add_argument('--batches', default='1,8,32,64')
  ap.add_argument('--K', type=int, default=16)
  ap.add_argument('--models', default=','.join(m[0] for m in MODELS))
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  dev = torch.device('cuda:0')
  r = np.random.default_rng(0)
  res = {'workload': '256x256 RGB, K=%d, random weights; host clock per call (each call ends in its own synchronise)' % args.K,
         'device': torch.cuda.get_device_name(0), 'models': {}}
  with tempfile.TemporaryDirectory() as root:
    for name, goal, kw in MODELS:
      if name not in args.models.split(','):
        continue
      modes = (False, True) if name in INCREMENTAL else (False,)
      md = model_dir(root, name, goal, kw, args.K)
      rows = {}
      u8 = r.integers(0, 256, (8, 256, 256, 3), dtype=np.uint8)
      f32 = pinned(u8.astype(np.float32) / np.float32(255.0))
      jnt = r.standard_normal((8, 7)).astype(np.float32)
      for inc in modes:
        sfx, ikw = ('_incremental', dict(incremental=True)) if inc else ('', {})
        torch.cuda.reset_peak_memory_stats()
        p1 = (GoalE2EVMCPredictor if goal else E2EVMCPredictor)(md, memcap=None, device=dev, **ikw)
        if goal:
          p1.set_goal(f32[7])
        row = timed(lambda i: p1.predict(f32[i % 8], jnt[i % 8]), args.calls, args.warmup)
        row['env_steps_per_s'] = round(1e3 / row['p50_ms'], 1)
        rows['batch1_float32' + sfx] = row
        print(name, 'batch-1' + sfx, row, flush=True)
        del p1
        torch.cuda.empty_cache()
      for B in [int(b) for b in args.batches.split(',')]:
        for fdt, inc in [(f, i) for f in ('float32', 'uint8') for i in modes]:
          sfx, ikw = ('_incremental', dict(incremental=True)) if inc else ('', {})
          torch.cuda.reset_peak_memory_stats()
          src = u8 if fdt == 'uint8' else u8.astype(np.float32) / np.float32(255.0)
          idx = [(np.arange(B) + i) % 8 for i in range(4)]
          frames = [pinned(src[ix]) for ix in idx]               # the caller's pinned frame arrays
          jn = [np.ascontiguousarray(jnt[ix]) for ix in idx]
          p = (BatchedGoalE2EVMCPredictor if goal else BatchedE2EVMCPredictor)(md, num_envs=B, memcap=None, device=dev,
                                                                               frame_dtype=fdt, **ikw)
          if goal:
            p.set_goal(src[idx[0]][::-1].copy())
          row = timed(lambda i: p.predict(frames[i % 4], jn[i % 4]), args.calls, args.warmup)
          row['env_steps_per_s'] = round(B * 1e3 / row['p50_ms'], 1)
          row['window_form'] = p.window_form
          rows['B%d_%s%s' % (B, fdt, sfx)] = row
          print(name, B, fdt + sfx, row, flush=True)
          del p
          torch.cuda.empty_cache()
      base = rows['batch1_float32']['env_steps_per_s']
      for k, v in rows.items():
        v['speedup_vs_batch1'] = round(v['env_steps_per_s'] / base, 2)
        if k.endswith('_incremental'):
          w = rows[k[:-len('_incremental')]]
          v['speedup_vs_windowed'] = round(v['env_steps_per_s'] / w['env_steps_per_s'], 2)
          v['peak_mem_vs_windowed'] = round(v['peak_mem_mb'] / w['peak_mem_mb'], 4)
      res['models'][name] = rows
  txt = json.dumps(res, indent=1)
  print(txt)
  if args.out:
    with open(args.out, 'w') as fp:
      fp.write(txt + '\n')


if __name__ == '__main__':
  main()
