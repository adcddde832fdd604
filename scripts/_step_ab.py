"""What the option A/B scripts (ema_step.py, clip_step.py, lr_schedule_step.py, skip_nonfinite_step.py, finetune_step.py,
variable_stats_step.py, loss_shaping_step.py, grad_accum_step.py) share: the common arguments, the geeco-f workload at bench.py's
shape, a model with its ``TrainStepRunner``, blocks timed with device events in alternating rounds, and the JSON file.  Each script
keeps its own forms, its stand-alone passes and its result fields.  Imported as ``import _step_ab``: that resolves when a script is
run as ``python scripts/<name>.py`` (its directory is then first on sys.path), which is the only way they are run."""
import argparse
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def arguments(profile, steps_help='steps per timed block'):
  """The parser with the arguments every script has; ``--out`` defaults to profiles/<profile>/step.json."""
  ap = argparse.ArgumentParser()
  ap.add_argument('--size', type=int, default=256)
  ap.add_argument('--window_size', type=int, default=16)
  ap.add_argument('--batch_size', type=int, default=32)
  ap.add_argument('--steps', type=int, default=40, help=steps_help)
  ap.add_argument('--rounds', type=int, default=7)
  ap.add_argument('--warmup', type=int, default=6)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', profile, 'step.json'))
  return ap


def workload(args, script):
  """geeco-f at the arguments' shape: the config, the oracle's parameters and one synthetic batch (torch, on the host).  Needs the GPU."""
  import torch
  from geeco_amd.params import create_e2evmc_config
  from oracle import geeco_oracle as O
  if not torch.cuda.is_available():
    raise SystemExit('%s measures on the GPU; none is visible' % script)
  H, K, N = args.size, args.window_size, args.batch_size
  kw = dict(proc_obs='dynimg', proc_tgt='dyndiff', window_size=K, img_height=H, img_width=H, batch_size=N)
  ocfg = O.make_config(**kw)
  feats, labels = O.synthetic_batch(ocfg, True, N, seed=3, H=H, W=H)
  return types.SimpleNamespace(
      dev=torch.device('cuda', torch.cuda.current_device()), H=H, K=K, N=N, kw=kw, cfg=create_e2evmc_config(kw),
      P=O.init_params(O.model_param_shapes(ocfg, True), seed=0), feats={k: torch.from_numpy(v) for k, v in feats.items()},
      labels={k: torch.from_numpy(v) for k, v in labels.items()})


def build(w, warmup=0, before_runner=None, **options):
  """A training model with ``options`` on the workload's parameters and batch, and its TrainStepRunner (one hipGraph per step) after
  ``warmup`` steps; ``before_runner(model)`` runs in between."""
  from geeco_amd import graph
  from geeco_amd.runtime import TrainStepRunner
  m = graph.GoalE2EVMC(w.cfg, w.N, w.dev, training=True, **options)
  m.store.load_numpy(w.P)
  m.load_batch(w.feats, w.labels)
  if before_runner is not None:
    before_runner(m)
  r = TrainStepRunner(m, use_graph=True)
  for _ in range(warmup):
    r.step()
  return m, r


def timed_block(step, n):
  """Milliseconds per call of ``n`` calls of ``step``, between two device events."""
  import torch
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  for _ in range(n):
    step()
  b.record()
  b.synchronize()
  return a.elapsed_time(b) / n


def alternate(forms, rounds, n, warm=0, scale=1.0):
  """{name: [a block of ``n`` calls per round]} of ``forms`` ({name: callable}), the forms alternating; ``warm`` untimed calls of each
  first; ``scale`` 1e3: microseconds."""
  for fn in forms.values():
    if warm:
      timed_block(fn, warm)
  blocks = {k: [] for k in forms}
  for _ in range(rounds):
    for k, fn in forms.items():
      blocks[k].append(timed_block(fn, n) * scale)
  return blocks


def medians(blocks):
  return {k: statistics.median(v) for k, v in blocks.items()}


def rounded(blocks, digits):
  return {k: [round(x, digits) for x in v] for k, v in blocks.items()}


def timing(args, method):
  return dict(steps_per_block=args.steps, rounds=args.rounds, warmup=args.warmup, method=method)


def write(results, out, show=None):
  print(json.dumps(results if show is None else show), flush=True)
  os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
  with open(out, 'w') as fp:
    json.dump(results, fp, indent=1, sort_keys=True)
    fp.write('\n')
  print('wrote', out)
