"""A/B of the Adam update between two builds of the library: SHA-256 of every output buffer of every entry point, and launch times.

  python scripts/dev/adam_ab.py --root <tree> --out hashes.json           # the buffers: p, m, v, the shadow arena, g_out
  python scripts/dev/adam_ab.py --root <tree> --out hashes.json --full    # ... one record per buffer and case, to locate a difference
  python scripts/dev/adam_ab.py --root <tree> --out times.json --time     # median launch time per entry point, in microseconds
  python scripts/dev/adam_ab.py --compare a.json b.json                   # exit status 1 and the differing keys unless identical
  python scripts/dev/adam_ab.py --spread parent1.json parent2.json ... --against new1.json ... --out timing.json

``--root``: the tree whose ``geeco_amd`` (with its built library) is imported; default: the tree this file is in.  One process per
tree, so the same file measures a checkout of another commit standing next to this one.  The kernel cases are those of
tests/test_clip_gpu.py (n = 5 and 1027, one piece and CLIP_PIECES, l2, grad_scale) times clip scale, guard verdict and multipliers;
the step cases are two captured steps (one eager step, the capture, two replays) of the two models of that file's step tests, without
any option and with EMA + clip + skip + multipliers.  Every output buffer of every case is hashed; the file holds one record per buffer
of a step and, for the kernel cases, one per entry point and buffer: the SHA-256 over the sorted "case | buffer=hash" lines of all its
cases (``--full``: the lines themselves).  ``--dry``: everything but the device (arguments, inputs, the list of cases).
"""
import argparse
import hashlib
import itertools
import json
import os
import sys

import numpy as np

NAN = float('nan')
LR_T = 1e-3
ADAM = dict(beta1=0.9, beta2=0.999, eps=1e-8)
CLIP_PIECES = {5: [(4, 1), (0, 4)], 1027: [(512, 515), (0, 256), (256, 256)]}      # tests/test_clip_gpu.py
MULTIPLIERS = (1.0, 0.1, 3.0)
H, K3, CLIP = 136, 3, 0.01                                                        # the step tests' shapes and clip norm
MODELS = {'e2e_vmc': (False, {}), 'goal residual': (True, dict(proc_obs='sequence', proc_tgt='residual'))}
ALL_OPTIONS = dict(ema_decay=0.9, clip_norm=CLIP, skip_nonfinite=True, lr_multipliers={'Encoder/conv[45]/': 0, 'Encoder/': 0.1})


def inputs(n):
  """p, g, m, v, shadow as numpy float32 (tests/test_clip_gpu.py: gradients ~0.1, parameters ~1)."""
  r = np.random.default_rng(2000 + n % 1013)
  p, g, m, s = (r.standard_normal(n).astype(np.float32) for _ in range(4))
  v = (r.standard_normal(n).astype(np.float32)) ** 2
  return p, g * np.float32(0.1), m * np.float32(0.1), v * np.float32(0.01), s


def whole4(pieces):
  """The pieces as the entry points that take whole float4s alone accept them: counts rounded down, empty pieces dropped."""
  return [(off, cnt & ~3) for off, cnt in pieces if cnt >= 4]


def kernel_cases():
  """(key, entry, n, pieces, options): every entry point at every shape and option value."""
  out = []
  for n, layout, l2, gs, ema in itertools.product((5, 1027), ('one', 'pieces'), (0.0, 1e-3), (1.0, 0.125), (False, True)):
    pieces = [(0, n)] if layout == 'one' else CLIP_PIECES[n]
    base = 'n=%d %s l2=%g gs=%g ema=%d' % (n, layout, l2, gs, ema)
    kw = dict(l2=l2, grad_scale=gs, ema=ema)
    if layout == 'one':
      out.append((base + ' adam_tf' + ('_ema' if ema else ''), 'whole', n, pieces, kw))
    out.append((base + ' segments' + ('_ema' if ema else ''), 'segments', n, whole4(pieces), kw))
    for s in (1.0, 0.37):
      out.append(('%s clip s=%g' % (base, s), 'clip', n, pieces, dict(kw, s=s)))
      for verdict in (0, 1):
        out.append(('%s guard s=%g verdict=%d' % (base, s, verdict), 'guard', n, pieces, dict(kw, s=s, verdict=verdict)))
    for mul in ((1.0,) * len(pieces), MULTIPLIERS[-len(pieces):]):
      for s, verdict in ((None, None), (1.0, None), (0.37, None), (0.37, 0), (0.37, 1)):
        out.append(('%s scaled mul=%s s=%s verdict=%s' % (base, mul, s, verdict), 'scaled', n, pieces, dict(kw, s=s, verdict=verdict, mul=mul)))
  return out


def sha(t):
  return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def scalars(torch, dev, o):
  """scal, the step counter, and [s, norm] / [verdict, 0, 0] as geeco_clip_scale / geeco_guard_decide leave them (None: not given)."""
  scal = torch.tensor([LR_T, 0, 0, 0], dtype=torch.float32, device=dev)
  step = torch.full((1,), 5, dtype=torch.int64, device=dev)
  clip = None if o.get('s') is None else torch.tensor([o['s'], 0.0], dtype=torch.float32, device=dev)
  guard = None if o.get('verdict') is None else torch.tensor([o['verdict'], 0, 0], dtype=torch.int64, device=dev)
  return scal, step, clip, guard


def launch(ops, entry, a, segs, sc, o, g_out):
  """One launch of ``entry`` on the arenas ``a`` = (p, g, m, v, shadow) with the device scalars ``sc`` of ``scalars``."""
  p, g, m, v, shadow = a
  scal, step, clip, guard = sc
  kw = dict(grad_scale=o['grad_scale'], l2=o['l2'], **ADAM)
  ekw = dict(ema=shadow, global_step=step, decay=0.99) if o['ema'] else {}
  if entry == 'whole':
    n = segs[0][2]
    if o['ema']:
      ops.adam_tf_ema(p, g, m, v, shadow, n, scal, step, 0.99, **kw)
    else:
      ops.adam_tf(p, g, m, v, n, scal, **kw)
  elif entry == 'segments':
    if o['ema']:
      ops.adam_tf_segments_ema(p, m, v, shadow, segs, scal, step, 0.99, g_out=g_out, **kw)
    else:
      ops.adam_tf_segments(p, m, v, segs, scal, g_out=g_out, **kw)
  elif entry == 'clip':
    ops.adam_tf_segments_clip(p, m, v, segs, scal, clip, g_out=g_out, **ekw, **kw)
  elif entry == 'guard':
    ops.adam_tf_segments_guard(p, m, v, segs, scal, clip, guard, g_out=g_out, **ekw, **kw)
  else:
    ops.adam_tf_segments_scaled(p, m, v, segs, list(o['mul']), scal, clip_dev=clip, guard=guard, g_out=g_out, **ekw, **kw)


def run_kernels(ops, torch, dev):
  out = {}
  for key, entry, n, pieces, o in kernel_cases():
    def on_dev(x):      # 5 NaN elements behind every arena: they are hashed too
      t = torch.full((x.size + 5,), NAN, dtype=torch.float32, device=dev)
      t[:x.size] = torch.from_numpy(x)
      return t
    a = [on_dev(x) for x in inputs(n)]
    g_out = None if entry == 'whole' else torch.full((n + 5,), NAN, dtype=torch.float32, device=dev)
    segs = [(a[1][off:off + cnt], off, cnt) for off, cnt in pieces]
    launch(ops, entry, a, segs, scalars(torch, dev, o), o, g_out)
    torch.cuda.synchronize()
    bufs = dict(zip(('p', 'm', 'v', 'shadow'), (a[0], a[2], a[3], a[4])))
    if g_out is not None:
      bufs['g_out'] = g_out
    for name, t in bufs.items():
      out['%s | %s' % (key, name)] = sha(t)
  return out


def run_steps(torch, dev):
  from geeco_amd import graph
  from geeco_amd.params import create_e2evmc_config
  from geeco_amd.runtime import TrainStepRunner
  from oracle import geeco_oracle as O
  out = {}
  for name, (goal, extra) in MODELS.items():
    ocfg = O.make_config(window_size=K3, img_height=H, img_width=H, batch_size=4, lr=1e-3, **extra)
    P = O.init_params(O.model_param_shapes(ocfg, goal), seed=1)
    feats, labels = O.synthetic_batch(ocfg, goal, 4, seed=3, H=H, W=H)
    for what, options in (('no option', {}), ('every option', ALL_OPTIONS)):
      model = (graph.GoalE2EVMC if goal else graph.E2EVMC)(create_e2evmc_config(ocfg._asdict()), 4, dev, training=True, **options)
      model.store.load_numpy(P)
      model.load_batch({k: torch.from_numpy(v) for k, v in feats.items()}, {k: torch.from_numpy(v) for k, v in labels.items()})
      runner = TrainStepRunner(model, use_graph=True, warmup=1)      # one eager step, then the capture and two replays
      for _ in range(3):
        runner.step()
      torch.cuda.synchronize()
      s = model.store
      bufs = dict(p=s.params, m=s.adam_m, v=s.adam_v, g=s.grads, step=s.global_step, scal=model.scal)
      for k in ('clip_out', 'clip_ws', 'guard'):
        if getattr(model, k) is not None:
          bufs[k] = getattr(model, k)
      if s.ema is not None:
        bufs['shadow'] = s.ema
      for k, t in bufs.items():
        out['step: %s, %s | %s' % (name, what, k)] = sha(t)
  return out


def grouped(rec):
  """The per-buffer records of the kernel cases folded to one per entry point and buffer; a step's records as they are."""
  out, digests, count = {}, {}, {}
  for k, h in sorted(rec.items()):
    if k.startswith('step:'):
      out[k] = h
      continue
    case, buf = k.split(' | ')
    group = '%s | %s' % (case.split(' ema=')[1].split(' ')[1], buf)
    digests.setdefault(group, hashlib.sha256()).update(('%s=%s\n' % (k, h)).encode())
    count[group] = count.get(group, 0) + 1
  out.update(('%s, %d cases' % (g, count[g]), d.hexdigest()) for g, d in digests.items())
  return out


def dump(rec, path):
  """JSON with one top-level key per line."""
  with open(path, 'w') as f:
    f.write('{\n' + ',\n'.join(' %s: %s' % (json.dumps(k), json.dumps(rec[k], sort_keys=True)) for k in sorted(rec)) + '\n}\n')


def bench_arena_size():
  """``store.size`` of bench.py's default model (geeco-f, RGB, K = 32; the batch size does not enter)."""
  from geeco_amd import graph
  from geeco_amd.params import create_e2evmc_config
  cfg = create_e2evmc_config(dict(proc_obs='dynimg', proc_tgt='dyndiff', window_size=32, img_channels=3, batch_size=32))
  return cfg, graph.build_store(cfg, True, 'cpu').size


TIMED = [('adam_tf', 'whole', False), ('adam_tf_ema', 'whole', True), ('adam_tf_segments', 'segments', False), ('adam_tf_segments_ema', 'segments', True),
         ('adam_tf_segments_clip', 'clip', False), ('adam_tf_segments_clip ema', 'clip', True), ('adam_tf_segments_guard', 'guard', False),
         ('adam_tf_segments_guard ema', 'guard', True), ('adam_tf_segments_scaled', 'scaled', False), ('adam_tf_segments_scaled ema', 'scaled', True)]


def run_times(ops, torch, dev, samples, batch):
  """Median over ``samples`` of the time of one launch, each sample ``batch`` launches between two device events; the pieces of the
  segment entry points are the two of the single-GPU step (runtime.gradient_buckets: everything but conv1 / conv2, then those)."""
  from geeco_amd import graph
  from geeco_amd.runtime import gradient_buckets
  cfg, n = bench_arena_size()
  store = graph.build_store(cfg, True, dev, ema=True)
  assert store.size == n
  early, late = gradient_buckets(store)
  r = np.random.default_rng(7)
  for t, scale in ((store.params, 1.0), (store.grads, 0.1), (store.ema, 1.0)):
    t.copy_(torch.from_numpy((r.standard_normal(n) * scale).astype(np.float32)))
  a = (store.params, store.grads, store.adam_m, store.adam_v, store.ema)
  out = {'arena_floats': int(n), 'samples': samples, 'launches_per_sample': batch, 'median_us': {}}
  for name, entry, ema in TIMED:
    ranges = [(0, n)] if entry == 'whole' else list(early) + list(late)
    if len(ranges) > 8:
      ranges = [(0, n)]
    segs = [(store.grads[off:off + cnt], off, cnt) for off, cnt in ranges]
    o = dict(l2=0.0, grad_scale=1.0, ema=ema, s=None if entry in ('whole', 'segments') else 1.0, verdict=1 if entry in ('guard', 'scaled') else None,
             mul=MULTIPLIERS[-len(segs):] if len(segs) <= 3 else (1.0,) * len(segs))
    sc = scalars(torch, dev, o)
    go = lambda: launch(ops, entry, a, segs, sc, o, None)
    for _ in range(20):
      go()
    times = []
    for _ in range(samples):
      t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      t0.record()
      for _ in range(batch):
        go()
      t1.record()
      t1.synchronize()
      times.append(t0.elapsed_time(t1) * 1e3 / batch)
    out['median_us'][name] = round(float(np.median(times)), 3)
    out.setdefault('pieces', {})[name] = len(segs)
  return out


def compare(a, b):
  A, B = json.load(open(a)), json.load(open(b))
  diff = sorted(k for k in set(A) | set(B) if A.get(k) != B.get(k))
  print('%d buffers in %s, %d in %s: %s' % (len(A), a, len(B), b, 'identical' if not diff else '%d differ' % len(diff)))
  for k in diff[:40]:
    print('  ' + k)
  return 1 if diff else 0


def spread(parents, news, out):
  """The parent's run-to-run spread per entry point is the margin: no run of the other build may be slower than the parent's slowest by more."""
  P, N = [json.load(open(f))['median_us'] for f in parents], [json.load(open(f))['median_us'] for f in news]
  rec, bad = {'arena_floats': json.load(open(parents[0]))['arena_floats']}, 0
  for k in P[0]:
    lo, hi = min(p[k] for p in P), max(p[k] for p in P)
    ok = all(x[k] <= hi + (hi - lo) for x in N)
    bad += not ok
    rec[k] = dict(parent_us=[p[k] for p in P], parent_spread_us=round(hi - lo, 3), new_us=[x[k] for x in N], within_spread=ok)
    print('%-30s parent %s (spread %.3f)  new %s  %s' % (k, [p[k] for p in P], hi - lo, [x[k] for x in N], 'ok' if ok else 'SLOWER'))
  dump(rec, out)
  return 1 if bad else 0


def main():
  ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument('--root', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
  ap.add_argument('--out')
  ap.add_argument('--time', action='store_true')
  ap.add_argument('--samples', type=int, default=200)
  ap.add_argument('--batch', type=int, default=10)
  ap.add_argument('--no-steps', action='store_true', help='the kernel cases alone')
  ap.add_argument('--full', action='store_true', help='one record per buffer and kernel case')
  ap.add_argument('--dry', action='store_true')
  ap.add_argument('--compare', nargs=2)
  ap.add_argument('--spread', nargs='+')
  ap.add_argument('--against', nargs='+')
  args = ap.parse_args()
  if args.compare:
    return compare(*args.compare)
  if args.spread:
    if not (args.against and args.out):
      ap.error('--spread needs --against and --out')
    return spread(args.spread, args.against, args.out)
  if not args.out and not args.dry:
    ap.error('--out is needed')
  if args.samples < 200:
    ap.error('at least 200 samples')
  sys.path.insert(0, os.path.abspath(args.root))
  if args.dry:
    cases = kernel_cases()
    for n in (5, 1027):
      assert all(x.dtype == np.float32 and x.size == n for x in inputs(n))
    assert len({c[0] for c in cases}) == len(cases)
    print('%d kernel cases over %s; %d step cases; arena of the timed launches: %d floats'
          % (len(cases), sorted({c[1] for c in cases}), 2 * len(MODELS), bench_arena_size()[1]))
    return 0
  import torch
  import geeco_amd
  from geeco_amd import ops
  print('geeco_amd of', os.path.dirname(os.path.abspath(geeco_amd.__file__)))
  dev = torch.device('cuda:0')
  if args.time:
    rec = run_times(ops, torch, dev, args.samples, args.batch)
  else:
    rec = run_kernels(ops, torch, dev)
    if not args.no_steps:
      rec.update(run_steps(torch, dev))
    print('%d buffers hashed' % len(rec))
    rec = rec if args.full else grouped(rec)
  dump(rec, args.out)
  print('%s: %d records' % (args.out, len(rec.get('median_us', rec))))
  return 0


if __name__ == '__main__':
  sys.exit(main())
