#!/usr/bin/env python
"""The fill through geeco_gather_windows_augmented under two builds of the library ("one body"): the product build
against a variant that scripts/dev/build_variant.sh made of another commit, e.g. the one before the augmented entry took an
instance of the shared gather body.

  python scripts/augment_one_body_fill.py --yardstick libgeeco_hip_parent.so [--out profiles/augment/one_body.json]

Protocol of 5.26: N = 32 windows of K = 16 frames; 'rgb' = 256 x 256 x 3 uint8 with shifts in -16..16, gain 1 +- 0.2, bias +- 0.1;
'depth' = 256 x 256 x 1 float32, the same shifts, no colour.  A block = 50 fills after 6 warm-up calls, device time by events
around the block.  5 blocks per library, the two libraries alternating block by block, every block in a fresh child process
(GEECO_DEV=1 GEECO_LIB=...).  Per stream the children also hash the filled buffer: the two libraries must agree bit for bit.
The yardstick is the other build: the product's median block must lie inside the min..max spread of the yardstick's blocks."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, K, H, W, SHIFT, GAIN, BIAS = 32, 16, 256, 256, 16, 0.2, 0.1
WARMUP, FILLS, BLOCKS = 6, 50, 5
STREAMS = {'rgb': (3, 'uint8'), 'depth': (1, 'float32')}


def child():
  """One block per stream under the library the environment names; prints {stream: [ms per fill, sha1 of the output]}."""
  import numpy as np
  import torch
  from geeco_amd import ops
  dev = torch.device('cuda:0')
  torch.manual_seed(5)      # the same frames in every child
  r = np.random.default_rng(5)
  shift = torch.from_numpy(r.integers(-SHIFT, SHIFT + 1, (N, 2)).astype(np.int32)).to(dev)
  result = {}
  for name, (C, dtype) in STREAMS.items():
    fe = H * W * C
    # every window has K frames of its own: N * K distinct resident frames
    frames = (torch.randint(0, 256, (N * K, fe), dtype=torch.uint8, device=dev) if dtype == 'uint8' else
              torch.rand((N * K, fe), dtype=torch.float32, device=dev))
    addr = torch.tensor([frames.data_ptr() + n * K * fe * frames.element_size() for n in range(N)], dtype=torch.int64, device=dev)
    kind = torch.full((N,), 0 if dtype == 'uint8' else 1, dtype=torch.int32, device=dev)
    colour = None
    if C == 3:
      colour = torch.from_numpy(np.concatenate([r.uniform(1 - GAIN, 1 + GAIN, (N, 3)), r.uniform(-BIAS, BIAS, (N, 3))],
                                               axis=1).astype(np.float32)).to(dev)
    out = torch.empty((N, K, H, W, C), dtype=torch.float32, device=dev)
    fill = lambda: ops.gather_windows_augmented_into(out, addr, kind, shift, colour, N, K, H, W, C)
    for _ in range(WARMUP):
      fill()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(FILLS):
      fill()
    t1.record()
    torch.cuda.synchronize()
    result[name] = [t0.elapsed_time(t1) / FILLS, hashlib.sha1(out.cpu().numpy().tobytes()).hexdigest()]
    del frames, out
  print('RESULT ' + json.dumps(result))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--yardstick', help='file name of the other build, next to libgeeco_hip.so')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'augment', 'one_body.json'))
  ap.add_argument('--child', action='store_true')
  args = ap.parse_args()
  if args.child:
    return child()
  libs = {'yardstick': args.yardstick, 'product': 'libgeeco_hip.so'}
  blocks = {lib: {s: [] for s in STREAMS} for lib in libs}
  hashes = {s: set() for s in STREAMS}
  for b in range(BLOCKS):
    for lib, name in libs.items():       # a child that fails or overruns ends the run: nothing more is started
      env = dict(os.environ, GEECO_DEV='1', GEECO_LIB=name)
      text = subprocess.run([sys.executable, os.path.abspath(__file__), '--child'], env=env, check=True, timeout=300,
                            stdout=subprocess.PIPE).stdout.decode()
      got = json.loads(next(l for l in text.splitlines() if l.startswith('RESULT '))[7:])
      for s, (ms, digest) in got.items():
        blocks[lib][s].append(round(ms, 5))
        hashes[s].add(digest)
      print(b, lib, {s: round(v[0], 5) for s, v in got.items()}, flush=True)
  report = dict(shape=dict(N=N, K=K, H=H, W=W, shift=SHIFT, gain=GAIN, bias=BIAS, streams=STREAMS), warmup=WARMUP, fills=FILLS,
                libraries=libs, unit='ms per fill, device events around a block', streams={})
  for s in STREAMS:
    y, p = blocks['yardstick'][s], blocks['product'][s]
    report['streams'][s] = dict(yardstick_blocks=y, product_blocks=p, yardstick_median=statistics.median(y),
                                product_median=statistics.median(p), yardstick_min=min(y), yardstick_max=max(y),
                                product_median_inside_yardstick_spread=min(y) <= statistics.median(p) <= max(y),
                                product_median_not_above_yardstick_max=statistics.median(p) <= max(y),
                                outputs_bitwise_equal=len(hashes[s]) == 1)
  with open(args.out, 'w') as f:
    json.dump(report, f, indent=1)
  print(json.dumps(report['streams'], indent=1))


if __name__ == '__main__':
  main()
