#!/usr/bin/env python
"""Records tests/golden/augmented_gather.npz: inputs and outputs of ops.gather_windows_augmented_into for the cases of
tests/test_augment_gpu.py::test_augmented_gather_reproduces_the_recorded_values, from the library that is loaded (a build of the
commit whose values are to be pinned; GEECO_DEV=1 GEECO_LIB=NAME picks another build).  Needs a GPU.

Per case i of GOLDEN_CASES: episode<i> [5][H * W * C] (uint8, or float32 multiples of 1 / 1024), colour<i> float32 [3][2 * C]
(gain[C], bias[C]) and out<i> float32 [offsets][shift launches][colour, None][3][3][H][W][C]."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import test_augment_gpu as T  # noqa: E402


def main():
  dev = torch.device('cuda:0')
  arrays = {}
  for i, (H, W, C, dtype) in enumerate(T.GOLDEN_CASES):
    r = np.random.default_rng(100 + i)
    episode = r.integers(0, 256, [5, H * W * C]).astype(np.uint8) if dtype == 'uint8' else \
        (r.integers(0, 1024, [5, H * W * C]) / 1024.0).astype(np.float32)
    colour = np.concatenate([r.uniform(0.5, 1.5, (3, C)), r.uniform(-0.3, 0.3, (3, C))], axis=1).astype(np.float32)
    out = np.stack([np.stack([np.stack([T.golden_gather(dev, episode, offset, H, W, C, shift, col) for col in (colour, None)])
                              for shift in T.golden_shifts(H, W)]) for offset in T.golden_offsets(dtype)])
    assert not np.isnan(out).any()
    arrays.update({'episode%d' % i: episode, 'colour%d' % i: colour, 'out%d' % i: out})
  np.savez_compressed(sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN, **arrays)


if __name__ == '__main__':
  main()
