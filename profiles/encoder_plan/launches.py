"""Conv-kernel launch lists (``ops.kernel_trace``) of two eager steps of geeco-f, e2e_vmc and seq_constant at N = 2, K = 4, 256x256:
``forward(True)``, ``backward(adam_prepare=True)``, ``apply_gradients()``, then one step through ``backward_and_apply``.  Needs a GPU.
Run from a tree's root (the native library built): ``python profiles/encoder_plan/launches.py > launches.txt``."""
import os, sys
sys.path.insert(0, os.getcwd())
import torch
from geeco_amd import graph, ops, runtime
from geeco_amd.params import create_e2evmc_config

CASES = [('geeco-f', 'GoalE2EVMC', dict(proc_obs='dynimg', proc_tgt='dyndiff')), ('e2e_vmc', 'E2EVMC', {}),
         ('seq_constant', 'GoalE2EVMC', dict(proc_obs='sequence', proc_tgt='constant'))]


def traced(tag, fn):
  names = ops.kernel_trace(fn)
  print('%s: %d kernels' % (tag, len(names)))
  for n in names:
    print('  ' + n)


def main():
  dev = torch.device('cuda:0')
  for tag, cls, kw in CASES:
    cfg = create_e2evmc_config(dict(kw, window_size=4, img_height=256, img_width=256, batch_size=2))
    m = getattr(graph, cls)(cfg, 2, dev, training=True)
    m.store.initialize(seed=0)
    gen = torch.Generator().manual_seed(1)
    for k, buf in m.inputs.items():
      buf.copy_(torch.rand(buf.shape, generator=gen))
    for step in range(2):
      traced('%s step %d forward' % (tag, step), lambda: m.forward(True))
      traced('%s step %d backward + apply_gradients' % (tag, step), lambda: (m.backward(adam_prepare=True), m.apply_gradients()))
    early, late = runtime.gradient_buckets(m.store)
    traced('%s forward' % tag, lambda: m.forward(True))
    traced('%s backward_and_apply' % tag, lambda: m.backward_and_apply(early, late))
    torch.cuda.synchronize()
    m.check_device_errors()
    print('%s loss %.6f' % (tag, float(m.loss)))


if __name__ == '__main__':
  main()
