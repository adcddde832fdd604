"""The conv kernels two eager training steps dispatch (``ops.kernel_trace``), for geeco-f, e2e_vmc and seq_constant at N = 2, K = 4,
256 x 256.  Needs a GPU.  Run from a tree's root: ``python profiles/ops_split/launches.py > launches.txt``."""
import os, sys
sys.path.insert(0, os.getcwd())
import torch
from geeco_amd import graph, ops
from geeco_amd.params import create_e2evmc_config
from oracle import geeco_oracle as O

CASES = [('geeco-f', 'GoalE2EVMC', True, dict(proc_obs='dynimg', proc_tgt='dyndiff')),
         ('seq_constant', 'GoalE2EVMC', True, dict(proc_obs='sequence', proc_tgt='constant')),
         ('e2e_vmc', 'E2EVMC', False, {})]
dev = torch.device('cuda:0')
for tag, cls, goal, kw in CASES:
  kw = dict(kw, window_size=4, img_height=256, img_width=256, batch_size=2)
  ocfg = O.make_config(**kw)
  feats, labels = O.synthetic_batch(ocfg, goal, 2, seed=11, H=256, W=256)
  model = getattr(graph, cls)(create_e2evmc_config(kw), 2, dev, training=True)
  model.store.load_numpy(O.init_params(O.model_param_shapes(ocfg, goal), seed=0))
  model.load_batch({k: torch.from_numpy(v) for k, v in feats.items()}, {k: torch.from_numpy(v) for k, v in labels.items()})
  for step in range(2):
    for what, fn in (('forward', lambda: model.forward(True)), ('backward', lambda: model.backward(adam_prepare=True)),
                     ('apply_gradients', model.apply_gradients)):
      names = ops.kernel_trace(fn)
      print('%s step %d %s: %d kernels' % (tag, step, what, len(names)))
      for n in names:
        print('  ' + n)
  torch.cuda.synchronize()
  print('%s loss %.6f' % (tag, float(model.loss)))
