"""Restatement of the fine-tuning option, written from its semantics and not from the code under test
(tests/test_finetune_cpu.py checks the host side against it, tests/test_finetune_gpu.py holds the device to it).

  multiplier of a variable = that of the FIRST pattern re.search finds in its name, 1 if none does; 0 = frozen
  lr of a variable         = float32(lr_t * multiplier): ONE float32 product, then the update of tests/_primitive_refs.py
  runs                     = the arena cut wherever the multiplier changes; a pad belongs to the variable in front of it; frozen
                             runs are left out
"""
import re

import numpy as np

import _primitive_refs as R

H = 136                 # the smallest frame tests/test_model_gpu.py builds; K = 3, N = 2 are its geeco-f / e2e_vmc rows at that size
K = 3
N = 2
MODELS = {'e2e_vmc': (False, {}), 'geeco-f': (True, dict(proc_obs='dynimg', proc_tgt='dyndiff'))}
_CASES = {}


def multipliers(table, names):
  """{name: multiplier} by the first-match rule (float32 values)."""
  out = {}
  for n in names:
    out[n] = 1.0
    for pat, mul in table.items():
      if re.search(pat, n):
        out[n] = float(np.float32(mul))
        break
  return out


def runs(offsets, size, mults):
  """[(offset, count, multiplier)]: element by element -- every float of the arena gets the multiplier of the last variable that
  starts at or before it, then equal neighbours are merged and the frozen stretches dropped."""
  per = np.ones(size, np.float64)
  names = sorted(offsets, key=lambda n: offsets[n])
  for i, n in enumerate(names):
    hi = offsets[names[i + 1]] if i + 1 < len(names) else size
    per[offsets[n]:hi] = mults[n]
  assert offsets[names[0]] == 0
  edges = [0] + [int(i) + 1 for i in np.flatnonzero(per[1:] != per[:-1])] + [size]
  return [(lo, hi - lo, float(per[lo])) for lo, hi in zip(edges[:-1], edges[1:]) if per[lo] != 0.0]


def cut(mults):
  """'full' / 'no_bottom' / 'decoder_only' from the per-variable multipliers."""
  enc = {n: m for n, m in mults.items() if re.search(r'Encoder/conv\d', n)}
  if all(m == 0.0 for m in enc.values()):
    return 'decoder_only'
  if all(m == 0.0 for n, m in enc.items() if re.search(r'/conv[12]/', n)):
    return 'no_bottom'
  return 'full'


def adam_ref(p, g, m, v, lr_t, mul, **kw):
  """p', m', v' (float64) and their bounds (tests/_primitive_refs.py: adam_ref / adam_bounds, the reference and tolerance of
  geeco_adam_tf) for one update of a piece at float32(lr_t * mul).  kw: b1, b2, eps, grad_scale, l2."""
  lr = float(np.float32(lr_t) * np.float32(mul))
  return R.adam_ref(p, g, m, v, lr, **kw), R.adam_bounds(p, g, m, v, lr, **kw)


def case(name):
  """(ocfg, cfg, goal, P, feats, labels): one model and batch per name, built once and left unchanged."""
  if name not in _CASES:
    from geeco_amd.params import create_e2evmc_config
    from oracle import geeco_oracle as O
    goal, extra = MODELS[name]
    ocfg = O.make_config(window_size=K, img_height=H, img_width=H, batch_size=N, lr=1e-3, **extra)
    P = O.init_params(O.model_param_shapes(ocfg, goal), seed=1)
    feats, labels = O.synthetic_batch(ocfg, goal, N, seed=3, H=H, W=H)
    _CASES[name] = (ocfg, create_e2evmc_config(ocfg._asdict()), goal, P, feats, labels)
  return _CASES[name]
