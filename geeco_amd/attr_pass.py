"""What the attribution passes share (attribution.py; perturbation.py; the consolidation: DESIGN 5.31): the
check of ``steps`` and ``seed``, the rule that turns a ``baseline=`` / ``fill=`` argument into one periodic device operand per image
input, and the bracket that keeps the clean inputs while a pass writes into the model's own input buffers.  No kernel is called here,
so all of it runs on a stub model with CPU tensors (tests/test_attr_pass_cpu.py)."""
from __future__ import annotations

import contextlib

import numpy as np
import torch


def check_steps_seed(who, steps=None, seed=None):
  """ValueError, with the reason, unless ``steps`` is an integer in 1 .. 2^20 and ``seed`` an integer >= 0 (None: not looked at)."""
  if steps is not None and (int(steps) != steps or not 1 <= int(steps) <= 1 << 20):
    raise ValueError('%s: steps=%r must be an integer >= 1' % (who, steps))
  if seed is not None and (int(seed) != seed or int(seed) < 0):
    raise ValueError('%s: seed=%r must be an integer >= 0' % (who, seed))


def periodic_operands(model, who, noun, value, keys, forms, cache, known=None):
  """{k: None (zeros) or the flat float32 device buffer the kernels repeat with its own length as the period} for the image inputs
  ``keys`` of ``model`` from ``value``, the ``noun`` ('baseline', 'fill') argument of pass ``who``.  ``value``: None; a dict by input
  name (``known``, default ``keys``: the model's image inputs as the refusal of any other name lists them; one of them that
  ``keys`` leaves out is passed over); or one array, which stands for 'rgb', and for 'target_rgb'
  where its shape is one of that input's forms too.  ``forms(k)``: the shapes input k accepts -- the whole input, a frame and,
  where the pass takes one, a colour.  ``cache`` keeps a buffer per key for the next call with an array of this size."""
  out = {k: None for k in keys}
  if value is None:
    return out
  if isinstance(value, dict):
    per_key = value
    known = list(keys if known is None else known)
    unknown = sorted(set(per_key) - set(known))
    if unknown:
      raise ValueError("%s: %s for %s, but the model's image inputs are %s" % (who, noun, ', '.join(unknown), ', '.join(known)))
  else:
    shape = tuple(np.shape(value))
    per_key = {k: value for k in keys if k == 'rgb' or (k == 'target_rgb' and shape in forms(k))}
  for k, b in per_key.items():
    if b is None or k not in out:
      continue
    b = torch.as_tensor(b, dtype=torch.float32)
    if tuple(b.shape) not in forms(k):
      named = ['%s %s' % f for f in zip(('the whole input', 'a frame', 'a colour'), forms(k))][::-1]
      raise ValueError("%s: %s for '%s' of shape %s; %s or %s" % (who, noun, k, tuple(b.shape), ', '.join(named[:-1]), named[-1]))
    if k not in cache or cache[k].numel() != b.numel():
      cache[k] = torch.empty(b.numel(), dtype=torch.float32, device=model.device)
    cache[k].copy_(b.reshape(-1), non_blocking=True)
    out[k] = cache[k]
  return out


@contextlib.contextmanager
def clean_inputs(model, keys, clean):
  """While a pass writes into ``model.inputs[k]``, k in ``keys``: their bits are saved in ``clean[k]`` on entry and copied back on
  exit, after an exception too -- the model then holds the batch ``load_batch`` left, not the step's perturbed input."""
  for k in keys:
    clean[k].copy_(model.inputs[k])
  try:
    yield
  finally:
    for k in keys:
      model.inputs[k].copy_(clean[k])
