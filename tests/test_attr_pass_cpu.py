"""What the attribution passes share (geeco_amd/attr_pass.py, ``decoder.resolve_heads``) without a GPU: the operand
rule on a stub model with CPU tensors -- every accepted form for both nouns, every refusal with its exact words, the buffer cache --
the clean-input bracket with an exception inside it, the head names on a literal table, and the shared ``steps`` / ``seed`` check."""
import types

import numpy as np
import pytest
import torch

N, K, H, W = 2, 3, 5, 7
RGB, TGT, DEPTH = (N, K, H, W, 3), (N, H, W, 3), (N, K, H, W, 1)
BASELINE = lambda model: (lambda k: (tuple(model.inputs[k].shape), tuple(model.inputs[k].shape[-3:])))
FILL = lambda model: (lambda k: BASELINE(model)(k) + (tuple(model.inputs[k].shape[-1:]),))


def _stub(goal=True, depth=False):
  shapes = dict(rgb=RGB, **(dict(target_rgb=TGT) if goal else {}), **(dict(depth=DEPTH) if depth else {}))
  return types.SimpleNamespace(device=torch.device('cpu'), inputs={k: torch.zeros(s) for k, s in shapes.items()})


def _flat(a):
  return np.asarray(a, np.float32).reshape(-1)


def _check(out, want):
  assert sorted(out) == sorted(want)
  for k, v in want.items():
    if v is None:
      assert out[k] is None, k
    else:
      assert out[k].dtype == torch.float32 and out[k].dim() == 1 and np.array_equal(out[k].numpy(), _flat(v)), k


@pytest.mark.parametrize('noun', ['baseline', 'fill'])
def test_periodic_operands_forms(noun):
  from geeco_amd.attr_pass import periodic_operands
  r = np.random.default_rng(71)
  model = _stub(depth=True)
  keys = ['rgb', 'target_rgb', 'depth']
  forms = (BASELINE if noun == 'baseline' else FILL)(model)
  run = lambda value, keys=keys: periodic_operands(model, 'who', noun, value, keys, forms, {})
  none = {k: None for k in keys}
  full, frame, tfull, dframe = (r.random(s, dtype=np.float32) for s in (RGB, RGB[-3:], TGT, DEPTH[-3:]))
  _check(run(None), none)
  _check(run(frame), dict(none, rgb=frame, target_rgb=frame))      # a frame fits both rgb inputs
  _check(run(full), dict(none, rgb=full))                          # shaped like rgb: rgb alone, the target stays black
  _check(run(frame, ['rgb']), dict(rgb=frame))
  _check(run({'target_rgb': tfull, 'depth': dframe, 'rgb': None}), dict(none, target_rgb=tfull, depth=dframe))
  _check(run({'target_rgb': torch.from_numpy(tfull)}), dict(none, target_rgb=tfull))      # tensors are taken too
  _check(periodic_operands(model, 'who', noun, {'depth': dframe}, ['rgb', 'target_rgb'], forms, {}, known=keys),
         dict(rgb=None, target_rgb=None))      # an input of a pass that is not run
  if noun == 'fill':
    colour, grey = r.random(3, dtype=np.float32), r.random(1, dtype=np.float32)
    _check(run(colour), dict(none, rgb=colour, target_rgb=colour))
    _check(run({'depth': grey, 'rgb': colour}), dict(none, rgb=colour, depth=grey))
  else:
    with pytest.raises(ValueError, match="^who: baseline for 'rgb' of shape \\(3,\\); a frame \\(5, 7, 3\\) or the whole input \\(2, 3, 5, 7, 3\\)$"):
      run(np.zeros(3, np.float32))


def test_periodic_operands_refusals():
  from geeco_amd.attr_pass import periodic_operands
  model = _stub(depth=True)
  keys = ['rgb', 'target_rgb', 'depth']
  bad = np.zeros((3, 3, 3), np.float32)
  cases = [('attributions', 'baseline', BASELINE, bad, keys,
            "attributions: baseline for 'rgb' of shape (3, 3, 3); a frame (5, 7, 3) or the whole input (2, 3, 5, 7, 3)"),
           ('perturbation_attributions', 'fill', FILL, bad, keys,
            "perturbation_attributions: fill for 'rgb' of shape (3, 3, 3); a colour (3,), a frame (5, 7, 3) or the whole input (2, 3, 5, 7, 3)"),
           ('perturbation_attributions', 'fill', FILL, {'depth': np.zeros(3, np.float32)}, keys,
            "perturbation_attributions: fill for 'depth' of shape (3,); a colour (1,), a frame (5, 7, 1) or the whole input (2, 3, 5, 7, 1)"),
           ('attributions', 'baseline', BASELINE, {'target_rgb': np.zeros(RGB, np.float32)}, keys,
            "attributions: baseline for 'target_rgb' of shape (2, 3, 5, 7, 3); a frame (5, 7, 3) or the whole input (2, 5, 7, 3)"),
           ('attributions', 'baseline', BASELINE, {'nope': bad, 'also': bad, 'rgb': None}, keys,
            "attributions: baseline for also, nope, but the model's image inputs are rgb, target_rgb, depth"),
           ('perturbation_attributions', 'fill', FILL, {'nope': bad}, ['target_rgb'],
            "perturbation_attributions: fill for nope, but the model's image inputs are rgb, depth, target_rgb")]
  for who, noun, forms, value, ks, words in cases:
    with pytest.raises(ValueError) as e:      # the listing: ``known``, in the caller's order (perturbation.PASSES'), else ``keys``
      periodic_operands(model, who, noun, value, ks, forms(model), {}, known=['rgb', 'depth', 'target_rgb'] if noun == 'fill' else None)
    assert str(e.value) == words


def test_periodic_operands_cache():
  """One buffer per key, reused for an array of the same size (whatever its form) and replaced for another size."""
  from geeco_amd.attr_pass import periodic_operands
  model, cache = _stub(), {}
  run = lambda value: periodic_operands(model, 'who', 'fill', value, ['rgb', 'target_rgb'], FILL(model), cache)
  a = run(np.full((H, W, 3), 1.0, np.float32))
  first = dict(a)
  b = run(np.full((H, W, 3), 2.0, np.float32))
  assert b['rgb'] is first['rgb'] and b['target_rgb'] is first['target_rgb'] and sorted(cache) == ['rgb', 'target_rgb']
  assert bool((b['rgb'] == 2.0).all()) and b['rgb'].numel() == H * W * 3
  c = run(np.full(3, 3.0, np.float32))
  assert c['rgb'] is not first['rgb'] and c['rgb'] is cache['rgb'] and c['rgb'].numel() == 3 and bool((c['rgb'] == 3.0).all())
  d = run({'rgb': np.full(3, 4.0, np.float32)})
  assert d['rgb'] is c['rgb'] and d['target_rgb'] is None and cache['target_rgb'] is c['target_rgb']      # (kept for a later call)
  assert run(None) == dict(rgb=None, target_rgb=None)


def test_clean_inputs_restores_after_an_exception():
  from geeco_amd.attr_pass import clean_inputs
  model = _stub()
  r = np.random.default_rng(72)
  loaded = {k: torch.from_numpy(r.random(tuple(v.shape), dtype=np.float32)) for k, v in model.inputs.items()}
  for k, v in loaded.items():
    model.inputs[k].copy_(v)
  buffers = {k: model.inputs[k] for k in model.inputs}
  clean = {k: torch.full_like(v, float('nan')) for k, v in model.inputs.items()}
  with clean_inputs(model, ['rgb'], clean):
    assert torch.equal(clean['rgb'], loaded['rgb']) and bool(torch.isnan(clean['target_rgb']).all())
    model.inputs['rgb'].fill_(7.0)
  assert torch.equal(model.inputs['rgb'], loaded['rgb'])
  with pytest.raises(ValueError, match='step 3'):
    with clean_inputs(model, ['rgb', 'target_rgb'], clean):
      model.inputs['rgb'].fill_(7.0)
      model.inputs['target_rgb'].fill_(8.0)
      raise ValueError('step 3')
  for k, v in loaded.items():      # the same buffers, the loaded bits
    assert model.inputs[k] is buffers[k] and torch.equal(model.inputs[k].view(torch.int32), v.view(torch.int32)), k


HEADS = [('fc_cmd_ee', 'cmd_ee', 3, 0, 1.0), ('fc_cmd_grp', 'logits_cmd_grp', 3, 1, 1.0), ('fc_pos_ee', 'pos_ee', 3, 0, 0.5)]


def test_resolve_heads():
  from geeco_amd.decoder import resolve_heads
  everything = {'cmd_ee', 'logits_cmd_grp', 'pos_ee'}
  assert resolve_heads(HEADS, None) == everything
  assert resolve_heads(HEADS, ('cmd_ee', 'cmd_grp')) == {'cmd_ee', 'logits_cmd_grp'}      # the short name
  assert resolve_heads(HEADS, ['logits_cmd_grp']) == {'logits_cmd_grp'}                   # and the long one
  assert resolve_heads(HEADS, 'pos_ee') == {'pos_ee'}                                     # a string is one name, not its letters
  assert resolve_heads(HEADS, ('cmd_ee', 'cmd_ee')) == {'cmd_ee'}
  for bad in ((), [], ('nope',), ('cmd_ee', 'nope'), 'cmd'):
    with pytest.raises(ValueError) as e:
      resolve_heads(HEADS, bad)
    assert str(e.value) == 'heads=%r: this model has the heads cmd_ee, cmd_grp, pos_ee' % (bad,)


def test_check_steps_seed():
  from geeco_amd.attr_pass import check_steps_seed
  from geeco_amd.attribution import check_attribution_arguments
  from geeco_amd.perturbation import check_perturbation_arguments
  for ok in (dict(steps=1, seed=0), dict(steps=1 << 20), dict(seed=1 << 40), dict(steps=np.int64(5), seed=np.int32(2)), dict(steps=4.0), dict()):
    check_steps_seed('who', **ok)
  for steps in (0, -1, 2.5, (1 << 20) + 1):
    with pytest.raises(ValueError) as e:
      check_steps_seed('who', steps=steps, seed=0)
    assert str(e.value) == 'who: steps=%r must be an integer >= 1' % (steps,)
  for seed in (-1, 0.5):
    with pytest.raises(ValueError) as e:
      check_steps_seed('who', steps=3, seed=seed)
    assert str(e.value) == 'who: seed=%r must be an integer >= 0' % (seed,)
  with pytest.raises(ValueError, match='steps=0'):      # steps is looked at first
    check_steps_seed('who', steps=0, seed=-1)
  # both passes' checks speak through it, under their own names
  with pytest.raises(ValueError, match='^attributions: steps=0 must be an integer >= 1$'):
    check_attribution_arguments('smoothgrad', 0, 0.0, 0)
  with pytest.raises(ValueError, match='^attributions: seed=-3 must be an integer >= 0$'):
    check_attribution_arguments('smoothgrad', 2, 0.0, -3)
  with pytest.raises(ValueError, match='^perturbation_attributions: steps=0 must be an integer >= 1$'):
    check_perturbation_arguments('rise', steps=0)
  with pytest.raises(ValueError, match='^perturbation_attributions: seed=-3 must be an integer >= 0$'):
    check_perturbation_arguments('occlusion', seed=-3)
  check_perturbation_arguments('occlusion', steps=0)      # the grid decides: ``steps`` is not read
