"""tests/_input_stage_refs.py on the CPU: the properties its input recipes claim (sign, where the extrema sit, the range floor, the
bound under its cap), its float64 reference against oracle.geeco_oracle.dynimg, the agreement of the expected-instance table
with the trace notes and instantiations of csrc/dynimg.hip and csrc/dynimg_goal.hip, a float32 emulation of the stage that
passes in two summation orders, and thirteen emulated wrong kernels that are each rejected by at least one case."""
import os
import re

import numpy as np
import pytest
import torch

import _input_stage_refs as R
from oracle import geeco_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the instantiations the two files launch, read off their dispatch code: 6 + 2 + 4 = 12
INSTANCES = [
    'dynimg_goal_onepass_kernel<false, false, 256, 1>', 'dynimg_goal_onepass_kernel<true, false, 256, 1>',
    'dynimg_goal_onepass_kernel<false, true, 256, 1>', 'dynimg_goal_onepass_kernel<true, true, 256, 1>',
    'dynimg_goal_onepass_kernel<false, true, 1024, 2>', 'dynimg_goal_onepass_kernel<true, true, 1024, 2>',
    'dynimg_goal_onepass2_kernel<false, false, 1024>', 'dynimg_goal_onepass2_kernel<true, false, 1024>',
    'dynimg_wsum3_kernel<false>', 'dynimg_wsum3_kernel<true>', 'dynimg_wsum_generic_kernel', 'dynimg_norm_kernel',
]

SMALL_FIRST = sorted(R.CASES, key=lambda c: c['N'] * c['K'] * c['HW'])


def _ids(cases):
  return [c['id'] for c in cases]


def test_alpha_is_the_oracles():
  for K in (1, 2, 3, 14):
    np.testing.assert_array_equal(R.alpha(K), O.dynimg_alpha(K))
  assert R.alpha(1)[0] == 0.0 and R.alpha(2).tolist() == [-0.5, 0.5]


@pytest.mark.parametrize('c', R.CASES, ids=_ids(R.CASES))
def test_case(c):
  """Per case: the recipe's properties; the reference against the oracle in float64; the right emulation passes, fused and
  unfused."""
  inp, ref = R.inputs(c['id']), R.reference(c['id'])
  R.check_recipe(c, inp, ref)
  N, K, HW, C = c['N'], c['K'], c['HW'], c['C']
  assert inp.x.dtype == np.float32 and inp.x.shape == (N, K, HW, C) and inp.tgt.shape == (N, HW, C)
  if inp.bytes is not None:
    np.testing.assert_array_equal(inp.x[..., :3], inp.bytes.astype(np.float32) / np.float32(255.0))
  sub = slice(0, min(N, 3))
  x64 = torch.from_numpy(inp.x[sub].astype(np.float64)).reshape(-1, K, HW, 1, C)
  np.testing.assert_allclose(ref.img[0][sub], O.dynimg(x64).numpy().reshape(-1, HW, C), rtol=0, atol=1e-12)
  pair = torch.from_numpy(np.stack([inp.x[sub, K - 1], inp.tgt[sub]], 1).astype(np.float64)).reshape(-1, 2, HW, 1, C)
  np.testing.assert_allclose(ref.img[1][sub], O.dynimg(pair).numpy().reshape(-1, HW, C), rtol=0, atol=1e-12)
  for fused in (True, False):
    cur, imgs = R.emulate(c, inp, fused=fused)
    assert R.accepts(c, ref, cur, imgs), (c['id'], fused)


def test_dispatch_restated():
  """The thresholds of goal_onepass_dispatch as the case table restates them, at their edges."""
  g = lambda entry, N, HW, C=3: R.geometry(dict(entry=entry, N=N, HW=HW, C=C))
  assert g('goal', 191, 64)['names'] == ['dynimg_goal_onepass_kernel<false, false, 256, 1>']
  assert g('goal', 192, 4)['names'] == ['dynimg_goal_onepass2_kernel<false, false, 1024>']
  assert g('goal', 96, 8192)['T'] == 256 and g('goal', 96, 8196)['T'] == 1024          # U = 2048 / 2049: one / two big blocks
  assert g('goal_u8', 3, 524304, 4) == dict(names=['dynimg_goal_onepass_kernel<true, true, 1024, 2>'], T=1024, UPT=2, bps=65,
                                             layout='unit', UNR=2, half=None)
  assert g('goal_u8', 2, 524304)['T'] == 256
  assert g('goal', 6, 262160)['bps'] == 65 and g('goal', 6, 262160)['half'] == 3 and g('goal', 193, 5184)['half'] == 97
  assert g('goal', 1, 65540)['bps'] == 65 and g('goal', 1, 65540)['T'] == 256
  src = open(os.path.join(ROOT, 'geeco_amd/csrc/dynimg_goal.hip')).read()
  assert 'cdiv64(U, 2048)' in src and '(long long)p.N * bps_big >= 192' in src and 'bps2 = (int)cdiv64(U, 1024)' in src
  assert 'cdiv64(U, 256)' in src and 'constexpr int UNR = DEPTH ? 2 : 3;' in src and 'constexpr int UNR = DEPTH ? 3 : 4;' in src


def test_notes_instances_and_cases_agree():
  notes = []
  for rel, launches in (('geeco_amd/csrc/dynimg.hip', 5), ('geeco_amd/csrc/dynimg_goal.hip', 3)):
    src = open(os.path.join(ROOT, rel)).read()
    found = re.findall(r'geeco_note_kernel\("([^"]+)"', src)
    assert len(re.findall(r'hipLaunchKernelGGL\(', src)) == len(found) == launches, rel
    # every note sits on the line in front of its launch and names the kernel launched there
    pairs = re.findall(r'geeco_note_kernel\("([a-z0-9_]+)[^\n]*\n\s*hipLaunchKernelGGL\(\(?([a-z0-9_]+)', src)
    assert len(pairs) == launches and all(a == b for a, b in pairs), rel
    notes += found
  goal = open(os.path.join(ROOT, 'geeco_amd/csrc/dynimg_goal.hip')).read()
  assert 'if constexpr (!U8) {' in goal                      # the two-sample form exists for float32 windows only
  spelled = set()
  for n in notes:
    if '%s' in n:
      for d in ('true', 'false'):
        for u in (('false',) if 'onepass2' in n else ('true',) if '1024, 2' in n else ('true', 'false')):
          spelled.add(n.replace('%s', d, 1).replace('%s', u, 1))
    else:
      spelled.add(n)
  assert len(INSTANCES) == len(set(INSTANCES)) == 12
  assert spelled == set(INSTANCES)
  assert R.expected_instances() == set(INSTANCES)
  for name in INSTANCES:
    assert any(name in R.geometry(c)['names'] for c in R.CASES), name


def _instance(c):
  return R.geometry(c)['names'][0]


def test_every_instance_gets_every_named_place():
  """Per instantiation, over its cases: min AND max were each planted at unit 0, the last unit, the last float4, lanes 0 and 63 of
  waves 1..3 (15 in 1024-thread blocks), in R, G, B and the depth; with several blocks, min in the first block and max in the
  last and the other way round; block 64 or later; slot 1; both recipes of one sign; every sample of an odd count."""
  seen = {}
  for c in R.CASES:
    g = R.geometry(c)
    _, _, plants = R._levels(c) if False else (None, None, R.inputs(c['id']).plants)
    s = seen.setdefault(_instance(c), dict(min=set(), max=set(), cross=set(), recipes=set(), odd=False, strided=False))
    s['recipes'].add(c['recipe'])
    s['strided'] |= c['strided'] is not None
    s['odd'] |= g['half'] is not None and c['N'] % 2 == 1
    for (n, img, ext), (p, ch) in plants.items():
      if img == 1 and c['entry'] in ('dynimg', 'rgbd'):
        continue
      if img == 0 and c['K'] == 1:
        continue
      t = R.tags_of(c, p, ch)
      s[ext] |= t | {w + '-' + l for w in t if w.startswith('wave') for l in t if l.startswith('lane')}
    for n in range(c['N']):
      for img in (0, 1):
        a, b = (R.tags_of(c, *plants[(n, img, e)]) for e in ('min', 'max'))
        if 'block0' in a and 'last-block' in b:
          s['cross'].add('min-first-max-last')
        if 'last-block' in a and 'block0' in b:
          s['cross'].add('max-first-min-last')
  for name, s in seen.items():
    goal = 'goal' in name
    big = '1024' in name
    want = {'unit0', 'last-unit', 'last-f4', 'R', 'G', 'B'}
    want |= {'wave%d-lane%d' % (w, l) for w in (1, 2, 3) for l in (0, 63)}
    if big:
      want |= {'wave15-lane0', 'wave15-lane63'}
    if name not in ('dynimg_wsum_generic_kernel', 'dynimg_wsum3_kernel<false>') and '<false, ' not in name:
      want.add('depth')
    if name != 'dynimg_norm_kernel':
      want |= {'block0', 'last-block', 'block64+'}
      assert s['cross'] == {'min-first-max-last', 'max-first-min-last'}, (name, s['cross'])
    if '1024, 2' in name:
      want.add('slot1')
    for ext in ('min', 'max'):
      assert want <= s[ext], (name, ext, sorted(want - s[ext]))
    assert {'pos', 'neg', 'planted-rgb'} <= s['recipes'], name
    if 'true' in name.split(',')[0] or name == 'dynimg_wsum3_kernel<true>':
      assert {'planted-depth', 'planted-mix'} <= s['recipes'], name
    if 'onepass2' in name:
      assert s['odd'], name
    if ', true, ' not in name:                                # float32 frames: strided views
      assert s['strided'], name


def test_shapes_reach_the_paths():
  ids = set(R.CASE_BY_ID)
  shapes = {(c['entry'], c['C'], c['N'], c['HW']) for c in R.CASES}
  for entry in ('goal', 'goal_u8'):
    for C in (3, 4):
      unr = 2 if C == 4 else 3
      ks = {c['K'] - 1 for c in R.CASES if c['entry'] == entry and c['C'] == C and R.geometry(c)['T'] == 256}
      assert {0, 1, unr - 1, unr, unr + 1, 2 * unr + 1} <= ks, (entry, C, ks)
      for HW in (4, 64, 1024, 1028, 1440):
        assert any(s[0] == entry and s[1] == C and s[3] == HW for s in shapes), (entry, C, HW)
      assert (entry, C, 1, 65540) in shapes
      unr = unr if entry == 'goal_u8' else unr + 1
      ks = {c['K'] - 1 for c in R.CASES if c['entry'] == entry and c['C'] == C and R.geometry(c)['T'] == 1024}
      assert {0, 1, unr - 1, unr, unr + 1, 2 * unr + 1} <= ks, (entry, C, ks)
      if entry == 'goal':
        assert {3 * unr, 3 * unr + 1} <= ks                    # groups = 3: mid() at g = 1 inside the steady loop
        assert {(entry, C, 192, 5184), (entry, C, 193, 5184), (entry, C, 192, 4096), (entry, C, 6, 262160)} <= shapes
      else:
        assert {(entry, C, 192, 5184), (entry, C, 192, 4000), (entry, C, 192, 8192), (entry, C, 3, 524304)} <= shapes
  gen = {(c['Cin'], c['Cpad'], c['HW'] % 2) for c in R.CASES if 'generic' in _instance(c)}
  assert {(4, 4, 1), (1, 1, 1), (3, 3, 0), (3, 4, 1), (5, 8, 1), (8, 8, 0)} <= gen
  assert any('generic' in _instance(c) and c['HW'] * c['Cpad'] % 4 and c['N'] == 2 for c in R.CASES)      # the norm kernel's scalar path
  assert any(R.geometry(c)['bps'] > 256 for c in R.DYNIMG_CASES)
  for name in ('dynimg_wsum3_kernel<false>', 'dynimg_wsum3_kernel<true>', 'dynimg_wsum_generic_kernel'):
    assert any(c['two_frame'] and _instance(c) == name for c in R.CASES), name
  assert len(ids) == len(R.CASES)
  # the largest case stays near 100 MB of device memory: three outputs and the float32 window
  worst = max(4 * c['N'] * c['HW'] * (3 * 4 + c['K'] * c['C'] + c['C']) for c in R.CASES)
  assert worst < 160e6, worst


@pytest.mark.parametrize('mut', R.MUTATIONS)
def test_wrong_kernel_is_rejected(mut):
  """Each emulated wrong kernel fails the GPU test's own acceptance on at least one case (smallest cases first)."""
  touched = 0
  for c in SMALL_FIRST:
    inp = R.inputs(c['id'])
    got = R.emulate(c, inp, mut=mut)
    if got is None:
      continue
    touched += 1
    if not R.accepts(c, R.reference(c['id']), *got):
      return
  raise AssertionError('%s: accepted by all %d cases it touches' % (mut, touched))


def test_each_mutation_is_rejected_in_every_form_it_touches():
  """Stronger, for the mutations of the min / max: every instantiation the mutation applies to has a rejecting case."""
  per = {}
  for c in SMALL_FIRST:
    if c['N'] * c['K'] * c['HW'] > 3e6:
      continue
    inp = R.inputs(c['id'])
    for mut in ('fold-from-0', 'pad-joins', 'depth-only', 'rgb-only', 'live-for-flive', 'last-slot-dropped', 'slot1-dropped'):
      key = (mut, _instance(c))
      if per.get(key):
        continue
      got = R.emulate(c, inp, mut=mut)
      if got is not None:
        per[key] = not R.accepts(c, R.reference(c['id']), *got)
  assert per and all(per.values()), sorted(k for k, v in per.items() if not v)
