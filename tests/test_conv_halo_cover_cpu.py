"""The case list of the LDS-halo / LDS-staged device tests (tests/native/conv_halo_cases.txt) runs every launch variant the models
reach and every instantiation the forward and input-gradient dispatchers can choose."""
import os
import subprocess

import pytest

import _conv_refs as R

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def cover(tmp_path_factory):
  """tests/native/conv_halo_cover.cpp evaluates geeco_amd/csrc/conv_halo_plan.h on the host: built with
  -fsanitize=address,undefined as a program of its own."""
  exe = str(tmp_path_factory.mktemp('cover') / 'conv_halo_cover')
  subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                  '-I' + os.path.join(HERE, '..', 'geeco_amd', 'csrc'), os.path.join(HERE, 'native', 'conv_halo_cover.cpp'),
                  '-o', exe], check=True, timeout=300)
  res = subprocess.run([exe, R.HALO_CASES_TXT], capture_output=True, text=True, timeout=120)
  assert res.returncode == 0, res.stdout[-2000:] + res.stderr
  lines = res.stdout.splitlines()
  cases = [l[len('case '):] for l in lines if l.startswith('case ')]
  sweep = [l[len('sweep '):] for l in lines if l.startswith('sweep ')]
  insts = [l[len('inst '):] for l in lines if l.startswith('inst ')]
  assert len(cases) + len(sweep) + len(insts) == len(lines)
  return cases, sweep, insts


def test_every_case_runs_the_variant_recorded_beside_it(cover):
  """A change of a plan that moves a case to another instantiation (or changes its item or block count, its rounds, the boundaries
  its blocks cross or its empty blocks) shows here, as a diff, and not as a device test that silently checks something else."""
  cases, _, _ = cover
  want = [l.strip() for l in open(R.HALO_CASES_TXT) if l.strip() and not l.startswith('#')]
  assert len(want) == len(cases) >= 45
  bad = [(g, w) for g, w in zip(cases, want) if g != w]
  assert not bad, '%d cases differ, the first:\n got  %s\n want %s' % (len(bad), *bad[0])


def test_every_variant_of_the_sweep_has_a_case(cover):
  """The sweep: the eight encoder layers at inputs 136 / 144 / 256 with 1..3 encoders and 1..512 frames, forward and input
  gradient, in every mask form the layer's entry points take.  Each of its keys (family, instantiation, one round or several, mask
  form) is the key of a case."""
  _, sweep, _ = cover
  have = {R.halo_key(c) for c in R.load_halo_cases(device_only=True)}
  assert len(sweep) >= 40, sweep
  missing = [k for k in sweep if k not in have]
  assert not missing, 'no case of conv_halo_cases.txt runs:\n  ' + '\n  '.join(missing)


def test_every_instantiation_has_a_case(cover):
  """Three LDS-staged gradients, three LDS-halo gradients, two stride-2 forwards and conv1's two: compiled and dispatched for any
  caller, so each is launched by a case under its exact name."""
  _, _, insts = cover
  assert len(insts) == len(set(insts)) == 10, insts
  ran = {c.inst for c in R.load_halo_cases(device_only=True)}
  missing = [i for i in insts if i not in ran]
  assert not missing, 'no case of conv_halo_cases.txt launches:\n  ' + '\n  '.join(missing)
  assert ran <= set(insts), sorted(ran - set(insts))


def test_the_cases_hold_the_edges(cover):
  """The edges the list is meant to hold, stated on the recorded plans (the cover holds those against the plan header)."""
  cs = R.load_halo_cases()
  dev = [c for c in cs if 'hostonly' not in c.flags]
  sel = lambda fam, d: [c for c in dev if c.family == fam and c.dir == d]
  # LDS-staged gradient: per instantiation and mask form one single round at G = 1 and a block that takes a second item across a
  # ci-block and an encoder boundary; the caps 256 / 512 / 768; two chunks (the minimum) and sixteen (the longest sum)
  lds = sel('lds', 'dgrad')
  caps = {'conv_s2_dgrad_lds_kernel<1, 16, 1, 4, 8>': 256, 'conv_s2_dgrad_lds_kernel<1, 16, 1, 2, 8>': 512,
          'conv_s2_dgrad_lds_kernel<2, 8, 1, 2, 4>': 768}
  assert {c.inst for c in lds} == set(caps)
  for inst, cap in caps.items():
    for form in ('none', 'mask', 'fields'):
      mine = [c for c in lds if c.inst == inst and R.halo_form(c) == form]
      assert any(c.G == 1 and c.rounds == 1 and c.blocks == c.items < cap for c in mine), (inst, form)
      assert any(c.G == 3 and c.rounds == 2 and c.blocks == cap and c.items % cap and {'cib', 'enc'} <= c.cross for c in mine), (inst, form)
  assert any(c.Cout == 32 for c in lds) and any(c.Cout == 256 for c in lds)
  assert any(c.H == 32 and c.W == 64 for c in lds)      # 2 x 2 tiles per frame: the interior -1 halo row and column
  assert any(c.H == 16 and c.W == 32 for c in lds)      # Ho = 8, Wo = 16: the smallest served wide shape
  declined = [c for c in cs if c.family == 'gemm']
  assert len(declined) == 1 and (declined[0].H // 2) % 8 != 0 and declined[0].dir == 'dgrad'
  # LDS-halo gradient: exact tiles and ragged tiles whose ranges cross frames and encoders with empty blocks; conv3 with fields at
  # both shapes and with reserved CUs (fewer blocks, longer ranges)
  for Cin, forms in ((32, ('none', 'mask')), (48, ('none', 'mask', 'fields'))):
    mine = [c for c in sel('halo', 'dgrad') if c.Cin == Cin]
    for form in forms:
      assert any(c.H % 8 == 0 and c.W % 64 == 0 and c.rounds == 1 for c in mine if R.halo_form(c) == form), (Cin, form)
      assert any(c.H % 8 and c.W % 64 and c.rounds > 1 and c.blocks == 256 and c.empty and {'frame', 'enc'} <= c.cross
                 for c in mine if R.halo_form(c) == form), (Cin, form)
  res = [c for c in dev if c.reserved]
  assert len(res) == 1 and res[0].blocks == 256 - res[0].reserved and res[0].rounds > 3 and 'fields' in res[0].flags
  # LDS-halo forward: exact tiles; tiles ragged both ways, one per block; more tiles than blocks, across frames and encoders
  for Cin in (32, 48):
    for form in ('plain', 'fields'):
      mine = [c for c in sel('halo', 'fwd') if c.Cin == Cin and R.halo_form(c) == form]
      assert any((c.H // 2) % 4 == 0 and (c.W // 2) % 16 == 0 for c in mine), (Cin, form)
      assert any((c.H // 2) % 4 and (c.W // 2) % 16 and c.rounds == 1 and c.G == 3 and c.blocks == c.items > 128 for c in mine), (Cin, form)
      assert any(c.items > 256 == c.blocks and c.rounds == 2 and c.empty and {'frame', 'enc'} <= c.cross for c in mine), (Cin, form)
  # conv1: exact and ragged tiles, more tiles than 768 blocks per encoder at G = 3, every form, one case without ReLU
  c1 = sel('conv1', 'fwd')
  for form, rgb in (('plain', False), ('bits', False), ('bits', True)):
    mine = [c for c in c1 if R.halo_form(c) == form and ('rgb' in c.flags) == rgb]
    assert any(c.H % 8 == 0 and c.W % 32 == 0 and c.rounds == 1 for c in mine), (form, rgb)
    assert any(c.H % 8 and c.W % 32 and c.G == 3 and c.blocks == 3 * 768 and c.rounds == 2 for c in mine), (form, rgb)
  assert sum('relu' not in c.flags for c in c1) == 1 and all('relu' in c.flags for c in dev if c.dir == 'fwd' and c.family != 'conv1')
  # the exact pass: every sum is an integer far below 2**24; the reference stays small
  for c in dev:
    assert (16 * c.Cout + 3 if c.dir == 'dgrad' else 36 * c.Cin + 3) <= 4099 < 2 ** 24, c.text
    Ho, Wo = R.halo_out_hw(c)
    out = c.G * c.N * (c.H * c.W * c.Cin if c.dir == 'dgrad' else Ho * Wo * c.Cout)
    assert out <= 13e6, (c.text, out)
