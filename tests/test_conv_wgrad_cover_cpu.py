"""The case list of the filter gradient's device tests (tests/native/conv_wgrad_cases.txt) runs every launch variant the models
reach and every instantiation the dispatcher can choose."""
import os
import subprocess

import pytest

import _conv_refs as R

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def cover(tmp_path_factory):
  """tests/native/conv_wgrad_cover.cpp evaluates geeco_amd/csrc/conv_wgrad_plan.h on the host: built with
  -fsanitize=address,undefined as a program of its own."""
  exe = str(tmp_path_factory.mktemp('cover') / 'conv_wgrad_cover')
  subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                  '-I' + os.path.join(HERE, '..', 'geeco_amd', 'csrc'), os.path.join(HERE, 'native', 'conv_wgrad_cover.cpp'),
                  '-o', exe], check=True, timeout=300)
  res = subprocess.run([exe, R.WGRAD_CASES_TXT], capture_output=True, text=True, timeout=120)
  assert res.returncode == 0, res.stdout[-2000:] + res.stderr
  lines = res.stdout.splitlines()
  cases = [l[len('case '):] for l in lines if l.startswith('case ')]
  sweep = [l[len('sweep '):] for l in lines if l.startswith('sweep ')]
  insts = [l[len('inst '):] for l in lines if l.startswith('inst ')]
  assert len(cases) + len(sweep) + len(insts) == len(lines)
  return cases, sweep, insts


def test_every_case_runs_the_variant_recorded_beside_it(cover):
  """A change of a plan that moves a case to another variant (or changes its slab count, its slab-sum kernel or the length of its
  longest slice) shows here, as a diff, and not as a device test that silently checks something else."""
  cases, _, _ = cover
  want = [l.strip() for l in open(R.WGRAD_CASES_TXT) if l.strip() and not l.startswith('#')]
  assert len(want) == len(cases) >= 35
  bad = [(g, w) for g, w in zip(cases, want) if g != w]
  assert not bad, '%d cases differ, the first:\n got  %s\n want %s' % (len(bad), *bad[0])


def test_every_variant_of_the_sweep_has_a_case(cover):
  """The sweep: the eight encoder layers at inputs 136 / 144 / 256 with 1..3 encoders and 1..512 frames, every layer taken as
  each family that can serve it.  Each of its keys (family, instantiation, slab-sum form, S == 1 or S > 1, regular or
  remainder-block form) is the key of a case."""
  _, sweep, _ = cover
  have = {R.wgrad_key(c) for c in R.load_wgrad_cases()}
  assert len(sweep) >= 12, sweep
  missing = [k for k in sweep if k not in have]
  assert not missing, 'no case of conv_wgrad_cases.txt runs:\n  ' + '\n  '.join(missing)


def test_every_instantiation_has_a_case(cover):
  """Six LDS variants, four generic tiles, conv1's kernel, the halo kernel and both slab-sum kernels: compiled and dispatched for
  any caller, so each is launched by a case, whether a model reaches it or not."""
  _, _, insts = cover
  assert len(insts) == len(set(insts)) == 14, insts
  ran = set()
  for c in R.load_wgrad_cases():
    ran.update(R.wgrad_kernel_names(c))
  missing = [i for i in insts if i not in ran]
  assert not missing, 'no case of conv_wgrad_cases.txt launches:\n  ' + '\n  '.join(missing)
  assert ran <= set(insts), sorted(ran - set(insts))


def test_the_cases_hold_the_edges(cover):
  """The edges the list is meant to hold, stated on the recorded plans (the cover holds those against the plan header)."""
  cs = R.load_wgrad_cases()
  fam = lambda f: [c for c in cs if c.family == f]
  # generic: direct write, ragged last slice, 9 Cin % 64 != 0, several column tiles, strides 1..3, odd sizes, three encoders
  gen = fam('generic')
  assert any(c.S == 1 and c.reduce == 'none' for c in gen)
  assert any(c.S > 1 and R.wgrad_pixels(c) % c.slice_px != 0 and (R.wgrad_pixels(c) % c.slice_px) % 64 != 0 for c in gen)
  assert any((9 * c.Cin) % 64 != 0 for c in gen) and any(c.Cout > 64 and c.Cout % 64 == 0 for c in gen)
  assert {1, 2, 3} <= {c.stride for c in gen} and any(c.stride == 2 and c.H % 2 and c.W % 2 for c in gen)
  assert any(c.G == 3 for c in gen)
  # LDS: every variant with one encoder and with three
  lds = fam('lds')
  for inst in {c.inst for c in lds}:
    assert {1, 3} <= {c.G for c in lds if c.inst == inst}, inst
  assert len({c.inst for c in lds}) == 6
  assert any((c.H // 2) % 2 == 1 for c in lds)
  # conv1: fewer tiles than slices, more at G = 1 and G = 3, ragged tiles
  c1 = fam('conv1')
  tiles1 = lambda c: c.N * -(-c.H // 4) * -(-c.W // 16)
  assert any(c.G == 1 and tiles1(c) < c.S for c in c1) and any(c.G == 1 and tiles1(c) > c.S for c in c1)
  assert any(c.G == 3 and tiles1(c) > c.S for c in c1) and all(c.H % 4 and c.W % 16 for c in c1)
  # halo: one, two and three encoders, one case in the remainder-block form
  halo = fam('halo')
  assert {1, 2, 3} <= {c.G for c in halo} and sum(c.remainder for c in halo) == 1
  # slab sum: both forms, S % 4 != 0, a short last wave share, a ragged last block, no bias gradient
  red = [c for c in cs if c.reduce != 'none']
  assert any(c.reduce == 'split' and 16 <= c.S < 20 and c.S % 4 for c in red) and any(c.reduce == 'plain' and c.S % 4 for c in red)
  assert any(((9 * c.Cin * c.Cout + c.Cout) // 4) % (64 if c.reduce == 'split' else 256) for c in red)
  assert any('nodb' in c.flags for c in red) and any('nodb' in c.flags and c.reduce == 'none' for c in cs)
  # the exact pass: every partial sum is an integer below 2**24 (|x|, |dz| <= 2)
  for c in cs:
    assert 4 * R.wgrad_pixels(c) < 2 ** 24 and R.wgrad_pixels(c) <= 17000, c.text
