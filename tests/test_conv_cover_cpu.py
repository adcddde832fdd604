"""The case list of the gather GEMM's device tests (tests/native/conv_gemm_cases.txt) runs every launch variant the model reaches."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def cover(tmp_path_factory):
  """tests/native/conv_variant_cover.cpp evaluates conv_plan / conv_gemm_grid (geeco_amd/csrc/conv_gemm_plan.h) on the host: built
  with -fsanitize=address,undefined as a program of its own."""
  exe = str(tmp_path_factory.mktemp('cover') / 'conv_variant_cover')
  subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                  '-I' + os.path.join(HERE, '..', 'geeco_amd', 'csrc'), os.path.join(HERE, 'native', 'conv_variant_cover.cpp'),
                  '-o', exe], check=True, timeout=300)
  res = subprocess.run([exe, os.path.join(HERE, 'native', 'conv_gemm_cases.txt')], capture_output=True, text=True, timeout=120)
  assert res.returncode == 0, res.stdout[-2000:] + res.stderr
  lines = res.stdout.splitlines()
  cases = [l[len('case '):] for l in lines if l.startswith('case ')]
  sweep = [l[len('sweep '):] for l in lines if l.startswith('sweep ')]
  factors = [int(l.split()[1]) for l in lines if l.startswith('sweepS ')]
  assert len(cases) + len(sweep) + len(factors) == len(lines)
  return cases, sweep, factors


def _key(case_line):
  return case_line.split('|')[1].rsplit(' S=', 1)[0].strip()


def _factor(case_line):
  return int(case_line.rsplit(' S=', 1)[1].split()[0])


def test_every_variant_of_the_sweep_has_a_case(cover):
  """The sweep: the eight encoder layers, forward for 1..512 frames and input gradient for 1..96, inputs 136 / 144 / 256, 1..3
  encoders, every layer taken as the gather GEMM's (a superset of what the other kernel families leave to it).  Each of its
  keys (direction, tile, uniform tap, split, classes, rotation, unequal class rows, ragged last tile) is the key of a case."""
  cases, sweep, _ = cover
  have = {_key(c) for c in cases}
  assert len(sweep) >= 40, sweep
  missing = [k for k in sweep if k not in have]
  assert not missing, 'no case of conv_gemm_cases.txt runs:\n  ' + '\n  '.join(missing)


def test_split_factors_of_the_cases_span_the_sweeps(cover):
  """The smallest and the largest split factor of the sweep (2 and 18) and a prime one beyond the slab sum's unroll of four."""
  cases, _, factors = cover
  assert (min(factors), max(factors)) == (2, 18), factors
  ran = {_factor(c) for c in cases}
  assert {2, 18} <= ran, sorted(ran)
  assert ran & {5, 7, 11, 13, 17}, sorted(ran)
  assert ran <= set(factors) | {1}, (sorted(ran), factors)


def test_every_case_runs_the_variant_recorded_beside_it(cover):
  """A change of the plan that moves a case to another variant shows here, as a diff, and not as a device test that silently
  checks something else."""
  cases, _, _ = cover
  want = [l.strip() for l in open(os.path.join(HERE, 'native', 'conv_gemm_cases.txt')) if l.strip() and not l.startswith('#')]
  assert len(want) == len(cases) >= 60
  bad = [(g, w) for g, w in zip(cases, want) if g != w]
  assert not bad, '%d cases differ, the first:\n got  %s\n want %s' % (len(bad), *bad[0])
