"""The case list of the fused encoder-bottom backward's device tests (tests/native/conv_bottom_cases.txt) runs every launch form the
models reach and all four instantiations of conv2_dgrad_conv1_wgrad_kernel."""
import os
import subprocess

import pytest

import _conv_refs as R

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def cover(tmp_path_factory):
  """tests/native/conv_bottom_cover.cpp evaluates fused_bottom_launch_plan (geeco_amd/csrc/conv_wgrad_plan.h) on the host and walks
  every block's range: built with -fsanitize=address,undefined as a program of its own."""
  exe = str(tmp_path_factory.mktemp('cover') / 'conv_bottom_cover')
  subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                  '-I' + os.path.join(HERE, '..', 'geeco_amd', 'csrc'), os.path.join(HERE, 'native', 'conv_bottom_cover.cpp'),
                  '-o', exe], check=True, timeout=300)
  res = subprocess.run([exe, R.BOTTOM_CASES_TXT], capture_output=True, text=True, timeout=120)
  assert res.returncode == 0, res.stdout[-2000:] + res.stderr
  lines = res.stdout.splitlines()
  cases = [l[len('case '):] for l in lines if l.startswith('case ')]
  sweep = [l[len('sweep '):] for l in lines if l.startswith('sweep ')]
  insts = [l[len('inst '):] for l in lines if l.startswith('inst ')]
  assert len(cases) + len(sweep) + len(insts) == len(lines)
  return cases, sweep, insts


def test_every_case_runs_the_form_recorded_beside_it(cover):
  """A change of the plan that moves a case to another form (or changes its blocks, its slab count, the length of its ranges, the
  boundaries its blocks cross or its empty blocks) shows here, as a diff, and not as a device test that silently checks something
  else."""
  cases, _, _ = cover
  want = [l.strip() for l in open(R.BOTTOM_CASES_TXT) if l.strip() and not l.startswith('#')]
  assert len(want) == len(cases) >= 20
  bad = [(g, w) for g, w in zip(cases, want) if g != w]
  assert not bad, '%d cases differ, the first:\n got  %s\n want %s' % (len(bad), *bad[0])


def test_every_form_of_the_sweep_has_a_case(cover):
  """The sweep: the models' launches (the sign-word entry point) at inputs 136 / 144 / 256 with 1..3 encoders, 1..512 frames and the
  step runner's reserved_cus (0, 16, 32).  Each of its keys (mask or bits, regular or remainder-block form, crossing kinds) is the
  key of a case."""
  _, sweep, _ = cover
  have = {R.bottom_key(c) for c in R.load_bottom_cases()}
  assert len(sweep) >= 3 and any('remainder' in k for k in sweep), sweep
  missing = [k for k in sweep if k not in have]
  assert not missing, 'no case of conv_bottom_cases.txt runs:\n  ' + '\n  '.join(missing)


def test_every_instantiation_has_a_case(cover):
  """<3, false>, <4, false>, <3, true>, <4, true>: each is launched by a case at exact tiles with one encoder and at tiles ragged in
  both directions with three."""
  _, _, insts = cover
  assert len(insts) == len(set(insts)) == 4, insts
  cs = R.load_bottom_cases()
  assert {c.inst for c in cs} == set(insts)
  for inst in insts:
    mine = [c for c in cs if c.inst == inst]
    assert any(c.G == 1 and c.H % 8 == 0 and c.W % 64 == 0 for c in mine), inst
    assert any(c.G == 3 and c.H % 8 == 2 and c.W % 64 == 2 for c in mine), inst


def _segment_crosses_frame(c):
  """The remainder block's segment [S0 per, tiles) holds tiles of two frames."""
  per_frame = -(-c.W // 64) * -(-c.H // 8)
  first = (c.S - 1) * c.per
  return c.remainder and first // per_frame != (c.tiles - 1) // per_frame


def test_the_cases_hold_the_edges(cover):
  """The edges the list is meant to hold, stated on the recorded plans (the cover holds those against the plan header)."""
  cs = R.load_bottom_cases()
  bits, mask = [c for c in cs if 'bits' in c.flags], [c for c in cs if 'mask' in c.flags]
  rem = lambda c: c.tiles - (c.S - 1) * c.per      # tiles of a remainder segment
  # the plans' own arithmetic
  for c in cs:
    assert c.tiles == c.N * -(-c.W // 64) * -(-c.H // 8) and c.slice_px == c.per * 512, c.text
    assert c.blocks == (c.S - c.remainder) * c.G + c.remainder <= 256 - c.reserved, c.text
    assert sum(end - first for _, _, first, end in R.bottom_ranges(c)) == c.tiles * c.G, c.text
    assert c.empty == sum(first == end for _, _, first, end in R.bottom_ranges(c)), c.text
  # empty ranges that must leave zero slabs, with one encoder and with three; a launch without any
  assert any(c.G == 1 and c.empty == 252 for c in cs) and any(c.G == 3 and c.empty == 219 for c in cs)
  assert any(c.empty == 0 for c in cs)
  # ranges of two and of three tiles; a 2-tile range that straddles a frame (three tiles per frame), float mask with dz1 and bits
  for form in (bits, mask):
    assert any(not c.remainder and c.per == 2 and 'frame' in c.cross and -(-c.W // 64) * -(-c.H // 8) == 3 for c in form)
  assert any(c.per == 3 and c.reserved == 128 and c.S == 42 and c.empty == 6 for c in cs)
  assert any('dz1' in c.flags and 'frame' in c.cross and c.W % 64 for c in cs)
  # two encoders on 128 blocks each
  assert any(c.G == 2 and c.S == 128 and not c.remainder and c.tiles == 129 for c in bits)
  assert any(c.G == 2 and c.S == 128 and not c.remainder for c in mask)
  # the remainder-block form: one tile per segment, ragged both ways, through dz1 and through bits + the deferred sum
  one = [c for c in cs if c.remainder and c.G == 3 and rem(c) == 1 and c.H % 8 and c.W % 64 and c.blocks == 256]
  assert any({'mask', 'dz1'} <= c.flags for c in one) and any({'bits', 'pending'} <= c.flags for c in one)
  # ... two tiles per segment (the double buffer, then the reduction area again), both instantiation classes
  assert any(c.remainder and c.G == 3 and rem(c) == 2 for c in bits) and any(c.remainder and c.G == 3 and rem(c) == 2 for c in mask)
  # ... reached through reserved CUs with two encoders (255 CUs), both entry points of the deferred form
  two = [c for c in cs if c.remainder and c.G == 2 and c.reserved == 1 and c.blocks == 255 and c.S == 128]
  assert any('bits' in c.flags for c in two) and any('mask' in c.flags for c in two)
  # ... a segment that crosses a frame itself
  assert any(_segment_crosses_frame(c) and rem(c) >= 3 for c in cs)
  assert all('enc' in c.cross for c in cs if c.remainder) and not any('enc' in c.cross for c in cs if not c.remainder)
  # bits where the row pitch exceeds W and the rows exceed H
  assert any(R.tiles_8x64(c.H, c.W) == (16, 128) and (c.H, c.W) == (10, 66) for c in bits)
  # CREAL = 3 slabs (stride 896) in a workspace sized for CREAL = 4 with the most slabs the workspace holds
  assert any(c.C == 3 and c.S == 256 for c in cs) and any(c.C == 3 and c.S == 86 and c.G == 3 for c in cs)
  # every entry point: plain, deferred with the float mask, bits with and without the deferred sum
  forms = {('bits' in c.flags, 'pending' in c.flags) for c in cs}
  assert forms == {(False, False), (False, True), (True, False), (True, True)}
  # the exact pass: |dz1| <= 384, every partial sum of dw1 / db1 an integer below 2**24; the largest case is 42240 pixels
  for c in cs:
    assert R.BOTTOM_EXACT_MAX * R.bottom_pixels(c) < 2 ** 24 and R.bottom_pixels(c) <= 42240, c.text
  assert R.BOTTOM_EXACT_MAX == 384
