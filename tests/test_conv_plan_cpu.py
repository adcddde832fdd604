"""The gather GEMM's host-side planning (geeco_amd/csrc/conv_gemm_plan.h) against a recorded table of launch parameters."""
import os
import subprocess


def test_conv_gemm_launch_parameters_match_the_recorded_table(tmp_path):
  """tests/native/conv_plan_table.cpp prints tile sizes, split-K factor, workspace bytes, per-class rows / taps / first tile,
  class rotation, grid, the uniform-tap and HWIO flags and the top-of-the-backward block range for 576 problems (the eight
  encoder layers, forward and input gradient, three input sizes, 1..3 encoders, four frame counts).  The expected output,
  tests/native/conv_plan_table.txt, was recorded from the planning code as it stood before conv_gemm_plan.h shared it (two
  copies of the grid setup); the header must reproduce it byte for byte.  Built with -fsanitize=address,undefined as a host
  program of its own."""
  here = os.path.dirname(os.path.abspath(__file__))
  csrc = os.path.join(here, '..', 'geeco_amd', 'csrc')
  exe = str(tmp_path / 'conv_plan_table')
  subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-fsanitize=address,undefined',
                  '-fno-sanitize-recover=undefined', '-I' + csrc, os.path.join(here, 'native', 'conv_plan_table.cpp'), '-o', exe],
                 check=True, timeout=300)
  res = subprocess.run([exe], capture_output=True, text=True, timeout=60)
  assert res.returncode == 0, res.stdout[-2000:] + res.stderr
  want = open(os.path.join(here, 'native', 'conv_plan_table.txt')).read()
  assert len(want.splitlines()) == 576
  if res.stdout != want:
    bad = [(a, b) for a, b in zip(res.stdout.splitlines(), want.splitlines()) if a != b]
    assert False, '%d lines differ, the first:\n got  %s\n want %s' % (len(bad), *bad[0]) if bad else 'line counts differ'
