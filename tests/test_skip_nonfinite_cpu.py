"""The host side of the opt-in skipping of optimiser steps whose gradient is not finite: the values ``skip_nonfinite``
takes, the restatement tests/_guard_ref.py against cases worked by hand, the command-line flags, the new entry points as header and
binding declare them and their refusals, and -- in float64, on the CPU -- that the poisoned batch of the GPU tests really has a
non-finite gradient and the clean one a finite one."""
import importlib.util
import os
import re

import numpy as np
import pytest

import _guard_ref as G

import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('geeco_guard_decide', 'geeco_adam_tf_segments_guard')


@pytest.mark.parametrize('bad', [0, -1, 1.0, 2.5, float('nan'), float('inf'), 'yes', [3], (1,), {}])
def test_bad_skip_nonfinite_is_refused_by_name(bad):
  from geeco_amd import estimator as est
  from geeco_amd.variables import check_skip_nonfinite
  with pytest.raises(ValueError, match='skip_nonfinite'):
    check_skip_nonfinite(bad)
  with pytest.raises(ValueError, match=r"params\['skip_nonfinite'\]"):
    est.Estimator(est.e2evmc_model_fn, None, est.RunConfig(), {'skip_nonfinite': bad})


def test_skip_nonfinite_off_and_on_values():
  from geeco_amd import estimator as est
  from geeco_amd.variables import check_skip_nonfinite
  assert check_skip_nonfinite(None) is None and check_skip_nonfinite(False) is None
  assert check_skip_nonfinite(True) == 100
  assert check_skip_nonfinite(1) == 1 and check_skip_nonfinite(7) == 7 and check_skip_nonfinite(np.int64(12)) == 12
  assert isinstance(check_skip_nonfinite(np.int64(12)), int)
  for ok in (None, False, True, 1, 250):
    est.Estimator(est.e2evmc_model_fn, None, est.RunConfig(), {'skip_nonfinite': ok})


def test_a_model_checks_skip_nonfinite():
  from geeco_amd import graph
  from geeco_amd.params import create_e2evmc_config
  cfg = create_e2evmc_config(dict(window_size=2, img_height=136, img_width=136))
  with pytest.raises(ValueError, match='skip_nonfinite'):
    graph.E2EVMC(cfg, 2, 'cpu', skip_nonfinite=0)
  with pytest.raises(ValueError, match='skip_nonfinite'):
    graph.GoalE2EVMC(cfg, 2, 'cpu', skip_nonfinite=1.5)


def test_restatement_by_hand():
  """Partials whose float32 sum is exact: norm, scale, verdict and counters as the semantics state them."""
  out2, guard = G.decide([9.0, 16.0], 0.0, [0, 4, 2])                 # norm 5, no clipping: applied, the row ends, the total stays
  assert out2.tolist() == [1.0, 5.0] and guard == [1, 4, 0]
  out2, guard = G.decide([9.0, 16.0], 2.5, [1, 0, 0])                 # clipped to 2.5: s = 0.5
  assert out2.tolist() == [0.5, 5.0] and guard == [1, 0, 0]
  out2, guard = G.decide([9.0, 16.0], 5.0, [1, 0, 0])                 # norm <= clip: exactly 1
  assert out2.tolist() == [1.0, 5.0]
  for bad in ([9.0, np.nan], [np.inf, 16.0], [3e38, 3e38]):           # NaN, infinity, a sum beyond float32
    out2, guard = G.decide(bad, 2.5, [1, 4, 2])
    assert out2[0] == 0.0 and not np.isfinite(out2[1]) and guard == [0, 5, 3], bad
  assert np.isinf(G.decide([3e38, 3e38], 0.0, [1, 0, 0])[0][1])
  # the order: 257 partials -- thread 0 adds the first and the last before the tree
  x = np.ones(257, np.float32)
  assert G.norm_f32(x) == np.sqrt(np.float32(257.0))
  # the float64 verdict from the inputs
  p, g = np.ones(3, np.float32), np.array([1.0, 2.0, 3.0], np.float32)
  assert G.total_grad_is_finite(p, g, 0.5, 0.25)
  assert not G.total_grad_is_finite(p, np.array([1.0, np.nan, 3.0], np.float32))
  assert not G.total_grad_is_finite(p, np.array([1.0, np.inf, 3.0], np.float32))
  assert not G.total_grad_is_finite(p, np.array([1.0, 2e19, 3.0], np.float32))        # finite, but its square is beyond float32
  assert G.total_grad_is_finite(p, np.array([1.0, 1.8e19, 3.0], np.float32))


def test_cli_flags_reach_params():
  spec = importlib.util.spec_from_file_location('train_e2evmc_cli_skip', os.path.join(ROOT, 'scripts', 'train_e2evmc.py'))
  cli = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(cli)
  args = cli.ARGPARSER.parse_args(['--skip_nonfinite'])
  assert cli.estimator_params(args, 'CFG') == {'e2evmc_config': 'CFG', 'log_steps': args.log_steps, 'debug': False, 'skip_nonfinite': True}
  both = cli.ARGPARSER.parse_args(['--skip_nonfinite', '--max_skipped_steps', '7', '--clip_norm', '2'])
  assert cli.estimator_params(both, 'CFG')['skip_nonfinite'] == 7 and cli.estimator_params(both, 'CFG')['clip_norm'] == 2.0
  off = cli.ARGPARSER.parse_args([])
  assert off.skip_nonfinite is False and 'skip_nonfinite' not in cli.estimator_params(off, 'CFG')
  with pytest.raises(ValueError, match='max_skipped_steps'):
    cli.estimator_params(cli.ARGPARSER.parse_args(['--max_skipped_steps', '7']), 'CFG')
  # not a field of the model config: e2evmc_config.json stays as the reference writes it
  from geeco_amd.params import create_e2evmc_config
  assert 'skip_nonfinite' not in create_e2evmc_config({})._asdict()


@pytest.mark.parametrize('name', NEW)
def test_header_and_binding_agree(name):
  from geeco_amd import _native, ops
  assert len(_native.SIGNATURES[name][1]) == len(_abi.functions()[name][1])      # (every type: test_abi_cpu.py::test_signature_matches_the_header)
  assert hasattr(_native.load(), name)
  assert callable(getattr(ops, name[len('geeco_'):]))


def test_abi_version_is_unchanged_and_the_additions_are_listed():
  from geeco_amd import _native
  assert _abi.define('GEECO_ABI_VERSION') == 7 == _native.ABI_VERSION
  assert set(NEW) <= set(_abi.added_within(7))
  sources = open(os.path.join(ROOT, 'geeco_amd', 'csrc', 'sources.sh')).read()
  assert ' guard ' in re.search(r'HIP_SOURCES="([^"]*)"', sources).group(1)


def test_host_side_refusals():
  """Bad arguments are refused before any launch, with a message (no GPU needed)."""
  import ctypes
  from geeco_amd import _native
  lib = _native.load()
  one = ctypes.c_void_p(64)
  err = lambda: (lib.geeco_last_error() or b'').decode()
  E = _native.GEECO_EINVAL
  for args in ((None, 1, 0.0, one, one), (one, 1, 0.0, None, one), (one, 1, 0.0, one, None), (one, 0, 0.0, one, one), (one, -3, 1.0, one, one)):
    assert lib.geeco_guard_decide(*args, None) == E and 'bad arguments' in err(), args
  for clip in (-1.0, -1e-30, float('nan'), float('inf'), -float('inf')):
    assert lib.geeco_guard_decide(one, 1, clip, one, one, None) == E and 'clip' in err(), clip
  seg = (_native.AdamSegment * 2)()
  seg[0].g, seg[0].p_off, seg[0].count = 64, 0, 10
  adam = (0.9, 0.999, 1e-8, 1.0, 0.0, None)
  guard = lib.geeco_adam_tf_segments_guard
  # a null guard, a null scale, a null arena, too many pieces
  assert guard(one, None, one, one, None, seg, 1, one, None, 0.0, one, None, *adam) == E and 'adam_tf_segments_guard: bad arguments' in err()
  assert guard(one, None, one, one, None, seg, 1, one, None, 0.0, None, one, *adam) == E and 'bad arguments' in err()
  assert guard(None, None, one, one, None, seg, 1, one, None, 0.0, one, one, *adam) == E and 'bad arguments' in err()
  assert guard(one, None, one, one, None, seg, 9, one, None, 0.0, one, one, *adam) == E and 'pieces' in err()
  # the checks of the clip entry
  assert guard(ctypes.c_void_p(68), None, one, one, None, seg, 1, one, None, 0.0, one, one, *adam) == E and '16-byte aligned' in err()
  seg[0].p_off = 2
  assert guard(one, None, one, one, None, seg, 1, one, None, 0.0, one, one, *adam) == E and 'multiple of 4' in err()
  seg[0].p_off = 0
  assert guard(one, None, one, one, one, seg, 1, one, None, 0.5, one, one, *adam) == E and 'step counter' in err()
  assert guard(one, None, one, one, one, seg, 1, one, one, 1.5, one, one, *adam) == E and 'decay' in err()


@pytest.mark.parametrize('name', list(G.MODELS))
def test_the_poisoned_batch_has_a_non_finite_gradient_and_the_clean_one_a_finite_one(name):
  """The float64 oracle on the batches tests/test_skip_nonfinite_gpu.py uses: the GPU tests rest on a checked condition.  The
  poison also reaches far: most of the gradient is NaN, not one element."""
  _, _, _, _, _, labels = G.case(name)
  clean = G.oracle_gradient(name)
  assert np.isfinite(clean).all() and 0.0 < float(np.sum(clean * clean)) < float(np.finfo(np.float32).max)
  bad = G.oracle_gradient(name, G.poisoned(labels))
  assert not np.isfinite(bad).all()
  print('%s: %d of %d gradient elements of the poisoned batch are not finite' % (name, int((~np.isfinite(bad)).sum()), bad.size))
  assert np.isnan(G.poisoned(labels)['cmd'][0, 0]) and np.isfinite(G.poisoned(labels)['cmd'][:, 3]).all()
  assert np.isfinite(labels['cmd']).all()      # (the shared case is left unchanged)
