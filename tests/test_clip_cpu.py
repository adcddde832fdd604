"""The host side of the opt-in global-norm gradient clipping: the values ``clip_norm`` takes, the float64 restatement
against a case worked by hand, the command-line flag, and the new entry points as header and binding declare them."""
import importlib.util
import math
import os
import re

import numpy as np
import pytest

import _clip_ref as C

import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('geeco_clip_ws_floats', 'geeco_grad_sumsq_segments', 'geeco_clip_scale', 'geeco_adam_tf_segments_clip')


@pytest.mark.parametrize('bad', [-1.0, -0.0001, float('nan'), float('inf'), -float('inf'), 1e39, 1e-46, 'tight', True, False, [5.0]])
def test_bad_clip_norm_is_refused_by_name(bad):
  from geeco_amd import estimator as est
  from geeco_amd.variables import check_clip_norm
  with pytest.raises(ValueError, match='clip_norm'):
    check_clip_norm(bad)
  with pytest.raises(ValueError, match=r"params\['clip_norm'\]"):
    est.Estimator(est.e2evmc_model_fn, None, est.RunConfig(), {'clip_norm': bad})


def test_clip_norm_off_and_on_values():
  from geeco_amd import estimator as est
  from geeco_amd.variables import check_clip_norm
  assert check_clip_norm(None) is None and check_clip_norm(0) is None and check_clip_norm(0.0) is None
  assert check_clip_norm(5) == 5.0 and isinstance(check_clip_norm(5), float)
  assert check_clip_norm(np.float32(0.5)) == 0.5 and check_clip_norm(1e30) == 1e30 and check_clip_norm(1e-30) == 1e-30
  est.Estimator(est.e2evmc_model_fn, None, est.RunConfig(), {'clip_norm': 5.0})
  est.Estimator(est.e2evmc_model_fn, None, est.RunConfig(), {'clip_norm': 0})


def test_a_model_checks_clip_norm():
  from geeco_amd import graph
  from geeco_amd.params import create_e2evmc_config
  cfg = create_e2evmc_config(dict(window_size=2, img_height=136, img_width=136))
  with pytest.raises(ValueError, match='clip_norm'):
    graph.E2EVMC(cfg, 2, 'cpu', clip_norm=-1.0)
  with pytest.raises(ValueError, match='clip_norm'):
    graph.GoalE2EVMC(cfg, 2, 'cpu', clip_norm=float('nan'))


def test_restatement_by_hand():
  """Three elements, every constant exact in float32: G = g / 2 + p / 4 = [1.5, 2, 0], norm = 2.5; c = 1.25 halves it."""
  p = np.array([1.0, -2.0, 0.5], np.float32)
  g = np.array([2.5, 5.0, -0.25], np.float32)
  m = np.array([0.25, 0.0, -0.5], np.float32)
  v = np.array([0.25, 0.0, 1.0], np.float32)
  kw = dict(grad_scale=0.5, l2=0.25)
  np.testing.assert_array_equal(C.total_grad(p, g, **kw), [1.5, 2.0, 0.0])
  assert C.global_norm(p, g, **kw) == 2.5
  assert C.clip_scale(2.5, 1.25) == 0.5
  assert C.clip_scale(2.5, 2.5) == 1.0 and C.clip_scale(2.5, 1e30) == 1.0 and C.clip_scale(0.0, 3.0) == 1.0      # norm <= c: exactly 1
  # G s = [0.75, 1, 0];  m' = m / 2 + G s / 2;  v' = 3 v / 4 + (G s)^2 / 4;  p' = p - m' / (2 sqrt(v'))
  p2, m2, v2 = C.clipped_adam_ref(p, g, m, v, 0.5, 0.5, b1=0.5, b2=0.75, eps=0.0, **kw)
  np.testing.assert_array_equal(m2, [0.5, 0.5, -0.25])
  np.testing.assert_array_equal(v2, [0.328125, 0.25, 0.75])
  np.testing.assert_allclose(p2, [1.0 - 0.25 / math.sqrt(0.328125), -2.5, 0.5 + 0.125 / math.sqrt(0.75)], rtol=1e-15)
  # s = 1 is the unclipped restatement
  import _primitive_refs as R
  for a, b in zip(C.clipped_adam_ref(p, g, m, v, 0.5, 1.0, **kw), R.adam_ref(p, g, m, v, 0.5, **kw)):
    np.testing.assert_array_equal(a, b)
  # the bounds: those of the unclipped step at the scaled constants, and strictly wider wherever the scaled gradient is not 0
  wide = C.clipped_adam_bounds(p, g, m, v, 0.5, 0.5, **kw)
  base = R.adam_bounds(p, g, m, v, 0.5, grad_scale=0.25, l2=0.125)
  for w, b in zip(wide, base):
    assert (w[:2] > b[:2]).all() and (w >= b).all() and (w < 2 * b + 1e-30).all()


def test_cli_flag_reaches_params():
  spec = importlib.util.spec_from_file_location('train_e2evmc_cli_clip', os.path.join(ROOT, 'scripts', 'train_e2evmc.py'))
  cli = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(cli)
  args = cli.ARGPARSER.parse_args(['--clip_norm', '5.0'])
  assert cli.estimator_params(args, 'CFG') == {'e2evmc_config': 'CFG', 'log_steps': args.log_steps, 'debug': False, 'clip_norm': 5.0}
  both = cli.ARGPARSER.parse_args(['--clip_norm', '2', '--ema_decay', '0.999'])
  assert cli.estimator_params(both, 'CFG')['clip_norm'] == 2.0 and cli.estimator_params(both, 'CFG')['ema_decay'] == 0.999
  off = cli.ARGPARSER.parse_args([])
  assert off.clip_norm == 0.0 and 'clip_norm' not in cli.estimator_params(off, 'CFG')
  # not a field of the model config: e2evmc_config.json stays as the reference writes it
  from geeco_amd.params import create_e2evmc_config
  assert 'clip_norm' not in create_e2evmc_config({})._asdict()


@pytest.mark.parametrize('name', NEW)
def test_header_and_binding_agree(name):
  from geeco_amd import _native
  assert len(_native.SIGNATURES[name][1]) == len(_abi.functions()[name][1])      # (every type: test_abi_cpu.py::test_signature_matches_the_header)
  assert hasattr(_native.load(), name)


def test_abi_version_is_unchanged_and_the_additions_are_listed():
  from geeco_amd import _native
  assert _abi.define('GEECO_ABI_VERSION') == 7 == _native.ABI_VERSION
  assert set(NEW) <= set(_abi.added_within(7))


def test_workspace_size_and_host_side_refusals():
  """One partial per chunk of 4096 floats; bad arguments are refused before any launch, with a message (no GPU needed)."""
  import ctypes
  from geeco_amd import _native
  lib = _native.load()
  ch = 4096
  assert [lib.geeco_clip_ws_floats(n) for n in (0, 1, ch - 1, ch, ch + 1, 3 * ch + 7)] == [0, 1, 1, 1, 2, 4]
  one = ctypes.c_void_p(64)
  seg = (_native.AdamSegment * 2)()
  seg[0].g, seg[0].p_off, seg[0].count = 64, 0, 10
  seg[1].g, seg[1].p_off, seg[1].count = 64, 9, 4
  err = lambda: (lib.geeco_last_error() or b'').decode()
  assert lib.geeco_grad_sumsq_segments(one, seg, 2, 100, 1.0, 0.0, one, None) == _native.GEECO_EINVAL and 'overlap' in err()
  assert lib.geeco_grad_sumsq_segments(one, seg, 1, 8, 1.0, 0.0, one, None) == _native.GEECO_EINVAL and 'outside the arena' in err()
  assert lib.geeco_grad_sumsq_segments(None, seg, 1, 100, 1.0, 1e-3, one, None) == _native.GEECO_EINVAL and 'l2' in err()
  assert lib.geeco_grad_sumsq_segments(one, seg, 9, 100, 1.0, 0.0, one, None) == _native.GEECO_EINVAL and 'pieces' in err()
  for clip in (0.0, -1.0, float('nan'), float('inf')):
    assert lib.geeco_clip_scale(one, 1, clip, one, None) == _native.GEECO_EINVAL and 'clip' in err(), clip
  assert lib.geeco_adam_tf_segments_clip(one, None, one, one, None, seg, 1, one, None, 0.0, None, 0.9, 0.999, 1e-8, 1.0, 0.0,
                                         None) == _native.GEECO_EINVAL and 'bad arguments' in err()
  seg[0].p_off = 2
  assert lib.geeco_adam_tf_segments_clip(one, None, one, one, None, seg, 1, one, None, 0.0, one, 0.9, 0.999, 1e-8, 1.0, 0.0,
                                         None) == _native.GEECO_EINVAL and 'multiple of 4' in err()
  seg[0].p_off = 0
  assert lib.geeco_adam_tf_segments_clip(one, None, one, one, one, seg, 1, one, one, 1.5, one, 0.9, 0.999, 1e-8, 1.0, 0.0,
                                         None) == _native.GEECO_EINVAL and 'decay' in err()
