"""The host side of the opt-in gradient accumulation over micro-batches: the values ``grad_accum_steps`` takes, the new
entry point as header, library and binding declare it, the command-line flag, the restatement tests/_grad_accum_ref.py against
cases worked by hand, and -- in float64, on the CPU -- the identity the option rests on: the mean of the micro-batch gradients is
the gradient of the concatenated batch."""
import importlib.util
import os
import re

import numpy as np
import pytest

import _grad_accum_ref as GA

import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = 'geeco_grad_accumulate_segments'


# ================================================================================================
# the option's values
# ================================================================================================
def test_grad_accum_steps_off_and_on_values():
  from geeco_amd import estimator as est
  from geeco_amd.variables import check_grad_accum_steps
  assert check_grad_accum_steps(None) is None and check_grad_accum_steps(1) is None
  assert check_grad_accum_steps(2) == 2 and check_grad_accum_steps(7) == 7 and check_grad_accum_steps(np.int64(3)) == 3
  assert isinstance(check_grad_accum_steps(np.int64(3)), int)
  for ok in (None, 1, 2, 7):
    est.Estimator(est.e2evmc_model_fn, None, est.RunConfig(), {'grad_accum_steps': ok})


@pytest.mark.parametrize('bad', [0, -1, 2.5, True, '2', 2.0, float('nan'), [2]])
def test_bad_grad_accum_steps_is_refused_by_name(bad):
  from geeco_amd import estimator as est
  from geeco_amd.variables import check_grad_accum_steps
  with pytest.raises(ValueError, match='grad_accum_steps'):
    check_grad_accum_steps(bad)
  with pytest.raises(ValueError, match=r"params\['grad_accum_steps'\]"):
    est.Estimator(est.e2evmc_model_fn, None, est.RunConfig(), {'grad_accum_steps': bad})


def test_a_model_checks_grad_accum_steps_and_it_is_training_only():
  from geeco_amd import graph
  from geeco_amd.params import create_e2evmc_config
  cfg = create_e2evmc_config(dict(window_size=2, img_height=136, img_width=136))
  with pytest.raises(ValueError, match='grad_accum_steps'):
    graph.E2EVMC(cfg, 2, 'cpu', grad_accum_steps=0)
  with pytest.raises(ValueError, match='grad_accum_steps'):
    graph.GoalE2EVMC(cfg, 2, 'cpu', grad_accum_steps=2.5)


def test_cli_flag_reaches_params():
  spec = importlib.util.spec_from_file_location('train_e2evmc_cli_accum', os.path.join(ROOT, 'scripts', 'train_e2evmc.py'))
  cli = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(cli)
  args = cli.ARGPARSER.parse_args(['--grad_accum_steps', '4'])
  assert cli.estimator_params(args, 'CFG') == {'e2evmc_config': 'CFG', 'log_steps': args.log_steps, 'debug': False, 'grad_accum_steps': 4}
  off = cli.ARGPARSER.parse_args([])
  assert off.grad_accum_steps == 1 and 'grad_accum_steps' not in cli.estimator_params(off, 'CFG')
  from geeco_amd.params import create_e2evmc_config
  assert 'grad_accum_steps' not in create_e2evmc_config({})._asdict()      # not a field of the model config


# ================================================================================================
# header, library, binding
# ================================================================================================
def test_header_library_and_binding_agree_and_the_abi_version_is_unchanged():
  from geeco_amd import _native, ops
  assert _abi.define('GEECO_ABI_VERSION') == 7 == _native.ABI_VERSION
  assert NEW in _abi.added_within(7)
  assert _native.SIGNATURES[NEW] == (_native._I, [_native._P, _native._P, _native._I, _native._L, _native._I, _native._P])
  lib = _native.load()
  assert hasattr(lib, NEW) and int(lib.geeco_abi_version()) == 7
  assert callable(ops.grad_accumulate_segments)
  sources = open(os.path.join(ROOT, 'geeco_amd', 'csrc', 'sources.sh')).read()
  assert ' grad_accum ' in re.search(r'HIP_SOURCES="([^"]*)"', sources).group(1)


def test_host_side_refusals():
  """Bad arguments are refused before any launch, with a message (no GPU needed: the addresses are never followed)."""
  import ctypes
  from geeco_amd import _native
  lib = _native.load()
  fn = lib.geeco_grad_accumulate_segments
  err = lambda: (lib.geeco_last_error() or b'').decode()
  E = _native.GEECO_EINVAL
  acc = ctypes.c_void_p(1 << 20)
  seg = (_native.AdamSegment * 9)()
  for k in range(9):
    seg[k].g, seg[k].p_off, seg[k].count = (1 << 24) + 64 * k, 8 * k, 8
  assert fn(None, seg, 1, 100, 0, None) == E and 'bad arguments' in err()
  assert fn(acc, None, 1, 100, 0, None) == E and 'bad arguments' in err()
  for nseg in (0, -1, 9):
    assert fn(acc, seg, nseg, 100, 0, None) == E and 'pieces' in err(), nseg
  assert fn(ctypes.c_void_p((1 << 20) + 4), seg, 1, 100, 0, None) == E and '16-byte aligned' in err()
  for field, bad, what in (('p_off', 2, 'multiple of 4'), ('p_off', -4, 'multiple of 4'), ('g', (1 << 24) + 4, '16-byte aligned'), ('g', 0, 'piece 0'),
                           ('count', 0, 'count >= 1'), ('count', -8, 'count >= 1')):
    good = getattr(seg[0], field)
    setattr(seg[0], field, bad)
    assert fn(acc, seg, 1, 100, 1, None) == E and what in err(), (field, bad, err())
    setattr(seg[0], field, good)
  # a piece not inside [0, n)
  for off, cnt, n in ((96, 8, 100), (100, 1, 100), (0, 101, 100), (104, 4, 100)):
    seg[0].p_off, seg[0].count = off, cnt
    assert fn(acc, seg, 1, n, 0, None) == E and 'outside the accumulator' in err(), (off, cnt, n)
  seg[0].p_off, seg[0].count = 0, 8
  # a source inside the range of the accumulator it is added to, at its start, across its end, and inside another piece's range
  for g in ((1 << 20), (1 << 20) + 16, (1 << 20) - 16, (1 << 20) + 32):
    seg[0].g = g
    assert fn(acc, seg, 2, 100, 0, None) == E and 'overlaps' in err(), g


# ================================================================================================
# the restatement
# ================================================================================================
def test_restatement_by_hand():
  nan, inf = np.nan, np.inf
  acc = np.array([1, 2, 3, 4, 5, 6, 7, nan, 9, 10], np.float32)
  g0, g1 = np.array([10, 20, 30, 40, 99], np.float32), np.array([-0.0, inf, 0.5], np.float32)
  pieces = [(g1, 4, 3), (g0, 0, 4)]      # [7, 10) belongs to no piece; g0's fifth float is slack
  add = GA.accumulate(acc, pieces, False)
  assert GA.same_floats(add, np.array([11, 22, 33, 44, 5, inf, 7.5, nan, 9, 10], np.float32))
  over = GA.accumulate(np.full(10, nan, np.float32), pieces, True)
  assert GA.same_floats(over, np.array([10, 20, 30, 40, -0.0, inf, 0.5, nan, nan, nan], np.float32))
  assert np.signbit(over[4]) and acc[0] == 1.0                    # -0 is kept as -0; the input is left alone
  # float32, not float64: 2^24 + 1 is 2^24
  assert GA.accumulate(np.array([2.0 ** 24], np.float32), [(np.ones(1, np.float32), 0, 1)], False)[0] == np.float32(2.0 ** 24)
  # the comparison tells +0 from -0 and a NaN from a number, and takes NaN for NaN
  assert not GA.same_floats(np.array([0.0], np.float32), np.array([-0.0], np.float32))
  assert not GA.same_floats(np.array([nan], np.float32), np.array([1.0], np.float32))
  assert not GA.same_floats(np.array([1.0], np.float32), np.array([nan], np.float32))
  assert GA.same_floats(np.array([nan, 1.0], np.float32), np.array([nan, 1.0], np.float32))


@pytest.mark.parametrize('n', [7, 1029])
def test_the_restatement_rejects_a_dropped_piece_and_an_add_in_overwrite_mode(n):
  """What a broken launch would leave is told from what the semantics ask for, on the data the GPU tests use."""
  g, acc = GA.special_floats(n, 1), np.random.default_rng(2).standard_normal(n + 5).astype(np.float32)
  cuts = GA.partition(n, 3, 5)
  assert sorted(cuts)[0][0] == 0 and sum(c for _, c in cuts) == n and all(off % 4 == 0 for off, _ in cuts)
  pieces = [(g[off:off + cnt], off, cnt) for off, cnt in cuts]
  for overwrite, start in ((False, acc), (True, np.full(n + 5, np.nan, np.float32))):
    want = GA.accumulate(start, pieces, overwrite)
    assert GA.same_floats(want, GA.accumulate(start, [(g, 0, n)], overwrite))      # any partition is the one-piece result
    assert GA.same_floats(want[n:], start[n:])
    for k in range(len(pieces)):      # a dropped piece
      assert not GA.same_floats(GA.accumulate(start, pieces[:k] + pieces[k + 1:], overwrite), want), (overwrite, k)
  # overwrite mode run as an add: onto NaN everything is NaN, onto numbers the sums are not the gradients
  want = GA.accumulate(np.full(n + 5, np.nan, np.float32), pieces, True)
  assert not GA.same_floats(GA.accumulate(np.full(n + 5, np.nan, np.float32), pieces, False), want)
  assert not GA.same_floats(GA.accumulate(acc, pieces, False), GA.accumulate(acc, pieces, True))


# ================================================================================================
# the identity the option rests on, in the oracle at float64
# ================================================================================================
U64 = 2.0 ** -53
BOUND = 1e-12           # relative to the largest gradient element
MARGIN = 16.0


@pytest.mark.parametrize('A', [2, 3])
@pytest.mark.parametrize('name', ['e2e_vmc', 'goal residual'])
def test_the_mean_of_the_micro_batch_gradients_is_the_gradient_of_the_concatenated_batch(name, A):
  """grad_scale = 1 / A on the summed gradient is 'mean of micro-batch means': for the unweighted losses (every term a mean over the
  batch's samples, the regulariser independent of the batch) that IS the gradient of the A * 4 batch.  In exact arithmetic the two are
  equal; in float64 they are the same sums of the same per-sample terms, associated differently.  Roundings that can differ, per
  gradient element, each relative to the sum S of the magnitudes of what is added:
    the sample axis       4 A - 1 additions in one order or another
    the scales            1 / (4 A) once, against 1 / 4 and then 1 / A: 2
    inside a sample       the reductions over pixels and time run in blocks whose boundaries may move with the batch size: pairwise
                          growth, 2 ceil(log2 T) with T = 4 A K H W, the longest sum there is (conv1's kernel, every pixel of every frame)
  R U64 S in all.  S is not observable from outside; what is: kappa = max_i sum_a |g_a[i]| / (A max |G|), the cancellation ACROSS the
  micro-batches, measured here with the oracle alone.  The check below holds R U64 kappa, with a factor MARGIN = 16 for the cancellation
  inside a micro-batch that kappa does not see, under BOUND = 1e-12, so the inputs keep the case inside the bound the test then applies."""
  import torch
  from oracle import geeco_oracle as O
  ocfg, _, goal, P = GA.case(name)
  batches = GA.micro_batches(name, A)
  grads = lambda f, l: np.concatenate([g.numpy().ravel() for g in O.OracleTrainer(ocfg, goal, P, dtype=torch.float64).loss_and_grads(f, l)[2].values()])
  micro = [grads(f, l) for f, l in batches]
  whole = grads(*GA.concatenated(batches))
  mean = sum(micro) / A
  top = float(np.abs(whole).max())
  T = 4 * A * GA.K3 * GA.H * GA.H
  R = (4 * A - 1) + 2 + 2 * int(np.ceil(np.log2(T)))
  kappa = float(np.max(sum(np.abs(g) for g in micro))) / (A * top)
  worst = float(np.abs(mean - whole).max()) / top
  print('%s A=%d: R = %d roundings, kappa = %.3f, derived bound %.3g, worst difference %.3g of the largest element %.3g'
        % (name, A, R, kappa, MARGIN * R * U64 * kappa, worst, top))
  assert top > 0.0 and np.isfinite(whole).all()
  assert MARGIN * R * U64 * kappa <= BOUND
  assert worst <= BOUND
  # ... and the micro-batches do differ: the identity is not that of equal batches
  assert float(np.abs(micro[0] - micro[1]).max()) > 1e-3 * top
