"""The host side of the learning-rate schedules: ``geeco_lr_schedule_eval`` -- the function the device evaluates --
against the float64 restatement tests/_lr_schedule_ref.py, anchors that can be checked by hand, the host-side refusals, the values
``lr_schedule`` takes, the command-line flags, and the new entry points as header and binding declare them.  No GPU."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

import _lr_schedule_ref as L

import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('geeco_adam_prepare_schedule', 'geeco_slab_reduce_batch_prepare_schedule', 'geeco_lr_schedule_eval')
BIG = 2 ** 31 + 12345                      # a step count an int32 does not hold
ULP4 = 4 * 2.0 ** -52                      # both sides are float64; pow / cos may differ in the last bits

W, DS = 5, 7
BOUNDS = (3, 10, 11, 2 ** 31 + 5)
VALUES = (1e-3, 1e-4, 1e-5, 1e-2, 3e-7)
SCHEDULES = {}
for _w in (0, W):
  _tag = ', warm-up' if _w else ''
  SCHEDULES['constant' + _tag] = L.schedule('constant', base_lr=1e-3, warmup_steps=_w)
  SCHEDULES['exponential' + _tag] = L.schedule('exponential', base_lr=1e-3, warmup_steps=_w, decay_steps=DS, decay_rate=0.96)
  SCHEDULES['exponential, staircase' + _tag] = L.schedule('exponential', base_lr=1e-3, warmup_steps=_w, decay_steps=DS, decay_rate=0.96,
                                                          staircase=True)
  SCHEDULES['cosine' + _tag] = L.schedule('cosine', base_lr=1e-3, warmup_steps=_w, decay_steps=DS)
  SCHEDULES['cosine, alpha' + _tag] = L.schedule('cosine', base_lr=3e-4, warmup_steps=_w, decay_steps=DS, alpha=0.1)
  SCHEDULES['piecewise' + _tag] = L.schedule('piecewise', warmup_steps=_w, boundaries=BOUNDS, values=VALUES)
SCHEDULES['piecewise, no boundary'] = L.schedule('piecewise', warmup_steps=2, values=(2e-3,))
SCHEDULES['piecewise, 8 boundaries'] = L.schedule('piecewise', warmup_steps=1, boundaries=range(0, 16, 2),
                                                  values=[1e-3 * (k + 1) for k in range(9)])


def _steps(sch):
  """0, w - 1, w, w + 1, every boundary and the step behind it, w + decay_steps and beyond, and a step above 2^31."""
  w = sch['warmup_steps']
  steps = {0, 1, w, w + 1, w + DS - 1, w + DS, w + DS + 1, w + 3 * DS + 2, BIG, BIG + w, 2 ** 40}
  if w:
    steps.add(w - 1)
  for b in sch['boundaries']:
    steps.update((w + b, w + b + 1))
  return sorted(steps)


@pytest.mark.parametrize('name', list(SCHEDULES))
def test_eval_against_the_restatement(name):
  from geeco_amd import ops
  sch = SCHEDULES[name]
  for s in _steps(sch):
    got, ref = ops.lr_schedule_eval(sch, s), L.lr_at(sch, s)
    if sch['kind'] == 'piecewise' and s >= sch['warmup_steps']:
      assert got == ref and got in [L.f32(v) for v in sch['values']], (name, s, got, ref)      # a value, exactly
    else:
      assert abs(got - ref) <= ULP4 * abs(ref), (name, s, got, ref)


def test_anchors_by_hand():
  from geeco_amd import ops
  ev = ops.lr_schedule_eval
  base = L.f32(3e-4)
  # cosine reaches alpha * base_lr at u = decay_steps and stays there
  cos = SCHEDULES['cosine, alpha, warm-up']
  floor = L.f32(0.1) * base
  assert [ev(cos, W + DS + k) for k in (0, 1, 100, BIG)] == [floor] * 4
  assert ev(cos, W) == base and base > ev(cos, W + 1) > ev(cos, W + DS - 1) > floor
  assert ev(SCHEDULES['cosine'], DS) == 0.0 and ev(SCHEDULES['cosine'], 0) == L.f32(1e-3)
  # exponential with staircase is constant within a period, and one factor of decay_rate lower in the next
  stair = SCHEDULES['exponential, staircase, warm-up']
  for period in (0, 1, 4):
    rates = {ev(stair, W + period * DS + k) for k in range(DS)}
    assert len(rates) == 1, period
    assert abs(rates.pop() - L.f32(1e-3) * L.f32(0.96) ** period) <= ULP4 * 1e-3
  smooth = SCHEDULES['exponential, warm-up']
  assert ev(smooth, W) == ev(stair, W) and ev(smooth, W + 1) < ev(stair, W + 1) and ev(smooth, W + DS) == ev(stair, W + DS)
  # warm-up: the last step is L0, the steps before it are its multiples
  for name, first in (('constant, warm-up', L.f32(1e-3)), ('cosine, alpha, warm-up', base), ('piecewise, warm-up', L.f32(VALUES[0]))):
    assert ev(SCHEDULES[name], W - 1) == first, name
    assert [ev(SCHEDULES[name], s) for s in range(W)] == [first * ((s + 1) / W) for s in range(W)], name
  # piecewise: u <= boundary i still runs value i
  pw = SCHEDULES['piecewise']
  assert [ev(pw, s) for s in (0, 3, 4, 10, 11, 12, 2 ** 31 + 5, 2 ** 31 + 6)] == [L.f32(VALUES[i]) for i in (0, 0, 1, 1, 2, 3, 3, 4)]


def _struct(**kw):
  from geeco_amd import ops
  return ops.lr_schedule_struct(L.schedule(**kw))


REFUSED = {
    'unknown kind': (lambda s: setattr(s, 'kind', 4), 'unknown kind'),
    'negative kind': (lambda s: setattr(s, 'kind', -1), 'unknown kind'),
    'decay_steps 0, exponential': (lambda s: setattr(s, 'decay_steps', 0), 'decay_steps'),
    'decay_steps 0, cosine': (lambda s: (setattr(s, 'kind', 2), setattr(s, 'decay_steps', 0)), 'decay_steps'),
    'negative warm-up': (lambda s: setattr(s, 'warmup_steps', -1), 'warmup_steps'),
    'negative warm-up, piecewise': (lambda s: (setattr(s, 'kind', 3), setattr(s, 'warmup_steps', -3)), 'warmup_steps'),
    '9 boundaries': (lambda s: (setattr(s, 'kind', 3), setattr(s, 'n_boundaries', 9)), 'n_boundaries'),
    '-1 boundaries': (lambda s: (setattr(s, 'kind', 3), setattr(s, 'n_boundaries', -1)), 'n_boundaries'),
    'equal boundaries': (lambda s: (setattr(s, 'kind', 3), setattr(s, 'n_boundaries', 2), s.boundaries.__setitem__(0, 4),
                                    s.boundaries.__setitem__(1, 4)), 'strictly increasing'),
    'falling boundaries': (lambda s: (setattr(s, 'kind', 3), setattr(s, 'n_boundaries', 3), s.boundaries.__setitem__(0, 1),
                                      s.boundaries.__setitem__(1, 9), s.boundaries.__setitem__(2, 8)), 'strictly increasing'),
    'NaN base_lr': (lambda s: setattr(s, 'base_lr', float('nan')), 'base_lr'),
    'infinite base_lr': (lambda s: setattr(s, 'base_lr', float('inf')), 'base_lr'),
    'negative base_lr': (lambda s: setattr(s, 'base_lr', -1e-3), 'base_lr'),
    'decay_rate 0': (lambda s: setattr(s, 'decay_rate', 0.0), 'decay_rate'),
    'negative decay_rate': (lambda s: setattr(s, 'decay_rate', -0.5), 'decay_rate'),
    'NaN decay_rate': (lambda s: setattr(s, 'decay_rate', float('nan')), 'decay_rate'),
    'infinite decay_rate': (lambda s: setattr(s, 'decay_rate', float('inf')), 'decay_rate'),
    'alpha above 1': (lambda s: (setattr(s, 'kind', 2), setattr(s, 'alpha', 1.5)), 'alpha'),
    'negative alpha': (lambda s: (setattr(s, 'kind', 2), setattr(s, 'alpha', -0.1)), 'alpha'),
    'NaN alpha': (lambda s: (setattr(s, 'kind', 2), setattr(s, 'alpha', float('nan'))), 'alpha'),
    'negative value': (lambda s: (setattr(s, 'kind', 3), setattr(s, 'n_boundaries', 1), s.values.__setitem__(1, -1e-3)), r'values\[1\]'),
    'NaN value': (lambda s: (setattr(s, 'kind', 3), s.values.__setitem__(0, float('nan'))), r'values\[0\]'),
    'infinite value': (lambda s: (setattr(s, 'kind', 3), setattr(s, 'n_boundaries', 2), s.boundaries.__setitem__(1, 5),
                                  s.values.__setitem__(2, float('inf'))), r'values\[2\]'),
}


@pytest.mark.parametrize('case', list(REFUSED))
def test_host_side_refusals(case):
  """All three entry points refuse the schedule before any launch, with the same message (no GPU is needed: nothing is launched)."""
  from geeco_amd import _native
  lib = _native.load()
  spoil, message = REFUSED[case]
  sch = _struct(kind='exponential', base_lr=1e-3, warmup_steps=2, decay_steps=5, decay_rate=0.5)
  spoil(sch)
  err = lambda: (lib.geeco_last_error() or b'').decode()
  one, out = ctypes.c_void_p(64), ctypes.c_double(-1.0)
  assert lib.geeco_lr_schedule_eval(ctypes.byref(sch), 3, ctypes.byref(out)) == _native.GEECO_EINVAL
  assert re.search(message, err()) and 'lr_schedule_eval' in err() and out.value == -1.0, err()
  assert lib.geeco_adam_prepare_schedule(one, ctypes.byref(sch), 0.9, 0.999, one, None) == _native.GEECO_EINVAL
  assert re.search(message, err()) and 'adam_prepare_schedule' in err(), err()
  assert lib.geeco_slab_reduce_batch_prepare_schedule(None, 0, one, ctypes.byref(sch), 0.9, 0.999, one, None) == _native.GEECO_EINVAL
  assert re.search(message, err()) and 'slab_reduce_batch_prepare_schedule' in err(), err()


def test_null_pointers_are_refused():
  from geeco_amd import _native
  lib = _native.load()
  sch = _struct(kind='constant', base_lr=1e-3, warmup_steps=2)
  err = lambda: (lib.geeco_last_error() or b'').decode()
  one, out = ctypes.c_void_p(64), ctypes.c_double()
  E = _native.GEECO_EINVAL
  assert lib.geeco_lr_schedule_eval(None, 0, ctypes.byref(out)) == E and 'null pointer' in err()
  assert lib.geeco_lr_schedule_eval(ctypes.byref(sch), 0, None) == E and 'null pointer' in err()
  assert lib.geeco_lr_schedule_eval(ctypes.byref(sch), -1, ctypes.byref(out)) == E and 'negative' in err()
  for args in ((None, ctypes.byref(sch), 0.9, 0.999, one, None), (one, None, 0.9, 0.999, one, None), (one, ctypes.byref(sch), 0.9, 0.999, None, None)):
    assert lib.geeco_adam_prepare_schedule(*args) == E and 'null pointer' in err()
    assert lib.geeco_slab_reduce_batch_prepare_schedule(None, 0, *args) == E and 'null pointer' in err()
  assert lib.geeco_lr_schedule_eval(ctypes.byref(sch), 0, ctypes.byref(out)) == 0 and out.value == L.f32(1e-3) / 2


def test_check_lr_schedule_off_and_normalised():
  from geeco_amd import ops
  from geeco_amd.variables import check_lr_schedule
  assert check_lr_schedule(None, 1e-3) is None
  assert check_lr_schedule({'kind': 'constant'}, 1e-3) is None and check_lr_schedule({'kind': 'constant', 'warmup_steps': 0}, 1e-3) is None
  assert check_lr_schedule({'kind': 'constant', 'warmup_steps': 3}, 1e-3) == L.schedule('constant', base_lr=1e-3, warmup_steps=3)
  assert check_lr_schedule({'kind': 'exponential', 'decay_steps': np.int64(9), 'decay_rate': 0.5, 'staircase': True}, 2e-3) == \
      L.schedule('exponential', base_lr=2e-3, decay_steps=9, decay_rate=0.5, staircase=True)
  assert check_lr_schedule({'kind': 'cosine', 'decay_steps': 4, 'warmup_steps': 2}, 1e-3) == L.schedule('cosine', base_lr=1e-3, warmup_steps=2, decay_steps=4)
  assert check_lr_schedule({'kind': 'cosine', 'decay_steps': 4, 'alpha': 1}, 1e-3)['alpha'] == 1.0
  pw = check_lr_schedule({'kind': 'piecewise', 'boundaries': [2, 5], 'values': [1e-3, 1e-4, 1e-5]}, 'ignored')
  assert pw == L.schedule('piecewise', boundaries=(2, 5), values=(1e-3, 1e-4, 1e-5))
  assert check_lr_schedule({'kind': 'piecewise', 'values': [1e-3]}, 0.5)['values'] == (1e-3,)
  # the normalised schedule is what the struct is made of, field by field
  st = ops.lr_schedule_struct(pw)
  assert (st.kind, st.n_boundaries, list(st.boundaries)[:2], st.warmup_steps) == (3, 2, [2, 5], 0)
  assert [st.values[i] for i in range(3)] == [L.f32(v) for v in (1e-3, 1e-4, 1e-5)]
  assert ops.lr_schedule_struct(st) is st


BAD = {
    'not a mapping': ('cosine', 'mapping'),
    'a number': (0.5, 'mapping'),
    'no kind': ({'decay_steps': 3}, 'kind'),
    'unknown kind': ({'kind': 'linear'}, 'kind'),
    'unknown field': ({'kind': 'cosine', 'decay_steps': 3, 'power': 2}, 'power'),
    'negative warm-up': ({'kind': 'constant', 'warmup_steps': -1}, 'warmup_steps'),
    'fractional warm-up': ({'kind': 'constant', 'warmup_steps': 2.5}, 'warmup_steps'),
    'no decay_steps': ({'kind': 'cosine'}, 'decay_steps'),
    'decay_steps 0': ({'kind': 'exponential', 'decay_steps': 0, 'decay_rate': 0.5}, 'decay_steps'),
    'no decay_rate': ({'kind': 'exponential', 'decay_steps': 5}, 'decay_rate'),
    'decay_rate 0': ({'kind': 'exponential', 'decay_steps': 5, 'decay_rate': 0.0}, 'decay_rate'),
    'decay_rate NaN': ({'kind': 'exponential', 'decay_steps': 5, 'decay_rate': float('nan')}, 'decay_rate'),
    'decay_rate below float32': ({'kind': 'exponential', 'decay_steps': 5, 'decay_rate': 1e-60}, 'decay_rate'),
    'staircase a number': ({'kind': 'exponential', 'decay_steps': 5, 'decay_rate': 0.5, 'staircase': 2}, 'staircase'),
    'alpha 1.5': ({'kind': 'cosine', 'decay_steps': 5, 'alpha': 1.5}, 'alpha'),
    'alpha negative': ({'kind': 'cosine', 'decay_steps': 5, 'alpha': -0.5}, 'alpha'),
    '9 boundaries': ({'kind': 'piecewise', 'boundaries': list(range(9)), 'values': [1e-3] * 10}, 'boundaries'),
    'equal boundaries': ({'kind': 'piecewise', 'boundaries': [3, 3], 'values': [1e-3] * 3}, 'boundaries'),
    'fractional boundary': ({'kind': 'piecewise', 'boundaries': [3.5], 'values': [1e-3] * 2}, 'boundaries'),
    'too few values': ({'kind': 'piecewise', 'boundaries': [3, 4], 'values': [1e-3] * 2}, 'values'),
    'no values': ({'kind': 'piecewise', 'boundaries': [3, 4]}, 'values'),
    'negative value': ({'kind': 'piecewise', 'boundaries': [3], 'values': [1e-3, -1e-3]}, 'values'),
    'infinite value': ({'kind': 'piecewise', 'boundaries': [3], 'values': [float('inf'), 1e-3]}, 'values'),
}


@pytest.mark.parametrize('case', list(BAD))
def test_bad_lr_schedule_is_refused_by_key_and_field(case):
  """check_lr_schedule, a model and the Estimator (at construction) all refuse it, naming the key and the field."""
  from geeco_amd import estimator as est
  from geeco_amd import graph
  from geeco_amd.params import create_e2evmc_config
  from geeco_amd.variables import check_lr_schedule
  bad, field = BAD[case]
  with pytest.raises(ValueError, match='lr_schedule.*' + field):
    check_lr_schedule(bad, 1e-3)
  cfg = create_e2evmc_config(dict(window_size=2, img_height=136, img_width=136))
  with pytest.raises(ValueError, match='lr_schedule.*' + field):
    graph.E2EVMC(cfg, 2, 'cpu', lr_schedule=bad)
  with pytest.raises(ValueError, match=r"params\['lr_schedule'\].*" + field):
    est.Estimator(est.e2evmc_model_fn, None, est.RunConfig(), {'lr_schedule': bad, 'e2evmc_config': cfg})
  with pytest.raises(ValueError, match=r"params\['lr_schedule'\].*" + field):
    est.Estimator(est.goal_e2evmc_model_fn, None, est.RunConfig(), {'lr_schedule': bad})


def test_bad_base_lr_is_refused_and_good_schedules_are_taken():
  from geeco_amd import estimator as est
  from geeco_amd import graph
  from geeco_amd.params import create_e2evmc_config
  from geeco_amd.variables import check_lr_schedule
  for lr in (-1e-3, float('nan'), float('inf'), 'fast', True):
    with pytest.raises(ValueError, match='lr_schedule.*base_lr'):
      check_lr_schedule({'kind': 'cosine', 'decay_steps': 3}, lr)
  cfg = create_e2evmc_config(dict(window_size=2, img_height=136, img_width=136, lr=-1.0))
  with pytest.raises(ValueError, match='lr_schedule.*base_lr'):
    graph.GoalE2EVMC(cfg, 2, 'cpu', lr_schedule={'kind': 'cosine', 'decay_steps': 3})
  est.Estimator(est.e2evmc_model_fn, None, est.RunConfig(), {'lr_schedule': {'kind': 'cosine', 'decay_steps': 3}})
  est.Estimator(est.e2evmc_model_fn, None, est.RunConfig(), {'lr_schedule': None})
  est.Estimator(est.e2evmc_model_fn, None, est.RunConfig(), {'lr_schedule': {'kind': 'constant'}})


def test_cli_flags_reach_params():
  spec = importlib.util.spec_from_file_location('train_e2evmc_cli_lr', os.path.join(ROOT, 'scripts', 'train_e2evmc.py'))
  cli = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(cli)
  from geeco_amd.variables import check_lr_schedule

  def params(*argv):
    return cli.estimator_params(cli.ARGPARSER.parse_args(list(argv)), 'CFG')

  assert 'lr_schedule' not in params()
  assert params('--lr_schedule', 'cosine', '--lr_warmup_steps', '2', '--lr_decay_steps', '4')['lr_schedule'] == \
      {'kind': 'cosine', 'warmup_steps': 2, 'decay_steps': 4, 'alpha': 0.0}
  assert params('--lr_schedule', 'cosine', '--lr_decay_steps', '4', '--lr_alpha', '0.25')['lr_schedule']['alpha'] == 0.25
  assert params('--lr_schedule', 'exponential', '--lr_decay_steps', '1000', '--lr_decay_rate', '0.96', '--lr_staircase')['lr_schedule'] == \
      {'kind': 'exponential', 'warmup_steps': 0, 'decay_steps': 1000, 'decay_rate': 0.96, 'staircase': True}
  pw = params('--lr_schedule', 'piecewise', '--lr_boundaries', '100,200', '--lr_values', '1e-3,1e-4,1e-5', '--lr_warmup_steps', '10')
  assert pw['lr_schedule'] == {'kind': 'piecewise', 'warmup_steps': 10, 'boundaries': [100, 200], 'values': [1e-3, 1e-4, 1e-5]}
  assert params('--lr_schedule', 'constant', '--lr_warmup_steps', '5')['lr_schedule'] == {'kind': 'constant', 'warmup_steps': 5}
  for p in (pw, params('--lr_schedule', 'constant', '--lr_warmup_steps', '5')):
    assert check_lr_schedule(p['lr_schedule'], 1e-3) is not None
  assert check_lr_schedule(params('--lr_schedule', 'constant')['lr_schedule'], 1e-3) is None
  with pytest.raises(ValueError, match='decay_steps'):      # a kind without the flag it needs is refused by name
    check_lr_schedule(params('--lr_schedule', 'cosine')['lr_schedule'], 1e-3, "params['lr_schedule']")
  from geeco_amd.params import create_e2evmc_config
  assert 'lr_schedule' not in create_e2evmc_config({})._asdict()      # not a field of the model config


@pytest.mark.parametrize('name', NEW)
def test_header_and_binding_agree(name):
  from geeco_amd import _native
  assert len(_native.SIGNATURES[name][1]) == len(_abi.functions()[name][1])      # (every type: test_abi_cpu.py::test_signature_matches_the_header)
  assert hasattr(_native.load(), name)


def test_struct_and_header_agree():
  """geeco_lr_schedule field by field: names, order, types and array lengths; the kinds in the header's order."""
  from geeco_amd import _native, variables
  assert _abi.define('GEECO_LR_BOUNDARIES_MAX') == _native.LR_BOUNDARIES_MAX == variables.LR_BOUNDARIES_MAX == 8
  types = {'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float}
  want = [(field, types[ctype] * length if length else types[ctype]) for field, ctype, length in _abi.struct_fields('geeco_lr_schedule')]
  assert _native.LrSchedule._fields_ == want
  assert ctypes.sizeof(_native.LrSchedule) == 144
  for i, kind in enumerate(_native.LR_KINDS):
    assert _abi.define('GEECO_LR_' + kind.upper()) == i, kind
  assert _native.LR_KINDS == variables.LR_KINDS


def test_abi_version_is_unchanged_and_the_additions_are_listed():
  from geeco_amd import _native
  assert _abi.define('GEECO_ABI_VERSION') == 7 == _native.ABI_VERSION
  assert set(NEW) <= set(_abi.added_within(7))
