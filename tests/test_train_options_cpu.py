"""The record of the training options (geeco_amd/train_options.py): ``TrainOptions.from_raw`` against the ``check_*`` functions under
both key wordings, each check run once per construction, the exclusion table against a restatement of the rules the three former sites
held (Estimator model_fn, TrainStepRunner, the model's constructor), the mode rule, and the constructors' signatures.  No GPU.

The accepted and refused values are those of the per-option files (test_ema_cpu.py, test_clip_cpu.py, test_lr_schedule_cpu.py,
test_skip_nonfinite_cpu.py, test_finetune_cpu.py, test_variable_stats_cpu.py, test_loss_shaping_cpu.py, test_grad_accum_cpu.py)."""
import inspect
import itertools

import numpy as np
import pytest

from geeco_amd import train_options as T
from geeco_amd.params import create_e2evmc_config
from geeco_amd.variables import model_variable_shapes

NAN, INF = float('nan'), float('inf')
CFG = create_e2evmc_config(dict(window_size=2, img_height=136, img_width=136))
NAMES = list(model_variable_shapes(CFG, False))
KEYS = (T.KEYWORD, T.PARAMS)

# public name -> (accepted raw values, refused raw values)
VALUES = {
    'ema_decay': ([None, 0, 0.0, 0.999, np.float32(0.5)], [1.0, 1, -0.5, 1.5, NAN, 'fast', True, [0.9]]),
    'clip_norm': ([None, 0, 0.0, 5, np.float32(0.5), 1e30, 1e-30], [-1.0, -0.0001, NAN, INF, -INF, 1e39, 1e-46, 'tight', True, False, [5.0]]),
    'lr_schedule': (
        [None, {'kind': 'constant'}, {'kind': 'constant', 'warmup_steps': 3},
         {'kind': 'exponential', 'decay_steps': np.int64(9), 'decay_rate': 0.5, 'staircase': True},
         {'kind': 'cosine', 'decay_steps': 4, 'warmup_steps': 2}, {'kind': 'cosine', 'decay_steps': 4, 'alpha': 1},
         {'kind': 'piecewise', 'boundaries': [2, 5], 'values': [1e-3, 1e-4, 1e-5]}, {'kind': 'piecewise', 'values': [1e-3]}],
        ['cosine', 0.5, {'decay_steps': 3}, {'kind': 'linear'}, {'kind': 'cosine', 'decay_steps': 3, 'power': 2},
         {'kind': 'constant', 'warmup_steps': -1}, {'kind': 'constant', 'warmup_steps': 2.5}, {'kind': 'cosine'},
         {'kind': 'exponential', 'decay_steps': 0, 'decay_rate': 0.5}, {'kind': 'exponential', 'decay_steps': 5},
         {'kind': 'exponential', 'decay_steps': 5, 'decay_rate': 0.0}, {'kind': 'exponential', 'decay_steps': 5, 'decay_rate': NAN},
         {'kind': 'exponential', 'decay_steps': 5, 'decay_rate': 1e-60},
         {'kind': 'exponential', 'decay_steps': 5, 'decay_rate': 0.5, 'staircase': 2}, {'kind': 'cosine', 'decay_steps': 5, 'alpha': 1.5},
         {'kind': 'cosine', 'decay_steps': 5, 'alpha': -0.5}, {'kind': 'piecewise', 'boundaries': list(range(9)), 'values': [1e-3] * 10},
         {'kind': 'piecewise', 'boundaries': [3, 3], 'values': [1e-3] * 3}, {'kind': 'piecewise', 'boundaries': [3.5], 'values': [1e-3] * 2},
         {'kind': 'piecewise', 'boundaries': [3, 4], 'values': [1e-3] * 2}, {'kind': 'piecewise', 'boundaries': [3, 4]},
         {'kind': 'piecewise', 'boundaries': [3], 'values': [1e-3, -1e-3]}, {'kind': 'piecewise', 'boundaries': [3], 'values': [INF, 1e-3]}]),
    'skip_nonfinite': ([None, False, True, 1, 7, 250, np.int64(12)], [0, -1, 1.0, 2.5, NAN, INF, 'yes', [3], (1,), {}]),
    'lr_multipliers': (
        [None, {}, {'conv': 1, 'LSTM': 1.0}, {'conv1': 1.0}, {'/conv1/kernel$': 0, 'conv1': 0.5, 'Encoder/': 0.1}, {'fc1': 3}],
        [{'conv1': bad} for bad in (-1.0, NAN, INF, True, '0.1', 1e39, None)] +
        [{'conv1': 0, 'conv9': 0.5}, {'conv(': 0.5}, [('conv1', 0.5)], 0.5]),
    'variable_stats': ([None, False, True, 'histograms'], [0, 1, 2.0, 'yes', 'scalars', 'histogram', [True], {}, 'all']),
    'loss_shaping': (
        [None, {}, {'sample_weights': False}, {'grp_class_weights': [1, 1.0, 1]}, {'label_smoothing': 0.0}, {'huber_delta': None},
         {'sample_weights': False, 'grp_class_weights': (1.0, 1.0, 1.0), 'label_smoothing': 0, 'huber_delta': {}},
         {'sample_weights': True, 'grp_class_weights': [1, 0.25, 2], 'label_smoothing': 0.1, 'huber_delta': 0.5},
         {'huber_delta': {'pos_obj': 2}}, {'grp_class_weights': np.array([0.0, 1.0, 1.0])}],
        ['huber', 1.0, [('huber_delta', 1.0)], {'hubber_delta': 1.0}, {'sample_weights': 1}, {'sample_weights': 'yes'},
         {'grp_class_weights': [1, 2]}, {'grp_class_weights': [1, 2, 3, 4]}, {'grp_class_weights': [1, -0.5, 1]},
         {'grp_class_weights': [1, NAN, 1]}, {'grp_class_weights': [1, INF, 1]}, {'grp_class_weights': '1,2,3'},
         {'grp_class_weights': 2.0}, {'label_smoothing': 1.0}, {'label_smoothing': -0.1}, {'label_smoothing': NAN},
         {'label_smoothing': True}, {'huber_delta': 0.0}, {'huber_delta': -1.0}, {'huber_delta': INF}, {'huber_delta': NAN},
         {'huber_delta': True}, {'huber_delta': {'cmd_vel': 1.0}}, {'huber_delta': {'logits_cmd_grp': 1.0}}, {'huber_delta': {'cmd_ee': 0}},
         {'huber_delta': [1.0]}]),
    'grad_accum_steps': ([None, 1, 2, 7, np.int64(3)], [0, -1, 2.5, True, '2', 2.0, NAN, [2]]),
}
CHECKS = {name: 'check_' + name for name in T.FIELDS}
ALL_ON = {'ema_decay': 0.999, 'clip_norm': 1.0, 'lr_schedule': {'kind': 'cosine', 'decay_steps': 4}, 'skip_nonfinite': True,
          'lr_multipliers': {'conv1': 0.5}, 'variable_stats': True, 'loss_shaping': {'huber_delta': 0.5}, 'grad_accum_steps': 2}


def _check(name, value, key):
  """The option's own check, called as the record's constructor must call it."""
  fn, k = getattr(T, CHECKS[name]), key % name
  extra = {'lr_schedule': (CFG.lr,), 'lr_multipliers': (NAMES,), 'loss_shaping': (CFG,)}.get(name, ())
  return fn(value, *extra, k)


def test_the_record_names_every_option_and_nothing_is_on_by_default():
  assert list(T.FIELDS) == ['ema_decay', 'clip_norm', 'lr_schedule', 'skip_nonfinite', 'lr_multipliers', 'variable_stats', 'loss_shaping',
                            'grad_accum_steps'] == list(VALUES)
  assert T.TrainOptions._fields == ('ema_decay', 'clip_norm', 'lr_schedule', 'skip_limit', 'lr_multipliers', 'variable_stats_mode',
                                    'loss_shaping', 'grad_accum')
  assert all(v is None for v in T.TrainOptions()) and T.TrainOptions.from_raw({}, CFG, NAMES) == T.TrainOptions()
  with pytest.raises(AttributeError):
    T.TrainOptions().clip_norm = 1.0


@pytest.mark.parametrize('key', KEYS)
@pytest.mark.parametrize('name', list(VALUES))
def test_the_constructor_yields_what_the_check_yields(name, key):
  accepted, refused = VALUES[name]
  for value in accepted:
    want = _check(name, value, key)
    got = T.TrainOptions.from_raw({name: value}, CFG, NAMES, key)
    assert getattr(got, T.FIELDS[name]) == want and type(getattr(got, T.FIELDS[name])) is type(want), (value, got)
    assert got == T.TrainOptions(**{T.FIELDS[name]: want})      # ... and no other field moved
  for value in refused:
    with pytest.raises(ValueError) as want:
      _check(name, value, key)
    assert key % name in str(want.value)
    with pytest.raises(ValueError) as got:
      T.TrainOptions.from_raw({name: value}, CFG, NAMES, key)
    assert str(got.value) == str(want.value), value


def test_from_params_picks_the_options_and_words_them_as_params():
  got = T.TrainOptions.from_params(dict(ALL_ON, e2evmc_config=CFG, shared_frames=True, log_steps=5), CFG, NAMES)
  assert got == T.TrainOptions.from_raw(ALL_ON, CFG, NAMES, T.PARAMS) and None not in got
  with pytest.raises(ValueError, match=r"params\['clip_norm'\]"):
    T.TrainOptions.from_params({'clip_norm': -1.0}, CFG, NAMES)
  with pytest.raises(TypeError, match='log_steps'):
    T.TrainOptions.from_raw({'log_steps': 5}, CFG, NAMES)
  # a model that is not training: the three training-only options are neither checked nor kept
  bad = dict(ALL_ON, lr_multipliers=0.5, variable_stats='all', grad_accum_steps=0)
  assert T.TrainOptions.from_raw(bad, CFG, NAMES, training=False) == got._replace(lr_multipliers=None, variable_stats_mode=None, grad_accum=None)


def test_each_check_runs_once_per_construction(monkeypatch):
  from geeco_amd import estimator as est
  counts = dict.fromkeys(VALUES, 0)

  def counted(name, fn):
    def f(*a, **k):
      counts[name] += 1
      return fn(*a, **k)
    return f
  for name in VALUES:
    monkeypatch.setattr(T, CHECKS[name], counted(name, getattr(T, CHECKS[name])))
  # the Estimator does not know the model's variables yet: lr_multipliers gets the mapping check alone, not its check_*
  e = est.Estimator(est.e2evmc_model_fn, None, est.RunConfig(), dict(ALL_ON, e2evmc_config=CFG))
  assert counts == dict(dict.fromkeys(VALUES, 1), lr_multipliers=0), counts
  assert e.options.grad_accum == 2 and e.options.skip_limit == 100 and e.options.lr_multipliers is None
  with pytest.raises(ValueError, match=r"params\['lr_multipliers'\]=0.5: must be None or a mapping"):
    est.Estimator(est.e2evmc_model_fn, None, est.RunConfig(), {'lr_multipliers': 0.5})
  # without a config: the schedule against lr 0.0, loss_shaping not at all
  counts.update(dict.fromkeys(VALUES, 0))
  est.Estimator(est.e2evmc_model_fn, None, est.RunConfig(), dict(ALL_ON, loss_shaping='unchecked'))
  assert counts == dict(dict.fromkeys(VALUES, 1), lr_multipliers=0, loss_shaping=0), counts
  # the record model_fn makes
  counts.update(dict.fromkeys(VALUES, 0))
  T.TrainOptions.from_params(dict(ALL_ON, e2evmc_config=CFG), CFG, NAMES)
  assert counts == dict.fromkeys(VALUES, 1), counts


# ================================================================================================
# the exclusion table
# ================================================================================================
ALONE = [(name, {name: ALL_ON[name]}) for name in VALUES if name != 'loss_shaping'] + [
    ('loss_shaping', {'loss_shaping': shaping}) for shaping in (
        {'sample_weights': True}, {'grp_class_weights': [1, 0.25, 2]}, {'sample_weights': True, 'grp_class_weights': [1, 0.25, 2]},
        {'label_smoothing': 0.1}, {'huber_delta': 0.5})] + [(None, {})]


def _former_rule(name, raw, world, dp, shared, key):
  """What the three sites refused before there was a table, as the text the tests matched (None: nothing was refused): model_fn's
  single-GPU rules by world size, TrainStepRunner's two for the forced data-parallel step, and lr_multipliers x shared_frames."""
  ranks = 'with %d ranks' % world if world > 1 else ''
  weighted = [e for e in ('sample_weights', 'grp_class_weights') if name == 'loss_shaping' and raw[name].get(e)]
  if (name in ('lr_multipliers', 'grad_accum_steps') and (world > 1 or dp)) or (name == 'variable_stats' and world > 1):
    return ['%s is single-GPU' % (key % name), ranks]
  if weighted and world > 1:
    return ['%s[%s] is single-GPU' % (key % name, '], ['.join(repr(e) for e in weighted)), ranks]
  if name == 'lr_multipliers' and shared:
    return ['%s with %s' % (key % name, key % 'shared_frames')]
  if shared and world > 1:
    return ['%s is single-GPU' % (key % 'shared_frames'), ranks]
  return None


@pytest.mark.parametrize('key', KEYS)
def test_the_table_refuses_what_the_three_sites_refused_and_nothing_else(key):
  refused = 0
  for (name, raw), world, dp, shared in itertools.product(ALONE, (1, 2), (False, True), (False, True)):
    options = T.TrainOptions.from_raw(raw, CFG, NAMES, key)
    want = _former_rule(name, raw, world, dp, shared, key)
    case = (raw, world, dp, shared)
    if want is None:
      T.check_exclusions(options, world, dp, shared, key)
      continue
    refused += 1
    with pytest.raises(ValueError) as e:
      T.check_exclusions(options, world, dp, shared, key)
    assert all(text in str(e.value) for text in want), (case, str(e.value))
    reasons = [reason for _, _, _, reason in T.EXCLUSIONS if str(e.value).endswith(reason)]
    assert len(reasons) == 1, (case, str(e.value))      # the rest of the message is one row's reason
  assert refused == 43      # 7 lr_multipliers, 6 grad_accum_steps, 4 variable_stats, 3 x 4 weighted losses, 7 x 2 shared_frames alone


def test_the_table_names_every_single_gpu_option_once():
  rows = [(name, entries, what) for name, entries, what, _ in T.EXCLUSIONS]
  assert sorted(r for r in rows if r[2] != 'shared_frames') == sorted([
      ('lr_multipliers', None, 'dp'), ('grad_accum_steps', None, 'dp'), ('variable_stats', None, 'ranks'),
      ('loss_shaping', ('sample_weights', 'grp_class_weights'), 'ranks'), ('shared_frames', None, 'ranks')])
  assert [r for r in rows if r[2] == 'shared_frames'] == [('lr_multipliers', None, 'shared_frames')]
  assert len({reason for _, _, _, reason in T.EXCLUSIONS}) == len(T.EXCLUSIONS)
  # the texts the GPU tests match
  with pytest.raises(ValueError, match=r"params\['loss_shaping'\]\['sample_weights'\] is single-GPU: with 2 ranks"):
    T.check_exclusions(T.TrainOptions.from_raw({'loss_shaping': {'sample_weights': True}}, CFG, NAMES), 2, key=T.PARAMS)
  with pytest.raises(ValueError, match='lr_multipliers with shared_frames'):
    T.check_exclusions(T.TrainOptions.from_raw({'lr_multipliers': {'conv1': 0}}, CFG, NAMES), shared_frames=True)
  with pytest.raises(ValueError, match='grad_accum_steps is single-GPU'):
    T.check_exclusions(T.TrainOptions.from_raw({'grad_accum_steps': 2}, CFG, NAMES), dp=True)


# ================================================================================================
# modes and constructors
# ================================================================================================
def test_the_mode_rule():
  from geeco_amd.estimator import ModeKeys
  full = T.TrainOptions.from_raw(ALL_ON, CFG, NAMES)
  assert full.for_mode(ModeKeys.TRAIN) is full
  assert full.for_mode(ModeKeys.EVAL) == T.TrainOptions(loss_shaping=full.loss_shaping) and full.loss_shaping is not None
  assert full.for_mode(ModeKeys.PREDICT) == T.TrainOptions()


def test_the_constructors_take_options_and_refuse_unknown_names():
  from geeco_amd import graph
  with pytest.raises(TypeError, match='no_such_option'):
    graph.E2EVMC(CFG, 2, 'cpu', no_such_option=1)
  with pytest.raises(TypeError, match='no_such_option'):
    graph.GoalE2EVMC(CFG, 2, 'cpu', no_such_option=1)
  for ctor in (graph._ModelBase, graph.GoalE2EVMC, graph.E2EVMC):
    sig = inspect.signature(ctor.__init__)
    assert not set(sig.parameters) & set(T.FIELDS), ctor
    assert any(p.kind is p.VAR_KEYWORD for p in sig.parameters.values()), ctor


def test_a_model_keeps_the_record_and_its_attributes():
  from geeco_amd import graph
  raw = dict(ALL_ON, ema_decay=None)
  full = T.TrainOptions.from_raw(raw, CFG, NAMES)
  m = graph.E2EVMC(CFG, 2, 'cpu', **raw)
  assert m.options == full and graph.E2EVMC(CFG, 2, 'cpu', options=full).options is full      # a checked record is taken as it is, alone
  with pytest.raises(TypeError, match='clip_norm'):
    graph.E2EVMC(CFG, 2, 'cpu', options=full, clip_norm=1.0)
  for field in T.TrainOptions._fields:
    assert getattr(m, field) == getattr(full, field), field
  assert m.lr_runs and m.backward_cut == 'full' and m.clip_ws is not None and m.clip_out is not None and m.guard is not None
  assert m.stats_plan is not None and m.store.accum is not None
  # a model that is not training: the option's values as far as an inference model has them, and none of the step's buffers
  e = graph.E2EVMC(CFG, 2, 'cpu', training=False, **dict(raw, variable_stats='all', grad_accum_steps=0))      # (ignored, as ever)
  assert graph.E2EVMC(CFG, 2, 'cpu', training=False, options=full).options == e.options
  assert e.options == full._replace(lr_multipliers=None, variable_stats_mode=None, grad_accum=None)
  assert (e.clip_norm, e.skip_limit, e.lr_schedule, e.loss_shaping) == (1.0, 100, full.lr_schedule, full.loss_shaping)
  assert (e.lr_multipliers, e.variable_stats_mode, e.grad_accum, e.lr_runs, e.backward_cut) == (None, None, None, None, 'full')
  assert e.clip_ws is None and e.clip_out is None and e.guard is None and e.stats_plan is None and e.store.accum is None
  plain = graph.E2EVMC(CFG, 2, 'cpu')
  assert plain.options == T.TrainOptions() and plain.clip_ws is None and plain.lr_runs is None and plain.stats_plan is None
