"""Fine-tuning, the host side: the multiplier table, the runs of the arena, the cut point of the backward, the argument
checks of geeco_adam_tf_segments_scaled, warm start on a CPU VariableStore, and the command line.  No GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import _finetune_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(**kw):
  from geeco_amd.params import create_e2evmc_config
  return create_e2evmc_config(dict(window_size=2, img_height=F.H, img_width=F.H, batch_size=2, **kw))


LAYOUTS = {
    'e2e_vmc': (False, {}),
    'geeco-f': (True, dict(proc_obs='dynimg', proc_tgt='dyndiff')),
    'geeco-f 256/128/64': (True, dict(proc_obs='dynimg', proc_tgt='dyndiff', dim_s_obs=256, dim_s_dyn=128, dim_s_diff=64)),
    'goal seq dyndiff 128/64': (True, dict(proc_obs='sequence', proc_tgt='dyndiff', dim_s_obs=128, dim_s_diff=64)),
}


def _store(layout):
  from geeco_amd.graph import build_store
  goal, extra = LAYOUTS[layout]
  return build_store(_cfg(**extra), goal, 'cpu')


# ================================================================================================
# check_lr_multipliers
# ================================================================================================
NAMES = ['VMC/ConvEncoder/conv1/kernel', 'VMC/ConvEncoder/conv1/bias', 'VMC/ConvEncoder/conv3/kernel', 'VMC/LSTMDecoder/fc1/kernel']


def test_the_off_forms_and_all_ones():
  from geeco_amd.variables import check_lr_multipliers
  assert check_lr_multipliers(None, NAMES) is None
  assert check_lr_multipliers({}, NAMES) is None
  assert check_lr_multipliers({'conv': 1, 'LSTM': 1.0}, NAMES) is None
  assert check_lr_multipliers({'conv1': 1.0}, NAMES) is None


def test_the_first_match_wins_and_the_unmatched_run_at_one():
  from geeco_amd.variables import check_lr_multipliers
  got = check_lr_multipliers({'/conv1/kernel$': 0, 'conv1': 0.5, 'Encoder/': 0.1}, NAMES)
  assert list(got) == NAMES
  assert got == {NAMES[0]: 0.0, NAMES[1]: 0.5, NAMES[2]: float(np.float32(0.1)), NAMES[3]: 1.0}
  assert got == F.multipliers({'/conv1/kernel$': 0, 'conv1': 0.5, 'Encoder/': 0.1}, NAMES)
  # re.search, not re.match: the pattern may sit anywhere in the name
  assert check_lr_multipliers({'fc1': 3}, NAMES)[NAMES[3]] == 3.0


@pytest.mark.parametrize('bad', [-1.0, float('nan'), float('inf'), True, '0.1', 1e39, None])
def test_bad_multipliers_are_rejected_with_the_key(bad):
  from geeco_amd.variables import check_lr_multipliers
  with pytest.raises(ValueError, match=r"params\['lr_multipliers'\].*conv1"):
    check_lr_multipliers({'conv1': bad}, NAMES, "params['lr_multipliers']")


def test_a_pattern_that_matches_nothing_and_other_bad_tables_are_rejected():
  from geeco_amd.variables import check_lr_multipliers
  with pytest.raises(ValueError, match=r'lr_multipliers.*conv9.*matches no variable'):
    check_lr_multipliers({'conv1': 0, 'conv9': 0.5}, NAMES)
  with pytest.raises(ValueError, match='not a regular expression'):
    check_lr_multipliers({'conv(': 0.5}, NAMES)
  with pytest.raises(ValueError, match='mapping'):
    check_lr_multipliers([('conv1', 0.5)], NAMES)
  with pytest.raises(ValueError, match='mapping'):
    check_lr_multipliers(0.5, NAMES)


# ================================================================================================
# runs
# ================================================================================================
TABLES = {
    'encoders x 0.1': {'Encoder/': 0.1},
    'bottom frozen': {'/conv[12]/': 0},
    'encoders frozen': {'Encoder/': 0},
    'three rates': {'/conv[12]/': 0, 'Encoder/conv8': 2.0, 'Encoder/': 0.1, 'fc1': 0.5},
}


@pytest.mark.parametrize('table', list(TABLES))
@pytest.mark.parametrize('layout', list(LAYOUTS))
def test_runs_against_the_reference_rule(layout, table):
  """Pads are absorbed (the element-wise reference gives every pad float to the variable in front of it), offsets and counts are
  multiples of 4, runs are disjoint, ascending, inside the arena, and no frozen float is in one."""
  from geeco_amd.variables import check_lr_multipliers, lr_multiplier_runs
  store = _store(layout)
  mults = check_lr_multipliers(TABLES[table], store.shapes)
  assert mults == F.multipliers(TABLES[table], store.shapes)
  got = lr_multiplier_runs(store.offsets, store.size, mults)
  assert got == F.runs(dict(store.offsets), store.size, mults)
  end = 0
  for off, cnt, mul in got:
    assert off % 4 == 0 and cnt % 4 == 0 and cnt >= 4 and off >= end and mul > 0.0
    end = off + cnt
  assert end <= store.size
  covered = np.zeros(store.size, bool)
  for off, cnt, _ in got:
    covered[off:off + cnt] = True
  for n, shp in store.shapes.items():
    o, c = store.offsets[n], int(np.prod(shp))
    assert covered[o:o + c].all() == (mults[n] != 0.0) and covered[o:o + c].any() == (mults[n] != 0.0), n
  # a layout with uniform-stride pads has them: the test would not see a pad handled wrongly otherwise
  if layout == 'geeco-f 256/128/64':
    assert store.size > sum(-(-int(np.prod(s)) // 4) * 4 for s in store.shapes.values())


def test_bottom_frozen_geeco_f_is_three_runs_and_the_models_limit():
  from geeco_amd.variables import check_lr_multipliers, lr_multiplier_runs
  store = _store('geeco-f')
  runs = lr_multiplier_runs(store.offsets, store.size, check_lr_multipliers({'/conv[12]/': 0}, store.shapes))
  assert len(runs) == 3 and all(mul == 1.0 for _, _, mul in runs)
  assert runs[0][0] == store.offsets['GoalVMC/ConvEncoder/conv3/kernel'] and runs[2][0] + runs[2][1] == store.size
  # every second layer of three encoders at its own rate: more runs than one launch takes
  mults = check_lr_multipliers({'/conv[1357]/': 0.5}, store.shapes)
  assert len(lr_multiplier_runs(store.offsets, store.size, mults)) > 8


def test_a_table_that_needs_more_than_eight_pieces_raises(monkeypatch):
  """The model's constructor refuses it with the count (no GPU: the check comes before any device buffer beyond the store)."""
  from geeco_amd import graph
  cfg = _cfg(proc_obs='dynimg', proc_tgt='dyndiff')
  with pytest.raises(ValueError, match=r'lr_multipliers.*into \d+ runs.*at most 8'):
    graph.GoalE2EVMC(cfg, 2, 'cpu', training=True, lr_multipliers={'/conv[1357]/': 0.5})
  with pytest.raises(ValueError, match='nothing to train'):
    graph.GoalE2EVMC(cfg, 2, 'cpu', training=True, lr_multipliers={'.': 0})


# ================================================================================================
# the cut point of the backward
# ================================================================================================
@pytest.mark.parametrize('table, want', [
    ({'Encoder/': 0, 'DynBuffEncoder/conv2/bias': 0.5}, 'decoder_only'),  # (listed behind 'Encoder/': it never applies ...)
    ({'DynBuffEncoder/conv2/bias': 0.5, 'Encoder/': 0}, 'full'),          # ... here it does: ONE trainable conv2 bias of ONE encoder
    ({'/conv[12]/': 0}, 'no_bottom'),
    ({'/conv[12]/': 0, 'Encoder/': 0.1}, 'no_bottom'),
    ({'/conv[12]/kernel': 0}, 'full'),                                     # the biases are still trained
    ({'ConvEncoder/conv[12]/': 0}, 'full'),                                # conv1 / conv2 of ONE encoder only
    ({'Encoder/': 0}, 'decoder_only'),
    ({'Encoder/': 0, 'lstm_cell': 0.5}, 'decoder_only'),
    ({'Encoder/': 0.1}, 'full'),
])
def test_the_cut_point(table, want):
  from geeco_amd.variables import backward_cut, check_lr_multipliers
  store = _store('geeco-f')
  mults = check_lr_multipliers(table, store.shapes)
  assert backward_cut(mults) == want == F.cut(mults)
  assert backward_cut(None) == 'full'


# ================================================================================================
# geeco_adam_tf_segments_scaled: what is refused before any launch
# ================================================================================================
def test_host_side_argument_checks_of_the_scaled_update_need_no_gpu():
  from geeco_amd import _native
  lib = _native.load()
  one = ctypes.c_void_p(64)

  def call(p=one, m=one, v=one, scal=one, segs=((64, 0, 8),), mul=(1.0,), nseg=None, ema=None, step=None, decay=0.0, lr_mul_null=False):
    arr = (_native.AdamSegment * max(len(segs), 1))()
    for a, (g, off, cnt) in zip(arr, segs):
      a.g, a.p_off, a.count = g, off, cnt
    muls = (ctypes.c_float * max(len(mul), 1))(*mul)
    rc = lib.geeco_adam_tf_segments_scaled(p, None, m, v, ema, arr, None if lr_mul_null else muls, len(segs) if nseg is None else nseg, scal,
                                           step, decay, None, None, 0.9, 0.999, 1e-8, 1.0, 0.0, None)
    return rc, lib.geeco_last_error()

  for kw in (dict(p=None), dict(m=None), dict(v=None), dict(scal=None), dict(lr_mul_null=True), dict(nseg=0), dict(nseg=9)):
    rc, msg = call(**kw)
    assert rc == _native.GEECO_EINVAL and b'adam_tf_segments_scaled' in msg and b'1..8 pieces' in msg, (kw, msg)
  rc, msg = call(segs=((64, 2, 8),))
  assert rc == _native.GEECO_EINVAL and b'adam_tf_segments_scaled: piece 0' in msg and b'multiple of 4' in msg
  rc, msg = call(segs=((68, 0, 8),))
  assert rc == _native.GEECO_EINVAL and b'16-byte aligned' in msg
  rc, msg = call(segs=((None, 0, 8),))
  assert rc == _native.GEECO_EINVAL and b'piece 0' in msg
  rc, msg = call(p=ctypes.c_void_p(68))
  assert rc == _native.GEECO_EINVAL and b'arenas must be 16-byte aligned' in msg
  for bad in (0.0, -0.5, float('nan'), float('inf')):
    rc, msg = call(segs=((64, 0, 8), (64, 8, 8)), mul=(1.0, bad))
    assert rc == _native.GEECO_EINVAL and b'adam_tf_segments_scaled: piece 1' in msg and b'multiplier' in msg, (bad, msg)
  rc, msg = call(ema=one, decay=0.9)
  assert rc == _native.GEECO_EINVAL and b'step counter' in msg
  rc, msg = call(ema=one, step=one, decay=1.0)
  assert rc == _native.GEECO_EINVAL and b'decay' in msg


# ================================================================================================
# warm start
# ================================================================================================
def _trained_store(layout, seed, step=7):
  s = _store(layout)
  s.initialize(seed=seed)
  s.adam_m.fill_(0.25)
  s.adam_v.fill_(0.5)
  s.global_step.fill_(step)
  return s


def _save(store, model_dir, fmt):
  from geeco_amd import estimator as est
  os.makedirs(model_dir, exist_ok=True)
  prefix = est.save_checkpoint(store, model_dir, 5, tf_bundle=(fmt == 'tf'))
  if fmt == 'tf':
    os.remove(prefix + '.pt')      # the TF bundle alone, as the published weights come
  return prefix


@pytest.mark.parametrize('fmt', ['pt', 'tf'])
def test_warm_start_a_subset_under_a_prefix_map(tmp_path, fmt):
  """geeco-f from an e2e_vmc checkpoint: GoalVMC/ConvEncoder takes VMC/ConvEncoder's weights, everything else keeps its fresh
  initialisation; moments and the step counter are zero afterwards and the shadow arena restarts from the parameters."""
  from geeco_amd import estimator as est
  from geeco_amd.graph import build_store
  old = _trained_store('e2e_vmc', seed=3)
  md = str(tmp_path / 'old')
  prefix = _save(old, md, fmt)
  goal, extra = LAYOUTS['geeco-f']
  new = build_store(_cfg(**extra), goal, 'cpu', ema=True)
  new.initialize(seed=9)
  new.adam_m.fill_(1.0)
  new.global_step.fill_(3)
  fresh = new.to_numpy('params')
  settings = dict(ckpt=md, vars=r'^GoalVMC/ConvEncoder/', name_map={'GoalVMC/ConvEncoder': 'VMC/ConvEncoder'})
  names = est.warm_start(new, settings)
  assert names == [n for n in new.shapes if n.startswith('GoalVMC/ConvEncoder/')] and len(names) == 16
  got, src = new.to_numpy('params'), old.to_numpy('params')
  for n in new.shapes:
    if n in names:
      assert np.array_equal(got[n], src[n.replace('GoalVMC/', 'VMC/')]), n
    else:
      assert np.array_equal(got[n], fresh[n]), n
  assert not new.adam_m.any() and not new.adam_v.any() and int(new.global_step.item()) == 0
  assert torch.equal(new.ema, new.params)
  # a checkpoint prefix works as the directory does
  again = build_store(_cfg(**extra), goal, 'cpu')
  again.initialize(seed=9)
  est.warm_start(again, dict(settings, ckpt=prefix))
  assert torch.equal(again.params, new.params)


@pytest.mark.parametrize('fmt', ['pt', 'tf'])
def test_warm_start_names_what_is_missing_or_misshapen(tmp_path, fmt):
  from geeco_amd import estimator as est
  old = _trained_store('e2e_vmc', seed=3)
  md = str(tmp_path / 'old')
  _save(old, md, fmt)
  new = _store('geeco-f')
  new.initialize(seed=9)
  before = new.params.clone()
  with pytest.raises(KeyError, match='GoalVMC/ConvEncoder/conv1/kernel'):       # no name map: the checkpoint has no GoalVMC scope
    est.warm_start(new, dict(ckpt=md, vars='ConvEncoder'))
  with pytest.raises(ValueError, match=r'GoalVMC/LSTMDecoder/lstm_cell/kernel.*\(\d+, 512\).*\(\d+, 512\)'):
    est.warm_start(new, dict(ckpt=md, vars='lstm_cell/kernel', name_map={'GoalVMC': 'VMC'}))
  assert torch.equal(new.params, before)                                        # a refused warm start touches nothing
  with pytest.raises(FileNotFoundError):
    est.warm_start(new, str(tmp_path / 'nowhere'))
  # a plain path selects every variable: same model, every weight taken
  twin = _store('e2e_vmc')
  twin.initialize(seed=1)
  assert len(est.warm_start(twin, md)) == len(twin.shapes) and torch.equal(twin.params, old.params)
  assert not twin.adam_m.any() and int(twin.global_step.item()) == 0


def test_warm_start_settings_are_validated_with_the_key():
  from geeco_amd import estimator as est
  assert est.check_warm_start(None) is None
  assert est.check_warm_start('/a/b') == {'ckpt': '/a/b', 'vars': '.*', 'name_map': {}}
  for bad in (5, {'vars': '.*'}, {'ckpt': '/a', 'what': 1}, {'ckpt': '/a', 'vars': '('}, {'ckpt': '/a', 'name_map': [1]}):
    with pytest.raises(ValueError, match=r"params\['warm_start_from'\]"):
      est.check_warm_start(bad, "params['warm_start_from']")
  with pytest.raises(ValueError, match=r"params\['warm_start_from'\]"):
    est.Estimator(est.e2evmc_model_fn, None, params={'warm_start_from': 5})
  with pytest.raises(ValueError, match=r"params\['lr_multipliers'\]"):
    est.Estimator(est.e2evmc_model_fn, None, params={'lr_multipliers': 0.5})


def test_a_run_that_resumes_its_own_checkpoint_is_not_warm_started(tmp_path, capsys):
  from geeco_amd import estimator as est
  theirs, ours = _trained_store('e2e_vmc', seed=3), _trained_store('e2e_vmc', seed=4, step=11)
  _save(theirs, str(tmp_path / 'theirs'), 'pt')
  for tag, own in (('fresh', False), ('resumed', True)):
    md = str(tmp_path / tag)
    if own:
      _save(ours, md, 'pt')
    e = est.Estimator(est.e2evmc_model_fn, md, est.RunConfig(init_seed=8), {'warm_start_from': str(tmp_path / 'theirs')})
    e._store = _store('e2e_vmc')
    e._store.initialize(seed=8)
    e._restore_once()
    want = ours if own else theirs
    assert torch.equal(e._store.params, want.params), tag
    assert int(e._store.global_step.item()) == (11 if own else 0)
    assert bool(e._store.adam_m.any()) == own
    out = capsys.readouterr().out
    n = len(e._store.shapes)
    assert ('is ignored' in out) == own and ('warm-started %d of %d' % (n, n) in out) == (not own)


# ================================================================================================
# the command line
# ================================================================================================
def _train_script():
  sys.path.insert(0, os.path.join(ROOT, 'scripts'))
  try:
    import train_e2evmc
  finally:
    sys.path.pop(0)
  return train_e2evmc


def test_the_training_script_parses_the_flags_into_params():
  t = _train_script()
  parse = lambda *argv: t.estimator_params(t.ARGPARSER.parse_args(list(argv)), None)
  assert 'lr_multipliers' not in parse() and 'warm_start_from' not in parse()
  assert list(parse('--lr_multipliers', 'Encoder/=0.1,fc1=2')['lr_multipliers'].items()) == [('Encoder/', 0.1), ('fc1', 2.0)]
  assert list(parse('--freeze_encoder_bottom')['lr_multipliers'].items()) == [('/conv[12]/', 0.0)]
  assert list(parse('--freeze_encoders')['lr_multipliers'].items()) == [('Encoder/', 0.0)]
  both = parse('--freeze_encoder_bottom', '--lr_multipliers', 'Encoder/=0.1')['lr_multipliers']
  assert list(both.items()) == [('/conv[12]/', 0.0), ('Encoder/', 0.1)]      # the shorthand first: the first match wins
  p = parse('--warm_start_from', '/w/model.ckpt-5', '--warm_start_vars', 'ConvEncoder', '--warm_start_map',
            'GoalVMC/ConvEncoder=VMC/ConvEncoder,GoalVMC/LSTMDecoder=VMC/LSTMDecoder')
  assert p['warm_start_from']['ckpt'] == '/w/model.ckpt-5' and p['warm_start_from']['vars'] == 'ConvEncoder'
  assert list(p['warm_start_from']['name_map'].items()) == [('GoalVMC/ConvEncoder', 'VMC/ConvEncoder'),
                                                            ('GoalVMC/LSTMDecoder', 'VMC/LSTMDecoder')]
  assert parse('--warm_start_from', '/w')['warm_start_from'] == {'ckpt': '/w', 'vars': '.*', 'name_map': {}}
  from geeco_amd import estimator as est
  assert est.check_warm_start(p['warm_start_from'])['name_map'] == p['warm_start_from']['name_map']
  for argv in (['--lr_multipliers', 'Encoder/'], ['--lr_multipliers', 'Encoder/=x'], ['--warm_start_map', 'A=B'], ['--warm_start_vars', 'x']):
    with pytest.raises(ValueError):
      parse(*argv)
