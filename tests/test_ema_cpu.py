"""The host side of the opt-in averaged weights: the decay schedule and the recurrence as known answers, the
VariableStore's state-dict forms, the TF bundle's tensor names, the refusals of a bad ``ema_decay`` and the command-line flag."""
import importlib.util
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _store(ema, seed=3):
  from geeco_amd.graph import build_store
  from geeco_amd.params import create_e2evmc_config
  cfg = create_e2evmc_config(dict(window_size=2, img_height=136, img_width=136))
  st = build_store(cfg, False, 'cpu', ema=ema)
  st.initialize(seed=seed)
  return st


def _recur(s, p, decay, t):
  """The update as the kernels evaluate it, in float32: p + (s - p) d_t."""
  from geeco_amd.variables import ema_decay_at
  d = ema_decay_at(decay, t)
  return np.float32(p) + (np.float32(s) - np.float32(p)) * d, d


def test_decay_schedule_known_answers():
  from geeco_amd.variables import ema_decay_at
  assert ema_decay_at(0.999, 1) == np.float32(2) / np.float32(11)             # the ramp: (1 + t) / (10 + t)
  assert ema_decay_at(0.999, 1).dtype == np.float32
  assert ema_decay_at(0.99, 89) == np.float32(90) / np.float32(99) < np.float32(0.99)
  # the min takes over where the ramp passes the decay: (1 + t) / (10 + t) = 0.99 at t = 890
  assert ema_decay_at(0.99, 889) == np.float32(890) / np.float32(899) < np.float32(0.99)
  assert ema_decay_at(0.99, 891) == np.float32(0.99) < np.float32(892) / np.float32(901)
  assert ema_decay_at(0.5, 8) == np.float32(0.5) and ema_decay_at(0.5, 7) == np.float32(8) / np.float32(17)
  assert ema_decay_at(0.999, 10**6) == np.float32(0.999)
  ramp = [float(ema_decay_at(0.9999, t)) for t in range(1, 200)]
  assert all(a < b for a, b in zip(ramp, ramp[1:]))


def test_recurrence_known_answers():
  # constant p leaves s fixed, exactly, at every step of the ramp
  s = np.float32(0.37)
  for t in range(1, 50):
    s, _ = _recur(s, np.float32(0.37), 0.999, t)
    assert s == np.float32(0.37)
  # after a jump of p the distance to the new constant shrinks by d per step: rate 1 - d
  s, p, decay = np.float32(1.0), np.float32(3.0), 0.9
  for t in range(1000, 1040):          # (past the ramp: d_t = decay)
    nxt, d = _recur(s, p, decay, t)
    assert d == np.float32(decay)
    np.testing.assert_allclose((p - nxt) / (p - s), decay, rtol=1e-5)
    s = nxt
  np.testing.assert_allclose(p - s, 2.0 * decay ** 40, rtol=1e-4)
  # ... and the form is the documented one: s - (s - p)(1 - d)
  s, p = np.float64(0.25), np.float64(-1.5)
  got, d = _recur(s, p, 0.999, 1)
  np.testing.assert_allclose(got, s - (s - p) * (1.0 - np.float64(d)), rtol=1e-6)


def test_variable_store_state_dict_forms():
  plain, ema = _store(False), _store(True, seed=4)
  assert plain.ema is None and 'ema' not in plain.state_dict()
  assert ema.ema.shape == ema.params.shape and ema.ema.dtype == torch.float32 and ema.ema.device == ema.params.device
  assert ema.ema.data_ptr() % 16 == 0
  assert torch.equal(ema.ema, ema.params)                       # the shadow starts equal to the parameters
  name = next(iter(ema.shapes))
  assert ema.ema_var(name).shape == ema.var(name).shape and ema.ema_var(name).data_ptr() == ema.ema.data_ptr() + 4 * ema.offsets[name]
  ema.ema.mul_(0.5)
  sd = ema.state_dict()
  assert torch.equal(sd['ema'], ema.ema) and set(sd) == set(plain.state_dict()) | {'ema'}
  # with -> with: restored; with -> without: ignored; without -> with: the shadow restarts from the checkpoint's parameters
  back = _store(True, seed=5)
  back.load_state_dict(sd)
  assert torch.equal(back.ema, ema.ema) and torch.equal(back.params, ema.params)
  plain.load_state_dict(sd)
  assert plain.ema is None and torch.equal(plain.params, ema.params)
  back.load_state_dict(_store(False, seed=6).state_dict())
  assert torch.equal(back.ema, back.params) and not torch.equal(back.params, ema.params)
  with pytest.raises(ValueError):
    plain.to_numpy('ema')
  with pytest.raises(ValueError):
    plain.shadow_view()
  # the shadow view: the same arenas, the shadow in the parameters' place
  view = ema.shadow_view()
  assert view is ema.shadow_view() and view.base is ema and ema.base is ema
  assert view.params.data_ptr() == ema.ema.data_ptr() and view.ema is None and view.global_step is ema.global_step
  assert torch.equal(view.var(name), ema.ema_var(name))


def test_tf_bundle_shadow_tensor_names(tmp_path):
  from geeco_amd import tf_checkpoint
  st = _store(True)
  st.ema.mul_(0.25)
  st.adam_m.fill_(0.5)
  st.global_step.fill_(9)
  prefix = str(tmp_path / 'model.ckpt-9')
  tf_checkpoint.export_checkpoint(st, prefix)
  t = tf_checkpoint.read_checkpoint(prefix)
  shadow = st.to_numpy('ema')
  for name in st.shapes:
    np.testing.assert_array_equal(t[name + '/ExponentialMovingAverage'], shadow[name])
  assert 'VMC/ConvEncoder/conv1/kernel/ExponentialMovingAverage' in t
  # read back into a store with the arena, one without, and as the parameters of an inference store
  back = _store(True, seed=8)
  tf_checkpoint.import_checkpoint(back, prefix)
  assert torch.equal(back.ema, st.ema) and torch.equal(back.params, st.params)
  assert all((v == 0.5).all() for v in back.to_numpy('adam_m').values()) and int(back.global_step) == 9
  plain = _store(False, seed=8)
  tf_checkpoint.import_checkpoint(plain, prefix)
  assert torch.equal(plain.params, st.params)
  tf_checkpoint.import_checkpoint(plain, prefix, load_optimizer=False, use_ema=True)
  assert torch.equal(plain.params, st.ema)
  # a bundle without shadow tensors: s = p on restore, KeyError naming the first missing tensor for use_ema
  bare = str(tmp_path / 'bare.ckpt-9')
  tf_checkpoint.export_checkpoint(_store(False, seed=11), bare)
  assert not any(k.endswith('/ExponentialMovingAverage') for k in tf_checkpoint.read_checkpoint(bare))
  tf_checkpoint.import_checkpoint(back, bare)
  assert torch.equal(back.ema, back.params) and not torch.equal(back.params, st.params)
  with pytest.raises(KeyError, match='VMC/ConvEncoder/conv1/kernel/ExponentialMovingAverage'):
    tf_checkpoint.import_checkpoint(plain, bare, load_optimizer=False, use_ema=True)


def test_restore_for_inference_use_ema(tmp_path):
  from geeco_amd import estimator as est
  st = _store(True)
  st.ema.mul_(0.25)
  st.global_step.fill_(3)
  est.save_checkpoint(st, str(tmp_path), keep_max=2)
  plain = _store(False, seed=8)
  est.restore_for_inference(plain, str(tmp_path), use_ema=True)
  assert torch.equal(plain.params, st.ema)
  est.restore_for_inference(plain, str(tmp_path))
  assert torch.equal(plain.params, st.params)
  bare = tmp_path / 'bare'
  bare.mkdir()
  est.save_checkpoint(_store(False), str(bare), keep_max=2)
  with pytest.raises(KeyError, match='VMC/ConvEncoder/conv1/kernel/ExponentialMovingAverage'):
    est.restore_for_inference(plain, str(bare), use_ema=True)


@pytest.mark.parametrize('bad', [1.0, 1, -0.5, 1.5, float('nan'), 'fast', True, [0.9]])
def test_bad_ema_decay_is_refused_by_name(bad):
  from geeco_amd import estimator as est
  from geeco_amd.variables import check_ema_decay
  with pytest.raises(ValueError, match='ema_decay'):
    check_ema_decay(bad)
  with pytest.raises(ValueError, match=r"params\['ema_decay'\]"):
    est.Estimator(est.e2evmc_model_fn, None, est.RunConfig(), {'ema_decay': bad})


def test_ema_decay_off_and_on_values():
  from geeco_amd import estimator as est
  from geeco_amd.variables import check_ema_decay
  assert check_ema_decay(None) is None and check_ema_decay(0) is None and check_ema_decay(0.0) is None
  assert check_ema_decay(0.999) == 0.999 and check_ema_decay(np.float32(0.5)) == 0.5
  est.Estimator(est.e2evmc_model_fn, None, est.RunConfig(), {'ema_decay': 0.999})
  est.Estimator(est.e2evmc_model_fn, None, est.RunConfig(), {'ema_decay': 0})


def test_a_training_model_needs_decay_and_arena_together():
  from geeco_amd import graph
  from geeco_amd.params import create_e2evmc_config
  cfg = create_e2evmc_config(dict(window_size=2, img_height=136, img_width=136))
  with pytest.raises(ValueError, match='ema_decay'):
    graph.E2EVMC(cfg, 2, 'cpu', ema_decay=2.0)


def test_cli_flag_reaches_params():
  spec = importlib.util.spec_from_file_location('train_e2evmc_cli', os.path.join(ROOT, 'scripts', 'train_e2evmc.py'))
  cli = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(cli)
  args = cli.ARGPARSER.parse_args(['--ema_decay', '0.999'])
  assert cli.estimator_params(args, 'CFG') == {'e2evmc_config': 'CFG', 'log_steps': args.log_steps, 'debug': False, 'ema_decay': 0.999}
  off = cli.ARGPARSER.parse_args([])
  assert off.ema_decay == 0.0 and 'ema_decay' not in cli.estimator_params(off, 'CFG')
  # not a field of the model config: e2evmc_config.json stays as the reference writes it
  from geeco_amd.params import create_e2evmc_config
  assert 'ema_decay' not in create_e2evmc_config({})._asdict()
