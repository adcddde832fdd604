"""The host side of opt-in loss shaping: the fp64 restatement against numbers worked by hand, the values
params['loss_shaping'] takes, ``pickplace_input_fn(sample_weight=fn)``, the new entry points as header and binding declare them, and the
training script's flags."""
import ctypes
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

import _loss_shaping_ref as R

import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('geeco_heads_loss_shaped_fwd_bwd', 'geeco_lstm_step_heads_shaped_fwd_bwd', 'geeco_loss_shaping_sizeof')


# ================================================================================================
# the reference against numbers derivable by hand
# ================================================================================================
MSE_PRED = [[4.0, 8.0, 12.0], [8.0, 1.0, 3.0]]
MSE_TARGET = [[1.0, 9.0, 2.0], [-5.0, -2.0, 6.0]]
# squared errors: row 0: 3^2 + 1^2 + 10^2 = 110; row 1: 13^2 + 3^2 + 3^2 = 187


@pytest.mark.parametrize('weights,expected', [
    (None, 49.5),                    # (110 + 187) / 6 elements
    ([1.2, 3.4], 767.8 / 6),         # (1.2 * 110 + 3.4 * 187) / (3 * 2 non-zero weights) = (132 + 635.8) / 6
    ([1.2, 0.0], 132.0 / 3),         # 1.2 * 110 / (3 * 1 non-zero weight)
    ([0.0, 0.0], 0.0)])              # no non-zero weight: 0 (safe division)
def test_weighted_mse_by_hand(weights, expected):
  pred = torch.tensor(MSE_PRED, dtype=torch.float64, requires_grad=True)
  loss = R.mse_loss(pred, MSE_TARGET, weights)
  assert abs(float(loss) - expected) <= 1e-12 * max(1.0, expected)
  loss.backward()
  if weights == [0.0, 0.0]:
    assert not pred.grad.any()
  elif weights == [1.2, 0.0]:
    assert not pred.grad[1].any() and torch.allclose(pred.grad[0], 2 * 1.2 / 3 * torch.tensor([3.0, -1.0, 10.0], dtype=torch.float64))


# logits 10 * I_3 with every label wrong: each term is log(e^10 + 2) - 0 = 10 + log(1 + 2 e^-10) = 10.0000908
XENT_TERM = 10.0 + math.log1p(2.0 * math.exp(-10.0))


@pytest.mark.parametrize('weights,expected', [
    ([1.2, 3.4, 5.6], 34.0003),      # (1.2 + 3.4 + 5.6) * 10.0000908 / 3 non-zero weights = 10.2 * 10.0000908 / 3
    ([1.2, 0.0, 0.0], 12.0001)])     # 1.2 * 10.0000908 / 1 non-zero weight
def test_weighted_cross_entropy_by_hand(weights, expected):
  assert abs(XENT_TERM - 10.0000908) < 1e-7
  loss = float(R.xent_loss(10.0 * torch.eye(3, dtype=torch.float64), [2, 0, 1], weights))
  assert abs(loss - sum(weights) * XENT_TERM / sum(w != 0 for w in weights)) < 1e-12
  assert abs(loss - expected) < 1e-4


def test_label_smoothing_by_hand():
  # y = [0.9 + 0.1/3, 0.1/3, 0.1/3]; log softmax([100, -100, -100]) = [0, -200, -200] to 1e-87: loss = 2 * (0.1/3) * 200 = 400 * 0.1 / 3
  loss = float(R.xent_loss(torch.tensor([[100.0, -100.0, -100.0]], dtype=torch.float64), [0], None, smoothing=0.1))
  assert abs(loss - 400.0 * 0.1 / 3.0) < 1e-12
  # an out-of-range label keeps an all-zero one-hot: with smoothing its target is eps / C everywhere
  y = R.smoothed_one_hot([3, -1, 1], 3, 0.3)
  assert torch.allclose(y[0], torch.full((3,), 0.1, dtype=torch.float64)) and torch.equal(y[0], y[1])
  assert torch.allclose(y[2], torch.tensor([0.1, 0.8, 0.1], dtype=torch.float64))
  assert not R.smoothed_one_hot([3], 3, 0.0).any()


def test_huber_by_hand():
  pred = torch.tensor([[1.5], [-1.4], [-1.0], [0.0]], dtype=torch.float64, requires_grad=True)
  # errors 0.5, -0.4, -1, -0.5, all within delta = 1: 0.5 * (0.25 + 0.16 + 1 + 0.25) / 4 = 0.83 / 4 = 0.2075
  quad = R.huber_loss(pred, [[1.0], [-1.0], [0.0], [0.5]], 1.0)
  assert abs(float(quad) - 0.2075) < 1e-12
  # errors 1.5, -2.4, -1, -1.5, all at or beyond delta = 1: delta * (a - delta / 2) = 1 + 1.9 + 0.5 + 1 = 4.4; / 4 = 1.1
  lin = R.huber_loss(pred, [[0.0], [1.0], [0.0], [1.5]], 1.0)
  assert abs(float(lin) - 1.1) < 1e-12
  lin.backward()      # d/de = delta * sign(e) beyond delta (and e = -1 at delta itself, the same value: C1), over 4 elements
  assert torch.allclose(pred.grad[:, 0], torch.tensor([1.0, -1.0, -1.0, -1.0], dtype=torch.float64) / 4)
  # the same four numbers as ONE sample of size 4, and with a sample weight
  assert abs(float(R.huber_loss([[1.5, -1.4, -1.0, 0.0]], [[1.0, -1.0, 0.0, 0.5]], 1.0, [3.0])) - 3 * 0.2075) < 1e-12


def test_class_weights_are_sample_weights_of_the_label():
  g = torch.Generator().manual_seed(5)
  logits = torch.randn(9, 3, generator=g, dtype=torch.float64)
  labels = torch.tensor([0, 1, 2, 2, 1, 0, 3, -1, 1])      # two out of range: class weight 0
  sw = torch.tensor([1.0, 0.5, 2.0, 0.0, 1.0, 1.0, 1.0, 2.0, 0.5], dtype=torch.float64)
  cw = torch.tensor([1.0, 0.25, 2.0], dtype=torch.float64)
  gathered = torch.tensor([1.0, 0.25, 2.0, 2.0, 0.25, 1.0, 0.0, 0.0, 0.25], dtype=torch.float64)
  a = R.xent_loss(logits, labels, sw, 0.1, class_weights=cw)
  b = R.xent_loss(logits, labels, sw * gathered, 0.1)
  assert float(a) == float(b)
  # without a class table an out-of-range label keeps its sample weight (and counts)
  c = R.xent_loss(logits, labels, sw, 0.0)
  per = -(R.smoothed_one_hot(labels, 3) * torch.log_softmax(logits, 1)).sum(1)
  assert abs(float(c) - float((sw * per).sum() / 8)) < 1e-12


# ================================================================================================
# params['loss_shaping']
# ================================================================================================
def _cfg(**kw):
  from geeco_amd.params import create_e2evmc_config
  return create_e2evmc_config(kw)


def test_check_loss_shaping_accepts_and_normalises():
  from geeco_amd.variables import check_loss_shaping
  cart, vel = _cfg(), _cfg(control_mode='velocity')
  assert check_loss_shaping(None, cart) is None
  for neutral in ({}, {'sample_weights': False}, {'grp_class_weights': [1, 1.0, 1]}, {'label_smoothing': 0.0}, {'huber_delta': None},
                  {'sample_weights': False, 'grp_class_weights': (1.0, 1.0, 1.0), 'label_smoothing': 0, 'huber_delta': {}}):
    assert check_loss_shaping(neutral, cart) is None, neutral
  full = check_loss_shaping({'sample_weights': True, 'grp_class_weights': [1, 0.25, 2], 'label_smoothing': 0.1, 'huber_delta': 0.5}, cart)
  assert full == {'sample_weights': True, 'grp_class_weights': (1.0, 0.25, 2.0), 'label_smoothing': 0.1,
                  'huber_delta': {'cmd_ee': 0.5, 'pos_ee': 0.5, 'pos_obj': 0.5}}
  one = check_loss_shaping({'huber_delta': {'pos_obj': 2}}, cart)
  assert one == {'sample_weights': False, 'grp_class_weights': None, 'label_smoothing': 0.0, 'huber_delta': {'pos_obj': 2.0}}
  v = check_loss_shaping({'huber_delta': 1.0, 'sample_weights': True}, vel)
  assert list(v['huber_delta']) == ['cmd_vel', 'cmd_ee', 'cmd_grp', 'pos_ee', 'pos_obj'] and v['sample_weights']
  assert check_loss_shaping({'grp_class_weights': np.array([0.0, 1.0, 1.0])}, cart)['grp_class_weights'] == (0.0, 1.0, 1.0)


@pytest.mark.parametrize('bad', [
    'huber', 1.0, [('huber_delta', 1.0)], {'hubber_delta': 1.0}, {'sample_weights': 1}, {'sample_weights': 'yes'},
    {'grp_class_weights': [1, 2]}, {'grp_class_weights': [1, 2, 3, 4]}, {'grp_class_weights': [1, -0.5, 1]},
    {'grp_class_weights': [1, float('nan'), 1]}, {'grp_class_weights': [1, float('inf'), 1]}, {'grp_class_weights': '1,2,3'},
    {'grp_class_weights': 2.0}, {'label_smoothing': 1.0}, {'label_smoothing': -0.1}, {'label_smoothing': float('nan')},
    {'label_smoothing': True}, {'huber_delta': 0.0}, {'huber_delta': -1.0}, {'huber_delta': float('inf')}, {'huber_delta': float('nan')},
    {'huber_delta': True}, {'huber_delta': {'cmd_vel': 1.0}}, {'huber_delta': {'logits_cmd_grp': 1.0}}, {'huber_delta': {'cmd_ee': 0}},
    {'huber_delta': [1.0]}])
def test_check_loss_shaping_refuses_by_name(bad):
  from geeco_amd import estimator as est
  from geeco_amd.variables import check_loss_shaping
  with pytest.raises(ValueError, match='loss_shaping'):
    check_loss_shaping(bad, _cfg())
  with pytest.raises(ValueError, match=r"params\['loss_shaping'\]"):
    est.Estimator(est.e2evmc_model_fn, None, est.RunConfig(), {'loss_shaping': bad, 'e2evmc_config': _cfg()})


def test_gripper_options_are_cartesian_only():
  from geeco_amd.variables import check_loss_shaping
  vel = _cfg(control_mode='velocity')
  with pytest.raises(ValueError, match='grp_class_weights.*cartesian'):
    check_loss_shaping({'grp_class_weights': [1, 2, 3]}, vel)
  with pytest.raises(ValueError, match='label_smoothing.*cartesian'):
    check_loss_shaping({'label_smoothing': 0.1}, vel)
  assert check_loss_shaping({'label_smoothing': 0.0}, vel) is None


def test_head_table_yields_kind_2_for_huber_heads():
  from geeco_amd.decoder import head_table
  from geeco_amd.variables import check_loss_shaping
  cart = _cfg()
  assert [h[3] for h in head_table(cart)] == [0, 1, 0, 0] == [h[3] for h in head_table(cart, None)]
  assert [h[3] for h in head_table(cart, check_loss_shaping({'huber_delta': 1.0}, cart))] == [2, 1, 2, 2]
  assert [h[3] for h in head_table(cart, check_loss_shaping({'huber_delta': {'pos_ee': 1.0}}, cart))] == [0, 1, 2, 0]
  assert [h[3] for h in head_table(cart, check_loss_shaping({'label_smoothing': 0.1}, cart))] == [0, 1, 0, 0]
  vel = _cfg(control_mode='velocity')
  assert [h[3] for h in head_table(vel, check_loss_shaping({'huber_delta': {'cmd_vel': 1.0, 'cmd_grp': 2.0}}, vel))] == [2, 0, 2, 0, 0]
  assert [h[:3] + h[4:] for h in head_table(cart, check_loss_shaping({'huber_delta': 1.0}, cart))] == [h[:3] + h[4:] for h in head_table(cart)]


# ================================================================================================
# pickplace_input_fn(sample_weight=fn)
# ================================================================================================
EPISODES, EP_LEN, K, BATCH = 2, 8, 3, 4      # 5 windows per episode: batches of 4, 4, 2 (the ragged last one)


@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
  from geeco_amd import input_fn as I
  root = str(tmp_path_factory.mktemp('loss_shaping_ds'))
  I.write_synthetic_dataset(root, EPISODES, episode_length=EP_LEN, img_hw=(16, 16))
  return root


def _run(root, mode='train', **kw):
  from geeco_amd import input_fn as I
  kw = dict(dict(window_size=K, batch_size=BATCH, seed=3, num_threads=2), **kw)
  return list(I.pickplace_input_fn(root, 'default', mode, **kw))


def _weight_fn(features, labels):
  return 0.5 + np.abs(labels['cmd'][:, 3]) + (features['step'][:, 0] % 2)


@pytest.mark.parametrize('extra', [{}, {'shuffle_windows': True, 'shuffle_buffer': 4}])
def test_input_fn_adds_the_weights_and_touches_nothing_else(dataset, extra):
  plain = _run(dataset, **extra)
  weighted = _run(dataset, sample_weight=_weight_fn, **extra)
  sizes = [len(f['step']) for f, _ in plain]
  assert sizes == [len(f['step']) for f, _ in weighted] and sizes[-1] < BATCH and sum(sizes) == EPISODES * (EP_LEN - 1 - K + 1)
  for (f0, l0), (f1, l1) in zip(plain, weighted):
    assert 'sample_weight' not in l0 and set(l1) == set(l0) | {'sample_weight'} and set(f1) == set(f0)
    w = l1['sample_weight']
    assert w.dtype == np.float32 and w.shape == (len(f0['step']),)
    np.testing.assert_array_equal(w, _weight_fn(f0, l0).astype(np.float32))
    for k in f0:
      assert np.asarray(f0[k]).tobytes() == np.asarray(f1[k]).tobytes(), k
    for k in l0:
      assert l0[k].tobytes() == l1[k].tobytes() and l0[k].dtype == l1[k].dtype, k


def test_input_fn_weighs_eval_and_synthetic_batches(dataset):
  from geeco_amd import input_fn as I
  ev = _run(dataset, mode='eval', sample_weight=lambda f, l: np.ones(len(f['step'])))
  assert ev and all(l['sample_weight'].tolist() == [1.0] * len(f['step']) for f, l in ev)
  syn = list(I.pickplace_input_fn('synthetic:2:16x16', 'default', 'train', window_size=K, batch_size=3, fetch_target=True,
                                  sample_weight=lambda f, l: np.arange(3)))
  ref = list(I.pickplace_input_fn('synthetic:2:16x16', 'default', 'train', window_size=K, batch_size=3, fetch_target=True))
  assert len(syn) == len(ref) == 2
  for (f1, l1), (f0, l0) in zip(syn, ref):
    assert l1['sample_weight'].dtype == np.float32 and l1['sample_weight'].tolist() == [0.0, 1.0, 2.0] and 'sample_weight' not in l0
    assert all(np.array_equal(f0[k], f1[k]) for k in f0) and all(np.array_equal(l0[k], l1[k]) for k in l0)


@pytest.mark.parametrize('fn,what', [
    (lambda f, l: -np.ones(len(f['step'])), '>= 0'), (lambda f, l: np.full(len(f['step']), np.nan), 'finite'),
    (lambda f, l: np.full(len(f['step']), np.inf), 'finite'), (lambda f, l: np.ones(len(f['step']) + 1), 'shape'),
    (lambda f, l: np.ones((len(f['step']), 1)), 'shape'), (lambda f, l: 1.0, 'shape'),
    (lambda f, l: np.ones(len(f['step']), dtype=bool), 'number')])
def test_input_fn_refuses_bad_weights(dataset, fn, what):
  from geeco_amd import input_fn as I
  with pytest.raises(ValueError, match='sample_weight.*' + re.escape(what)):
    list(I.pickplace_input_fn('synthetic:1:16x16', 'default', 'train', window_size=K, batch_size=2, sample_weight=fn))
  with pytest.raises(ValueError, match='sample_weight'):
    I.pickplace_input_fn(dataset, 'default', 'train', window_size=K, sample_weight=np.ones(4))


# ================================================================================================
# the C ABI
# ================================================================================================
def test_abi_version_symbols_and_struct_layout():
  from geeco_amd import _native
  assert _abi.define('GEECO_ABI_VERSION') == 7 == _native.ABI_VERSION
  added = _abi.added_within(7)
  lib = _native.load()
  for name in NEW:
    assert name in added, name
    assert hasattr(lib, name) and name in _native.SIGNATURES, name
  # the documented layout: two pointers and an int64 stride, then six floats
  S = _native.LossShaping
  fields = [(n, getattr(S, n).offset, getattr(S, n).size) for n, _ in S._fields_]
  assert fields == [('sample_weight', 0, 8), ('sample_weight_stride', 8, 8), ('class_weight', 16, 8), ('label_smoothing', 24, 4),
                    ('huber_delta', 28, 20)]
  assert ctypes.sizeof(S) == 48 == lib.geeco_loss_shaping_sizeof()
  assert [f[0] for f in _abi.struct_fields('geeco_loss_shaping')] == [n for n, _ in S._fields_]
  # the shaped entry points: the signatures they extend with the struct behind Hfc
  for base, shaped in (('geeco_heads_loss_fwd_bwd', NEW[0]), ('geeco_lstm_step_heads_fwd_bwd', NEW[1])):
    a, b = _native.SIGNATURES[base][1], _native.SIGNATURES[shaped][1]
    at = [i for i, t in enumerate(b) if t is ctypes.POINTER(S)]
    assert len(at) == 1 and b[:at[0]] + b[at[0] + 1:] == a


def test_shaped_entry_points_check_their_arguments_without_a_gpu():
  """GEECO_EINVAL with a message naming the argument, before any launch (the pointers are never followed)."""
  from geeco_amd import _native
  lib = _native.load()
  one = ctypes.c_void_p(16)
  ptrs = lambda n: (ctypes.c_void_p * n)(*([16] * n))

  def call(kinds, shaping, shaped=True):
    n = len(kinds)
    heads = (n, ptrs(n), ptrs(n), (ctypes.c_int * n)(*([3] * n)), (ctypes.c_int * n)(*kinds), (ctypes.c_float * n)(*([1.0] * n)), ptrs(n),
             (ctypes.c_int64 * n)(*([3] * n)))
    tail = (one, one, 0, None, None, None, None, None, one, None)
    if not shaped:
      return lib.geeco_heads_loss_fwd_bwd(one, one, one, *heads, 1.0, 4, 128, 128, *tail)
    return lib.geeco_heads_loss_shaped_fwd_bwd(one, one, one, *heads, 1.0, 4, 128, 128, ctypes.byref(shaping) if shaping is not None else None,
                                               *tail)

  def shaping(eps=0.0, deltas=(), cw=False):
    s = _native.LossShaping()
    s.label_smoothing = eps
    for i, d in enumerate(deltas):
      s.huber_delta[i] = d
    if cw:
      s.class_weight = 16
    return s
  err = lambda: lib.geeco_last_error().decode()
  assert call([0, 1], None) == _native.GEECO_EINVAL and 'shaping' in err()
  for eps in (1.0, -0.25, float('nan'), 1.5):
    assert call([0, 1], shaping(eps=eps)) == _native.GEECO_EINVAL and 'label_smoothing' in err(), eps
  for d in (0.0, -1.0, float('inf'), float('nan')):
    assert call([2, 1], shaping(deltas=[d])) == _native.GEECO_EINVAL and 'huber_delta[0]' in err(), d
  assert call([0, 2], shaping(deltas=[0.0, 0.0])) == _native.GEECO_EINVAL and 'huber_delta[1]' in err()
  assert call([0, 0], shaping(cw=True)) == _native.GEECO_EINVAL and 'class_weight' in err()
  assert call([1, 1], shaping(cw=True)) == _native.GEECO_EINVAL and 'class_weight' in err()
  # the unshaped entry point keeps refusing kind 2
  assert call([2, 1], None, shaped=False) == _native.GEECO_EINVAL and 'kind 2' in err()
  assert call([0, 3], shaping()) == _native.GEECO_EINVAL and 'kind 3' in err()


# ================================================================================================
# the training script
# ================================================================================================
def test_cli_flags_reach_params():
  spec = importlib.util.spec_from_file_location('train_e2evmc_cli_loss_shaping', os.path.join(ROOT, 'scripts', 'train_e2evmc.py'))
  cli = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(cli)
  parse = lambda *argv: cli.estimator_params(cli.ARGPARSER.parse_args(list(argv)), 'CFG')
  assert 'loss_shaping' not in parse()
  assert parse('--loss_grp_class_weights', '1,0.2,1')['loss_shaping'] == {'grp_class_weights': [1.0, 0.2, 1.0]}
  assert parse('--loss_label_smoothing', '0.1')['loss_shaping'] == {'label_smoothing': 0.1}
  assert parse('--loss_huber_delta', '1.0')['loss_shaping'] == {'huber_delta': 1.0}
  assert parse('--loss_grp_class_weights', '1,0.2,1', '--loss_label_smoothing', '0.1', '--loss_huber_delta', '2')['loss_shaping'] == \
      {'grp_class_weights': [1.0, 0.2, 1.0], 'label_smoothing': 0.1, 'huber_delta': 2.0}
  with pytest.raises(ValueError, match='--loss_grp_class_weights'):
    parse('--loss_grp_class_weights', '1,x,1')
  from geeco_amd.variables import check_loss_shaping
  assert check_loss_shaping(parse('--loss_grp_class_weights', '1,0.2,1', '--loss_huber_delta', '2')['loss_shaping'], _cfg()) is not None
