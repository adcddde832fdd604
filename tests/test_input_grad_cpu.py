"""Input gradients, host side (no GPU): the float64 restatements of tests/_input_grad_ref.py against autograd of the
oracle and against central differences, the tie rule, the exported symbols, and the refusals of ``input_gradients``."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _input_grad_ref as R
from oracle import geeco_oracle as O

import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('geeco_conv1_dgrad', 'geeco_pack_pixels_bwd', 'geeco_dynimg_bwd_ws_bytes', 'geeco_dynimg_bwd')


def _rel(a, b):
  return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


@pytest.mark.parametrize('N,K,shape', [(2, 1, (3, 4, 3)), (2, 2, (5, 3, 3)), (3, 4, (4, 5, 4)), (1, 7, (6, 2, 3))])
def test_dynimg_bwd_ref_is_autograd_of_the_oracle_without_ties(N, K, shape):
  r = np.random.default_rng(5)
  frames, g = r.random((N, K) + shape), r.standard_normal((N,) + shape)
  if K > 1:      # (K = 1: alpha = [0], D is all zeros -- every element ties, and the frames' gradient is exactly 0 either way)
    assert R.extrema_margin(frames) > 0
  ref = R.dynimg_bwd_ref(g, frames)
  assert _rel(ref, R.dynimg_autograd(g, frames)) < 1e-12 if K > 1 else not ref.any()


def test_dynimg_bwd_ref_shares_a_tie_evenly_and_the_oracle_does_not():
  """Two pixels that hold identical values in every frame: their sums are bitwise equal, and they are the maximum.  TF 1.15's
  reduce_max gradient gives each half of the term; torch's ``max(dim)`` (the oracle's) gives one of them all of it."""
  r = np.random.default_rng(6)
  K, shape = 3, (4, 4, 3)
  frames = r.random((1, K) + shape)
  alpha = O.dynimg_alpha(K)
  for t in range(K):
    frames[0, t, 1, 2, 0] = frames[0, t, 3, 0, 1] = 2.0 if alpha[t] > 0 else -1.0
  D = np.tensordot(alpha.astype(np.float64), frames[0], axes=(0, 0))
  assert D[1, 2, 0] == D[3, 0, 1] == D.max() and (D == D.max()).sum() == 2
  g = r.standard_normal((1,) + shape)
  g[0, 1, 2, 0] = g[0, 3, 0, 1] = 0.0      # their own g_i / r terms out of the way: what is left is the shared term
  ref = R.dynimg_bwd_ref(g, frames)
  t = int(np.argmax(np.abs(alpha)))
  a, b = ref[0, t, 1, 2, 0], ref[0, t, 3, 0, 1]
  assert a == b and a != 0.0
  auto = R.dynimg_autograd(g, frames)
  pa, pb = auto[0, t, 1, 2, 0], auto[0, t, 3, 0, 1]
  assert pa != pb and (pa == 0.0 or pb == 0.0)                  # the oracle's min(dim) / max(dim): one index takes it all
  assert abs((pa + pb) - (a + b)) <= 1e-12 * abs(a + b)       # the same total
  mask = np.ones(shape, bool)
  mask[1, 2, 0] = mask[3, 0, 1] = False
  assert _rel(ref[0][:, mask], auto[0][:, mask]) < 1e-12        # and every other element agrees


@pytest.mark.parametrize('F,H,W,Cin', [(1, 1, 1, 3), (2, 3, 5, 3), (2, 6, 4, 4)])
def test_conv1_dgrad_ref_is_autograd_of_the_oracle(F, H, W, Cin):
  r = np.random.default_rng(7)
  dz, w = r.standard_normal((F, H, W, 32)), r.standard_normal((3, 3, Cin, 32))
  x = torch.zeros(F, H, W, Cin, dtype=torch.float64, requires_grad=True)
  O.conv2d_same(x, torch.tensor(w), torch.zeros(32, dtype=torch.float64), 1, relu=False).backward(torch.tensor(dz))
  assert _rel(R.conv1_dgrad_ref(dz, w), x.grad.numpy()) < 1e-12


def test_central_differences_agree_with_both():
  r = np.random.default_rng(8)
  # conv1: linear in x, so the difference quotient is exact up to rounding
  F, H, W, Cin = 1, 4, 3, 3
  dz, w, x0 = r.standard_normal((F, H, W, 32)), r.standard_normal((3, 3, Cin, 32)), r.standard_normal((F, H, W, Cin))
  fwd = lambda x: float((O.conv2d_same(torch.tensor(x), torch.tensor(w), torch.zeros(32, dtype=torch.float64), 1, relu=False).numpy() * dz).sum())
  num, h = np.zeros_like(x0), 1e-3
  for i in np.ndindex(*x0.shape):
    e = np.zeros_like(x0); e[i] = h
    num[i] = (fwd(x0 + e) - fwd(x0 - e)) / (2 * h)
  assert _rel(num, R.conv1_dgrad_ref(dz, w)) < 1e-6
  # the dynamic image: smooth away from ties (the planted extrema keep a step of 1e-5 far from one)
  N, K, shape = 1, 3, (3, 2, 3)
  frames, g = R.plant_extrema(r.random((N, K) + shape), seed=1), r.standard_normal((N,) + shape)
  assert R.extrema_margin(frames) > 1e-2
  f2 = lambda fr: float((O.dynimg(torch.tensor(fr)).numpy() * g).sum())
  num, h = np.zeros_like(frames), 1e-5
  for i in np.ndindex(*frames.shape):
    e = np.zeros_like(frames); e[i] = h
    num[i] = (f2(frames + e) - f2(frames - e)) / (2 * h)
  ref = R.dynimg_bwd_ref(g, frames)
  assert _rel(num, ref) < 1e-6 and _rel(num, R.dynimg_autograd(g, frames)) < 1e-6


def test_pack_bwd_ref_is_the_adjoint_of_the_channel_pack():
  r = np.random.default_rng(9)
  a, b, g = r.standard_normal((2, 5, 3)), r.standard_normal((2, 5, 1)), r.standard_normal((2, 5, 4))
  da, db = R.pack_bwd_ref(g, 3, C2=1)
  packed = np.concatenate([a, b], axis=-1)
  assert abs((packed * g).sum() - ((a * da).sum() + (b * db).sum())) < 1e-12      # <pack(a, b), g> == <a, da> + <b, db>
  da2, _ = R.pack_bwd_ref(g, 3, d_src=a)
  assert np.array_equal(da2, a + g[..., :3])


def test_header_library_and_binding_export_the_entry_points():
  from geeco_amd import _native
  assert _abi.define('GEECO_ABI_VERSION') == 7 == _native.ABI_VERSION
  lib = ctypes.CDLL(_native.LIB_PATH)
  lib.geeco_abi_version.restype = ctypes.c_int
  assert lib.geeco_abi_version() == 7
  for name in SYMBOLS:
    assert name in _abi.functions(), name
    assert name in _native.SIGNATURES, name
    assert hasattr(lib, name), name
  assert 'input_grad' in open(os.path.join(ROOT, 'geeco_amd', 'csrc', 'sources.sh')).read().split('"')[1].split()
  # the argument counts of binding and header agree
  for name in SYMBOLS:
    assert len(_abi.functions()[name][1]) == len(_native.SIGNATURES[name][1]), name
  lib.geeco_dynimg_bwd_ws_bytes.restype = ctypes.c_int64
  lib.geeco_dynimg_bwd_ws_bytes.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int]
  assert lib.geeco_dynimg_bwd_ws_bytes(2, 136 * 136, 3) >= 2 * (-(-136 * 136 * 3 // 1024)) * 32
  # a layer the conv1 kernel was not built for is refused before anything is launched (no device needed to ask)
  lib.geeco_conv1_dgrad.restype = ctypes.c_int
  lib.geeco_conv1_dgrad.argtypes = _native.SIGNATURES['geeco_conv1_dgrad'][1]
  assert lib.geeco_conv1_dgrad(None, None, None, 1, 0, 0, 0, 1, 4, 4, 3, 48, None) == _native.GEECO_ENOSUP
  assert lib.geeco_conv1_dgrad(None, None, None, 1, 0, 0, 0, 1, 4, 4, 5, 32, None) == _native.GEECO_ENOSUP


def test_input_gradients_refuses_with_the_reason():
  from geeco_amd import graph
  from geeco_amd.params import create_e2evmc_config
  kw = dict(img_height=136, img_width=136, window_size=2)
  cfg = create_e2evmc_config(kw)
  with pytest.raises(ValueError, match='training=False'):
    graph.E2EVMC(cfg, 2, 'cpu', training=False).check_input_gradients()
  with pytest.raises(ValueError, match='shared_frames'):
    graph.E2EVMC(cfg, 2, 'cpu', training=True, shared_frames=4).check_input_gradients()
  m = graph.GoalE2EVMC(create_e2evmc_config(dict(kw, proc_obs='dynimg', proc_tgt='dyndiff')), 2, 'cpu', training=True)
  m.check_input_gradients()      # a plain training model passes

  class Windows:
    def pointers(self):
      return None
  dense = m.inputs['rgb']
  m.inputs['rgb'] = Windows()
  with pytest.raises(ValueError, match="'rgb' bound as uint8 window addresses"):
    m.check_input_gradients()
  m.inputs['rgb'] = dense
  m.backward_cut = 'no_bottom'
  with pytest.raises(ValueError, match="backward_cut='no_bottom'"):
    m.check_input_gradients()
  m.backward_cut = 'full'
  with pytest.raises(ValueError, match='training stack'):
    graph.E2EVMC(cfg, 2, 'cpu', training=False).enc.input_gradient()


def test_select_loss_heads():
  from geeco_amd import graph
  from geeco_amd.params import create_e2evmc_config
  d = graph.E2EVMC(create_e2evmc_config(dict(img_height=136, img_width=136, window_size=2, lambda_aux=0.5)), 2, 'cpu').decoder
  table = d._head_args(False)[0][6]
  assert table == [1.0, 1.0, 0.5, 0.5]
  d.select_loss_heads(('cmd_ee',))
  assert d._head_args(False)[0][6] == [1.0, 0.0, 0.0, 0.0]
  d.select_loss_heads(('cmd_grp', 'pos_obj'))
  assert d._head_args(False)[0][6] == [0.0, 1.0, 0.0, 1.0]
  with pytest.raises(ValueError, match='cmd_ee'):
    d.select_loss_heads(('nonsense',))
  d.select_loss_heads(None)
  assert d._head_args(False)[0][6] == table
