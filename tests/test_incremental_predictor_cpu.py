"""Incremental predictor (batched_predictor.py incremental=True, step_models.E2EVMCStep / GoalE2EVMCStep, csrc/predict_io.hip) without a
GPU: the C ABI of its two entries and their host-side argument checks, the feature-ring specification its kernel is held to on
the GPU (FeatureRingModel below; tests/test_incremental_predictor_gpu.py compares the kernel against it bitwise), and the premise
that makes caching legitimate: in the oracle a window's state_t is a function of frame t alone."""
import ctypes
import os
import re

import numpy as np
import torch

from oracle import geeco_oracle as O
from test_batched_predictor_cpu import Batch1Window

import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('geeco_predict_pack_newest', 'geeco_predict_push_features')
MODES = {'plain': 0, 'constant': 1, 'residual': 2}


class FeatureRingModel:
  """B envs' rings of the last K feature vectors [cells][ch] and joint states [J], and the decoder states gathered from them.

  push: reset[b] -> every slot of env b = the new feature / joint state; else the slot at the head is overwritten; the head moves
  to (p + 1) % K either way.  states[t][b], t = 0..K-1 oldest first, come from slots p + 1, .., p + K - 1, p (mod K); per cell the
  columns are plain [feat | jnt], constant [feat | jnt | tgt], residual [tgt - feat | jnt] (float32 subtraction)."""

  def __init__(self, B, K, cells, ch, J, mode):
    self.B, self.K, self.cells, self.ch, self.J, self.mode = B, K, cells, ch, J, mode
    self.feat = np.zeros((B, K, cells, ch), np.float32)
    self.jnt = np.zeros((B, K, J), np.float32)
    self.heads = np.zeros(B, np.int32)
    self.Ctot = ch + J + (ch if mode == 'constant' else 0)

  def push(self, feat, jnt, reset, tgt=None):
    B, K = self.B, self.K
    states = np.zeros((K, B, self.cells * self.Ctot), np.float32)
    for b in range(B):
      p = int(self.heads[b])
      if reset[b]:
        self.feat[b][:] = feat[b]
        self.jnt[b][:] = jnt[b]
      else:
        self.feat[b][p] = feat[b]
        self.jnt[b][p] = jnt[b]
      self.heads[b] = (p + 1) % K
      for t in range(K):
        s = (p + 1 + t) % K
        states[t, b] = self.state_row(self.feat[b, s], self.jnt[b, s], None if tgt is None else tgt[b])
    return states

  def state_row(self, f, j, tgt):
    jj = np.broadcast_to(j, (self.cells, self.J))
    if self.mode == 'plain':
      cols = [f, jj]
    elif self.mode == 'constant':
      cols = [f, jj, tgt]
    else:
      cols = [tgt - f, jj]
    return np.concatenate(cols, axis=1).reshape(-1)

  def window(self, b):
    """Env b's K feature vectors and joint states, oldest first (heads[b] = the oldest slot once the push has moved it on)."""
    order = [(int(self.heads[b]) + t) % self.K for t in range(self.K)]
    return self.feat[b, order], self.jnt[b, order]


def test_entries_declared_exported_typed_at_abi_7():
  from geeco_amd import _native, ops
  for name in ENTRIES:
    assert name in _abi.functions(), name
    assert name in _native.SIGNATURES, name
  lib = ctypes.CDLL(_native.LIB_PATH)
  for name in ENTRIES:
    assert hasattr(lib, name), name
  assert _native.ABI_VERSION == 7 and _native.load().geeco_abi_version() == 7
  for mode, v in MODES.items():
    assert ops.PREDICT_FEAT_MODES[mode] == v
    assert _abi.define('GEECO_PREDICT_FEAT_' + mode.upper()) == v, mode
  assert callable(ops.predict_pack_newest_into) and callable(ops.predict_push_features_into)


def test_argument_checks_need_no_gpu():
  """Every rejection comes back as -1 with its message, before any launch."""
  from geeco_amd import _native
  lib = _native.load()
  one = ctypes.c_void_p(256)
  err = lambda: lib.geeco_last_error()
  pack = lambda fr, u8, B, HW, C, x=one: lib.geeco_predict_pack_newest(fr, u8, B, HW, C, x, None)
  assert pack(None, 0, 2, 64, 3) == -1 and b'null pointer' in err()
  assert pack(one, 0, 2, 64, 3, x=None) == -1 and b'null pointer' in err()
  assert pack(one, 0, 0, 64, 3) == -1 and b'B=0' in err()
  assert pack(one, 0, 2, 64, 5) == -1 and b'C=5' in err()
  assert pack(one, 1, 2, 64, 4) == -1 and b'uint8 frames are RGB' in err()
  assert pack(one, 0, 2, 0, 3) == -1 and b'HW=0' in err()

  def push(feat=one, tgt=one, mode=0, B=2, K=3, cells=4, ch=256, J=7, ring=one, heads=one, states=one, stride=None):
    stride = 4 * (ch + J + (ch if mode == 1 else 0)) if stride is None else stride
    return lib.geeco_predict_push_features(feat, one, one, one, tgt, mode, B, K, cells, ch, J, ring, one, heads, states, stride, None)
  assert push(feat=None) == -1 and b'null pointer' in err()
  assert push(ring=None) == -1 and b'null pointer' in err()
  assert push(heads=None) == -1 and b'null pointer' in err()
  assert push(states=None) == -1 and b'null pointer' in err()
  assert push(tgt=None, mode=1) == -1 and b'null pointer' in err()
  assert push(tgt=None, mode=2) == -1 and b'null pointer' in err()
  assert push(mode=3) == -1 and b'mode=3' in err()
  assert push(mode=-1) == -1 and b'mode=-1' in err()
  assert push(B=0) == -1 and b'B=0' in err()
  assert push(K=0) == -1 and b'K=0' in err()
  assert push(K=65) == -1 and b'K=65' in err()
  assert push(ch=0) == -1 and b'ch=0' in err()
  assert push(J=0) == -1 and b'J=0' in err()
  assert push(stride=4 * 263 - 1) == -1 and b'state_stride' in err()
  assert push(mode=1, stride=4 * 263) == -1 and b'state_stride' in err()      # constant needs room for the target's columns


def test_ring_model_agrees_with_batch1_windows():
  """The B-env feature ring, gathered oldest first, equals B independent batch-1 windows ('first-frame padding, then slide') over
  random call sequences with random reset masks; the states are the per-cell concat of those windows."""
  r = np.random.default_rng(0)
  cells, ch, J = 4, 8, 3
  for B, K in ((1, 1), (3, 2), (4, 3), (5, 16)):
    for mode in MODES:
      rm = FeatureRingModel(B, K, cells, ch, J, mode)
      ref_f = [Batch1Window(K) for _ in range(B)]
      ref_j = [Batch1Window(K) for _ in range(B)]
      pending = np.ones(B, bool)
      tgt = r.standard_normal((B, cells, ch)).astype(np.float32)
      for call in range(50):
        if call and r.random() < 0.5:
          for b in np.flatnonzero(r.random(B) < 0.3):
            pending[b] = True
            ref_f[b].reset()
            ref_j[b].reset()
        if call == 25:
          tgt = r.standard_normal((B, cells, ch)).astype(np.float32)      # a goal change mid-episode
        f = r.standard_normal((B, cells, ch)).astype(np.float32)
        j = r.standard_normal((B, J)).astype(np.float32)
        states = rm.push(f, j, pending, tgt)
        pending[:] = False
        assert states.shape == (K, B, cells * rm.Ctot)
        for b in range(B):
          wf, wj = ref_f[b].feed(f[b]), ref_j[b].feed(j[b])
          gf, gj = rm.window(b)
          np.testing.assert_array_equal(gf, wf)
          np.testing.assert_array_equal(gj, wj)
          assert 0 <= rm.heads[b] < K
          for t in range(K):
            row = states[t, b].reshape(cells, rm.Ctot)
            np.testing.assert_array_equal(row[:, ch:ch + J], np.broadcast_to(wj[t], (cells, J)))
            if mode == 'residual':
              np.testing.assert_array_equal(row[:, :ch], tgt[b] - wf[t])
            else:
              np.testing.assert_array_equal(row[:, :ch], wf[t])
            if mode == 'constant':
              np.testing.assert_array_equal(row[:, ch + J:], np.broadcast_to(tgt[b], (cells, ch)))


def _premise(goal, kw):
  """model_forward on sliding windows == lstm_decoder over states built from conv_encoder run on ONE frame of ONE env at a time,
  each distinct frame encoded exactly once (the cache), in float64.  Bound: float64 sums of at most 9 * 256 products per output
  through 8 layers in a possibly different blocking (batch of one instead of B): a few thousand eps64 ~ 1e-12 relative; 1e-10
  leaves two decades."""
  K, B, T, H, W = 3, 2, 5, 136, 136
  cfg = O.make_config(batch_size=B, window_size=K, img_height=H, img_width=W, **kw)
  P = {k: torch.tensor(v, dtype=torch.float64) for k, v in O.init_params(O.model_param_shapes(cfg, goal), seed=3).items()}
  r = np.random.default_rng(11)
  frames = torch.tensor(r.random((T, B, H, W, 3)), dtype=torch.float64)
  jnts = torch.tensor(r.standard_normal((T, B, 7)), dtype=torch.float64)
  tgt = torch.tensor(r.random((B, H, W, 3)), dtype=torch.float64)
  scope = 'GoalVMC' if goal else 'VMC'
  cache = {}

  def feat(t, b):
    if (t, b) not in cache:
      cache[(t, b)] = O.conv_encoder(frames[t, b][None], P, scope + '/ConvEncoder')
    return cache[(t, b)]
  tgt_feat = [O.conv_encoder(tgt[b][None], P, scope + '/ConvEncoder') for b in range(B)] if goal else None
  for t in range(T):
    idx = [max(0, t - K + 1 + i) for i in range(K)]                    # first-frame padding, then slide
    feats = {'rgb': frames[idx].permute(1, 0, 2, 3, 4), 'jnt_state': jnts[idx].permute(1, 0, 2)}
    if goal:
      feats['target_rgb'] = tgt
    ref, _ = O.model_forward(feats, P, cfg, goal)
    states = []
    for s in idx:
      rows = []
      for b in range(B):
        f, j = feat(s, b), jnts[s, b][None]
        if not goal:
          rows.append(O.state_concatenation(f, j))
        elif cfg.proc_tgt == 'constant':
          rows.append(O.representation_concatenation(f, tgt_feat[b], j))
        else:
          rows.append(O.state_concatenation(tgt_feat[b] - f, j))
      states.append(torch.cat(rows, dim=0))
    ep = O.lstm_decoder(states, P, scope + '/LSTMDecoder', cfg)
    for key, name in (('cmd_ee', 'pred_cmd_ee'), ('logits_cmd_grp', 'logits_cmd_grp'), ('pos_ee', 'pred_aux_ee'),
                      ('pos_obj', 'pred_aux_obj')):
      np.testing.assert_allclose(ep[name].numpy(), ref[key].numpy(), rtol=1e-10, atol=1e-10, err_msg='%s call %d' % (key, t))
  assert len(cache) == T * B          # every frame went through the encoder once


def test_oracle_premise_e2e_vmc():
  _premise(False, dict())


def test_oracle_premise_sequence_constant():
  _premise(True, dict(proc_obs='sequence', proc_tgt='constant'))


def test_oracle_premise_sequence_residual():
  _premise(True, dict(proc_obs='sequence', proc_tgt='residual'))
