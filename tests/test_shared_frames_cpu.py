"""Shared-frame training, host side (no GPU): ``DeviceWindows.frame_table`` on fake resident episodes, and the premise of
the feature on the float64 oracle -- conv_encoder sees one frame at a time, so the loss of dense overlapping windows is the
loss from each DISTINCT frame encoded once and gathered into the windows."""
import numpy as np
import pytest
import torch

from _fake_frames import FE, K, FakeFrames, windows as _windows
from oracle import geeco_oracle as O

def _expect(segments, k=K):
  """address of every frame of every window, straight from the definition"""
  out = []
  for frames, starts, _ in segments:
    esz = 1 if frames.dtype == torch.uint8 else 4
    for s in starts:
      out.append([frames.base + (s + t) * FE * esz for t in range(k)])
  return np.asarray(out, np.int64)


def _check_table(table, index, used, want, capacity):
  assert table.dtype == np.int64 and table.shape == (capacity,)
  assert index.dtype == np.int32 and index.shape == want.shape
  np.testing.assert_array_equal(table[index], want)
  flat = want.ravel()
  first_use = flat[np.sort(np.unique(flat, return_index=True)[1])]       # distinct addresses in first-use order
  assert used == len(first_use)
  np.testing.assert_array_equal(table[:used], first_use)
  assert not table[used:].any()                                          # zero padding = unused slots


CASES = {
    'one episode': lambda: [(FakeFrames(1 << 20, 9), [0, 1, 2, 3], 255.0)],
    'gaps': lambda: [(FakeFrames(1 << 20, 9), [0, 1, 2, 5], 255.0)],
    'two episodes': lambda: [(FakeFrames(1 << 20, 8), [4, 5], 255.0), (FakeFrames(1 << 22, 8), [0, 1], 255.0)],
    'float32': lambda: [(FakeFrames(1 << 20, 9, torch.float32), [2, 3, 3], 1.0)],
}


@pytest.mark.parametrize('name', list(CASES))
def test_frame_table_indexes_every_window_frame(name):
  segs = CASES[name]()
  want = _expect(segs)
  n = len(want)
  cap = n + 2 * (K - 1)
  table, index, tindex, used = _windows(segs).frame_table(cap)
  assert tindex is None
  _check_table(table, index, used, want, cap)


def test_frame_table_distinct_counts():
  t, i, _, used = _windows(CASES['one episode']()).frame_table(16)
  assert used == 4 + K - 1 and i.tolist() == [[0, 1, 2], [1, 2, 3], [2, 3, 4], [3, 4, 5]]
  _, i, _, used = _windows(CASES['gaps']()).frame_table(8)
  assert used == 8 and i.tolist() == [[0, 1, 2], [1, 2, 3], [2, 3, 4], [5, 6, 7]]
  _, i, _, used = _windows(CASES['two episodes']()).frame_table(8)
  assert used == 8 and i.tolist() == [[0, 1, 2], [1, 2, 3], [4, 5, 6], [5, 6, 7]]


def test_frame_table_with_a_target_stream():
  """Targets are rows of the same table: one slot per episode (all its windows share the goal frame), numbered behind the
  window frames; a target that IS one of the window frames shares that frame's slot."""
  ep_a, ep_b = FakeFrames(1 << 20, 8), FakeFrames(1 << 22, 8)
  tg_a, tg_b = FakeFrames(1 << 24, 1), FakeFrames(1 << 25, 1)
  segs = [(ep_a, [4, 5], 255.0), (ep_b, [0, 1], 255.0)]
  tsegs = [(tg_a, [0, 0], 255.0), (tg_b, [0, 0], 255.0)]
  table, index, tindex, used = _windows(segs).frame_table(10, _windows(tsegs, k=1, squeeze=True))
  _check_table(table, np.concatenate([index.ravel(), tindex]), used,
               np.concatenate([_expect(segs).ravel(), _expect(tsegs, 1).ravel()]), 10)
  assert used == 10 and tindex.dtype == np.int32 and tindex.tolist() == [8, 8, 9, 9]
  # the goal frame inside the windowed tensor itself (row 7 of episode a)
  tsegs = [(ep_a, [7, 7], 255.0), (ep_b, [3, 3], 255.0)]
  table, index, tindex, used = _windows(segs).frame_table(8, _windows(tsegs, k=1, squeeze=True))
  assert used == 8 and tindex.tolist() == [3, 3, 7, 7]
  np.testing.assert_array_equal(table[tindex], _expect(tsegs, 1).ravel())


def test_frame_table_refusals():
  dw = _windows(CASES['gaps']())
  with pytest.raises(ValueError, match='8 distinct frames'):
    dw.frame_table(7)
  mixed = _windows([(FakeFrames(1 << 20, 8), [4, 5], 255.0), (FakeFrames(1 << 22, 8, torch.float32), [0, 1], 1.0)])
  with pytest.raises(ValueError, match='mixes uint8 and float32'):
    mixed.frame_table(16)
  with pytest.raises(IndexError, match='outside the 9 resident frames'):
    _windows([(FakeFrames(1 << 20, 9), [7], 255.0)]).frame_table(16)
  with pytest.raises(RuntimeError, match='each rank must upload'):
    dw.frame_table(16, device='cuda:1')
  two = _windows([(FakeFrames(1 << 20, 8), [0], 255.0), (FakeFrames(1 << 22, 8, device='cuda:1'), [0], 255.0)])
  with pytest.raises(RuntimeError, match='several devices'):
    two.frame_table(16)
  with pytest.raises(ValueError, match='single frames'):
    dw.frame_table(16, _windows(CASES['one episode']()))


def test_shared_frames_capacity_rule():
  from geeco_amd.estimator import shared_frames_capacity
  assert shared_frames_capacity(True, 32, 16, False) == 62       # N + 2 (K - 1)
  assert shared_frames_capacity(True, 32, 16, True) == 64        # + one goal frame per episode
  assert shared_frames_capacity(40, 32, 16, True) == 40


def test_models_refuse_what_has_nothing_to_share():
  """The constructor checks come before any device allocation."""
  from geeco_amd import graph
  from geeco_amd.params import create_e2evmc_config
  kw = dict(img_height=136, img_width=136, window_size=3)
  for extra, goal, msg in ((dict(proc_obs='dynimg', proc_tgt='dyndiff'), True, 'dynimg'),
                           (dict(proc_obs='sequence', proc_tgt='dyndiff'), True, 'dyndiff'),
                           (dict(img_channels=4), False, 'RGB-D'),
                           (dict(proc_obs='sequence', proc_tgt='residual', img_channels=4), True, 'RGB-D')):
    cfg = create_e2evmc_config(dict(kw, **extra))
    with pytest.raises(ValueError, match=msg):
      (graph.GoalE2EVMC if goal else graph.E2EVMC)(cfg, 4, 'cpu', training=True, shared_frames=8)


@pytest.mark.parametrize('goal,proc_tgt', [(False, 'constant'), (True, 'constant'), (True, 'residual')])
def test_premise_on_the_oracle(goal, proc_tgt):
  """float64: model_forward's loss on dense overlapping windows == the loss from conv_encoder run ONCE per distinct frame, the
  features gathered into the windows.  Equal to rounding (the batched convolution may sum in another order)."""
  H = 136
  ocfg = O.make_config(proc_obs='sequence', proc_tgt=proc_tgt, window_size=K, img_height=H, img_width=H, batch_size=4)
  P = {k: torch.tensor(v, dtype=torch.float64) for k, v in O.init_params(O.model_param_shapes(ocfg, goal), seed=3).items()}
  feats, labels = O.synthetic_batch(ocfg, goal, 4, seed=5, H=H, W=H)
  r = np.random.default_rng(7)
  episode = r.random([9, H, H, 3])
  index = np.asarray([[s + t for t in range(K)] for s in (0, 1, 2, 5)])
  tindex = np.asarray([8, 8, 8, 8])
  f = {k: torch.tensor(v, dtype=torch.float64) if v.dtype.kind == 'f' else torch.tensor(v) for k, v in feats.items()}
  l = {k: torch.tensor(v, dtype=torch.float64) for k, v in labels.items()}
  f['rgb'] = torch.tensor(episode[index])
  if goal:
    f['target_rgb'] = torch.tensor(episode[tindex])
  pred, _ = O.model_forward(f, P, ocfg, goal)
  loss_dense, _ = O.model_loss(pred, O.build_targets(f, l, ocfg), P, ocfg)
  # each distinct frame once
  scope = 'GoalVMC' if goal else 'VMC'
  feat = O.conv_encoder(torch.tensor(episode), P, scope + '/ConvEncoder')          # [9][2][2][ch]
  states = []
  for t in range(K):
    ft, jt = feat[index[:, t]], f['jnt_state'][:, t]
    if not goal:
      states.append(O.state_concatenation(ft, jt))
    elif proc_tgt == 'constant':
      states.append(O.representation_concatenation(ft, feat[tindex], jt))
    else:
      states.append(O.state_concatenation(feat[tindex] - ft, jt))
  ep = O.lstm_decoder(states, P, scope + '/LSTMDecoder', ocfg)
  pred2 = {'cmd_ee': ep['pred_cmd_ee'], 'logits_cmd_grp': ep['logits_cmd_grp'], 'pos_ee': ep['pred_aux_ee'],
           'pos_obj': ep['pred_aux_obj']}
  loss_shared, _ = O.model_loss(pred2, O.build_targets(f, l, ocfg), P, ocfg)
  assert abs(float(loss_dense) - float(loss_shared)) <= 1e-12 * abs(float(loss_dense)), (float(loss_dense), float(loss_shared))
