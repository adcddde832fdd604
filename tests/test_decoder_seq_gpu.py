"""The one-launch K-step inference decoder (geeco_lstm_seq_heads_fwd) on the GPU: against the float64 oracle's lstm_cell loop + fc1
+ heads, step 0 without wh, bitwise independence of a sample from N / its index / its neighbours, against the launch-per-step
chain it replaces inside LSTMDecoder, and through the batched predictor classes."""
import numpy as np
import pytest
import torch

from oracle import geeco_oracle as O
from test_batched_predictor_gpu import _model_dir, _streams
from test_incremental_predictor_gpu import _compare, _oracle_outputs

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-5, 2e-5      # the per-kernel standard
CARTESIAN = (3, 3, 3, 3)
G = 1                        # samples per workgroup of the kernel


def _velocity_sizes():
  from geeco_amd import graph
  from geeco_amd.params import create_e2evmc_config
  return tuple(h[2] for h in graph.head_table(create_e2evmc_config(dict(control_mode='velocity'))))


class Problem:
  """Random decoder inputs in float32 (gates far from saturation) and the float64 oracle's outputs for them."""

  def __init__(self, seed, N, T, H, Hfc, sizes, D=20, pad=12):
    r = np.random.default_rng(seed)
    f32 = np.float32
    self.N, self.T, self.H, self.Hfc, self.sizes, self.D, self.pad = N, T, H, Hfc, tuple(sizes), D, pad
    self.zx = r.standard_normal((T, N, 4 * H)).astype(f32)
    self.kernel = r.standard_normal((D + H, 4 * H)).astype(f32) / f32(np.sqrt(H))      # lstm_cell/kernel: wh = rows D..
    self.bias = (0.1 * r.standard_normal(4 * H)).astype(f32)
    self.fc1_w = (r.standard_normal((H, Hfc)) / np.sqrt(H)).astype(f32)
    self.fc1_b = (0.1 * r.standard_normal(Hfc)).astype(f32)
    self.heads_w = [(r.standard_normal((Hfc, s)) / np.sqrt(Hfc)).astype(f32) for s in sizes]
    self.heads_b = [(0.1 * r.standard_normal(s)).astype(f32) for s in sizes]

  def oracle(self, zx=None):
    """O.lstm_cell over x_t = zx_t with the kernel [I | wh] (the identity rows hand zx through exactly), then fc1 and the heads as
    O.lstm_decoder forms them."""
    zx = self.zx if zx is None else zx
    T, N, H = zx.shape[0], zx.shape[1], self.H
    t64 = lambda a: torch.tensor(a, dtype=torch.float64)
    kernel = torch.cat([torch.eye(4 * H, dtype=torch.float64), t64(self.kernel[self.D:])], dim=0)
    c = h = torch.zeros(N, H, dtype=torch.float64)
    for t in range(T):
      c, h = O.lstm_cell(t64(zx[t]), c, h, kernel, t64(self.bias))
    net = torch.relu(h @ t64(self.fc1_w) + t64(self.fc1_b))
    preds = torch.cat([net @ t64(w) + t64(b) for w, b in zip(self.heads_w, self.heads_b)], dim=1)
    return preds.numpy(), h.numpy(), c.numpy()

  def run(self, dev, zx=None, state=True, kernel=None):
    """The kernel on zx rows of pitch 4H + pad and wh inside the [D + H][4H] cell kernel; returns preds (and h_last, c_last)."""
    from geeco_amd import ops
    zx = self.zx if zx is None else zx
    T, N, H = zx.shape[0], zx.shape[1], self.H
    ldz = 4 * H + self.pad
    buf = torch.full((T * N, ldz), 1e30, device=dev)
    buf[:, :4 * H] = torch.from_numpy(zx.reshape(T * N, 4 * H)).to(dev)
    d = lambda a: torch.from_numpy(a).to(dev)
    W = d(self.kernel if kernel is None else kernel)
    preds = torch.full((N, sum(self.sizes)), float('nan'), device=dev)
    h_last = torch.full((N, H), float('nan'), device=dev) if state else None
    c_last = torch.full((N, H), float('nan'), device=dev) if state else None
    ok = ops.lstm_seq_heads_into(preds, buf, W[self.D:], d(self.bias), d(self.fc1_w), d(self.fc1_b), [d(w) for w in self.heads_w],
                                 [d(b) for b in self.heads_b], list(self.sizes), N, T, H, self.Hfc, ldz, 4 * H, h_last=h_last,
                                 c_last=c_last)
    assert ok
    torch.cuda.synchronize()
    return (preds.cpu().numpy(),) + ((h_last.cpu().numpy(), c_last.cpu().numpy()) if state else ())


@pytest.mark.parametrize('table', ['cartesian', 'velocity'])
@pytest.mark.parametrize('Hfc', [64, 128])
@pytest.mark.parametrize('N', sorted({1, 2, G + 1, 37}))
@pytest.mark.parametrize('T', [1, 2, 3, 16])
def test_parity_with_float64_oracle(dev, T, N, Hfc, table):
  """preds, h_last and c_last within rtol 2e-5 + atol 2e-5 of the oracle; zx rows strided, wh inside the cell kernel; the same
  preds bitwise when h_last / c_last are NULL."""
  sizes = CARTESIAN if table == 'cartesian' else _velocity_sizes()
  pb = Problem(1000 * T + 10 * N + Hfc + len(sizes), N, T, 128, Hfc, sizes)
  want = pb.oracle()
  got = pb.run(dev)
  for g, w, what in zip(got, want, ('preds', 'h_last', 'c_last')):
    print('%s T=%d N=%d Hfc=%d %s: max abs err %.3g' % (what, T, N, Hfc, table, np.abs(g - w).max()))
  for g, w, what in zip(got, want, ('preds', 'h_last', 'c_last')):
    np.testing.assert_allclose(g, w, rtol=RTOL, atol=ATOL, err_msg=what)
  alone, = pb.run(dev, state=False)
  np.testing.assert_array_equal(alone, got[0])


@pytest.mark.parametrize('T,H,Hfc', [(17, 128, 128), (33, 128, 64), (64, 128, 128), (5, 100, 64), (4, 32, 128), (3, 1, 64)])
def test_parity_at_the_kernels_own_boundaries(dev, T, H, Hfc):
  """What the kernel treats differently: more steps than one staged chunk of zx (16), the longest T, state widths below 128
  (units and weight rows the workgroup masks off), down to one unit."""
  pb = Problem(7 * T + H, 3, T, H, Hfc, CARTESIAN)
  for g, w, what in zip(pb.run(dev), pb.oracle(), ('preds', 'h_last', 'c_last')):
    print('%s T=%d H=%d: max abs err %.3g' % (what, T, H, np.abs(g - w).max()))
    np.testing.assert_allclose(g, w, rtol=RTOL, atol=ATOL, err_msg=what)


def test_step0_ignores_wh(dev):
  """T = 1: the zero state meets no wh at all -- a wh full of NaN still gives the oracle's finite predictions."""
  pb = Problem(5, 5, 1, 128, 128, CARTESIAN)
  poisoned = pb.kernel.copy()
  poisoned[pb.D:] = np.nan
  preds, h_last, c_last = pb.run(dev, kernel=poisoned)
  want = pb.oracle()
  assert np.isfinite(preds).all() and np.isfinite(h_last).all() and np.isfinite(c_last).all()
  np.testing.assert_allclose(preds, want[0], rtol=RTOL, atol=ATOL)
  np.testing.assert_array_equal(preds, pb.run(dev)[0])


@pytest.mark.parametrize('T', [3, 16])
def test_a_samples_output_is_independent_of_the_batch_bitwise(dev, T):
  """One sample alone (N = 1), then inside N = 37 at index 0, 36 and 17, each time among different random neighbours: four
  bit-identical rows of preds, h_last and c_last."""
  N = 37
  pb = Problem(11, 1, T, 128, 128, _velocity_sizes())
  ref = pb.run(dev)
  assert np.isfinite(ref[0]).all()
  for i, idx in enumerate((0, N - 1, 17)):
    zx = np.random.default_rng(100 + i).standard_normal((T, N, 4 * pb.H)).astype(np.float32)
    zx[:, idx] = pb.zx[:, 0]
    got = pb.run(dev, zx=zx)
    for g, w, what in zip(got, ref, ('preds', 'h_last', 'c_last')):
      np.testing.assert_array_equal(g[idx], w[0], err_msg='%s at index %d' % (what, idx))
    assert not np.array_equal(got[0][(idx + 1) % N], ref[0][0])


def _decoder(dev, one_launch, N=3, T=3, D=1052, seed=3):
  from geeco_amd import graph
  from geeco_amd.params import create_e2evmc_config
  from geeco_amd.variables import VariableStore
  cfg = create_e2evmc_config(dict(window_size=T))
  scope = 'VMC/LSTMDecoder'
  st = VariableStore(O.decoder_param_shapes(scope, D, O.make_config(window_size=T)), dev)
  st.initialize(seed=seed)
  r = np.random.default_rng(seed)
  for name, shp in st.shapes.items():
    if name.endswith('/bias'):
      st.var(name).copy_(torch.from_numpy((0.1 * r.standard_normal(shp)).astype(np.float32)))
  d = graph.LSTMDecoder(st, scope, cfg, N, T, D, False, one_launch=one_launch)
  d.states.copy_(torch.from_numpy(r.standard_normal((T, N, D)).astype(np.float32)))
  labels = torch.zeros(N, 8, device=dev)
  d.targets, d.target_strides = [labels] * len(d.heads), [8] * len(d.heads)
  return d


def test_equals_the_chain_it_replaces(dev):
  """LSTMDecoder with the one-launch path on and off, same variables and states (N = 3, T = 3, D = 1052): preds within the
  batched-vs-batch-1 tolerance of DESIGN 5.11; with it on the decoder holds no gates / c / h history."""
  on, off = _decoder(dev, True), _decoder(dev, False)
  assert torch.equal(on.store.params, off.store.params) and torch.equal(on.states, off.states)
  assert on.one_launch and not off.one_launch
  on.forward(False)
  off.forward(False)
  torch.cuda.synchronize()
  assert on.one_launch                                     # the call did not decline
  assert on.gates is None and on.c is None and on.h is None and on.z is None
  assert off.gates is not None and off.c is not None and off.h is not None
  assert np.abs(off.preds.cpu().numpy()).max() > 1e-3
  np.testing.assert_allclose(on.preds.cpu().numpy(), off.preds.cpu().numpy(), rtol=1e-4, atol=2e-5)
  # training decoders and one-step decoders never take it
  from geeco_amd import graph
  assert not graph.LSTMDecoder(on.store, on.scope, on.cfg, 3, 1, 1052, False, one_launch=True).one_launch
  assert not graph.LSTMDecoder(on.store, on.scope, on.cfg, 3, 3, 1052, True, one_launch=True).one_launch


PUBLIC = [
    (False, dict(), True),
    (False, dict(), False),
    (True, dict(proc_obs='sequence', proc_tgt='residual'), True),
]


@pytest.mark.parametrize('goal,extra,incremental', PUBLIC)
def test_through_the_batched_predictors(dev, tmp_path, goal, extra, incremental):
  """136 x 136, K = 3, B = 3, K + 4 calls with one env reset and (goal model) one goal change: the predictor's decoder runs the
  one-launch path and every output matches the float64 oracle on the same windows."""
  from geeco_amd.batched_predictor import BatchedE2EVMCPredictor, BatchedGoalE2EVMCPredictor
  from test_incremental_predictor_gpu import ATOL as PA, RTOL as PR
  assert (PR, PA) == (1e-4, 2e-5)
  S, K, B = 136, 3, 3
  kw = dict(window_size=K, img_height=S, img_width=S, **extra)
  cfg, P = _model_dir(str(tmp_path), goal, kw)
  C, T = cfg.img_channels, K + 4
  r = np.random.default_rng(41 + goal + 2 * incremental)
  frames, jnts = _streams(r, B, T, S, S, C)
  tgt = r.random((B, S, S, C), dtype=np.float32)
  cls = BatchedGoalE2EVMCPredictor if goal else BatchedE2EVMCPredictor
  p = cls(str(tmp_path), num_envs=B, memcap=None, device=dev, incremental=incremental)
  dec = p._model.decoder
  assert dec.one_launch and dec.T == K and dec.gates is None and dec.h is None
  if goal:
    p.set_goal(tgt)
  ocfg = O.make_config(batch_size=B, **kw)
  Pt = {k: torch.tensor(v, dtype=torch.float64) for k, v in P.items()}
  since = [[] for _ in range(B)]
  for t in range(T):
    if t == K + 1:
      p.reset([B - 1])
      since[B - 1] = []
    if goal and t == K + 2:
      g = r.random((S, S, C), dtype=np.float32)
      tgt[0] = g
      p.set_goal(g, env_ids=[0])
    out = p.predict(frames[t], jnts[t])
    idx = np.zeros((K, B), dtype=np.int64)
    for b in range(B):
      since[b].append(t)
      w = since[b][-K:]
      idx[:, b] = [w[0]] * (K - len(w)) + w
    wf = np.stack([frames[idx[:, b], b] for b in range(B)], axis=1)
    wj = np.stack([jnts[idx[:, b], b] for b in range(B)], axis=1)
    _compare(out, _oracle_outputs(ocfg, Pt, goal, wf, wj, tgt), cfg.control_mode == 'cartesian', 'vs oracle, call %d' % t)
  assert dec.one_launch


def test_estimator_models_keep_the_chain(dev):
  """Models built without the argument (Estimator: train, evaluate, predict) run today's decoder."""
  from geeco_amd import graph
  from geeco_amd.params import create_e2evmc_config
  cfg = create_e2evmc_config(dict(window_size=3, img_height=136, img_width=136, batch_size=2))
  for training in (False, True):
    m = graph.E2EVMC(cfg, 2, dev, training=training)
    assert not m.decoder.one_launch and m.decoder.gates is not None and m.decoder.h is not None
