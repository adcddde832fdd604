"""Input gradients on the GPU: the three entry points against the float64 restatements of tests/_input_grad_ref.py,
the whole pass against the oracle under the device's ReLU decisions, head selection through the Estimator, and the saliency script.

Tolerances: conv1's input gradient to the per-kernel standard of tests/test_kernels_gpu.py (rtol 2e-5 + atol 2e-5 at unit-scale
inputs); everything that normalises or sums over a sample to ``rel_max`` and ``rel_l2`` <= 2e-5 of tests/_relu_taps.py; the channel
pack's adjoint bitwise (it moves floats and adds at most once per element).

tests/test_input_grad_variants_gpu.py holds the three entry points at every instantiation and launch form (the one-float dynimg
kernels, strided and misaligned layouts, ties across blocks, the flat sample, null outputs) with NaN slack and a derived bound per
element, and the chunk loop of ``input_gradient`` with repeated calls.  What this file still holds on its own: the whole pass against
the oracle under the device's ReLU decisions in every mode, with the training step's bitwise twin; head selection through the
Estimator; scripts/saliency.py."""
import hashlib
import importlib.util
import os

import numpy as np
import pytest
import torch

import _input_grad_ref as R
import _relu_taps as T
from oracle import geeco_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HI, LO = 5.0, -4.0      # planted pixel values: beyond every input range of the tests (rgb in [0, 1], depth in [0.5, 3])


def _close(a, b, rtol, atol, what=''):
  a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
  assert a.shape == b.shape, (what, a.shape, b.shape)
  err, tol = np.abs(a - b), atol + rtol * np.abs(b)
  print('%s: max err %.3e, max |ref| %.3e' % (what, err.max(), np.abs(b).max()))
  assert np.all(err <= tol), '%s: max err %.3e (tol %.3e) at %s' % (what, err.max(), tol.flat[err.argmax()],
                                                                     np.unravel_index(err.argmax(), err.shape))


def _norms(got, ref, what):
  e_max, e_l2 = T.rel_max(got, ref), T.rel_l2(got, ref)
  print('%s: rel_max %.3e, rel_l2 %.3e (bound %.0e)' % (what, e_max, e_l2, T.GRAD_TOL))
  assert np.isfinite(np.asarray(got)).all(), what
  assert e_max <= T.GRAD_TOL and e_l2 <= T.GRAD_TOL, (what, e_max, e_l2)


# ---- 1. geeco_conv1_dgrad ------------------------------------------------------------------------------------------------
CONV1_CASES = [(1, 1, 1, 1, 3), (1, 2, 3, 5, 3), (2, 3, 17, 19, 4), (1, 2, 64, 67, 3), (3, 2, 136, 136, 3)]


@pytest.mark.parametrize('G,F,H,W,Cin', CONV1_CASES)
def test_conv1_dgrad(dev, G, F, H, W, Cin):
  from geeco_amd import ops
  r = np.random.default_rng(31)
  dz = r.standard_normal([G, F, H, W, 32]).astype(np.float32)
  dz *= r.random(dz.shape) < 0.5                       # about half the entries zero, as after a ReLU gradient
  w = (r.standard_normal([G, 3, 3, Cin, 32]) / np.sqrt(9 * 32)).astype(np.float32)
  dx = torch.full((G, F, H, W, 4), float('nan'), device=dev)
  assert ops.conv1_dgrad_into(dx, torch.tensor(dz, device=dev), torch.tensor(w, device=dev), G, F * H * W * 32, 9 * Cin * 32,
                              F * H * W * 4, F, H, W, Cin)
  torch.cuda.synchronize()
  got = dx.cpu().numpy()
  for g in range(G):
    _close(got[g][..., :Cin], R.conv1_dgrad_ref(dz[g], w[g]), 2e-5, 2e-5, 'conv1 dgrad, group %d' % g)      # every element
  if Cin == 3:
    assert not got[..., 3].any() and not np.signbit(got[..., 3]).any()      # exactly +0


def test_conv1_dgrad_refuses_other_layers(dev):
  from geeco_amd import ops
  dz, w, dx = torch.zeros(1, 4, 4, 48, device=dev), torch.zeros(3, 3, 3, 48, device=dev), torch.full((1, 4, 4, 4), 7.0, device=dev)
  assert ops.conv1_dgrad_into(dx, dz, w, 1, 0, 0, 0, 1, 4, 4, 3, Cout=48) is False
  assert ops.conv1_dgrad_into(dx, dz, w, 1, 0, 0, 0, 1, 4, 4, 8, Cout=32) is False
  torch.cuda.synchronize()
  assert bool((dx == 7.0).all())      # nothing was launched


# ---- 2. geeco_pack_pixels_bwd --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('accumulate', [False, True], ids=['overwrite', 'accumulate'])
@pytest.mark.parametrize('rgbd', [False, True], ids=['rgb', 'rgbd'])
def test_pack_pixels_bwd_is_bitwise(dev, accumulate, rgbd):
  """Strided source: frame t of an [N][K] window stack, as the time-major pack reads it."""
  from geeco_amd import ops
  r = np.random.default_rng(32)
  N, K, HW, t = 3, 4, 17 * 19, 2
  g = r.standard_normal([N, HW, 4]).astype(np.float32)
  a0 = r.standard_normal([N, K, HW, 3]).astype(np.float32)
  b0 = r.standard_normal([N, K, HW, 1]).astype(np.float32)
  a, b = torch.tensor(a0, device=dev), torch.tensor(b0, device=dev)
  kw = dict(d_src2=b[:, t], src2_sample_stride=K * HW, C2=1, accumulate2=accumulate) if rgbd else {}
  ops.pack_pixels_bwd_into(a[:, t], torch.tensor(g, device=dev), K * HW * 3, N, HW, 3, 4, accumulate=accumulate, **kw)
  torch.cuda.synchronize()
  ra, rb = R.pack_bwd_ref(g, 3, d_src=a0[:, t] if accumulate else None, C2=1, d_src2=b0[:, t] if accumulate else None)
  want_a, want_b = a0.copy(), b0.copy()
  want_a[:, t] = ra
  if rgbd:
    want_b[:, t] = rb
  assert np.array_equal(a.cpu().numpy(), want_a) and np.array_equal(b.cpu().numpy(), want_b)      # the other frames untouched


# ---- 3. geeco_dynimg_bwd -------------------------------------------------------------------------------------------------
def _dynimg_bwd(dev, g, frames, accumulate, two_frame, Cpad=4):
  """Device run on frames [N][K][HW][C] (two_frame: K == 2, frame 1 passed as frames2) -> d_frames as numpy, and the start values."""
  from geeco_amd import ops
  N, K, HW, C = frames.shape
  r = np.random.default_rng(33)
  start = r.standard_normal(frames.shape).astype(np.float32) if accumulate else np.full(frames.shape, np.nan, np.float32)
  gp = np.full([N, HW, Cpad], np.nan, np.float32)      # channels >= C are ignored: NaN there must not reach the result
  gp[..., :C] = g
  ws = ops.dynimg_bwd_ws(N, HW, C, dev)
  gd = torch.tensor(gp, device=dev)
  if two_frame:
    f0, f1 = torch.tensor(frames[:, 0].copy(), device=dev), torch.tensor(frames[:, 1].copy(), device=dev)
    d0, d1 = torch.tensor(start[:, 0].copy(), device=dev), torch.tensor(start[:, 1].copy(), device=dev)
    ops.dynimg_bwd_into(d0, gd, f0, 2, N, HW, C, Cpad, ws, HW * C, 0, HW * C, 0, accumulate=accumulate, frames2=f1, d_frames2=d1,
                        accumulate2=accumulate)
    torch.cuda.synchronize()
    return np.stack([d0.cpu().numpy(), d1.cpu().numpy()], axis=1), start
  fd, dd = torch.tensor(frames, device=dev), torch.tensor(start, device=dev)
  ops.dynimg_bwd_into(dd, gd, fd, K, N, HW, C, Cpad, ws, K * HW * C, HW * C, K * HW * C, HW * C, accumulate=accumulate)
  torch.cuda.synchronize()
  return dd.cpu().numpy(), start


DYN_CASES = [(1, 1, 4, 3, False), (2, 2, 36, 3, True), (3, 4, 17 * 19, 4, False), (2, 16, 136 * 136, 3, False)]


@pytest.mark.parametrize('accumulate', [False, True], ids=['overwrite', 'accumulate'])
@pytest.mark.parametrize('N,K,HW,C,two_frame', DYN_CASES)
def test_dynimg_bwd(dev, N, K, HW, C, two_frame, accumulate):
  r = np.random.default_rng(34)
  frames = r.random([N, K, HW, C], dtype=np.float32)
  g = r.standard_normal([N, HW, C]).astype(np.float32)
  if K > 1:
    R.plant_extrema(frames, seed=2)
    assert R.extrema_margin(frames) >= 1e-3      # fp32 and fp64 agree on the positions
  ref = R.dynimg_bwd_ref(g, frames)
  got, start = _dynimg_bwd(dev, g, frames, accumulate, two_frame)
  again, _ = _dynimg_bwd(dev, g, frames, accumulate, two_frame)
  assert np.array_equal(got, again)              # fixed summation order, no atomics
  delta = got.astype(np.float64) - start if accumulate else got
  if K == 1:      # alpha = [0]
    assert not ref.any() and (np.array_equal(got, start) if accumulate else not got.any())
    return
  if accumulate:  # (what the one fp32 addition into the start values rounds away is not the kernel's error: compare before it)
    plain, _ = _dynimg_bwd(dev, g, frames, False, two_frame)
    assert np.array_equal(got, start + plain)
    delta = plain
  _norms(delta, ref, 'dynimg_bwd N=%d K=%d HW=%d C=%d' % (N, K, HW, C))


def test_dynimg_bwd_shares_a_tie_evenly(dev):
  """Two bitwise-equal maxima (two elements identical in every frame): each takes half of the maximum's term."""
  r = np.random.default_rng(35)
  N, K, HW, C = 1, 3, 40, 3
  frames = r.random([N, K, HW, C], dtype=np.float32)
  alpha = O.dynimg_alpha(K)
  i, j = (7, 1), (29, 2)
  for t in range(K):
    frames[0, t][i] = frames[0, t][j] = 2.0 if alpha[t] > 0 else -1.0
    frames[0, t, 3, 0] = -1.0 if alpha[t] > 0 else 2.0      # (a unique minimum)
  g = r.standard_normal([N, HW, C]).astype(np.float32)
  g[0][i] = g[0][j] = 0.0
  got, _ = _dynimg_bwd(dev, g, frames, False, False)
  ref = R.dynimg_bwd_ref(g, frames)
  assert ref[0, 0][i] == ref[0, 0][j] != 0.0
  for t in range(K):
    assert got[0, t][i] == got[0, t][j]
  _norms(got, ref, 'dynimg_bwd with a tie')


# ---- 4. the whole pass ---------------------------------------------------------------------------------------------------
def _mk(cfg_kw, goal, N, H, seed=1):
  ocfg = O.make_config(**dict(cfg_kw, img_height=H, img_width=H, batch_size=N))
  P = O.init_params(O.model_param_shapes(ocfg, goal), seed=seed)
  r = np.random.default_rng(seed + 1)
  for k in P:
    if k.endswith('/bias'):
      P[k] = (0.05 * r.standard_normal(P[k].shape)).astype(np.float32)
  feats, labels = O.synthetic_batch(ocfg, goal, N, seed=seed + 2, H=H, W=H)
  return ocfg, P, feats, labels


def _build(ocfg, goal, P, feats, labels, dev):
  from geeco_amd import graph
  from geeco_amd.params import create_e2evmc_config
  model = (graph.GoalE2EVMC if goal else graph.E2EVMC)(create_e2evmc_config(ocfg._asdict()), feats['rgb'].shape[0], dev, training=True)
  model.store.load_numpy(P)
  model.load_batch({k: torch.from_numpy(v) for k, v in feats.items()}, {k: torch.from_numpy(v) for k, v in labels.items()})
  return model


def _plant(feats, ocfg, goal):
  """Planted extrema for every dynamic image the graph forms (the buffer image of geeco-f; the (frame, target) pair images), in
  channel 0 of four fixed pixels; asserts the margins in float64 before anything runs on the device."""
  rgb, K = feats['rgb'], ocfg.window_size
  N, _, H, W, _ = rgb.shape
  pA, pB, pC, pD = (3, 5), (H - 2, 7), (11, W - 3), (H // 2, W // 2)
  stack = lambda f: np.concatenate([f['rgb'], f['depth']], -1) if ocfg.img_channels == 4 else f['rgb']
  tgt_of = lambda f: np.concatenate([f['target_rgb'], f['target_depth']], -1) if ocfg.img_channels == 4 else f['target_rgb']
  if goal and ocfg.proc_obs == 'dynimg' and K > 1:
    alpha = O.dynimg_alpha(K)
    for t in range(K):
      rgb[:, t, pA[0], pA[1], 0] = HI if alpha[t] > 0 else LO
      rgb[:, t, pB[0], pB[1], 0] = LO if alpha[t] > 0 else HI
  pairs = []
  if goal and (ocfg.proc_obs == 'dynimg' or ocfg.proc_tgt == 'dyndiff'):      # alpha of a pair = (-0.5, 0.5)
    ts = [K - 1] if ocfg.proc_obs == 'dynimg' else range(K)
    for t in ts:
      rgb[:, t, pC[0], pC[1], 0], rgb[:, t, pD[0], pD[1], 0] = LO, HI
    feats['target_rgb'][:, pC[0], pC[1], 0], feats['target_rgb'][:, pD[0], pD[1], 0] = HI, LO
    pairs = [np.stack([stack(feats)[:, t], tgt_of(feats)], 1) for t in ts]
  if goal and ocfg.proc_obs == 'dynimg' and K > 1:
    assert R.extrema_margin(stack(feats)) >= 1e-3
  for p in pairs:
    assert R.extrema_margin(p) >= 1e-3


def _frame_gradient_refs(model, ocfg, goal, feats, dx_ref):
  """Step two: the float64 input-stage adjoints applied to the oracle's d(loss)/d(x_in) (dx_ref[(scope, call)] [N][H][W][C])."""
  K, C = ocfg.window_size, ocfg.img_channels
  frames = (np.concatenate([feats['rgb'], feats['depth']], -1) if C == 4 else feats['rgb']).astype(np.float64)
  tgt = None
  if goal:
    tgt = (np.concatenate([feats['target_rgb'], feats['target_depth']], -1) if C == 4 else feats['target_rgb']).astype(np.float64)
  d_frames, d_tgt = np.zeros_like(frames), (np.zeros_like(tgt) if goal else None)
  sc = model.enc.scopes

  def pair(g, t):
    d = R.dynimg_bwd_ref(g, np.stack([frames[:, t], tgt], 1))
    d_frames[:, t] += d[:, 0]
    d_tgt[...] += d[:, 1]

  if not goal:
    for k in range(K):
      d_frames[:, k] += dx_ref[(sc[0], k)]
  elif model.mode == 'dynimg':
    d_frames[:, K - 1] += dx_ref[(sc[0], 0)]
    d_frames += R.dynimg_bwd_ref(dx_ref[(sc[1], 0)], frames)
    pair(dx_ref[(sc[2], 0)], K - 1)
  elif model.mode in ('seq_constant', 'seq_residual'):
    d_tgt += dx_ref[(sc[0], 0)]
    for k in range(K):
      d_frames[:, k] += dx_ref[(sc[0], 1 + k)]
  else:
    for k in range(K):
      d_frames[:, k] += dx_ref[(sc[0], k)]
      pair(dx_ref[(sc[1], k)], k)
  out = {'rgb': d_frames[..., :3]}
  if goal:
    out['target_rgb'] = d_tgt[..., :3]
  if C == 4:
    out['depth'] = d_frames[..., 3:]
    if goal:
      out['target_depth'] = d_tgt[..., 3:]
  return out


GRAPH_CASES = [
    ('geeco-f rgb', dict(proc_obs='dynimg', proc_tgt='dyndiff', window_size=4), True, 2, 160),
    ('geeco-f rgbd', dict(proc_obs='dynimg', proc_tgt='dyndiff', window_size=3, img_channels=4, lambda_aux=0.5), True, 2, 136),
    ('e2e_vmc rgb', dict(window_size=3), False, 2, 144),
    ('goal seq constant', dict(proc_obs='sequence', proc_tgt='constant', window_size=2), True, 2, 136),
    ('goal seq residual', dict(proc_obs='sequence', proc_tgt='residual', window_size=3), True, 2, 136),
    ('goal seq dyndiff', dict(proc_obs='sequence', proc_tgt='dyndiff', window_size=2), True, 2, 136),
    ('geeco-f N=1 K=1', dict(proc_obs='dynimg', proc_tgt='dyndiff', window_size=1), True, 1, 136),
]


@pytest.mark.parametrize('name,cfg_kw,goal,N,H', GRAPH_CASES, ids=[c[0] for c in GRAPH_CASES])
def test_input_gradients_whole_graph(dev, name, cfg_kw, goal, N, H):
  ocfg, P, feats, labels = _mk(dict(cfg_kw, lr=1e-3), goal, N, H)
  _plant(feats, ocfg, goal)
  model = _build(ocfg, goal, P, feats, labels, dev)
  twin = _build(ocfg, goal, P, feats, labels, dev)
  C = ocfg.img_channels
  model.forward(backward_too=True)
  torch.cuda.synchronize()
  masks = T.snapshot_masks(model.enc)
  model.backward()
  torch.cuda.synchronize()
  st = model.store
  before = {k: getattr(st, k).clone() for k in ('params', 'adam_m', 'adam_v', 'grads')}
  step0 = int(st.global_step.item())
  grads = model.input_gradients()
  torch.cuda.synchronize()
  for k, v in before.items():
    assert torch.equal(getattr(st, k), v), k
  assert int(st.global_step.item()) == step0 and st.ema is None

  # step one: the oracle under the device's ReLU decisions on the device's conv1 inputs, those as float64 leaves
  tap, slots = T.device_tap(model, goal, masks, C)
  leaves = {}

  def inputs_fn(scope, call):
    g, f0, n = slots[(scope, call)]
    leaves[(scope, call)] = x = model.enc.x_in[g][f0:f0 + n][..., :C].cpu().double().requires_grad_(True)
    return x
  tap.inputs_fn = inputs_fn
  O.OracleTrainer(ocfg, goal, P, dtype=torch.float64).loss_and_grads(feats, labels, tap=tap)
  T.check_decisions(tap.stats)
  assert sorted(leaves) == sorted(slots) and all(x.grad is not None for x in leaves.values())
  dx_ref = {k: x.grad.numpy() for k, x in leaves.items()}
  dx = model.enc.dx_in.cpu().numpy()
  order = sorted(slots)
  got = np.concatenate([dx[slots[k][0]][slots[k][1]:slots[k][1] + slots[k][2]][..., :C].reshape(-1) for k in order])
  _norms(got, np.concatenate([dx_ref[k].reshape(-1) for k in order]), '%s: dx_in' % name)
  if C == 3:
    assert not dx[..., 3].any()

  # step two: the float64 input-stage adjoints on top
  refs = _frame_gradient_refs(model, ocfg, goal, feats, dx_ref)
  assert sorted(grads) == sorted(refs)
  for k, ref in refs.items():
    assert tuple(grads[k].shape) == tuple(feats[k].shape), k
    _norms(grads[k].cpu().numpy(), ref, '%s: d %s' % (name, k))

  # the training step is what it was: one on this model equals one on a twin that never ran the pass, bitwise
  model.train_step()
  twin.train_step()
  torch.cuda.synchronize()
  for k in ('params', 'adam_m', 'adam_v', 'grads'):
    assert torch.equal(getattr(st, k), getattr(twin.store, k)), k
  assert float(model.loss) == float(twin.loss) and int(st.global_step.item()) == int(twin.store.global_step.item()) == step0 + 1


# ---- 5. head selection through the Estimator ---------------------------------------------------------------------------
def _digest(path):
  with open(path, 'rb') as f:
    return hashlib.sha256(f.read()).hexdigest()


def test_estimator_input_gradients_heads(dev, tmp_path):
  from geeco_amd import estimator as est, graph
  from geeco_amd.params import create_e2evmc_config
  from geeco_amd.synthetic import synthetic_batches
  cfg = create_e2evmc_config(dict(proc_obs='dynimg', proc_tgt='dyndiff', window_size=2, img_height=136, img_width=136, batch_size=2))
  input_fn = synthetic_batches(2, 2, 2, (136, 136), 3, True, seed=77)
  batches = list(input_fn())
  e = est.Estimator(est.goal_e2evmc_model_fn, model_dir=str(tmp_path), params={'e2evmc_config': cfg, 'use_hipgraph': False})
  feats_only = [{k: v for k, v in f.items() if k in ('rgb', 'target_rgb', 'jnt_state', 'step')} for f, _ in batches]
  preds = list(e.predict(lambda: iter(feats_only)))
  ckpt = est.save_checkpoint(e._store, str(tmp_path), 5) + '.pt'
  digest, state = _digest(ckpt), {k: getattr(e._store, k).clone() for k in ('params', 'adam_m', 'adam_v')}
  listing, step0 = sorted(os.listdir(str(tmp_path))), int(e._store.global_step.item())
  ee = list(e.input_gradients(input_fn, heads=('cmd_ee',)))
  full = list(e.input_gradients(input_fn))
  assert len(ee) == len(full) == len(preds) == 2
  assert _digest(ckpt) == digest and sorted(os.listdir(str(tmp_path))) == listing and int(e._store.global_step.item()) == step0
  for k, v in state.items():
    assert torch.equal(getattr(e._store, k), v), k
  # the same pass on a model whose decoder got the weights (1, 0, 0, 0)
  model = graph.GoalE2EVMC(cfg, 2, dev, training=True)
  model.store.params.copy_(e._store.params)
  model.decoder.head_weights = [1.0, 0.0, 0.0, 0.0]
  for b, (f, l) in enumerate(batches):
    model.load_batch({k: torch.as_tensor(v) for k, v in f.items()}, {k: torch.as_tensor(v) for k, v in l.items()})
    model.forward(backward_too=True)
    model.backward()
    want = {k: v.cpu().numpy() for k, v in model.input_gradients().items()}
    torch.cuda.synchronize()
    assert sorted(want) == ['rgb', 'target_rgb']
    for k, v in want.items():
      assert np.array_equal(ee[b][k], v), k
      assert v.any() and not np.array_equal(ee[b][k], full[b][k]), k      # another loss, another gradient
    assert ee[b]['loss'] != full[b]['loss']
    for k, v in preds[b].items():
      assert np.array_equal(ee[b][k], v) and np.array_equal(full[b][k], v), k
  with pytest.raises(ValueError, match='cmd_ee'):
    next(e.input_gradients(input_fn, heads=('no_such_head',)))


# ---- 6. scripts/saliency.py ----------------------------------------------------------------------------------------------
def test_saliency_script_synthetic(dev, tmp_path):
  spec = importlib.util.spec_from_file_location('saliency_script', os.path.join(ROOT, 'scripts', 'saliency.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  out = str(tmp_path / 'sal.npz')
  mod.main(['--synthetic', '--img_size', '136', '--window_size', '2', '--num_windows', '3', '--batch_size', '2', '--heads', 'cmd_grp',
            '--out', out])
  z = np.load(out)
  assert z['rgb'].shape == z['grad_rgb'].shape == (3, 2, 136, 136, 3)
  assert z['target_rgb'].shape == z['grad_target_rgb'].shape == (3, 136, 136, 3)
  assert z['saliency'].shape == (3, 2, 136, 136) and z['saliency_target'].shape == (3, 136, 136)
  assert np.array_equal(z['saliency'], np.abs(z['grad_rgb']).max(axis=-1)) and z['saliency'].any()
  assert np.array_equal(z['saliency_target'], np.abs(z['grad_target_rgb']).max(axis=-1))
  assert z['loss'].shape == (2,) and np.isfinite(z['loss']).all()
