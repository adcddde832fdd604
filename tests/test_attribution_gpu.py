"""Attributions on the GPU: the three kernels against the float32 restatements of tests/_attribution_ref.py, and the
whole pass against the fp64 oracle differentiated at the same path points.

Standards.  Path point at sigma = 0, accumulate and finish (attr, saliency, sample_sum): BITWISE the host model.  Path point at
sigma > 0: the bound of tests/test_augment_scene_gpu.py (``bound``: 1e-6 + 3e-6 sigma) on the same generator, and different from
the sigma = 0 result.  Whole pass: the standard of tests/test_input_grad_gpu.py -- the oracle's backward under the device's ReLU
decisions at every path point, ``rel_max`` and ``rel_l2`` <= ``_relu_taps.GRAD_TOL``.  The path points the oracle is differentiated
at are the device's, read back from a twin model that the path-point kernel wrote with the pass's own arguments, after they have
been compared with the host-built points (bitwise at sigma = 0, within ``bound`` for SmoothGrad): a point that differs from the
device's in its last bits could take another side of a ReLU than the device did, which is a property of the model, not an error.
The completeness gap, per sample, is compared with the oracle's gap at the same M (the oracle's loss of each sample alone, over N); it
is not asserted to be small.  Its bound: each of its three terms (the sample's attribution sum, loss_n(x), loss_n(b)) is held to a
relative GRAD_TOL, so |gap_n - gap_ref_n| <= GRAD_TOL * (sum |attr_ref_n| + |loss_n(x)| + |loss_n(b)|).
``test_baseline_forms_reach_the_kernels`` and the Estimator / script tests at the end compare with the host model on the device's
own gradient (bitwise), not with the oracle: what they check is routing, not arithmetic."""
import os

import numpy as np
import pytest
import torch

import _attribution_ref as A
import _input_grad_ref as R
import _relu_taps as T
import test_input_grad_gpu as G
from oracle import geeco_oracle as O
from test_augment_scene_gpu import bound

pytestmark = pytest.mark.gpu
KEY = 0x85a308d3243f6a88
GRID_PASS = 2048 * 256 * 4      # elements of one pass of the grid-stride loops (csrc/attribution.hip: AT_MAX_BLOCKS x AT_THREADS x 4)


def _bits(a):
  return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _dev(a, dev, offset=0):
  """``a`` on the device; ``offset`` floats past a 16-byte boundary (1..3: the one-float access path)."""
  a = np.asarray(a, np.float32)
  buf = torch.empty(a.size + 4, dtype=torch.float32, device=dev)
  t = buf[offset:offset + a.size].view(a.shape)
  t.copy_(torch.from_numpy(a))
  return t


def _baseline(r, kind, shape, C):
  if kind == 'null':
    return None
  if kind == 'full':
    return r.random(shape, dtype=np.float32)
  return r.random(shape[-3:-1] + (C,), dtype=np.float32)      # one frame, broadcast


# (shape [N][frames][H][W][C], baseline kind, offset of the tensors): the vector tail (n = 4 k + 3), more than one grid pass, frame
# baselines whose period is and is not a multiple of 4, a null and a full baseline, the one-float path
POINT_CASES = [
    ((1, 1, 1, 5, 3), 'null', 0), ((1, 1, 1, 5, 3), 'full', 0), ((1, 1, 1, 5, 3), 'frame', 1),      # n = 15 = 4 * 3 + 3
    ((2, 3, 17, 19, 3), 'frame', 0),      # period 969, no multiple of 4
    ((2, 3, 6, 6, 4), 'frame', 0),        # period 144, C = 4: the 16-byte baseline path
    ((2, 2, 8, 8, 3), 'frame', 0),        # period 192, C = 3, a multiple of 4
    ((2, 3, 17, 19, 3), 'full', 3),
    ((1, 2, 620, 620, 3), 'frame', 0),    # 2 306 400 elements: more than one pass of the grid (2 097 152)
]
IDS = ['%s-%s-off%d' % ('x'.join(map(str, s)), k, o) for s, k, o in POINT_CASES]


@pytest.mark.parametrize('shape,kind,offset', POINT_CASES, ids=IDS)
def test_path_point(dev, shape, kind, offset):
  from geeco_amd import ops
  r = np.random.default_rng(41)
  n = int(np.prod(shape))
  x = r.random(shape, dtype=np.float32)
  b = _baseline(r, kind, shape, shape[-1])
  xd, bd = _dev(x, dev, offset), (None if b is None else _dev(b, dev, offset if kind == 'full' else 0))
  dst = _dev(np.full(shape, np.nan, np.float32), dev, offset)
  for alpha in (0.0, 0.375, 1.0):
    ops.attr_path_point_into(dst, xd, bd, alpha)
    got = dst.cpu().numpy()
    assert np.array_equal(_bits(got), _bits(A.path_point(x, b, alpha))), alpha
  if kind == 'null':
    assert np.array_equal(_bits(got), _bits(x))      # alpha = 1 from black: the input itself
  # the noise: within the generator's bound of the float64 restatement, different from the clean point, the same on a second run
  sigma, alpha, step = 0.15, 0.375, 5
  clean = A.path_point(x, b, alpha)
  ops.attr_path_point_into(dst, xd, bd, alpha, sigma, KEY, step)
  noisy = dst.cpu().numpy()
  ops.attr_path_point_into(dst, xd, bd, alpha, sigma, KEY, step)
  assert np.array_equal(_bits(noisy), _bits(dst.cpu().numpy()))
  want = clean.astype(np.float64) + np.float64(np.float32(sigma)) * A.noise(KEY, step, n).reshape(shape)
  err = np.abs(noisy - want).max()
  print('path point %s: max noise err %.3e (bound %.3e)' % (shape, err, bound(sigma)))
  assert err <= bound(sigma)
  assert (noisy != clean).mean() > 0.99
  ops.attr_path_point_into(dst, xd, bd, alpha, sigma, KEY, step + 1)      # another step, other noise
  assert (dst.cpu().numpy() != noisy).mean() > 0.99


def test_path_point_noise_does_not_depend_on_the_access_path(dev):
  """z(key, step, i) alone: the aligned and the one-float launch give the same bits."""
  from geeco_amd import ops
  x = np.random.default_rng(42).random(4 * 700 + 3, dtype=np.float32)
  out = []
  for offset in (0, 2):
    xd, dst = _dev(x, dev, offset), _dev(np.zeros_like(x), dev, offset)
    ops.attr_path_point_into(dst, xd, None, 1.0, 0.2, KEY, 3)
    out.append(dst.cpu().numpy())
  assert np.array_equal(_bits(out[0]), _bits(out[1]))


@pytest.mark.parametrize('overwrite', [True, False], ids=['overwrite', 'add'])
@pytest.mark.parametrize('n,offset', [(4 * 11 + 3, 0), (4 * 11 + 3, 1), (GRID_PASS + 4 * 301 + 1, 0)], ids=['tail', 'one-float', 'two-passes'])
def test_accumulate(dev, n, offset, overwrite):
  from geeco_amd import ops
  r = np.random.default_rng(43)
  acc0, g = r.standard_normal(n).astype(np.float32), r.standard_normal(n).astype(np.float32)
  g[::7] = -0.0
  if overwrite:
    acc0[::5] = np.nan      # whatever the accumulator held is gone
  for weight in (1.0 / 3.0, 1.0):
    acc = _dev(acc0, dev, offset)
    ops.attr_accumulate_into(acc, _dev(g, dev, offset), weight, overwrite)
    assert np.array_equal(_bits(acc.cpu().numpy()), _bits(A.accumulate(acc0, g, weight, overwrite))), weight


FINISH_CASES = [
    ((1, 1, 1, 5, 3), 'null', 0), ((2, 3, 17, 19, 3), 'frame', 0), ((2, 3, 6, 6, 4), 'frame', 0), ((2, 2, 8, 8, 3), 'frame', 0),
    ((3, 2, 5, 7, 1), 'full', 0), ((2, 1, 9, 7, 2), 'frame', 1), ((2, 3, 17, 19, 3), 'full', 3),
    ((2, 1, 1030, 1024, 3), 'frame', 0),      # 527 360 four-pixel units: more than one pass of the grid (524 288); 773 groups per slot of the sum
]


@pytest.mark.parametrize('multiply', [1, 0], ids=['times-input', 'plain'])
@pytest.mark.parametrize('shape,kind,offset', FINISH_CASES, ids=['%s-%s-off%d' % ('x'.join(map(str, s)), k, o) for s, k, o in FINISH_CASES])
def test_finish(dev, shape, kind, offset, multiply):
  from geeco_amd import ops
  r = np.random.default_rng(44)
  N, frames, H, W, C = shape
  x, acc = r.random(shape, dtype=np.float32), r.standard_normal(shape).astype(np.float32)
  b = _baseline(r, kind, shape, C)
  want_attr, want_sal, want_sum = A.finish(acc, x, b, multiply)
  xd, bd = _dev(x, dev, offset), (None if b is None else _dev(b, dev, offset if kind == 'full' else 0))
  runs = []
  for in_place in (False, True, False):
    accd = _dev(acc, dev, offset)
    attr = accd if in_place else _dev(np.full(shape, np.nan, np.float32), dev, offset)
    sal, sums = _dev(np.full(shape[:-1], np.nan, np.float32), dev, offset), torch.full((N,), float('nan'), device=dev)
    ops.attr_finish_into(attr, sal, sums, accd, xd if multiply else None, bd, multiply, N, frames, H * W, C)
    runs.append((attr.cpu().numpy(), sal.cpu().numpy(), sums.cpu().numpy()))
  for got_attr, got_sal, got_sum in runs:      # out of place, in place, and again: all the host model's bits
    assert np.array_equal(_bits(got_attr), _bits(want_attr))
    assert np.array_equal(_bits(got_sal), _bits(want_sal))
    assert np.array_equal(_bits(got_sum), _bits(want_sum)), (got_sum, want_sum)
  assert np.abs(want_sum - want_attr.astype(np.float64).reshape(N, -1).sum(1)).max() <= 1e-5 * np.abs(want_attr).reshape(N, -1).sum(1).max()


def test_wrappers_refuse_bad_arguments(dev):
  from geeco_amd import ops
  t = lambda *s: torch.zeros(*s, device=dev)
  with pytest.raises(ValueError, match='does not divide'):
    ops.attr_path_point_into(t(10), t(10), t(3), 0.5)
  with pytest.raises(ValueError, match='dst of 8'):
    ops.attr_path_point_into(t(8), t(10), None, 0.5)
  with pytest.raises(ValueError, match='sigma'):
    ops.attr_path_point_into(t(8), t(8), None, 0.5, sigma=-1.0)
  with pytest.raises(ValueError, match='contiguous'):
    ops.attr_accumulate_into(t(4, 4)[:, :2], t(8), 1.0, True)
  with pytest.raises(ValueError, match='C=5'):
    ops.attr_finish_into(t(10), t(2), t(1), t(10), t(10), None, 1, 1, 1, 2, 5)
  buf = t(16)
  from geeco_amd._native import GeecoNativeError
  with pytest.raises(GeecoNativeError, match='overlaps'):
    ops.attr_path_point_into(buf[:8], buf[4:12], None, 0.5)


# ---- the whole pass ------------------------------------------------------------------------------------------------------------
M = 3
PASS_CASES = [
    ('e2e_vmc rgb', dict(window_size=2), False, 2, 136),
    ('goal seq residual', dict(proc_obs='sequence', proc_tgt='residual', window_size=2), True, 2, 136),
    ('geeco-f rgb', dict(proc_obs='dynimg', proc_tgt='dyndiff', window_size=3), True, 2, 136),
    ('geeco-f rgbd', dict(proc_obs='dynimg', proc_tgt='dyndiff', window_size=3, img_channels=4, lambda_aux=0.5), True, 2, 136),
]


def _image_keys(feats):
  return [k for k in A.IMAGE_KEYS if k in feats]


def _oracle_gradient_at(twin, ocfg, goal, P, feats_m, labels):
  """d(loss)/d(image inputs) in float64 at the inputs the twin holds (``feats_m`` = their host copy): the two steps of
  tests/test_input_grad_gpu.py's whole-graph test -- the oracle under the device's ReLU decisions, then the float64 input-stage
  adjoints."""
  C = ocfg.img_channels
  twin.forward(backward_too=True)
  torch.cuda.synchronize()
  masks = T.snapshot_masks(twin.enc)
  tap, slots = T.device_tap(twin, goal, masks, C)
  leaves = {}

  def inputs_fn(scope, call):
    g, f0, n = slots[(scope, call)]
    leaves[(scope, call)] = x = twin.enc.x_in[g][f0:f0 + n][..., :C].cpu().double().requires_grad_(True)
    return x
  tap.inputs_fn = inputs_fn
  loss = O.OracleTrainer(ocfg, goal, P, dtype=torch.float64).loss_and_grads(feats_m, labels, tap=tap)[0]
  T.check_decisions(tap.stats)
  dx_ref = {k: x.grad.numpy() for k, x in leaves.items()}
  return G._frame_gradient_refs(twin, ocfg, goal, feats_m, dx_ref), float(loss)


def _oracle_loss(ocfg, goal, P, feats, labels):
  return float(O.OracleTrainer(ocfg, goal, P, dtype=torch.float64).loss_and_grads(feats, labels)[0])


def _oracle_sample_losses(ocfg, goal, P, feats, labels):
  """float64 [N]: each sample's share of the batch-mean loss -- the oracle's loss of the sample alone, over N (no L2 term in these
  configurations; every loss term is a mean over the batch)."""
  N = feats['rgb'].shape[0]
  one = lambda d, n: {k: v[n:n + 1] for k, v in d.items()}
  return np.array([_oracle_loss(ocfg, goal, P, one(feats, n), one(labels, n)) for n in range(N)]) / N


# integrated gradients on all four; SmoothGrad on a per-frame model and on geeco-f (the loop and the kernels are the same ones)
PASS_RUNS = [(c, 'integrated_gradients') for c in PASS_CASES] + [(PASS_CASES[0], 'smoothgrad'), (PASS_CASES[2], 'smoothgrad')]


@pytest.mark.parametrize('case,method', PASS_RUNS, ids=['%s-%s' % (c[0], m) for c, m in PASS_RUNS])
def test_attributions_against_the_oracle(dev, case, method):
  name, cfg_kw, goal, N, H = case
  from geeco_amd import ops
  from geeco_amd.attribution import input_key
  ig = method == 'integrated_gradients'
  ocfg, P, feats, labels = G._mk(dict(cfg_kw, lr=1e-3), goal, N, H)
  G._plant(feats, ocfg, goal)
  keys = _image_keys(feats)
  sigma, seed = (0.0, 0) if ig else (0.05, 7)
  r = np.random.default_rng(45)
  # integrated gradients: black for the goal models (a time-constant baseline puts a dynamic image on the 1e-6 of its range at
  # alpha -> 0, where float32 and float64 part); a frame baseline for e2e_vmc, which forms no dynamic image
  base = {k: None for k in keys}
  if ig and not goal:
    base['rgb'] = (0.25 * r.random(feats['rgb'].shape[-3:], dtype=np.float32)).astype(np.float32)
  model = G._build(ocfg, goal, P, feats, labels, dev)
  twin = G._build(ocfg, goal, P, feats, labels, dev)
  st = model.store
  before = {k: getattr(st, k).clone() for k in ('params', 'adam_m', 'adam_v')}
  step0 = int(st.global_step.item())
  out = model.attributions(method, M, baseline={k: v for k, v in base.items() if v is not None} or None, noise_std=sigma, seed=seed)
  torch.cuda.synchronize()
  model.check_device_errors()
  for k, v in before.items():
    assert torch.equal(getattr(st, k), v), k
  assert int(st.global_step.item()) == step0 and st.ema is None
  for k in keys:      # the clean inputs are back, bit for bit
    assert np.array_equal(_bits(model.inputs[k].cpu().numpy()), _bits(feats[k])), k

  # the reference: the oracle at the device's path points, which are the host model's
  clean = {k: torch.from_numpy(feats[k]).to(dev) for k in keys}
  based = {k: (None if base[k] is None else torch.from_numpy(base[k]).to(dev).reshape(-1)) for k in keys}
  mean = {k: np.zeros(feats[k].shape, np.float64) for k in keys}
  for m in range(M):
    alpha = (m + 0.5) / M if ig else 1.0
    feats_m = dict(feats)
    for k in keys:
      ops.attr_path_point_into(twin.inputs[k], clean[k], based[k], alpha, sigma, input_key(seed, k), m)
      feats_m[k] = twin.inputs[k].cpu().numpy()
      want = A.path_point(feats[k], base[k], alpha, sigma, A.input_key(seed, k), m)
      if ig:
        assert np.array_equal(_bits(feats_m[k]), _bits(want)), (k, m)
      else:
        assert np.abs(feats_m[k] - want).max() <= bound(sigma) and (feats_m[k] != feats[k]).mean() > 0.99, (k, m)
    if ig and ocfg.proc_obs == 'dynimg' and goal:
      stack = np.concatenate([feats_m['rgb'], feats_m['depth']], -1) if ocfg.img_channels == 4 else feats_m['rgb']
      assert R.extrema_margin(stack) >= 1e-4      # fp32 and fp64 agree on the extrema of the scaled window too
    grads_m, _ = _oracle_gradient_at(twin, ocfg, goal, P, feats_m, labels)
    for k in keys:
      mean[k] += grads_m[k] / M
  ref = {k: (feats[k].astype(np.float64) - A.baseline_of(base[k], feats[k].size).reshape(feats[k].shape)) * mean[k] if ig else mean[k]
         for k in keys}
  for k in keys:
    assert tuple(out[k].shape) == feats[k].shape
    G._norms(out[k].cpu().numpy(), ref[k], '%s %s: attr %s' % (name, method, k))
  sal = out['saliency'].cpu().numpy()
  assert np.array_equal(sal, np.abs(out['rgb'].cpu().numpy()).max(-1)) and sal.any()
  if goal:
    assert np.array_equal(out['saliency_target'].cpu().numpy(), np.abs(out['target_rgb'].cpu().numpy()).max(-1))
  sums_ref = sum(ref[k].reshape(N, -1).sum(1) for k in keys)
  scale = sum(np.abs(ref[k]).reshape(N, -1).sum(1) for k in keys)
  got_sums = out['sample_sum'].cpu().numpy().astype(np.float64)
  print('%s %s: sample_sum %s, ref %s' % (name, method, got_sums, sums_ref))
  assert np.all(np.abs(got_sums - sums_ref) <= T.GRAD_TOL * scale), (got_sums, sums_ref, scale)
  for k in keys:      # the per-input sums are the host order's, bit for bit, on the device's attributions
    assert np.array_equal(_bits(out['sample_sum_by_input'][k].cpu().numpy()),
                          _bits([A.sample_sum(a) for a in out[k].cpu().numpy()])), k
  loss_x = _oracle_loss(ocfg, goal, P, feats, labels)
  assert abs(float(out['loss']) - loss_x) <= 1e-4 * abs(loss_x)
  if ig:
    feats_b = dict(feats)
    for k in keys:
      feats_b[k] = A.baseline_of(base[k], feats[k].size).reshape(feats[k].shape)
    loss_b = _oracle_loss(ocfg, goal, P, feats_b, labels)
    assert abs(float(out['loss_baseline']) - loss_b) <= 1e-4 * abs(loss_b)
    # per sample: the decoder's per-sample loss terms against the oracle's loss of each sample alone
    lx, lb = _oracle_sample_losses(ocfg, goal, P, feats, labels), _oracle_sample_losses(ocfg, goal, P, feats_b, labels)
    assert abs(lx.sum() - loss_x) <= 1e-12 * abs(loss_x) and abs(lb.sum() - loss_b) <= 1e-12 * abs(loss_b)
    gap_ref = sums_ref - (lx - lb)
    gap = out['completeness_gap'].cpu().numpy()
    assert gap.shape == (N,) and gap.dtype == np.float64
    print('%s: completeness gap %s, oracle %s at M = %d (loss %.6f, at the baseline %.6f)' % (name, gap, gap_ref, M, loss_x, loss_b))
    assert np.all(np.abs(gap - gap_ref) <= T.GRAD_TOL * (scale + np.abs(lx) + np.abs(lb))), (gap, gap_ref)
    batch_gap = got_sums.sum() - (float(out['loss']) - float(out['loss_baseline']))      # what the batch-mean losses give
    assert abs(gap.sum() - batch_gap) <= T.GRAD_TOL * (abs(loss_x) + abs(loss_b))
  else:
    assert 'completeness_gap' not in out


def test_one_step_at_alpha_one_is_the_plain_input_gradient(dev):
  """M = 1, alpha = 1, sigma = 0 through the kernels: bit for bit ``input_gradients()``; and a training step after the pass equals
  the step of a twin that never ran it."""
  from geeco_amd import ops
  name, cfg_kw, goal, N, H = PASS_CASES[2]
  ocfg, P, feats, labels = G._mk(dict(cfg_kw, lr=1e-3), goal, N, H)
  model, twin = G._build(ocfg, goal, P, feats, labels, dev), G._build(ocfg, goal, P, feats, labels, dev)
  twin.forward(backward_too=True)
  twin.backward()
  plain = {k: v.clone() for k, v in twin.input_gradients().items()}
  # the kernels called so: the point at alpha = 1 from black into the input buffers, the gradient accumulated with weight 1
  clean = {k: model.inputs[k].clone() for k in plain}
  for k in plain:
    ops.attr_path_point_into(model.inputs[k], clean[k], None, 1.0, 0.0, 0, 0)
    assert torch.equal(model.inputs[k], clean[k])
  model.forward(backward_too=True)
  model.backward()
  got = model.input_gradients()
  for k, g in got.items():
    acc, sal, sums = torch.full_like(g, float('nan')), torch.empty(g.shape[:-1], device=dev), torch.empty(N, device=dev)
    ops.attr_accumulate_into(acc, g.contiguous(), 1.0, True)
    ops.attr_finish_into(acc, sal, sums, acc, None, None, 0, N, 1 if k.startswith('target') else ocfg.window_size, H * H, 3)
    assert torch.equal(acc, plain[k]), k
    assert torch.equal(sal, plain[k].abs().amax(-1)), k
  # smoothgrad with no noise and one step is that pass through the public entry
  out = model.attributions('smoothgrad', 1, noise_std=0.0)
  for k in plain:
    assert torch.equal(out[k], plain[k]), k
  torch.cuda.synchronize()
  st = model.store
  model.train_step()
  twin.train_step()
  torch.cuda.synchronize()
  for k in ('params', 'adam_m', 'adam_v', 'grads'):
    assert torch.equal(getattr(st, k), getattr(twin.store, k)), k
  assert float(model.loss) == float(twin.loss) and int(st.global_step.item()) == int(twin.store.global_step.item()) == 1


def test_refusals_reach_the_pass_unchanged(dev):
  """What ``check_input_gradients`` refuses, ``attributions`` refuses with the same words, before anything runs."""
  from geeco_amd import graph
  from geeco_amd.params import create_e2evmc_config
  cfg = create_e2evmc_config(dict(window_size=2, img_height=136, img_width=136, batch_size=2))
  cases = [(dict(training=False), 'training=False'), (dict(shared_frames=4), 'shared_frames')]
  for kw, words in cases:
    model = graph.E2EVMC(cfg, 2, dev, **kw)
    with pytest.raises(ValueError) as plain:
      model.check_input_gradients()
    assert words in str(plain.value)
    for method in ('integrated_gradients', 'smoothgrad'):
      with pytest.raises(ValueError) as got:
        model.attributions(method, 3)
      assert str(got.value) == str(plain.value)
  model = graph.E2EVMC(cfg, 2, dev)
  for kw, words in [(dict(method='gradient', steps=3), 'method'), (dict(method='smoothgrad', steps=0), 'steps'),
                    (dict(method='integrated_gradients', steps=2, noise_std=0.1), 'noise_std'),
                    (dict(method='integrated_gradients', steps=2, baseline=np.zeros((3, 3, 3), np.float32)), 'baseline')]:
    with pytest.raises(ValueError, match=words):
      model.attributions(**kw)


# ---- the baseline forms at model level ---------------------------------------------------------------------------------------------
def _forms(feats, r):
  """(what, the ``baseline=`` argument, the baseline each input must see) for a goal model's rgb / target_rgb."""
  rgb, tgt = feats['rgb'].shape, feats['target_rgb'].shape
  full, frame, tframe = r.random(rgb, dtype=np.float32), r.random(rgb[-3:], dtype=np.float32), r.random(tgt[-3:], dtype=np.float32)
  return [('dict: a full array and the target frame\'s own', {'rgb': full, 'target_rgb': tframe}, {'rgb': full, 'target_rgb': tframe}),
          ('one frame: both rgb inputs', frame, {'rgb': frame, 'target_rgb': frame}),
          ('one array shaped like rgb: rgb alone, the target from black', full, {'rgb': full}),
          ('torch tensors are taken too', {'target_rgb': torch.from_numpy(tframe)}, {'target_rgb': tframe})]


@pytest.mark.parametrize('rgbd', [False, True], ids=['goal seq residual', 'geeco-f rgbd'])
def test_baseline_forms_reach_the_kernels(dev, rgbd):
  """Every form ``baseline=`` takes puts the right array behind the right input: one step of integrated gradients equals the
  kernels called by hand with that baseline on a twin -- the path point at alpha = 0.5, the plain pass, the host model's finish on
  the twin's gradient -- bit for bit.  RGB-D: the depth inputs take theirs through the dict form."""
  from geeco_amd import ops
  name, cfg_kw, goal, N, H = PASS_CASES[3 if rgbd else 1]
  ocfg, P, feats, labels = G._mk(dict(cfg_kw, lr=1e-3), goal, N, H)
  keys = _image_keys(feats)
  r = np.random.default_rng(46)
  if rgbd:
    d, td = r.random(feats['depth'].shape[-3:], dtype=np.float32), r.random(feats['target_depth'].shape, dtype=np.float32)
    forms = [('depth: a frame and a full target array', {'depth': d, 'target_depth': td}, {'depth': d, 'target_depth': td})]
  else:
    forms = _forms(feats, r)
  model, twin = G._build(ocfg, goal, P, feats, labels, dev), G._build(ocfg, goal, P, feats, labels, dev)
  clean = {k: torch.from_numpy(feats[k]).to(dev) for k in keys}
  for what, arg, seen in forms:
    out = model.attributions('integrated_gradients', 1, baseline=arg)
    for k in keys:
      b = seen.get(k)
      ops.attr_path_point_into(twin.inputs[k], clean[k], None if b is None else torch.from_numpy(b).to(dev).reshape(-1), 0.5)
    twin.forward(backward_too=True)
    twin.backward()
    grads = {k: v.cpu().numpy() for k, v in twin.input_gradients().items()}
    for k in keys:
      frames = feats[k].reshape((N, -1) + feats[k].shape[-3:])
      attr, sal, sums = A.finish(A.accumulate(None, grads[k], 1.0, True).reshape(frames.shape), frames, seen.get(k), True)
      assert np.array_equal(_bits(out[k].cpu().numpy()), _bits(attr.reshape(feats[k].shape))), (what, k)
      assert np.array_equal(_bits(out['sample_sum_by_input'][k].cpu().numpy()), _bits(sums)), (what, k)
      assert attr.any(), (what, k)
    assert np.array_equal(_bits(model.inputs['rgb'].cpu().numpy()), _bits(feats['rgb'])), what
  with pytest.raises(ValueError, match="baseline for 'rgb' of shape"):
    model.attributions('integrated_gradients', 1, baseline={'rgb': np.zeros((3, 3, 3), np.float32)})
  with pytest.raises(ValueError, match='baseline for nope'):
    model.attributions('integrated_gradients', 1, baseline={'nope': np.zeros((H, H, 3), np.float32)})


# ---- through the Estimator and the script ------------------------------------------------------------------------------------------
def test_estimator_attributions(dev, tmp_path):
  """``Estimator.attributions`` beside ``input_gradients``: the model's pass per batch with the heads selected, as numpy, with the
  predictions ``predict()`` yields; the store and the model_dir untouched; the Estimator-level refusals reach it."""
  from geeco_amd import estimator as est, graph
  from geeco_amd.params import create_e2evmc_config
  from geeco_amd.synthetic import synthetic_batches
  cfg = create_e2evmc_config(dict(proc_obs='dynimg', proc_tgt='dyndiff', window_size=2, img_height=136, img_width=136, batch_size=2))
  input_fn = synthetic_batches(2, 2, 2, (136, 136), 3, True, seed=78)
  batches = list(input_fn())
  e = est.Estimator(est.goal_e2evmc_model_fn, model_dir=str(tmp_path), params={'e2evmc_config': cfg, 'use_hipgraph': False})
  feats_only = [{k: v for k, v in f.items() if k in ('rgb', 'target_rgb', 'jnt_state', 'step')} for f, _ in batches]
  preds = list(e.predict(lambda: iter(feats_only)))
  state = {k: getattr(e._store, k).clone() for k in ('params', 'adam_m', 'adam_v')}
  listing, step0 = sorted(os.listdir(str(tmp_path))), int(e._store.global_step.item())
  frame = np.random.default_rng(47).random((136, 136, 3), dtype=np.float32)
  ig = list(e.attributions(input_fn, method='integrated_gradients', steps=2, baseline=frame, heads=('cmd_ee',)))
  sg = list(e.attributions(input_fn, method='smoothgrad', steps=2, noise_std=0.1, seed=3))
  assert len(ig) == len(sg) == 2 and sorted(os.listdir(str(tmp_path))) == listing and int(e._store.global_step.item()) == step0
  for k, v in state.items():
    assert torch.equal(getattr(e._store, k), v), k
  model = graph.GoalE2EVMC(cfg, 2, dev, training=True)
  model.store.params.copy_(e._store.params)
  for b, (f, l) in enumerate(batches):
    model.load_batch({k: torch.as_tensor(v) for k, v in f.items()}, {k: torch.as_tensor(v) for k, v in l.items()})
    for got, heads, kw in ((ig[b], ('cmd_ee',), dict(method='integrated_gradients', steps=2, baseline=frame)),
                           (sg[b], None, dict(method='smoothgrad', steps=2, noise_std=0.1, seed=3))):
      model.decoder.select_loss_heads(heads)
      want = model.attributions(**kw)
      torch.cuda.synchronize()
      tensors = sorted(k for k, v in want.items() if torch.is_tensor(v) and k not in ('loss', 'loss_baseline'))
      assert sorted(set(got) - set(preds[b]) - {'loss', 'loss_baseline'}) == tensors and 'sample_sum_by_input' not in got
      for k in tensors:
        assert isinstance(got[k], np.ndarray) and np.array_equal(got[k], want[k].cpu().numpy()), k
      assert got['loss'] == float(want['loss']) and isinstance(got['loss'], float)
      assert got['rgb'].shape == f['rgb'].shape and got['saliency'].shape == f['rgb'].shape[:-1] and got['rgb'].any()
      for k, v in preds[b].items():
        assert np.array_equal(got[k], v), k
    assert ig[b]['completeness_gap'].shape == (2,) and isinstance(ig[b]['loss_baseline'], float)
    assert 'completeness_gap' not in sg[b] and 'loss_baseline' not in sg[b]
    assert ig[b]['loss'] != sg[b]['loss']      # another selection of heads, another loss
  with pytest.raises(ValueError, match='cmd_ee'):
    next(e.attributions(input_fn, heads=('no_such_head',)))
  with pytest.raises(ValueError, match='attributions: method'):
    e.attributions(input_fn, method='gradient')
  cfg1 = create_e2evmc_config(dict(window_size=2, img_height=136, img_width=136, batch_size=2))
  shared = est.Estimator(est.e2evmc_model_fn, model_dir=None, params={'e2evmc_config': cfg1, 'use_hipgraph': False, 'shared_frames': 8})
  for call, who in ((shared.attributions, 'attributions'), (shared.input_gradients, 'input_gradients')):
    with pytest.raises(ValueError, match=r"%s: params\['shared_frames'\]" % who):
      next(call(input_fn))


@pytest.mark.parametrize('method', ['integrated_gradients', 'smoothgrad'])
def test_saliency_script_methods(dev, tmp_path, method):
  import importlib.util
  spec = importlib.util.spec_from_file_location('saliency_script_attr', os.path.join(G.ROOT, 'scripts', 'saliency.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  out = str(tmp_path / 'attr.npz')
  mod.main(['--synthetic', '--img_size', '136', '--window_size', '2', '--num_windows', '3', '--batch_size', '2', '--method', method,
            '--steps', '2', '--noise_std', '0.05', '--out', out])
  z = np.load(out)
  assert z['rgb'].shape == z['attr_rgb'].shape == (3, 2, 136, 136, 3) and z['attr_target_rgb'].shape == (3, 136, 136, 3)
  assert 'grad_rgb' not in z.files and z['attr_rgb'].any()
  assert np.array_equal(z['saliency'], np.abs(z['attr_rgb']).max(-1)) and np.array_equal(z['saliency_target'], np.abs(z['attr_target_rgb']).max(-1))
  assert z['sample_sum'].shape == (3,) and z['loss'].shape == (2,) and np.isfinite(z['loss']).all()
  if method == 'integrated_gradients':
    assert z['completeness_gap'].shape == (3,) and z['loss_baseline'].shape == (2,) and np.isfinite(z['completeness_gap']).all()
  else:
    assert 'completeness_gap' not in z.files
