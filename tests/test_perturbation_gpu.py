"""Perturbation attributions on the GPU: the four kernels BITWISE against the float32 restatements of
tests/_perturbation_ref.py, and the whole pass bitwise against a plain loop on the same model -- each occluded input built on the
host from the restatement, ``load_batch`` + ``forward``, scores and map in numpy float32 in the stated order.  That comparison
rests on the forward being run-to-run bitwise at these shapes, which ``_forward_is_bitwise`` establishes on the model first (the
pass and the loop run the same launches on the same bits).  The score is also held to float64 within the bound of a float32 sum
derived at ``test_score``; the RISE masks' keep-share to the binomial bound of tests/test_perturbation_cpu.py."""
import os

import numpy as np
import pytest
import torch

import _perturbation_ref as P
import test_input_grad_gpu as G
from test_perturbation_cpu import rise_share_bound

pytestmark = pytest.mark.gpu
KEY = 0x243f6a8885a308d3
H5, W7 = 5, 7


def _bits(a):
  return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want):
  return np.array_equal(_bits(got.cpu().numpy() if torch.is_tensor(got) else got), _bits(want))


def _dev(a, dev, offset=0):
  """``a`` on the device; ``offset`` floats past a 16-byte boundary (1..3: the one-float access path)."""
  a = np.asarray(a, np.float32)
  buf = torch.empty(a.size + 4, dtype=torch.float32, device=dev)
  t = buf[offset:offset + a.size].view(a.shape)
  t.copy_(torch.from_numpy(a))
  return t


def _fill(r, kind, shape):
  return {'none': None, 'colour': r.random(shape[-1:], dtype=np.float32), 'frame': r.random(shape[-3:], dtype=np.float32),
          'full': r.random(shape, dtype=np.float32)}[kind]


# ---- apply -------------------------------------------------------------------------------------------------------------------------
# patch 2 x 3 on stride 2 x 2: H - ph = 3 is no multiple of the stride, the clamped last row overlaps its neighbour; the image; more
GRIDS = [((2, 3), (2, 2)), ((5, 7), (1, 1)), ((9, 8), (2, 2))]


@pytest.mark.parametrize('offset', [0, 1], ids=['aligned', 'one-float'])
@pytest.mark.parametrize('C', [1, 3, 4])
def test_apply_occlusion(dev, C, offset):
  from geeco_amd import ops
  r = np.random.default_rng(51)
  shape = (2, 2, H5, W7, C)
  x = r.random(shape, dtype=np.float32)
  x.reshape(-1)[::11] = -0.0
  xd = _dev(x, dev, offset)
  for patch, stride in GRIDS:
    desc = ops.perturb_desc('occlusion', H5, W7, patch=patch, stride=stride)
    M = ops.perturb_steps(desc)
    assert M == len(P.occlusion_grid(H5, W7, patch, stride)[2])
    for kind in ('none', 'colour', 'frame', 'full'):
      fill = _fill(r, kind, shape)
      fd = None if fill is None else _dev(fill.reshape(-1), dev, offset if kind == 'full' else 0)
      inc = _dev(np.full(shape, np.nan, np.float32), dev, offset)
      for m in range(M):
        want = P.apply(x, fill, P.occlusion_field(H5, W7, patch, stride, m, 2))
        whole = _dev(np.full(shape, np.nan, np.float32), dev, offset)
        ops.perturb_apply_into(whole, xd, fd, desc, m)
        assert _same(whole, want), (patch, kind, m)
        ops.perturb_apply_into(inc, xd, fd, desc, m, prev_step=m - 1)      # every consecutive pair, the row wrap included
        assert _same(inc, want), (patch, kind, m, 'incremental')
      if M > 2:      # and a pair that is not consecutive
        ops.perturb_apply_into(inc, xd, fd, desc, 1, prev_step=M - 1)
        assert _same(inc, P.apply(x, fill, P.occlusion_field(H5, W7, patch, stride, 1, 2)))
    ops.perturb_apply_into(inc, xd, xd.clone().reshape(-1), desc, M - 1)      # fill = the input: the input's bits
    assert _same(inc, x)
  x4 = x[:, 0]      # [N][H][W][C]: one frame per sample (the target frame)
  got = _dev(np.zeros(x4.shape, np.float32), dev, offset)
  ops.perturb_apply_into(got, _dev(x4, dev, offset), None, desc, 0)
  assert _same(got, P.apply(x4, None, P.occlusion_field(H5, W7, *GRIDS[-1], 0, 2)))


# ---- the RISE field ----------------------------------------------------------------------------------------------------------------
RISE_CASES = [(5, 7, 3), (8, 8, 4)]


def _device_field(ops, dev, desc, step, N, H, W, offset=0, sample0=0):
  """o [N][H][W] as the accumulate kernel sees it: den after an overwriting step."""
  num, den = _dev(np.zeros((N, H, W), np.float32), dev, offset), _dev(np.zeros((N, H, W), np.float32), dev, offset)
  ops.perturb_accumulate_into(num, den, torch.ones(N, device=dev), desc, step, True, sample0=sample0)
  assert torch.equal(num, den)      # d = 1: num = 1 * o
  return den.cpu().numpy()


@pytest.mark.parametrize('H,W,g', RISE_CASES)
def test_rise_field(dev, H, W, g):
  from geeco_amd import ops
  N = 3
  r = np.random.default_rng(52)
  for seed_key in (KEY, KEY ^ 0xffff0000ffff):
    desc = ops.perturb_desc('rise', H, W, grid=g, keep_prob=0.5, key=seed_key)
    for step in (0, 5):
      want = P.rise_field(H, W, g, 0.5, seed_key, step, N)
      assert want.min() >= 0 and want.max() <= 1
      got = _device_field(ops, dev, desc, step, N, H, W)
      assert _same(got, want), (step,)      # bits and shifts are the restatement's: every weight is
      assert _same(_device_field(ops, dev, desc, step, N, H, W, offset=1), want)      # the one-float path
      # a launch over samples 1..2 alone draws what the whole-grid launch drew for them
      assert _same(_device_field(ops, dev, desc, step, 2, H, W, sample0=1), want[1:])
      # the apply kernel sees the same field: from x = 0 with fill 1, x + o * (1 - 0) = o; and the mix on data, both paths
      for C in (1, 3, 4):
        shape = (N, 2, H, W, C)
        x, fill = r.random(shape, dtype=np.float32), r.random((H, W, C), dtype=np.float32)
        for offset in (0, 1):
          dst = _dev(np.full(shape, np.nan, np.float32), dev, offset)
          ops.perturb_apply_into(dst, _dev(np.zeros(shape, np.float32), dev, offset), torch.ones(C, device=dev), desc, step)
          assert _same(dst, np.broadcast_to(want[:, None, :, :, None], shape)), (C, offset)
          ops.perturb_apply_into(dst, _dev(x, dev, offset), _dev(fill.reshape(-1), dev), desc, step, prev_step=step)      # (RISE: a whole rewrite)
          assert _same(dst, P.apply(x, fill, want)), (C, offset)
        sub = _dev(np.full((2,) + shape[1:], np.nan, np.float32), dev)
        ops.perturb_apply_into(sub, _dev(x[1:], dev), _dev(fill.reshape(-1), dev), desc, step, sample0=1)
        assert _same(sub, P.apply(x[1:], fill, want[1:])), C
    assert not np.array_equal(_device_field(ops, dev, desc, 0, N, H, W), _device_field(ops, dev, desc, 1, N, H, W))


@pytest.mark.parametrize('H,W,g', RISE_CASES)
def test_rise_bits_and_shifts(dev, H, W, g):
  """The draws themselves, read off the device's field.  The bits: where (y + dy) and (x + dx) are multiples of the cell size both
  interpolation weights are 0 and o = 1 - bit[(y + dy) / ch][(x + dx) / cw] exactly, for the restatement's (dy, dx).  The shift: the
  restatement's bits under every OTHER shift give a field that differs from the device's (asserted mask by mask, so a wrong shift
  word cannot hide behind the interpolation), and under the restatement's own shift the same bits."""
  from geeco_amd import ops
  N, ch, cw = 3, -(-H // g), -(-W // g)
  corners = 0
  for key in (KEY, KEY ^ 0xffff0000ffff):
    desc = ops.perturb_desc('rise', H, W, grid=g, keep_prob=0.5, key=key)
    for step in (0, 5):
      got = _device_field(ops, dev, desc, step, N, H, W)
      for n in range(N):
        bits, dy, dx = P.rise_draws(H, W, g, 0.5, key, step, n)
        for y in range(H):
          for x in range(W):
            if (y + dy) % ch == 0 and (x + dx) % cw == 0:
              assert got[n, y, x] == 1 - bits[(y + dy) // ch, (x + dx) // cw], (key, step, n, y, x)
              corners += 1
        for sy in range(ch):
          for sx in range(cw):
            assert _same(got[n], P.rise_mask(H, W, g, bits, sy, sx)) == ((sy, sx) == (dy, dx)), (key, step, n, sy, sx)
  assert corners >= 12 * 4


@pytest.mark.parametrize('H,W,g', RISE_CASES)
def test_rise_keep_share(dev, H, W, g):
  """The mean keep-share of the device's masks over 256 steps x 3 samples, inside the binomial bound the restatement met on the CPU."""
  from geeco_amd import ops
  N, steps = 3, 256
  desc = ops.perturb_desc('rise', H, W, grid=g, keep_prob=0.5, key=KEY)
  num, den = torch.empty(N, H, W, device=dev), torch.empty(N, H, W, device=dev)
  ones = torch.ones(N, device=dev)
  for m in range(steps):
    ops.perturb_accumulate_into(num, den, ones, desc, m, m == 0)
  p, bound = rise_share_bound(H, W, g, 0.5, steps * N)
  share = 1.0 - float(den.double().mean()) / steps
  print('RISE %dx%d g=%d on the device: keep share %.4f, p %.4f, bound %.4f' % (H, W, g, share, p, bound))
  assert abs(share - p) <= bound


# ---- score -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [1, 3])
@pytest.mark.parametrize('OT', [1, 7, 32])
def test_score(dev, N, OT):
  """Bitwise the float32 restatement, and float64 within the bound of a float32 sum: each term w (p - p0)^2 carries three
  roundings (difference, square, weighting by 0 or 1 is exact: two count, three are allowed), and a recursive sum of n terms adds at
  most (n - 1) more, so |d - d64| <= (n + 2) u sum_j |term_j| to first order, u = 2^-24; the slack factor (1 + (n + 2) u) covers the
  second order.  n = OT <= 32."""
  from geeco_amd import ops
  r = np.random.default_rng(53)
  p, p0 = r.standard_normal((N, OT)).astype(np.float32), r.standard_normal((N, OT)).astype(np.float32)
  u = 2.0 ** -24
  for what, w in (('none', np.zeros(OT)), ('some', (np.arange(OT) % 3 == 0).astype(np.float64)), ('all', np.ones(OT))):
    d = torch.full((N,), float('nan'), device=dev)
    ops.perturb_score_into(d, _dev(p, dev), _dev(p0, dev, 1), _dev(w, dev))
    got = d.cpu().numpy()
    assert _same(got, P.score(p, p0, w)), what
    terms = w * (p.astype(np.float64) - p0.astype(np.float64)) ** 2
    bound = (OT + 2) * u * (1 + (OT + 2) * u) * np.abs(terms).sum(1)
    assert np.all(np.abs(got - terms.sum(1)) <= bound), (what, got, terms.sum(1))
    if what == 'none':
      assert not got.any()


# ---- accumulate and finish ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('offset', [0, 1], ids=['aligned', 'one-float'])
@pytest.mark.parametrize('H,W', [(5, 7), (8, 8)])
def test_accumulate_and_finish(dev, H, W, offset):
  from geeco_amd import ops
  N, r = 3, np.random.default_rng(54)
  occ = ops.perturb_desc('occlusion', H, W, patch=(2, 3), stride=(2, 2))
  rise = ops.perturb_desc('rise', H, W, grid=3 if H == 5 else 4, keep_prob=0.5, key=KEY)
  fields = [P.occlusion_field(H, W, (2, 3), (2, 2), m, N) for m in (0, 1, 4)] + [P.rise_field(H, W, rise.grid, 0.5, KEY, m, N) for m in (0, 1)]
  steps = [(occ, 0), (occ, 1), (occ, 4), (rise, 0), (rise, 1)]
  scores = r.standard_normal((len(steps), N)).astype(np.float32)
  scores[1, 1] = np.nan      # sample 1, step 1: the NaN reaches the pixels that step hid and no other
  runs = []
  for _ in range(2):
    num, den = _dev(np.full((N, H, W), np.nan, np.float32), dev, offset), _dev(np.full((N, H, W), np.nan, np.float32), dev, offset)
    want_num = want_den = None
    for m, (desc, step) in enumerate(steps):
      ops.perturb_accumulate_into(num, den, _dev(scores[m], dev), desc, step, m == 0)      # overwrite, then add
      want_num, want_den = P.accumulate(want_num, want_den, scores[m], fields[m], m == 0)
      assert _same(num, want_num) and _same(den, want_den), m
    sal = _dev(np.full((N, H, W), np.nan, np.float32), dev, offset)
    ops.perturb_finish_into(sal, num, den)
    runs.append(sal.cpu().numpy())
  assert _same(runs[0], P.finish(want_num, want_den)) and _same(runs[1], runs[0])      # two runs, the same bits
  assert np.array_equal(np.isnan(runs[0][1]), fields[1][1] != 0) and np.isnan(runs[0][1]).any() and not np.isnan(runs[0][[0, 2]]).any()
  # den == 0 gives +0: the first occlusion step alone leaves most of the image unseen
  num, den, sal = (_dev(np.full((N, H, W), np.nan, np.float32), dev, offset) for _ in range(3))
  ops.perturb_accumulate_into(num, den, _dev(scores[0], dev), occ, 0, True)
  ops.perturb_finish_into(sal, num, den)
  got = sal.cpu().numpy()
  assert _same(got, P.finish(*P.accumulate(None, None, scores[0], fields[0], True)))
  assert (den.cpu().numpy() == 0).sum() == N * (H * W - 6) and not _bits(got[den.cpu().numpy() == 0]).any()


def test_wrappers_refuse_bad_arguments(dev):
  """Every refusal raises before a launch: nothing was written."""
  from geeco_amd import ops
  from geeco_amd._native import GeecoNativeError
  t = lambda *s: torch.zeros(*s, device=dev)
  occ, rise = ops.perturb_desc('occlusion', 5, 7, patch=(2, 3), stride=(2, 2)), ops.perturb_desc('rise', 5, 7, grid=3, keep_prob=0.5)
  dst = torch.full((2, 2, 5, 7, 3), 7.0, device=dev)
  for call, words in [(lambda: ops.perturb_apply_into(dst, t(2, 2, 5, 7, 3), None, occ, 9), 'outside the grid'),
                      (lambda: ops.perturb_apply_into(dst, t(2, 2, 5, 7, 3), None, occ, 0, prev_step=9), 'prev_step'),
                      (lambda: ops.perturb_apply_into(dst, t(2, 2, 5, 7, 3), None, occ, -1), 'step'),
                      (lambda: ops.perturb_apply_into(dst, t(2, 2, 7, 5, 3), None, occ, 0), 'dst'),
                      (lambda: ops.perturb_apply_into(t(2, 2, 7, 5, 3), t(2, 2, 7, 5, 3), None, occ, 0), '5 x 7 images'),
                      (lambda: ops.perturb_apply_into(t(2, 5, 7, 5), t(2, 5, 7, 5), None, occ, 0), 'C in 1..4'),
                      (lambda: ops.perturb_apply_into(dst, t(2, 2, 5, 7, 3), t(9), occ, 0), 'does not divide'),
                      (lambda: ops.perturb_apply_into(dst, t(2, 2, 5, 7, 3).double(), None, occ, 0), 'contiguous float32'),
                      (lambda: ops.perturb_apply_into(dst, t(2, 2, 5, 7, 3), None, dict(), 0), 'perturb_desc'),
                      (lambda: ops.perturb_apply_into(dst, t(2, 2, 5, 7, 3), None, rise, 0, sample0=-1), 'sample0'),
                      (lambda: ops.perturb_score_into(t(2), t(2, 7), t(2, 6), t(7)), 'perturb_score'),
                      (lambda: ops.perturb_score_into(t(3), t(2, 7), t(2, 7), t(7)), 'perturb_score'),
                      (lambda: ops.perturb_accumulate_into(t(2, 5, 7), t(2, 5, 7), t(3), occ, 0, True), 'perturb_accumulate'),
                      (lambda: ops.perturb_accumulate_into(t(2, 7, 5), t(2, 7, 5), t(2), occ, 0, True), 'perturb_accumulate'),
                      (lambda: ops.perturb_accumulate_into(t(2, 5, 7), t(2, 5, 7), t(2), occ, 9, True), 'outside the grid'),
                      (lambda: ops.perturb_finish_into(t(8), t(8), t(9)), 'perturb_finish')]:
    with pytest.raises(ValueError, match=words):
      call()
  buf = t(2 * 2 * 5 * 7 * 3 + 8)
  a, b = buf[:420].view(2, 2, 5, 7, 3), buf[4:424].view(2, 2, 5, 7, 3)
  with pytest.raises(GeecoNativeError, match='overlaps'):
    ops.perturb_apply_into(a, b, None, occ, 0)
  with pytest.raises(GeecoNativeError, match='overlaps'):
    ops.perturb_accumulate_into(buf[:70].view(2, 5, 7), buf[35:105].view(2, 5, 7), t(2), occ, 0, True)
  with pytest.raises(GeecoNativeError, match='overlaps'):
    ops.perturb_finish_into(buf[:8], buf[4:12], buf[16:24])
  torch.cuda.synchronize()
  assert bool((dst == 7.0).all()) and not bool(buf.any())


# ---- the whole pass ----------------------------------------------------------------------------------------------------------------
PASS_CASES = [
    ('e2e_vmc rgb', dict(window_size=2), False),
    ('geeco-f rgb', dict(proc_obs='dynimg', proc_tgt='dyndiff', window_size=2), True),
    ('geeco-f rgbd', dict(proc_obs='dynimg', proc_tgt='dyndiff', window_size=2, img_channels=4, lambda_aux=0.5), True),
]
N2, H136 = 2, 136
OCC = dict(patch=64, stride=48)      # 3 x 3 positions: 9 steps


def _model(case, dev, training=True):
  from geeco_amd import graph
  from geeco_amd.params import create_e2evmc_config
  name, cfg_kw, goal = case
  ocfg, Pm, feats, labels = G._mk(dict(cfg_kw, lr=1e-3), goal, N2, H136)
  model = (graph.GoalE2EVMC if goal else graph.E2EVMC)(create_e2evmc_config(ocfg._asdict()), N2, dev, training=training)
  model.store.load_numpy(Pm)
  _load(model, feats, labels)
  return model, feats, labels


def _load(model, feats, labels=None):
  as_t = lambda d: {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in d.items()}
  model.load_batch(as_t(feats), None if labels is None else as_t(labels))


def _forward(model):
  model.forward()
  torch.cuda.synchronize()
  return model.decoder.preds.cpu().numpy().copy()


def _forward_is_bitwise(model):
  """Two forwards on identical input bits give identical predictions at this shape: what lets the loop below be compared bitwise."""
  first = _forward(model)
  for _ in range(2):
    assert np.array_equal(_bits(_forward(model)), _bits(first))
  return first


def _host_loop(model, feats, labels, passes, fields_of, fill_of_key, w):
  """The plain loop: per pass and step the occluded inputs built on the host, load_batch + forward, the prediction score and the
  map in numpy float32."""
  p0 = _forward(model)
  out = {}
  for name in passes:
    fields = fields_of(name)
    scores = np.empty((len(fields), N2), np.float32)
    for m, o in enumerate(fields):
      occluded = dict(feats)
      for k in P_KEYS[name]:
        if k in feats:
          occluded[k] = P.apply(feats[k], fill_of_key(k), o)
      _load(model, occluded, labels)
      scores[m] = P.score(_forward(model), p0, w)
    _load(model, feats, labels)
    sal, den = P.saliency(fields, scores)
    out[name] = (scores, sal, den)
  return p0, out


P_KEYS = {'rgb': ('rgb', 'depth'), 'target_rgb': ('target_rgb', 'target_depth')}


# every model as built for training; the headline model also as built for inference (training=False)
PASS_RUNS = [(c, True) for c in PASS_CASES] + [(PASS_CASES[1], False)]


@pytest.mark.parametrize('case,training', PASS_RUNS, ids=['%s-%s' % (c[0], 'training' if t else 'inference') for c, t in PASS_RUNS])
def test_occlusion_pass_is_the_host_loop(dev, case, training):
  from geeco_amd.perturbation import PASSES
  assert PASSES == P_KEYS
  model, feats, labels = _model(case, dev, training)
  goal = case[2]
  passes = ['rgb', 'target_rgb'] if goal else ['rgb']
  _forward_is_bitwise(model)
  st = model.store
  before = {k: getattr(st, k).clone() for k in ('params', 'adam_m', 'adam_v')}
  step0 = int(st.global_step.item())
  r = np.random.default_rng(55)
  frame = r.random((H136, H136, 3), dtype=np.float32)
  fills = {'rgb': frame, 'target_rgb': frame}
  if 'depth' in feats:
    fills = {'rgb': frame, 'depth': np.array([2.0], np.float32), 'target_depth': r.random(feats['target_depth'].shape, dtype=np.float32)}
  heads = ('cmd_ee', 'cmd_grp') if case[0] == 'geeco-f rgb' else None      # some columns, and all
  w = model._perturb_head_weights(heads)
  out = model.perturbation_attributions('occlusion', fill=fills if 'depth' in feats else frame, heads=heads, **OCC)
  torch.cuda.synchronize()
  model.check_device_errors()
  after = _forward(model)
  for k, v in before.items():
    assert torch.equal(getattr(st, k), v), k
  assert int(st.global_step.item()) == step0
  for k in [k for ks in P_KEYS.values() for k in ks if k in feats]:      # the clean inputs are back, bit for bit
    assert _same(model.inputs[k], feats[k]), k
  fields = [P.occlusion_field(H136, H136, (64, 64), (48, 48), m, N2) for m in range(9)]
  p0, ref = _host_loop(model, feats, labels, passes, lambda name: fields, lambda k: fills.get(k), w)
  assert np.array_equal(_bits(after), _bits(p0))      # ... and the forward at them
  off = 0
  for key, v in model.predictions().items():
    assert _same(out['predictions'][key], p0[:, off:off + v.shape[1]]), key
    off += v.shape[1]
  for name in passes:
    tail = '' if name == 'rgb' else '_target'
    scores, sal, den = ref[name]
    print('%s %s: scores %s' % (case[0], name, scores.max(0)))
    assert _same(out['scores' + tail], scores), name
    assert _same(out['saliency' + tail], sal) and _same(out['coverage' + tail], den), name
    assert out['saliency' + tail].shape == (N2, H136, H136) and out['patch_scores' + tail].shape == (3, 3, N2)
    assert _same(out['patch_scores' + tail], scores.reshape(3, 3, N2)) and scores.any() and (den >= 1).all()
  assert ('saliency_target' in out) == goal


def test_rise_pass_is_the_host_loop(dev):
  from geeco_amd.attribution import input_key
  case = PASS_CASES[1]
  model, feats, labels = _model(case, dev, training=False)
  _forward_is_bitwise(model)
  kw = dict(grid=4, keep_prob=0.5, steps=6, seed=9)
  colour = np.array([0.25, 0.5, 0.75], np.float32)
  out = model.perturbation_attributions('rise', fill=colour, inputs='rgb', **kw)
  torch.cuda.synchronize()
  assert 'saliency_target' not in out and 'patch_scores' not in out
  fields = [P.rise_field(H136, H136, 4, 0.5, input_key(9, 'rgb'), m, N2) for m in range(6)]
  w = model._perturb_head_weights(None)
  _, ref = _host_loop(model, feats, labels, ['rgb'], lambda name: fields, lambda k: colour, w)
  scores, sal, den = ref['rgb']
  assert _same(out['scores'], scores) and _same(out['saliency'], sal) and _same(out['coverage'], den) and scores.all()
  tgt = model.perturbation_attributions('rise', fill=colour, inputs=['target_rgb'], **kw)      # another input, another key
  assert 'saliency' not in tgt and not _same(tgt['coverage_target'], den)


def test_fill_equal_to_the_input_scores_zero(dev):
  model, feats, labels = _model(PASS_CASES[1], dev)
  for method, kw in (('occlusion', OCC), ('rise', dict(grid=4, steps=3))):
    out = model.perturbation_attributions(method, fill={k: feats[k] for k in ('rgb', 'target_rgb')}, **kw)
    for k in ('scores', 'saliency', 'scores_target', 'saliency_target'):
      assert not _bits(out[k].cpu().numpy()).any(), (method, k)      # exactly +0
    # (every pixel is under some patch of the grid; three random masks may leave a pixel unhidden, where the map is +0 by the rule)
    assert bool((out['coverage'] > 0).all()) if method == 'occlusion' else bool((out['coverage'] > 0).any())


def test_loss_score_and_refusals(dev):
  from geeco_amd import graph
  from geeco_amd.params import create_e2evmc_config
  model, feats, labels = _model(PASS_CASES[1], dev)
  out = model.perturbation_attributions('occlusion', score='loss', inputs='rgb', **OCC)
  torch.cuda.synchronize()
  scores = out['scores'].cpu().numpy()
  model.forward()
  l0 = model.decoder.sample_losses().cpu().numpy()
  u = 2.0 ** -24
  for m in range(9):      # the loop by hand: float64 differences of sample_losses(), rounded to float32 once
    _load(model, dict(feats, rgb=P.apply(feats['rgb'], None, P.occlusion_field(H136, H136, (64, 64), (48, 48), m, N2))), labels)
    model.forward()
    lm = model.decoder.sample_losses().cpu().numpy()
    # both sides are float64 dot products of <= 8 terms (relative 8 * 2^-53 each) and one rounding to float32
    assert np.all(np.abs(scores[m] - (lm - l0)) <= 2 * u * np.abs(lm - l0) + 16 * 2.0 ** -53 * (np.abs(lm) + np.abs(l0))), m
  assert scores.all()
  _load(model, feats, labels)
  assert model.decoder.head_weights is None
  # a selection of heads for the scored loss is gone before the pass's last forward: the model's loss is the training loss again
  model.forward()
  l_train = float(model.loss)
  picked = model.perturbation_attributions('occlusion', score='loss', heads=('cmd_ee',), inputs='target_rgb', **OCC)
  assert float(model.loss) == l_train and model.decoder.head_weights is None
  assert picked['scores_target'].any() and not torch.equal(picked['scores_target'], out['scores'])
  _load(model, feats)      # no labels
  with pytest.raises(ValueError, match="score='loss' needs the labels"):
    model.perturbation_attributions('occlusion', score='loss', **OCC)
  model.perturbation_attributions('occlusion', inputs='target_rgb', **OCC)      # the prediction score needs none
  shaped = graph.GoalE2EVMC(model.cfg, N2, dev, training=True, loss_shaping=dict(label_smoothing=0.1))
  _load(shaped, feats, labels)
  with pytest.raises(ValueError, match='per-sample loss terms'):
    shaped.perturbation_attributions('occlusion', score='loss', **OCC)
  for kw, words in [(dict(method='blur'), 'method'), (dict(method='occlusion', patch=0), 'patch'), (dict(method='rise', grid=40), 'grid'),
                    (dict(method='occlusion', inputs='depth'), 'inputs'), (dict(method='occlusion', heads=('nope',)), 'heads'),
                    (dict(method='occlusion', fill=np.zeros((3, 3, 3), np.float32)), "fill for 'rgb' of shape"),
                    (dict(method='occlusion', fill={'nope': np.zeros(3, np.float32)}), 'fill for nope')]:
    with pytest.raises(ValueError, match=words):
      model.perturbation_attributions(**kw)
  cfg = create_e2evmc_config(dict(window_size=2, img_height=136, img_width=136, batch_size=2))
  shared = graph.E2EVMC(cfg, 2, dev, training=False, shared_frames=4)
  with pytest.raises(ValueError, match='perturbation_attributions: shared_frames'):
    shared.perturbation_attributions('occlusion')
  bound = graph.E2EVMC(cfg, 2, dev, training=False)
  bound.inputs['rgb'] = type('Bound', (), {'pointers': None})()
  with pytest.raises(ValueError, match="perturbation_attributions: input 'rgb' bound as uint8 window addresses"):
    bound.perturbation_attributions('occlusion')


def test_sample_losses_into_is_the_allocating_product(dev):
  """``LSTMDecoder.sample_losses_into(out)``, the form both passes call inside their loops, gives the bits of the product
  ``sample_losses()`` used to allocate for: rows.double() @ coef, under the training loss and under a selection of heads."""
  model, feats, labels = _model(PASS_CASES[0], dev)
  d = model.decoder
  results = []
  for heads in (None, ('cmd_ee',), None):
    d.select_loss_heads(heads)
    model.forward()
    rows, coef = d.sample_loss_terms()
    want = rows.double() @ torch.tensor(coef, dtype=torch.float64, device=rows.device)
    out = torch.full((N2,), float('nan'), dtype=torch.float64, device=dev)
    assert d.sample_losses_into(out) is True
    assert torch.equal(out.view(torch.int64), want.view(torch.int64)) and bool(want.all()), heads
    assert torch.equal(d.sample_losses().view(torch.int64), want.view(torch.int64)), heads
    results.append(want)
  assert not torch.equal(results[0], results[1]) and torch.equal(results[0], results[2])      # the coefficients follow the selection


@pytest.mark.parametrize('who', ['perturb_accumulate_into', 'attr_accumulate_into'])
def test_an_exception_inside_a_pass_leaves_the_loaded_batch(dev, monkeypatch, who):
  """A ValueError raised on the host by the second accumulation of a pass reaches the caller; afterwards every image input holds the
  loaded batch's bits, not the step's perturbed input, and the decoder's selection of heads is what it was."""
  from geeco_amd import ops
  model, feats, labels = _model(PASS_CASES[0], dev)
  d = model.decoder
  d.select_loss_heads(('cmd_ee',))
  selected = list(d.head_weights)
  real, calls = getattr(ops, who), []

  def second_call_raises(*args, **kw):
    calls.append(1)
    if len(calls) == 2:
      raise ValueError('the second call of %s' % who)
    return real(*args, **kw)
  monkeypatch.setattr(ops, who, second_call_raises)
  with pytest.raises(ValueError, match='the second call of %s' % who):
    if who == 'perturb_accumulate_into':
      model.perturbation_attributions('occlusion', score='loss', heads=('cmd_grp',), **OCC)
    else:
      model.attributions('integrated_gradients', 3)
  monkeypatch.setattr(ops, who, real)
  torch.cuda.synchronize()
  model.check_device_errors()
  assert len(calls) == 2
  for k in [k for ks in P_KEYS.values() for k in ks if k in feats]:
    assert _same(model.inputs[k], feats[k]), k
  assert d.head_weights == selected
  out = model.perturbation_attributions('occlusion', **OCC)      # the next pass starts from the loaded batch
  assert _same(model.inputs['rgb'], feats['rgb']) and bool(out['scores'].any())


# ---- through the Estimator and the script ------------------------------------------------------------------------------------------
def test_estimator_perturbation_attributions(dev, tmp_path):
  from geeco_amd import estimator as est, graph
  from geeco_amd.params import create_e2evmc_config
  from geeco_amd.synthetic import synthetic_batches
  cfg = create_e2evmc_config(dict(proc_obs='dynimg', proc_tgt='dyndiff', window_size=2, img_height=136, img_width=136, batch_size=2))
  input_fn = synthetic_batches(2, 2, 2, (136, 136), 3, True, seed=79)
  batches = list(input_fn())
  e = est.Estimator(est.goal_e2evmc_model_fn, model_dir=str(tmp_path), params={'e2evmc_config': cfg, 'use_hipgraph': False})
  feats_only = [{k: v for k, v in f.items() if k in ('rgb', 'target_rgb', 'jnt_state', 'step')} for f, _ in batches]
  preds = list(e.predict(lambda: iter(feats_only)))
  state = {k: getattr(e._store, k).clone() for k in ('params', 'adam_m', 'adam_v')}
  listing = sorted(os.listdir(str(tmp_path)))
  unlabelled = lambda: iter([f for f, _ in batches])      # the features alone: the prediction score needs no labels
  occ = list(e.perturbation_attributions(unlabelled, method='occlusion', heads=('cmd_ee',), **OCC))
  rise = list(e.perturbation_attributions(input_fn, method='rise', grid=4, steps=3, seed=5, inputs='rgb', score='loss'))
  assert len(occ) == len(rise) == 2 and sorted(os.listdir(str(tmp_path))) == listing
  for k, v in state.items():
    assert torch.equal(getattr(e._store, k), v), k
  model = graph.GoalE2EVMC(cfg, 2, dev, training=False)
  model.store.params.copy_(e._store.params)
  for b, (f, l) in enumerate(batches):
    _load(model, {k: np.asarray(v) for k, v in f.items()}, {k: np.asarray(v) for k, v in l.items()})
    for got, kw in ((occ[b], dict(method='occlusion', heads=('cmd_ee',), **OCC)),
                    (rise[b], dict(method='rise', grid=4, steps=3, seed=5, inputs='rgb', score='loss'))):
      want = model.perturbation_attributions(**kw)
      torch.cuda.synchronize()
      tensors = sorted(k for k, v in want.items() if torch.is_tensor(v))
      assert sorted(set(got) - set(preds[b])) == tensors
      for k in tensors:
        assert isinstance(got[k], np.ndarray) and np.array_equal(_bits(got[k]), _bits(want[k].cpu().numpy())), k
      for k, v in preds[b].items():
        assert np.array_equal(got[k], v), k
    assert occ[b]['saliency'].shape == occ[b]['saliency_target'].shape == (2, 136, 136) and occ[b]['patch_scores'].shape == (3, 3, 2)
    assert rise[b]['scores'].shape == (3, 2) and 'saliency_target' not in rise[b] and occ[b]['saliency'].any()
  with pytest.raises(ValueError, match='perturbation_attributions: method'):
    e.perturbation_attributions(input_fn, method='gradient')
  with pytest.raises(ValueError, match="score='loss' needs the labels"):
    next(e.perturbation_attributions(unlabelled, score='loss'))
  cfg1 = create_e2evmc_config(dict(window_size=2, img_height=136, img_width=136, batch_size=2))
  shared = est.Estimator(est.e2evmc_model_fn, model_dir=None, params={'e2evmc_config': cfg1, 'use_hipgraph': False, 'shared_frames': 8})
  with pytest.raises(ValueError, match=r"perturbation_attributions: params\['shared_frames'\]"):
    next(shared.perturbation_attributions(input_fn))


@pytest.mark.parametrize('method', ['occlusion', 'rise'])
def test_saliency_script_perturbation_methods(dev, tmp_path, method):
  import importlib.util
  spec = importlib.util.spec_from_file_location('saliency_script_perturb', os.path.join(G.ROOT, 'scripts', 'saliency.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  out = str(tmp_path / 'perturb.npz')
  mod.main(['--synthetic', '--img_size', '136', '--window_size', '2', '--num_windows', '3', '--batch_size', '2', '--method', method,
            '--patch', '64', '--stride', '48', '--grid', '4', '--steps', '5', '--fill', '0.5,0.5,0.5', '--out', out])
  z = np.load(out)
  M = 9 if method == 'occlusion' else 5
  shapes = {'rgb': (3, 2, 136, 136, 3), 'target_rgb': (3, 136, 136, 3), 'saliency': (3, 136, 136), 'saliency_target': (3, 136, 136),
            'coverage': (3, 136, 136), 'coverage_target': (3, 136, 136), 'scores': (3, M), 'scores_target': (3, M)}
  if method == 'occlusion':
    shapes.update(patch_scores=(3, 3, 3), patch_scores_target=(3, 3, 3))
  assert {k: z[k].shape for k in z.files} == shapes
  assert z['saliency'].any() and np.isfinite(z['saliency']).all() and (z['coverage'] > 0).all()
  if method == 'occlusion':
    assert np.array_equal(z['patch_scores'].reshape(3, 9), z['scores'])
