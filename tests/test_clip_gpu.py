"""The opt-in global-norm gradient clipping on the GPU: the three entry points of csrc/clip.hip, the step that calls
them, and the Estimator / data-parallel surface on top.  Reference: tests/_clip_ref.py (float64).

Roundings of the sum of squares (U = 2^-24 each; every term is >= 0, so a relative bound per rounding carries to the sum), counted
from the reduction order csrc/clip.hip documents, longest path:
  a term G^2         G = g gs + l2 p is two products and a sum, |dG| <= 2 U A with A = |g gs| + |l2 p|, and the square is one more:
                     |d(G^2)| <= 4 U |G| A + U G^2.  Relative to the sum that is TERMS = (4 sum |G| A + S) / S roundings, computed
                     from the INPUTS in float64 (5 when nothing cancels in G; the inputs here keep |l2 p| far below |g gs|)
  inside a chunk     16 serial additions per thread (4 float4s) + 6 levels of the wave butterfly + 3 additions of the 4 wave sums = 25
  over the chunks    ceil(nchunks / 256) serial additions per thread + 6 + 3
norm and s add the two roundings of the square root and the division.  For the largest case (70 001 elements, 18 chunks) that is
5 + 25 + 10 = 40 U = 2.4e-6 for the sum, below the 1e-5 the feature promises.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import _clip_ref as C
import _primitive_refs as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float('nan')
U = R.U
CH = 4096                       # GEECO_CLIP_CHUNK of csrc/clip.hip (test_clip_cpu.py pins it through geeco_clip_ws_floats)
IN_CHUNK = 16 + 6 + 3           # roundings inside a chunk (module docstring)
ADAM = dict(beta1=0.9, beta2=0.999, eps=1e-8)
LR_T = 1e-3

_INPUTS = {}


def _inputs(n):
  """p, g, m, v, shadow as numpy float32, once per size and left unchanged (gradients ~0.1, parameters ~1: l2 p stays far below g gs)."""
  if n not in _INPUTS:
    r = np.random.default_rng(2000 + n % 1013)
    p, g, m, s = (r.standard_normal(n).astype(np.float32) for _ in range(4))
    v = (r.standard_normal(n).astype(np.float32)) ** 2
    _INPUTS[n] = (p, g * np.float32(0.1), m * np.float32(0.1), v * np.float32(0.01), s)
  return _INPUTS[n]


def _dev(dev, a, slack=5):
  """numpy array -> flat device tensor with ``slack`` NaN elements behind it (they must stay NaN)."""
  t = torch.full((a.size + slack,), NAN, dtype=torch.float32, device=dev)
  t[:a.size] = torch.from_numpy(a)
  return t


def _bits(t):
  return t.detach().cpu().numpy().view(np.uint32)


def _scalars(dev, t=5):
  scal = torch.zeros(4, dtype=torch.float32, device=dev)
  scal[0] = LR_T
  return scal, torch.full((1,), t, dtype=torch.int64, device=dev)


def _norm_on_device(dev, p, segments, n, clip, grad_scale=1.0, l2=0.0):
  """The two launches: (partials with NaN slack, out2 with NaN slack, number of chunks)."""
  from geeco_amd import ops
  nch = ops.clip_ws_floats(n)
  assert nch == -(-n // CH)
  partials = torch.full((nch + 3,), NAN, dtype=torch.float32, device=dev)
  out2 = torch.full((2 + 3,), NAN, dtype=torch.float32, device=dev)
  ops.grad_sumsq_segments(partials, p, segments, n, grad_scale=grad_scale, l2=l2)
  ops.clip_scale(out2, partials, nch, clip)
  torch.cuda.synchronize()
  assert torch.isnan(partials[nch:]).all() and torch.isnan(out2[2:]).all()
  return partials, out2, nch


# ================================================================================================
# kernels
# ================================================================================================
@pytest.mark.parametrize('n', [1, 3, 4, 5, CH - 1, CH, CH + 1, 3 * CH + 7, 70001])
def test_sum_of_squares_against_float64(dev, n):
  """Every partial, their sum, norm and s against the float64 restatement within the counted roundings; the slack behind every
  buffer stays NaN (a read of it would poison the sum, a write would show)."""
  p0, g0 = _inputs(n)[:2]
  for l2 in (0.0, 1e-3):
    for gscale in (1.0, 0.125):
      p, g = _dev(dev, p0), _dev(dev, g0)
      G = C.total_grad(p0, g0, gscale, l2)
      A = np.abs(g0.astype(np.float64) * gscale) + np.abs(np.float64(np.float32(l2)) * p0.astype(np.float64))
      S = float(np.sum(G * G))
      norm = C.global_norm(p0, g0, gscale, l2)
      clip = float(np.float32(0.1 * norm))
      partials, out2, nch = _norm_on_device(dev, p if l2 else None, [(g, 0, n)], n, clip, gscale, l2)
      assert torch.isnan(p[n:]).all() and torch.isnan(g[n:]).all()
      terms = (4.0 * float(np.sum(np.abs(G) * A)) + S) / S
      over_chunks = -(-nch // 256) + 6 + 3
      count = terms + IN_CHUNK + over_chunks
      assert count * U < 1e-5, count
      got = partials[:nch].cpu().numpy().astype(np.float64)
      for k in range(nch):
        Gk, Ak = G[k * CH:(k + 1) * CH], A[k * CH:(k + 1) * CH]
        Sk = float(np.sum(Gk * Gk))
        bound = (4.0 * float(np.sum(np.abs(Gk) * Ak)) + Sk) * U + IN_CHUNK * U * Sk
        assert abs(got[k] - Sk) <= bound, (n, l2, gscale, k, got[k], Sk, bound)
      s_dev, norm_dev = (float(x) for x in out2[:2].cpu().numpy())
      err_norm, err_s = abs(norm_dev - norm) / norm, abs(s_dev - C.clip_scale(norm, clip)) / C.clip_scale(norm, clip)
      print('n=%d l2=%g gscale=%g: %d chunks, %.1f roundings allowed; norm off by %.2f U, s by %.2f U' % (n, l2, gscale, nch, count + 2,
                                                                                                        err_norm / U, err_s / U))
      assert err_norm <= (count + 1) * U and err_s <= (count + 2) * U
      assert 0.0 < s_dev < 1.0
      # norm <= clip: s is exactly 1
      _, out_b, _ = _norm_on_device(dev, p if l2 else None, [(g, 0, n)], n, float(np.float32(norm * 1.001)), gscale, l2)
      assert _bits(out_b[:1])[0] == np.float32(1.0).view(np.uint32) and _bits(out_b[1:2])[0] == _bits(out2[1:2])[0]


N_PART = 3 * CH + 7
# cuts at multiples of 4 that are no multiples of CH (4, 2000, 4100, 8196, 8200, 12292) and one at an odd offset (6001)
PARTITIONS = {
    '2 pieces': [(2000, N_PART - 2000), (0, 2000)],
    '3 pieces': [(6001, N_PART - 6001), (0, 2000), (2000, 4001)],
    '8 pieces': [(8196, 4), (0, 4), (6001, 2195), (12292, 3), (2000, 2100), (8200, 4092), (4, 1996), (4100, 1901)],
}


def _pieces(dev, g, g0, cuts, own):
  """The pieces as slices of the arena ``g`` (a slice at an odd offset is not 16-byte aligned); piece ``own`` in a buffer of its own."""
  out = []
  for i, (off, cnt) in enumerate(cuts):
    src = torch.from_numpy(g0[off:off + cnt].copy()).to(dev) if i == own else g[off:off + cnt]
    out.append((src, off, cnt))
  return out


@pytest.mark.parametrize('l2', [0.0, 1e-3])
@pytest.mark.parametrize('name', list(PARTITIONS))
def test_any_partition_gives_the_one_piece_partials(dev, name, l2):
  """Partials, norm and s are bit for bit those of the one-piece call, whatever the cuts, the order of the pieces and where a
  piece's gradients live."""
  n, cuts = N_PART, PARTITIONS[name]
  covered = np.zeros(n, int)
  for off, cnt in cuts:
    covered[off:off + cnt] += 1
  assert (covered == 1).all()
  p0, g0 = _inputs(n)[:2]
  p, g = _dev(dev, p0), _dev(dev, g0)
  clip = 0.5
  one = _norm_on_device(dev, p, [(g, 0, n)], n, clip, 0.125, l2)
  for own in (1, len(cuts) - 1):
    got = _norm_on_device(dev, p, _pieces(dev, g, g0, cuts, own), n, clip, 0.125, l2)
    np.testing.assert_array_equal(_bits(got[0]), _bits(one[0]), err_msg='partials, piece %d in its own buffer' % own)
    np.testing.assert_array_equal(_bits(got[1]), _bits(one[1]), err_msg='s, norm')
  assert float(one[1][0]) < 1.0      # (clipping is active: s is not the trivial 1)


def test_an_uncovered_stretch_adds_nothing(dev):
  """l2 = 0: pieces that leave [2000, 4100) and the last 3 elements out give the one-piece partials of a gradient zeroed there."""
  n = N_PART
  p0, g0 = _inputs(n)[:2]
  zeroed = g0.copy()
  zeroed[2000:4100] = 0
  zeroed[12292:] = 0
  one = _norm_on_device(dev, None, [(_dev(dev, zeroed), 0, n)], n, 0.5, 0.125)
  cuts = [c for c in PARTITIONS['8 pieces'] if c[0] not in (2000, 12292)]
  got = _norm_on_device(dev, None, _pieces(dev, _dev(dev, g0), g0, cuts, 2), n, 0.5, 0.125)
  np.testing.assert_array_equal(_bits(got[0]), _bits(one[0]))
  np.testing.assert_array_equal(_bits(got[1]), _bits(one[1]))
  full = _norm_on_device(dev, None, [(_dev(dev, g0), 0, n)], n, 0.5, 0.125)
  assert not np.array_equal(_bits(full[0]), _bits(one[0]))


def _scale_of_one(dev):
  """[s, norm] as geeco_clip_scale leaves it for a clip far above the norm: s == 1.0f."""
  _, out2, _ = _norm_on_device(dev, None, [(torch.ones(8, device=dev), 0, 8)], 8, 1e30)
  assert float(out2[0]) == 1.0
  return out2


# n = 5: offsets are multiples of 4, so the five elements split into at most two pieces; n = 1027: three, the last one with the tail
CLIP_PIECES = {5: [(4, 1), (0, 4)], 1027: [(512, 515), (0, 256), (256, 256)]}


@pytest.mark.parametrize('ema', [False, True], ids=['plain', 'shadow arena'])
@pytest.mark.parametrize('n', [5, 1027])
def test_scale_one_is_bitwise_the_unclipped_kernels(dev, n, ema):
  """clip_dev[0] == 1.0f: p, m, v (and the shadow arena, and g_out) bit for bit as geeco_adam_tf / geeco_adam_tf_ema leave them from the
  same inputs, as one piece and in pieces; on the multiple-of-4 part also as geeco_adam_tf_segments[_ema] leave them."""
  from geeco_amd import ops
  p0, g0, m0, v0, s0 = _inputs(n)
  one = _scale_of_one(dev)
  for l2 in (0.0, 1e-3):
    for gscale in (1.0, 0.125):
      kw = dict(grad_scale=gscale, l2=l2, **ADAM)
      scal, step = _scalars(dev)
      ekw = dict(global_step=step, decay=0.99) if ema else {}

      def fresh():
        return [_dev(dev, x) for x in (p0, g0, m0, v0, s0)]

      def clipped(pieces_of):
        p, g, m, v, s = fresh()
        g_out = torch.full((n + 5,), NAN, device=dev)
        ops.adam_tf_segments_clip(p, m, v, pieces_of(g), scal, one, ema=s if ema else None, g_out=g_out, **ekw, **kw)
        return p, g_out, m, v, s

      ref = fresh()
      if ema:
        ops.adam_tf_ema(ref[0], ref[1], ref[2], ref[3], ref[4], n, scal, step, 0.99, **kw)
      else:
        ops.adam_tf(ref[0], ref[1], ref[2], ref[3], n, scal, **kw)
      for what, pieces_of in (('one piece', lambda g: [(g, 0, n)]),
                              ('pieces', lambda g: [(g[off:off + cnt], off, cnt) for off, cnt in CLIP_PIECES[n]])):
        got = clipped(pieces_of)
        torch.cuda.synchronize()
        for name, x, y in zip(('p', 'g_out', 'm', 'v', 'shadow'), got, ref):
          np.testing.assert_array_equal(_bits(x), _bits(y), err_msg='%s, %s: n=%d l2=%g gscale=%g' % (name, what, n, l2, gscale))
      assert not np.array_equal(_bits(ref[0][:n]), p0.view(np.uint32))      # (the update did run)
      # ... and the unclipped segments entry points on the part they take (multiples of 4)
      n4 = n & ~3
      seg = fresh()
      segs = [(seg[1][:n4], 0, n4)]
      if ema:
        ops.adam_tf_segments_ema(seg[0], seg[2], seg[3], seg[4], segs, scal, step, 0.99, **kw)
      else:
        ops.adam_tf_segments(seg[0], seg[2], seg[3], segs, scal, **kw)
      got = clipped(lambda g: [(g[:n4], 0, n4)])
      torch.cuda.synchronize()
      for name, x, y in zip(('p', 'm', 'v', 'shadow'), (got[0], got[2], got[3], got[4]), (seg[0], seg[2], seg[3], seg[4])):
        np.testing.assert_array_equal(_bits(x), _bits(y), err_msg='%s against the segments entry point: n=%d' % (name, n))


@pytest.mark.parametrize('l2', [0.0, 1e-3])
def test_clipping_proper(dev, l2):
  """clip = 0.1 norm: p, m, v against the float64 restatement within its bounds, the shadow arena within the 2 ulp of the kernel test of
  the averaged weights (tests/test_ema_gpu.py), from the three launches as the model issues them; nothing moves outside the pieces."""
  from geeco_amd import ops
  n, gscale, t, decay = 1027, 0.125, 7, 0.9
  p0, g0, m0, v0, s0 = _inputs(n)
  pieces = [(512, 515), (0, 256)]                       # [256, 512) belongs to no piece
  covered = np.zeros(n, bool)
  for off, cnt in pieces:
    covered[off:off + cnt] = True
  norm = float(np.sqrt(np.sum(np.where(covered, C.total_grad(p0, g0, gscale, l2), 0.0) ** 2)))
  clip = float(np.float32(0.1 * norm))
  p, g, m, v, s = (_dev(dev, x) for x in (p0, g0, m0, v0, s0))
  scal, step = _scalars(dev, t)
  segs = [(g[off:off + cnt], off, cnt) for off, cnt in pieces]
  _, out2, _ = _norm_on_device(dev, p, segs, n, clip, gscale, l2)
  s_dev = float(out2[0])
  assert abs(s_dev - 0.1) < 1e-6 and abs(float(out2[1]) - norm) <= 60 * U * norm
  ops.adam_tf_segments_clip(p, m, v, segs, scal, out2, ema=s, global_step=step, decay=decay, grad_scale=gscale, l2=l2, **ADAM)
  torch.cuda.synchronize()
  kw = dict(grad_scale=gscale, l2=l2)
  refs = C.clipped_adam_ref(p0, g0, m0, v0, LR_T, s_dev, **kw)
  bounds = C.clipped_adam_bounds(p0, g0, m0, v0, LR_T, s_dev, **kw)
  for name, got, init, ref, bound in zip('pmv', (p, m, v), (p0, m0, v0), refs, bounds):
    host = got[:n].cpu().numpy()
    print('%s: %.3f of its bound' % (name, R.worst_ratio(host[covered], ref[covered], bound[covered])))
    R.assert_within(host[covered], ref[covered], bound[covered], name)
    np.testing.assert_array_equal(host.view(np.uint32)[~covered], init.view(np.uint32)[~covered], err_msg=name + ' outside the pieces')
    assert torch.isnan(got[n:]).all(), name
  # ... and the update is the clipped one: far from the unclipped restatement wherever the gradient matters
  plain = R.adam_ref(p0, g0, m0, v0, LR_T, **kw)[1]
  assert np.abs(plain - refs[1])[covered].max() > 1e3 * bounds[1][covered].max()
  # the shadow arena: p' + (s - p') d_t from the device's own p'
  d = min(np.float32(decay), (np.float32(1) + np.float32(t)) / (np.float32(10) + np.float32(t)))
  p_new, shadow = p[:n].cpu().numpy(), s[:n].cpu().numpy()
  want = s0.astype(np.float64) - (s0.astype(np.float64) - p_new.astype(np.float64)) * (1.0 - np.float64(d))
  ulp = np.spacing(np.maximum(np.abs(s0), np.abs(p_new)).astype(np.float32)).astype(np.float64)
  assert (np.abs(shadow.astype(np.float64) - want)[covered] <= 2.0 * ulp[covered]).all()
  np.testing.assert_array_equal(shadow.view(np.uint32)[~covered], s0.view(np.uint32)[~covered])
  assert torch.isnan(s[n:]).all() and torch.isnan(g[n:]).all() and np.array_equal(_bits(g[:n]), g0.view(np.uint32))


# ================================================================================================
# the step
# ================================================================================================
H = 136                 # the shapes of tests/test_shared_frames_gpu.py
K3 = 3
MODELS = {'e2e_vmc': (False, {}), 'goal residual': (True, dict(proc_obs='sequence', proc_tgt='residual'))}
CLIP = 0.01             # below the norm of every step these tests take (each asserts it)
_CASES = {}


def _case(name):
  """(ocfg, cfg, goal, P, feats, labels), once per model and left unchanged."""
  if name not in _CASES:
    from geeco_amd.params import create_e2evmc_config
    from oracle import geeco_oracle as O
    goal, extra = MODELS[name]
    ocfg = O.make_config(window_size=K3, img_height=H, img_width=H, batch_size=4, lr=1e-3, **extra)
    P = O.init_params(O.model_param_shapes(ocfg, goal), seed=1)
    feats, labels = O.synthetic_batch(ocfg, goal, 4, seed=3, H=H, W=H)
    _CASES[name] = (ocfg, create_e2evmc_config(ocfg._asdict()), goal, P, feats, labels)
  return _CASES[name]


def _model(dev, name, **kw):
  from geeco_amd import graph
  ocfg, cfg, goal, P, feats, labels = _case(name)
  model = (graph.GoalE2EVMC if goal else graph.E2EVMC)(cfg, 4, dev, training=True, **kw)
  model.store.load_numpy(P)
  model.load_batch({k: torch.from_numpy(v) for k, v in feats.items()}, {k: torch.from_numpy(v) for k, v in labels.items()})
  return model


def _same_state(a, b, what=''):
  for name in ('params', 'adam_m', 'adam_v', 'grads'):
    assert torch.equal(getattr(a.store, name).view(torch.int32), getattr(b.store, name).view(torch.int32)), (what, name)
  assert int(a.store.global_step.item()) == int(b.store.global_step.item()), what


@pytest.mark.parametrize('name', list(MODELS))
def test_two_clipped_steps_against_the_oracle(dev, name):
  """train_step twice with clip_norm below the norm: the parameters against the float64 oracle's gradients (under the device's ReLU
  decisions, tests/_relu_taps.py) pushed through the float64 clipped Adam, at the post-Adam tolerance of tests/test_model_gpu.py
  (2.5 lr); the logged norm against the oracle's at 1e-4 relative."""
  import _relu_taps as T
  from oracle import geeco_oracle as O
  ocfg, _, goal, P, feats, labels = _case(name)
  model = _model(dev, name, clip_norm=CLIP)
  assert model.clip_ws.numel() == -(-model.store.size // CH) and model.clip_out.numel() == 2
  ref_p = {k: v.astype(np.float64) for k, v in P.items()}
  ref_m = {k: np.zeros_like(v) for k, v in ref_p.items()}
  ref_v = {k: np.zeros_like(v) for k, v in ref_p.items()}
  for t in (1, 2):
    model.forward(backward_too=True)
    torch.cuda.synchronize()
    masks = T.snapshot_masks(model.enc)       # this step's decisions (train_step runs the same forward again)
    model.train_step()
    torch.cuda.synchronize()
    tap, _ = T.device_tap(model, goal, masks, ocfg.img_channels)
    oracle = O.OracleTrainer(ocfg, goal, ref_p, dtype=torch.float64)
    _, _, grads, _, _ = oracle.loss_and_grads(feats, labels, tap=tap)
    G = {k: g.numpy() for k, g in grads.items()}                # the gradient of the total loss
    norm = float(np.sqrt(sum(float(np.sum(g * g)) for g in G.values())))
    s_dev, norm_dev = (float(x) for x in model.clip_out.cpu().numpy())
    print('%s step %d: norm %.6g (oracle %.6g), s %.6g' % (name, t, norm_dev, norm, s_dev))
    assert norm > CLIP and abs(norm_dev - norm) <= 1e-4 * norm
    assert abs(s_dev - C.clip_scale(norm, CLIP)) <= 1e-4 * s_dev
    lr_t = R.lr_t_ref(ocfg.lr, 0.9, 0.999, t)
    for k in ref_p:
      ref_p[k], ref_m[k], ref_v[k] = C.clipped_adam_ref(ref_p[k], G[k], ref_m[k], ref_v[k], lr_t, C.clip_scale(norm, CLIP))
  assert int(model.store.global_step.item()) == 2
  got = model.store.to_numpy('params')
  for k, v in ref_p.items():
    np.testing.assert_allclose(got[k], v, rtol=0, atol=2.5 * ocfg.lr, err_msg=k)
  moved = np.concatenate([(got[k] - P[k]).ravel() for k in P])
  assert np.abs(moved).max() > 0.5 * ocfg.lr


@pytest.mark.parametrize('name', list(MODELS))
def test_the_schedules_clip_alike(dev, name):
  """backward_and_apply(early, late) under clipping is train_step under clipping, bitwise in p, m, v, g and [s, norm] (the partial sums do
  not depend on the pieces); clip_norm = 1e30 is bitwise the model built without the option; an abandoned step leaks no pieces."""
  from geeco_amd.runtime import gradient_buckets
  a, b = _model(dev, name, clip_norm=CLIP), _model(dev, name, clip_norm=CLIP)
  early, late = gradient_buckets(a.store)
  assert early and late and a.can_apply_beside_bottom()
  for _ in range(2):
    a.forward(backward_too=True)
    a.backward_and_apply(early, late)
    b.train_step()
  torch.cuda.synchronize()
  _same_state(a, b, 'backward_and_apply against train_step')
  assert torch.equal(a.clip_out.view(torch.int32), b.clip_out.view(torch.int32)) and 0.0 < float(a.clip_out[0]) < 1.0
  assert torch.equal(a.clip_ws.view(torch.int32), b.clip_ws.view(torch.int32))
  assert a._clip_calls == [] and not a._prepared
  # far above any norm: the scale is 1.0f and the step is the unclipped one
  c, d = _model(dev, name, clip_norm=1e30), _model(dev, name)
  for _ in range(2):
    c.train_step()
    d.train_step()
  torch.cuda.synchronize()
  _same_state(c, d, 'clip_norm = 1e30 against no option')
  assert float(c.clip_out[0]) == 1.0 and float(c.clip_out[1]) > CLIP
  assert not torch.equal(c.store.params, b.store.params)
  # a step abandoned between the early pieces and the last one
  g = a.store.grads
  for m, abandon in ((a, True), (b, False)):
    m.forward(backward_too=True)
    m.backward(adam_prepare=True)
    if abandon:
      m.apply_gradients_of([(g[off:off + n], off, n) for off, n in early], last=False)
      assert len(m._clip_calls) == 1
  a.forward(backward_too=True)
  assert a._clip_calls == []
  a.backward_and_apply(early, late)
  b.train_step()
  torch.cuda.synchronize()
  _same_state(a, b, 'after an abandoned step')


class _CountingLibrary:
  """Stands in for the loaded library: counts the calls of every entry point that is handed a stream (each is one launch or a fixed few)."""

  def __init__(self, lib):
    self._lib, self.calls = lib, []

  def __getattr__(self, name):
    fn = getattr(self._lib, name)
    if not name.startswith('geeco_') or name in ('geeco_last_error', 'geeco_clip_ws_floats') or name.endswith('_bytes'):
      return fn

    def counted(*a):
      self.calls.append(name)
      return fn(*a)
    return counted


def test_a_model_without_the_option_is_untouched(dev, monkeypatch):
  """No clip buffers, none of the new entry points, and the calls of a step are those of the clipped step minus the two launches in
  front of the optimiser pass -- in both schedules; the captured step replays."""
  from geeco_amd import _native
  from geeco_amd.runtime import TrainStepRunner, gradient_buckets
  off, on = _model(dev, 'e2e_vmc'), _model(dev, 'e2e_vmc', clip_norm=CLIP)
  assert off.clip_norm is None and off.clip_ws is None and off.clip_out is None and off._clip_calls == []
  early, late = gradient_buckets(off.store)
  counter = _CountingLibrary(_native.load())
  monkeypatch.setattr(_native, '_lib', counter)
  new = ('geeco_grad_sumsq_segments', 'geeco_clip_scale', 'geeco_adam_tf_segments_clip')

  def calls_of(step):
    del counter.calls[:]
    step()
    torch.cuda.synchronize()
    return list(counter.calls)

  def beside(m):
    m.forward(backward_too=True)
    m.backward_and_apply(early, late)

  plain_off, plain_on = calls_of(off.train_step), calls_of(on.train_step)
  assert plain_off.count('geeco_adam_tf') == 1 and not any(c in plain_off for c in new)
  assert [plain_on.count(c) for c in new] == [1, 1, 1] and 'geeco_adam_tf' not in plain_on
  assert len(plain_on) == len(plain_off) + 2
  assert [c for c in plain_on if c not in new] == [c for c in plain_off if c != 'geeco_adam_tf']
  side_off, side_on = calls_of(lambda: beside(off)), calls_of(lambda: beside(on))
  assert side_off.count('geeco_adam_tf_segments') == 2 and not any(c in side_off for c in new)
  assert [side_on.count(c) for c in new] == [1, 1, 2] and 'geeco_adam_tf_segments' not in side_on
  assert len(side_on) == len(side_off) + 2
  monkeypatch.undo()
  # captured: the replayed step of either model is its eager step
  for m in (off, on):
    twin = _model(dev, 'e2e_vmc', clip_norm=m.clip_norm)
    for _ in range(2):
      twin.train_step()
    for _ in range(3):
      twin.train_step()
    r = TrainStepRunner(m, use_graph=True, warmup=1)      # one more eager step, then the capture and two replays
    assert r.beside_bottom
    for _ in range(3):
      r.step()
    torch.cuda.synchronize()
    assert r._graphs is not None and len(r._graphs) == 1
    _same_state(m, twin, 'replayed against eager, clip_norm=%r' % (m.clip_norm,))


# ================================================================================================
# Estimator
# ================================================================================================
def _events(model_dir):
  return [json.loads(l) for l in open(os.path.join(model_dir, 'events.jsonl'))]


def test_estimator_clips_and_logs_the_norm(dev, tmp_path):
  """Three steps of e2e_vmc on a two-episode synthetic dataset: with params['clip_norm'] every events.jsonl line carries grad_norm, the
  norm before clipping (finite, positive, above the bound: the steps were clipped); without it -- the key absent, None or 0 -- the
  key is not written and the losses are bitwise those of a run whose params never named the option; a checkpoint round-trips."""
  from geeco_amd import estimator as est
  from geeco_amd import input_fn as I
  from geeco_amd.graph import build_store
  from geeco_amd.params import create_e2evmc_config
  root = str(tmp_path / 'ds')
  I.write_synthetic_dataset(root, 2, episode_length=9, img_hw=(H, H), seed=5)
  batches = list(I.pickplace_input_fn(root, 'default', 'train', window_size=K3, batch_size=4, num_threads=2))
  assert len(batches) == 3
  cfg = create_e2evmc_config(dict(window_size=K3, img_height=H, img_width=H, batch_size=4))
  plain = {'e2evmc_config': cfg, 'log_steps': 1, 'debug': False}
  runs = {}
  for tag, extra in (('never', {}), ('zero', {'clip_norm': 0}), ('none', {'clip_norm': None}), ('on', {'clip_norm': CLIP}),
                     ('on + ema', {'clip_norm': CLIP, 'ema_decay': 0.9})):
    md = str(tmp_path / tag.replace(' + ', '_'))
    e = est.Estimator(est.e2evmc_model_fn, md, est.RunConfig(init_seed=4), dict(plain, **extra))
    e.train(input_fn=lambda: iter(batches))
    runs[tag] = (e, md, _events(md))
  for tag in ('never', 'zero', 'none'):
    ev = runs[tag][2]
    assert len(ev) == 3 and not any('grad_norm' in line for line in ev), tag
    assert [line['loss'] for line in ev] == [line['loss'] for line in runs['never'][2]], tag
    (spec, _, _), = runs[tag][0]._specs.values()
    assert spec.model.clip_ws is None and spec.model.clip_out is None
  on = runs['on'][2]
  print('grad_norm per step:', [line['grad_norm'] for line in on], 'losses', [line['loss'] for line in on])
  assert len(on) == 3 and all(np.isfinite(line['grad_norm']) and line['grad_norm'] > CLIP for line in on)
  assert on[0]['loss'] == runs['never'][2][0]['loss'] and on[2]['loss'] != runs['never'][2][2]['loss']       # the same start, another path
  assert [line['grad_norm'] for line in runs['on + ema'][2]] == [line['grad_norm'] for line in on]
  assert runs['on + ema'][0]._store.ema is not None
  assert torch.equal(runs['on + ema'][0]._store.params, runs['on'][0]._store.params)
  # the checkpoint holds what it held: nothing of the option is state
  e, md, _ = runs['on']
  back = build_store(cfg, False, 'cpu')
  est.load_checkpoint(back, est.latest_checkpoint(md))
  for name in ('params', 'adam_m', 'adam_v', 'global_step'):
    assert torch.equal(getattr(back, name), getattr(e._store, name).cpu()), name
  assert int(back.global_step.item()) == 3


# ================================================================================================
# data parallel: two ranks sharing the test GPU over gloo (the harness of tests/test_dp_gpu.py)
# ================================================================================================
def _dp_worker(rank, world, port, q):
  sys.path.insert(0, ROOT)
  sys.path.insert(0, os.path.join(ROOT, 'tests'))
  import test_dp_gpu as D
  D._child_watchdog()
  os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
  from geeco_amd import dist as gdist
  from geeco_amd import graph
  from geeco_amd.params import create_e2evmc_config
  from geeco_amd.runtime import TrainStepRunner
  torch.cuda.set_device(0)
  gdist.init_from_env('gloo')
  feats, labels = D._batch(4)
  lo, hi = gdist.shard_bounds(4)
  model = graph.GoalE2EVMC(create_e2evmc_config(D.KW), hi - lo, 'cuda:0', training=True, clip_norm=CLIP)
  if rank == 0:
    model.store.initialize(seed=9)
  gdist.broadcast_variables(model.store)
  model.load_batch({k: torch.from_numpy(v[lo:hi]) for k, v in feats.items()}, {k: torch.from_numpy(v[lo:hi]) for k, v in labels.items()})
  runner = TrainStepRunner(model, use_graph=True, warmup=1)     # the default form: step 1 eager, steps 2-3 replayed
  assert runner.dp and runner.split_adam
  norms = []
  for _ in range(3):
    runner.step()
    torch.cuda.synchronize()
    norms.append(model.clip_out.cpu().numpy().copy())
  q.put((rank, model.store.params.detach().cpu().numpy(), np.stack(norms)))
  torch.distributed.destroy_process_group()


def test_two_ranks_clip_like_one_process(dev):
  """Replicas hold the same exchanged gradients and run the same schedule: bitwise identical parameters and norms; and they equal the
  single-process clipped run on the global batch at the tolerance tests/test_dp_gpu.py holds the unclipped step to."""
  import test_dp_gpu as D
  from geeco_amd import graph
  from geeco_amd.params import create_e2evmc_config
  ctx = mp.get_context('spawn')
  q = ctx.Queue()
  port = 27600 + os.getpid() % 1000
  procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
  for p in procs:
    p.start()
  res = sorted(D._results(procs, q, 2), key=lambda t: t[0])
  for p in procs:
    p.join(timeout=60)
    assert p.exitcode == 0
  feats, labels = D._batch(4)
  model = graph.GoalE2EVMC(create_e2evmc_config(D.KW), 4, dev, training=True, clip_norm=CLIP)
  model.store.initialize(seed=9)
  model.load_batch({k: torch.from_numpy(v) for k, v in feats.items()}, {k: torch.from_numpy(v) for k, v in labels.items()})
  norms = []
  for _ in range(3):
    model.train_step()
    torch.cuda.synchronize()
    norms.append(model.clip_out.cpu().numpy().copy())
  ref, norms = model.store.params.detach().cpu().numpy(), np.stack(norms)
  np.testing.assert_array_equal(res[0][1], res[1][1])                               # replicas stay identical
  np.testing.assert_array_equal(res[0][2].view(np.uint32), res[1][2].view(np.uint32))
  assert (norms[:, 1] > CLIP).all() and (norms[:, 0] < 1.0).all()
  np.testing.assert_allclose(res[0][2], norms, rtol=2e-4)
  np.testing.assert_allclose(res[0][1], ref, rtol=0, atol=3e-4)
  frac_close = np.mean(np.abs(res[0][1] - ref) < 2e-5)
  assert frac_close > 0.99, frac_close
