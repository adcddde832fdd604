"""Perturbation attributions without a GPU: the occluder grid of the library's host function against the formula and
the restatement of tests/_perturbation_ref.py, the mirrored description, the argument checks, and the statistics of the restated
RISE masks (the bound the GPU test holds the device to is first met by the reference alone)."""
import ctypes

import numpy as np
import pytest

import _abi
import _perturbation_ref as P


def rise_share_bound(H, W, g, keep_prob, masks):
  """(p, bound) for the mean of keep = 1 - o over ``masks`` independent masks.  A mask's mean is sum_b a_b bit_b with a_b >= 0,
  sum_b a_b = 1 (bilinear weights), bits independent Bernoulli(p), p = threshold / 2^32: its expectation is p whatever the shift,
  and its variance p (1 - p) sum_b a_b^2 <= p (1 - p) max_b a_b.  A bit reaches the pixels within one cell of it either way, at
  most (2 ch)(2 cw) of the H W, each with weight <= 1 / (H W): max_b a_b <= min(1, 4 ch cw / (H W)).  The bound is six standard
  deviations of the mean of ``masks`` such draws."""
  p = P.keep_threshold(keep_prob) / 2.0 ** 32
  ch, cw = -(-H // g), -(-W // g)
  var = p * (1 - p) * min(1.0, 4.0 * ch * cw / (H * W))
  return p, 6.0 * np.sqrt(var / masks)


@pytest.mark.parametrize('size,patch,stride', [(H, ph, sy) for H in (1, 5, 7, 16, 136) for ph in (1, 2, 3, 5, 64, 200) for sy in (1, 2, 3, 48, 500)])
def test_grid_covers_every_pixel_and_matches_the_formula(size, patch, stride):
  pos = P.positions(size, patch, stride)
  p = min(patch, size)
  G = 1 if patch >= size else int(np.ceil((size - patch) / stride)) + 1
  assert len(pos) == G and pos == [min(j * stride, size - p) for j in range(G)]
  covered = np.zeros(size, bool)
  for y in pos:
    assert 0 <= y and y + p <= size
    covered[y:y + p] = True
  assert pos[0] == 0 and pos[-1] == size - p and covered[0] and covered[-1]
  assert covered.all() or stride > p      # a stride within the patch leaves no gap (a wider one samples: those pixels get +0)


@pytest.mark.parametrize('H,W,patch,stride', [(5, 7, (2, 3), (2, 2)), (5, 7, (5, 7), (1, 1)), (5, 7, (9, 8), (2, 2)), (136, 136, (64, 64), (48, 48)),
                                              (256, 256, (64, 64), (32, 32)), (7, 5, (7, 2), (3, 2))])
def test_library_grid_is_the_restated_grid(H, W, patch, stride):
  from geeco_amd import ops
  Gy, Gx, rects = P.occlusion_grid(H, W, patch, stride)
  desc = ops.perturb_desc('occlusion', H, W, patch=patch, stride=stride)
  assert ops.perturb_steps(desc) == Gy * Gx == len(rects)
  for m, rect in enumerate(rects):
    assert ops.perturb_patch(desc, m) == (Gy, Gx, rect), m
    assert P.occlusion_field(H, W, patch, stride, m, 1).sum() == (rect[1] - rect[0]) * (rect[3] - rect[2])
  if (H, W, patch) == (136, 136, (64, 64)):
    assert (Gy, Gx) == (3, 3) and rects[-1] == (72, 136, 72, 136)      # the 9 steps of the whole-pass test; the last one clamped
  from geeco_amd._native import GeecoNativeError
  with pytest.raises(GeecoNativeError, match='outside the grid'):
    ops.perturb_patch(desc, Gy * Gx)
  rise = ops.perturb_desc('rise', H, W, grid=3, keep_prob=0.5)
  assert ops.perturb_patch(rise, 7) == (0, 0, (0, 0, 0, 0))


def test_description_mirrors_the_header():
  from geeco_amd import _native, ops
  kinds = {'int32_t': ctypes.c_int32, 'uint32_t': ctypes.c_uint32, 'uint64_t': ctypes.c_uint64}
  fields = _abi.struct_fields('geeco_perturb_desc')
  assert [(f, kinds[t]) for f, t, length in fields if length is None] == list(_native.PerturbDesc._fields_)
  assert _native.load().geeco_perturb_desc_sizeof() == ctypes.sizeof(_native.PerturbDesc) == 48
  assert [(n, _abi.define(n)) for n in _abi.defines('GEECO_PERTURB_')] == [('GEECO_PERTURB_' + m.upper(), i) for i, m in enumerate(_native.PERTURB_METHODS)]
  for name in ('geeco_perturb_patch', 'geeco_perturb_apply', 'geeco_perturb_score', 'geeco_perturb_accumulate', 'geeco_perturb_finish',
               'geeco_perturb_desc_sizeof'):
    assert name in _abi.added_within(7) and name in _native.SIGNATURES
  assert ops.perturb_desc('rise', 8, 8, grid=4, keep_prob=0.5).keep_threshold == 1 << 31 == P.keep_threshold(0.5)
  assert ops.perturb_desc('rise', 8, 8, grid=4, keep_prob=1e-12).keep_threshold == 1
  assert ops.perturb_desc('rise', 8, 8, grid=4, keep_prob=1 - 1e-12).keep_threshold == (1 << 32) - 1


def test_description_refuses_bad_arguments():
  from geeco_amd import ops
  for kw, words in [(dict(method='blur'), 'method'), (dict(method='occlusion', patch=(0, 2), stride=(1, 1)), 'patch'),
                    (dict(method='occlusion', patch=(2, 2), stride=None), 'stride'), (dict(method='occlusion', patch=(2.5, 2), stride=(1, 1)), 'patch'),
                    (dict(method='rise', grid=1, keep_prob=0.5), 'grid'), (dict(method='rise', grid=32, keep_prob=0.5), 'grid'),
                    (dict(method='rise', grid=4, keep_prob=0.0), 'keep_prob'), (dict(method='rise', grid=4, keep_prob=1.0), 'keep_prob'),
                    (dict(method='rise', grid=4, keep_prob=0.5, key=1 << 64), 'key')]:
    with pytest.raises(ValueError, match=words):
      ops.perturb_desc(H=8, W=8, **kw)
  with pytest.raises(ValueError, match='H=0'):
    ops.perturb_desc('occlusion', 0, 8, patch=(1, 1), stride=(1, 1))


def test_pass_arguments_are_checked():
  from geeco_amd.perturbation import check_perturbation_arguments as check
  check('occlusion', patch=64, stride=(48, 48))
  check('occlusion')
  check('rise', grid=7, keep_prob=0.5, steps=6, score='loss', seed=3)
  for kw, words in [(dict(method='smoothgrad'), 'method'), (dict(method='occlusion', score='gradient'), 'score'),
                    (dict(method='occlusion', patch=0), 'patch'), (dict(method='occlusion', patch=(2, 2, 2)), 'patch'),
                    (dict(method='occlusion', stride=(1.5, 1)), 'stride'), (dict(method='rise', grid=1), 'grid'), (dict(method='rise', grid=2.0), 'grid'),
                    (dict(method='rise', keep_prob=1.0), 'keep_prob'), (dict(method='rise', steps=0), 'steps'),
                    (dict(method='rise', seed=-1), 'seed')]:
    with pytest.raises(ValueError, match='perturbation_attributions: ' + words):
      check(**kw)


def test_restated_fields_and_estimator():
  """The restatement on its own: hard fields, exact copies, the NaN rule and the map of a two-step pass worked by hand."""
  o0, o1 = P.occlusion_field(2, 3, (1, 2), (1, 1), 0, 1), P.occlusion_field(2, 3, (1, 2), (1, 1), 1, 1)
  assert o0.tolist() == [[[1, 1, 0], [0, 0, 0]]] and o1.tolist() == [[[0, 1, 1], [0, 0, 0]]]
  x = np.array([-0.0, 1.5, 2.5, 3.5, 4.5, 5.5], np.float32).reshape(1, 2, 3, 1)
  got = P.apply(x, np.array([9.0], np.float32), o0)
  assert got.reshape(-1).tolist() == [9, 9, 2.5, 3.5, 4.5, 5.5]
  assert np.array_equal(P.apply(x, x, o0).view(np.uint32), x.view(np.uint32))      # fill = the input: the input's bits, -0 included
  sal, den = P.saliency([o0, o1], np.array([[2.0], [np.nan]], np.float32))
  assert den.tolist() == [[[1, 2, 1], [0, 0, 0]]]
  assert sal[0, 0, 0] == 2 and np.isnan(sal[0, 0, 1:]).all() and (sal[0, 1] == 0).all() and not np.signbit(sal[0, 1]).any()
  assert P.score([[1, 2, 4]], [[0, 0, 1]], [1, 0, 1]).tolist() == [10.0]


@pytest.mark.parametrize('H,W,g', [(5, 7, 3), (8, 8, 4)])
def test_restated_rise_masks(H, W, g):
  """o in [0, 1]; a mask is a function of (key, step, sample) alone; the mean keep-share over 256 steps x 3 samples sits inside
  the binomial bound (derived in ``rise_share_bound``) the GPU test then holds the device to."""
  key, N, steps = 0x243f6a8885a308d3, 3, 256
  fields = np.stack([P.rise_field(H, W, g, 0.5, key, m, N) for m in range(steps)])
  assert fields.min() >= 0 and fields.max() <= 1 and ((fields > 0) & (fields < 1)).any()
  assert np.array_equal(P.rise_field(H, W, g, 0.5, key, 5, 1, sample0=2)[0], fields[5, 2])
  assert not np.array_equal(fields[0], fields[1]) and not np.array_equal(fields[0, 0], fields[0, 1])
  bits, dy, dx = P.rise_draws(H, W, g, 0.5, key, 0, 0)
  assert bits.shape == (g + 1, g + 1) and set(np.unique(bits)) <= {0.0, 1.0} and 0 <= dy < -(-H // g) and 0 <= dx < -(-W // g)
  p, bound = rise_share_bound(H, W, g, 0.5, steps * N)
  share = float((1.0 - fields.astype(np.float64)).mean())
  print('RISE %dx%d g=%d: keep share %.4f, p %.4f, bound %.4f' % (H, W, g, share, p, bound))
  assert abs(share - p) <= bound < 0.1
  p3, bound3 = rise_share_bound(H, W, g, 0.25, steps)
  share3 = float((1.0 - np.stack([P.rise_field(H, W, g, 0.25, key + 1, m, 1) for m in range(steps)]).astype(np.float64)).mean())
  assert abs(share3 - p3) <= bound3 and abs(share3 - p) > bound      # the threshold follows keep_prob
