"""Every instantiation the seven entry points of csrc/attribution.hip and csrc/perturbation.hip can launch, one small case each:
the name ``ops.kernel_trace`` records is exactly the expected one, and the result has the bits of the numpy restatements
(tests/_attribution_ref.py, tests/_perturbation_ref.py; no tolerance anywhere).

tests/test_attribution_gpu.py and tests/test_perturbation_gpu.py hold the arithmetic at more shapes (tails, two grid passes, every
fill form) but never look at the trace, and their images (5 x 7, C in {1, 3, 4}) reach ``perturb_apply_kernel``'s 16-byte path for
C = 4 alone and no C = 2 instantiation at all.  The 57 instantiations, and what selects each template argument:

  attr_path_point_kernel<V, BV>            4    V: dst and x 16-byte aligned; BV: a baseline, its period % 4 == 0, 16-byte aligned
  attr_accumulate_kernel<V, O>             4    V: acc and g aligned; O: overwrite
  attr_finish_kernel<C, V, BV>            16    V: attr, saliency, acc, x aligned; BV as above (multiply_by_input)
  attr_sample_sum_kernel<V>                2    V: attr aligned and S = frames * HW * C a multiple of 4
  perturb_apply_kernel<C, V, R>           16    V: HW * C % 4 == 0, dst and x aligned; R: RISE
  perturb_apply_patch_kernel<C>            4    occlusion with prev_step >= 0
  perturb_score_kernel                     1
  perturb_accumulate_kernel<V, R, O>       8    V: HW % 4 == 0, num and den aligned
  perturb_finish_kernel<V>                 2    V: saliency, num, den aligned

Every one is reachable through the ``ops.*_into`` wrappers; ``test_the_cases_name_all_57`` counts them.  Shapes: N = 2, two frames,
images 4 x 4 (HW * C a multiple of 4 for every C) and 5 x 7 (for C = 4 alone); tensors at a 16-byte boundary and one float past it;
a colour (period C) and a frame (period HW * C) as baseline / fill; RISE with g = 3; the patch (2, 3) on stride (2, 2).  Each case
prints one ``launch <case>: <trace>`` line (profiles/attr_core/launches_*.txt keeps them)."""
import numpy as np
import pytest
import torch

import _attribution_ref as A
import _perturbation_ref as P
from test_perturbation_gpu import KEY, _bits, _dev, _same

pytestmark = pytest.mark.gpu
N, FRAMES = 2, 2
IMAGES = [(4, 4), (5, 7)]
PATCH, STRIDE, G = (2, 3), (2, 2), 3
B = lambda flag: 'true' if flag else 'false'


def _traced(case, want, fn):
  """``fn()`` under the trace: exactly the kernels ``want``, in order."""
  from geeco_amd import ops
  names = ops.kernel_trace(fn)
  torch.cuda.synchronize()
  print('launch %s: %s' % (case, ', '.join(names)))
  assert names == want, (case, names, want)


def _periodic(r, kind, shape, dev, offset=0):
  """(host array or None, device view): 'none'; a 'colour' (period C; for C = 4 that is a multiple of 4, so ``offset`` 1 is what
  keeps it off the 16-byte form); a 'frame' (period HW * C)."""
  if kind == 'none':
    return None, None
  b = r.random(shape[-1:] if kind == 'colour' else shape[-3:], dtype=np.float32)
  return b, _dev(b.reshape(-1), dev, offset)


# ---- attribution.hip ---------------------------------------------------------------------------------------------------------------
POINT_CASES = [(v, bv) for v in (True, False) for bv in (True, False)]


@pytest.mark.parametrize('v,bv', POINT_CASES, ids=['V%d-BV%d' % c for c in POINT_CASES])
def test_path_point_variant(dev, v, bv):
  from geeco_amd import ops
  r = np.random.default_rng(61)
  shape = (N, FRAMES, 4, 4, 3)
  x = r.random(shape, dtype=np.float32)
  x.reshape(-1)[::11] = -0.0
  b, bd = _periodic(r, 'frame' if bv else 'colour', shape, dev)      # period 48 | period 3
  xd, dst = _dev(x, dev, 0 if v else 1), _dev(np.full(shape, np.nan, np.float32), dev, 0 if v else 1)
  _traced('path_point V=%d BV=%d' % (v, bv), ['attr_path_point_kernel<%s, %s>' % (B(v), B(bv))],
          lambda: ops.attr_path_point_into(dst, xd, bd, 0.375))
  assert _same(dst, A.path_point(x, b, 0.375))


@pytest.mark.parametrize('v,o', POINT_CASES, ids=['V%d-O%d' % c for c in POINT_CASES])
def test_accumulate_variant(dev, v, o):
  from geeco_amd import ops
  r = np.random.default_rng(62)
  n = N * FRAMES * 4 * 4 * 3
  acc0, g = r.standard_normal(n).astype(np.float32), r.standard_normal(n).astype(np.float32)
  g[::7] = -0.0
  if o:
    acc0[::5] = np.nan      # whatever the accumulator held is gone
  acc, gd = _dev(acc0, dev, 0 if v else 1), _dev(g, dev, 0 if v else 1)
  _traced('accumulate V=%d O=%d' % (v, o), ['attr_accumulate_kernel<%s, %s>' % (B(v), B(o))],
          lambda: ops.attr_accumulate_into(acc, gd, 1.0 / 3.0, o))
  assert _same(acc, A.accumulate(acc0, g, 1.0 / 3.0, o))


# (C, V, BV, image): the sixteen forms on 4 x 4, where S = 32 C is a multiple of 4 and the sample sum's form follows the alignment;
# on 5 x 7 with C = 1 the tensors are aligned and S = 70 is not: the one-float sample sum behind the 16-byte finish
FINISH_CASES = [(C, v, bv, (4, 4)) for C in (1, 2, 3, 4) for v in (True, False) for bv in (True, False)] + [(1, True, False, (5, 7))]


@pytest.mark.parametrize('C,v,bv,image', FINISH_CASES, ids=['C%d-V%d-BV%d-%dx%d' % ((c[0], c[1], c[2]) + c[3]) for c in FINISH_CASES])
def test_finish_variant(dev, C, v, bv, image):
  from geeco_amd import ops
  r = np.random.default_rng(63)
  shape = (N, FRAMES) + image + (C,)
  HW, off = image[0] * image[1], 0 if v else 1
  x, acc = r.random(shape, dtype=np.float32), r.standard_normal(shape).astype(np.float32)
  acc.reshape(-1)[::11] = -0.0
  b, bd = _periodic(r, 'frame' if bv else 'colour', shape, dev, 0 if bv else 1)
  sv = v and (FRAMES * HW * C) % 4 == 0
  want = ['attr_finish_kernel<%d, %s, %s>' % (C, B(v), B(bv)), 'attr_sample_sum_kernel<%s>' % B(sv)]
  accd, xd = _dev(acc, dev, off), _dev(x, dev, off)
  attr, sal = _dev(np.full(shape, np.nan, np.float32), dev, off), _dev(np.full(shape[:-1], np.nan, np.float32), dev, off)
  sums = torch.full((N,), float('nan'), device=dev)
  _traced('finish C=%d V=%d BV=%d %dx%d' % ((C, v, bv) + image), want,
          lambda: ops.attr_finish_into(attr, sal, sums, accd, xd, bd, True, N, FRAMES, HW, C))
  want_attr, want_sal, want_sum = A.finish(acc, x, b, True)
  assert _same(attr, want_attr) and _same(sal, want_sal) and _same(sums, want_sum)


# ---- perturbation.hip --------------------------------------------------------------------------------------------------------------
def _desc(ops, rise, H, W):
  if rise:
    return ops.perturb_desc('rise', H, W, grid=G, keep_prob=0.5, key=KEY)
  return ops.perturb_desc('occlusion', H, W, patch=PATCH, stride=STRIDE)


def _field(rise, H, W, step):
  return P.rise_field(H, W, G, 0.5, KEY, step, N) if rise else P.occlusion_field(H, W, PATCH, STRIDE, step, N)


# (C, one-float offset, RISE, image): V = the frames start on multiples of four floats (HW * C % 4 == 0) and the tensors are aligned
APPLY_CASES = [(C, off, rise, (4, 4)) for C in (1, 2, 3, 4) for off in (0, 1) for rise in (False, True)] + \
              [(C, 0, rise, (5, 7)) for C in (1, 2, 3, 4) for rise in (False, True)]


@pytest.mark.parametrize('C,off,rise,image', APPLY_CASES, ids=['C%d-off%d-R%d-%dx%d' % ((c[0], c[1], c[2]) + c[3]) for c in APPLY_CASES])
def test_apply_variant(dev, C, off, rise, image):
  from geeco_amd import ops
  r = np.random.default_rng(64)
  H, W = image
  shape = (N, FRAMES, H, W, C)
  x = r.random(shape, dtype=np.float32)
  x.reshape(-1)[::11] = -0.0
  v = off == 0 and (H * W * C) % 4 == 0
  desc, o = _desc(ops, rise, H, W), _field(rise, H, W, 1)
  assert o.any()
  xd = _dev(x, dev, off)
  for kind in ('none', 'colour', 'frame'):      # the baseline's form is a runtime argument of this kernel: one name for all three
    fill, fd = _periodic(r, kind, shape, dev)
    dst = _dev(np.full(shape, np.nan, np.float32), dev, off)
    _traced('apply C=%d off=%d R=%d %dx%d fill=%s' % (C, off, rise, H, W, kind), ['perturb_apply_kernel<%d, %s, %s>' % (C, B(v), B(rise))],
            lambda: ops.perturb_apply_into(dst, xd, fd, desc, 1))
    assert _same(dst, P.apply(x, fill, o)), kind


@pytest.mark.parametrize('C', [1, 2, 3, 4])
def test_apply_patch_variant(dev, C):
  """The incremental form: dst holds step 0, the launch writes step 1's patch and what step 0 hid outside it."""
  from geeco_amd import ops
  r = np.random.default_rng(65)
  shape = (N, FRAMES, 4, 4, C)
  x = r.random(shape, dtype=np.float32)
  x.reshape(-1)[::11] = -0.0
  desc = _desc(ops, False, 4, 4)
  xd, dst = _dev(x, dev), _dev(np.full(shape, np.nan, np.float32), dev)
  for kind in ('none', 'colour'):
    fill, fd = _periodic(r, kind, shape, dev)
    ops.perturb_apply_into(dst, xd, fd, desc, 0)
    _traced('apply_patch C=%d fill=%s' % (C, kind), ['perturb_apply_patch_kernel<%d>' % C],
            lambda: ops.perturb_apply_into(dst, xd, fd, desc, 1, prev_step=0))
    assert _same(dst, P.apply(x, fill, _field(False, 4, 4, 1))), kind


def test_score_variant(dev):
  from geeco_amd import ops
  r = np.random.default_rng(66)
  p, p0 = r.standard_normal((N, 7)).astype(np.float32), r.standard_normal((N, 7)).astype(np.float32)
  w = (np.arange(7) % 3 != 1).astype(np.float32)
  d = torch.full((N,), float('nan'), device=dev)
  pd, p0d, wd = _dev(p, dev), _dev(p0, dev, 1), _dev(w, dev)
  _traced('score', ['perturb_score_kernel'], lambda: ops.perturb_score_into(d, pd, p0d, wd))
  assert _same(d, P.score(p, p0, w))


# (one-float offset, RISE, overwrite, image): V = HW % 4 == 0 and num, den aligned
ACCUMULATE_CASES = [(off, rise, o, (4, 4)) for off in (0, 1) for rise in (False, True) for o in (True, False)] + [(0, False, False, (5, 7))]


@pytest.mark.parametrize('off,rise,o,image', ACCUMULATE_CASES, ids=['off%d-R%d-O%d-%dx%d' % ((c[0], c[1], c[2]) + c[3]) for c in ACCUMULATE_CASES])
def test_perturb_accumulate_variant(dev, off, rise, o, image):
  from geeco_amd import ops
  r = np.random.default_rng(67)
  H, W = image
  v = off == 0 and (H * W) % 4 == 0
  desc, field = _desc(ops, rise, H, W), _field(rise, H, W, 1)
  num0, den0 = r.standard_normal((N, H, W)).astype(np.float32), r.random((N, H, W), dtype=np.float32)
  if o:
    num0[:], den0[:] = np.nan, np.nan      # not read
  d = np.array([0.75, np.nan], np.float32)      # sample 1: the NaN reaches the pixels the step hid and no other
  num, den, dd = _dev(num0, dev, off), _dev(den0, dev, off), _dev(d, dev)
  _traced('perturb_accumulate off=%d R=%d O=%d %dx%d' % (off, rise, o, H, W),
          ['perturb_accumulate_kernel<%s, %s, %s>' % (B(v), B(rise), B(o))], lambda: ops.perturb_accumulate_into(num, den, dd, desc, 1, o))
  want_num, want_den = P.accumulate(num0, den0, d, field, o)
  assert _same(num, want_num) and _same(den, want_den)
  assert np.array_equal(np.isnan(want_num[1]), field[1] != 0) and field[1].any() and not np.isnan(want_num[0]).any()


@pytest.mark.parametrize('v', [True, False], ids=['V1', 'V0'])
def test_perturb_finish_variant(dev, v):
  from geeco_amd import ops
  r = np.random.default_rng(68)
  num, den = r.standard_normal((N, 5, 7)).astype(np.float32), r.random((N, 5, 7), dtype=np.float32)
  den.reshape(-1)[::3] = 0.0      # no step hid the pixel: +0
  num.reshape(-1)[4] = np.nan
  off = 0 if v else 1
  sal, numd, dend = _dev(np.full((N, 5, 7), np.nan, np.float32), dev, off), _dev(num, dev, off), _dev(den, dev, off)
  _traced('perturb_finish V=%d' % v, ['perturb_finish_kernel<%s>' % B(v)], lambda: ops.perturb_finish_into(sal, numd, dend))
  want = P.finish(num, den)
  assert _same(sal, want) and not _bits(want.reshape(-1)[::3]).any() and np.isnan(want).sum() == 1


def test_the_cases_name_all_57():
  """The tables above, through the same name rules, name every instantiation the two files compile: 57."""
  names = {'attr_path_point_kernel<%s, %s>' % (B(v), B(bv)) for v, bv in POINT_CASES}
  names |= {'attr_accumulate_kernel<%s, %s>' % (B(v), B(o)) for v, o in POINT_CASES}
  for C, v, bv, image in FINISH_CASES:
    names |= {'attr_finish_kernel<%d, %s, %s>' % (C, B(v), B(bv)), 'attr_sample_sum_kernel<%s>' % B(v and (FRAMES * image[0] * image[1] * C) % 4 == 0)}
  names |= {'perturb_apply_kernel<%d, %s, %s>' % (C, B(off == 0 and (im[0] * im[1] * C) % 4 == 0), B(rise)) for C, off, rise, im in APPLY_CASES}
  names |= {'perturb_apply_patch_kernel<%d>' % C for C in (1, 2, 3, 4)} | {'perturb_score_kernel'}
  names |= {'perturb_accumulate_kernel<%s, %s, %s>' % (B(off == 0 and (im[0] * im[1]) % 4 == 0), B(rise), B(o)) for off, rise, o, im in ACCUMULATE_CASES}
  names |= {'perturb_finish_kernel<%s>' % B(v) for v in (True, False)}
  assert len(names) == 57, sorted(names)
