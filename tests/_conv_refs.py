"""fp64 references, rounding bounds, seeded inputs and the case list for the gather GEMM (geeco_amd/csrc/conv_gemm.hip):
tests/test_conv_gemm_variants_gpu.py holds the device side, tests/test_conv_refs_cpu.py shows that the bounds reject wrong kernels,
tests/test_conv_cover_cpu.py that the case list (tests/native/conv_gemm_cases.txt) runs every launch variant the model reaches.
The same four parts for the filter gradient (geeco_conv3x3_wgrad) are at the end of this file: tests/native/conv_wgrad_cases.txt,
tests/test_conv_wgrad_variants_gpu.py, tests/test_conv_wgrad_refs_cpu.py, tests/test_conv_wgrad_cover_cpu.py.  Behind them the same
four parts for the LDS-halo and LDS-staged forwards and input gradients: tests/native/conv_halo_cases.txt,
tests/test_conv_halo_variants_gpu.py, tests/test_conv_halo_refs_cpu.py, tests/test_conv_halo_cover_cpu.py.  Last, for the fused
encoder-bottom backward (conv2's input gradient + conv1's filter gradient in one kernel): tests/native/conv_bottom_cases.txt,
tests/test_conv_bottom_variants_gpu.py, tests/test_conv_bottom_refs_cpu.py, tests/test_conv_bottom_cover_cpu.py.

Everything here is written from the definition of tf.layers.conv2d(kernel_size=3, padding='SAME') on NHWC tensors with an HWIO
kernel, not from the kernels: the padded input is built explicitly, the output is the sum over the nine taps of a strided window
times that tap's [Cin][Cout] matrix, and the input gradient scatters dz times the transposed matrix back to the window's pixels.
float64 throughout, on the float32 values the device is given.  comparison helpers: tests/_primitive_refs.py.
"""
import collections
import functools
import math
import os
import re

import numpy as np
import torch

from _primitive_refs import U, assert_within, within, worst_ratio      # noqa: F401  (one import for the tests of this family)


# --------------------------------------------------------------------------------------------------------------------------
# TF SAME padding
# --------------------------------------------------------------------------------------------------------------------------
def same_pad(size, stride, k=3):
  """out = ceil(size / stride); pad_total = max((out - 1) * stride + k - size, 0); the smaller half goes on top / left."""
  out = -(-size // stride)
  total = max((out - 1) * stride + k - size, 0)
  return out, total // 2, total - total // 2


def _mm(a, b):
  """[M][K] @ [K][N] in float64 on torch's thread pool (tests/conftest.py sizes it to the cores the job owns)."""
  return (torch.from_numpy(np.ascontiguousarray(a)) @ torch.from_numpy(np.ascontiguousarray(b))).numpy()


def _fwd(x, w, stride):
  N, H, W, Cin = x.shape
  Cout = w.shape[3]
  Ho, pt, pb = same_pad(H, stride)
  Wo, pl, pr = same_pad(W, stride)
  xp = np.zeros((N, H + pt + pb, W + pl + pr, Cin))
  xp[:, pt:pt + H, pl:pl + W] = x
  y = np.zeros((N * Ho * Wo, Cout))
  for ky in range(3):
    for kx in range(3):
      win = xp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride]
      y += _mm(win.reshape(N * Ho * Wo, Cin), w[ky, kx])
  return y.reshape(N, Ho, Wo, Cout)


def _dgrad(dz, w, in_hw, stride):
  N, Ho, Wo, Cout = dz.shape
  H, W = in_hw
  Cin = w.shape[2]
  ho, pt, pb = same_pad(H, stride)
  wo, pl, pr = same_pad(W, stride)
  assert (ho, wo) == (Ho, Wo), (dz.shape, in_hw, stride)
  dxp = np.zeros((N, H + pt + pb, W + pl + pr, Cin))
  flat = dz.reshape(N * Ho * Wo, Cout)
  for ky in range(3):
    for kx in range(3):
      # y[i][j] takes xp[s i + ky][s j + kx] . w[ky][kx], so that pixel receives dz[i][j] . w[ky][kx]^T
      dxp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride] += _mm(flat, w[ky, kx].T).reshape(N, Ho, Wo, Cin)
  return np.ascontiguousarray(dxp[:, pt:pt + H, pl:pl + W])


def conv_fwd_ref(x, w, b, stride, relu):
  """x [N][H][W][Cin], w [3][3][Cin][Cout], b [Cout] or None -> (y, mag, pre): y = relu(pre) or pre, pre = conv + bias, and mag the
  same operation on |x|, |w|, |b| without ReLU: per element, the sum of the magnitudes of its terms."""
  x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
  b = np.zeros(w.shape[3]) if b is None else np.asarray(b, np.float64)
  pre = _fwd(x, w, stride) + b
  mag = _fwd(np.abs(x), np.abs(w), stride) + np.abs(b)
  return (np.maximum(pre, 0.0) if relu else pre), mag, pre


def conv_dgrad_ref(dz, w, in_hw, stride, mask):
  """dz [N][Ho][Wo][Cout], w [3][3][Cin][Cout] (the forward's HWIO kernel), mask [N][H][W][Cin] or None -> (dx, mag, pre):
  dx = pre where mask > 0 (everywhere without a mask), else 0; mag as in conv_fwd_ref, without the mask."""
  dz, w = np.asarray(dz, np.float64), np.asarray(w, np.float64)
  pre = _dgrad(dz, w, in_hw, stride)
  mag = _dgrad(np.abs(dz), np.abs(w), in_hw, stride)
  dx = pre if mask is None else np.where(np.asarray(mask) > 0, pre, 0.0)
  return dx, mag, pre


def dgrad_terms(in_hw, stride, Cout):
  """[H][W][1]: the number of products in one element of the input gradient = (taps that reach the pixel) * Cout.  Pixel Y of the
  input is read by output row i through tap ky when s i + ky = Y + pad_top: per axis, the ky in 0..2 congruent to Y + pad_top
  modulo s (stride 2: one or two, i.e. 1 / 2 / 2 / 4 taps for the four parity classes; stride 1: all nine)."""
  H, W = in_hw
  _, pt, _ = same_pad(H, stride)
  _, pl, _ = same_pad(W, stride)
  ty = np.array([sum((Y + pt - k) % stride == 0 for k in range(3)) for Y in range(H)])
  tx = np.array([sum((X + pl - k) % stride == 0 for k in range(3)) for X in range(W)])
  return (ty[:, None] * tx[None, :])[:, :, None] * float(Cout)


# --------------------------------------------------------------------------------------------------------------------------
# bounds
# --------------------------------------------------------------------------------------------------------------------------
def conv_bound(mag, terms, S):
  """(terms + S + 4) U mag per element, U = 2**-24, for an element that is a sum of at most ``terms`` products (forward: 9 Cin;
  input gradient: the pixel's tap count * Cout, dgrad_terms) computed in float32 in ``S`` split-K slabs.
    products: each is rounded once, alone or inside a fused multiply-add              -> U mag in all;
    additions: a sum of n terms takes n - 1 additions in whatever order (MFMA accumulation chains, the order of the K-steps);
         each moves the result by at most U times a partial sum of magnitudes <= mag   -> (terms - 1) U mag;
    slabs: S - 1 further additions of partial sums                                    -> (S - 1) U mag;
    bias: one addition                                                                -> U mag;
    in all (terms + S) U mag to first order.  The remaining 4 U mag hold the second-order terms, (1 + U)^n - 1 - n U < n^2 U^2:
    0.33 U at n = 2304 + 18, the longest sum of the case list.
  The bound is worst case: the rounding errors of a real sum add like a random walk and use about 1 / sqrt(terms) of it.  It still
  separates: one dropped term of typical size is mag / terms, above the bound until terms^2 reaches 1 / U (terms = 4096)."""
  return (np.asarray(terms, np.float64) + S + 4.0) * U * mag


def conv_expect(pre, mag, terms, S, relu=False, mask=None):
  """-> (ref, bound, keep) per element for a launch with ReLU (forward) or a mask (input gradient).
    no ReLU, no mask: ref = pre under conv_bound.
    ReLU: where pre > bound the float32 sum is positive too: ref = pre under the bound; where pre < -bound it is negative: ref = 0
         with bound 0; where |pre| <= bound either is possible: the element is left out (keep = False) -- the callers require that
         share to stay below 0.1 %.
    mask: the mask is data, not a computed sign: where it is not > 0 the result is 0 with bound 0, elsewhere pre under the bound."""
  assert not (relu and mask is not None)
  bound = np.broadcast_to(conv_bound(mag, terms, S), pre.shape).copy()
  ref = pre.copy()
  keep = np.ones(pre.shape, bool)
  if relu:
    keep = np.abs(pre) > bound
    neg = pre < -bound
    ref[neg] = 0.0
    bound[neg] = 0.0
  if mask is not None:
    off = ~(np.asarray(mask) > 0)
    ref[off] = 0.0
    bound[off] = 0.0
  return ref, bound, keep


LEFT_OUT_MAX = 1e-3


def left_out(keep):
  return 1.0 - float(np.mean(keep)) if keep.size else 0.0


# --------------------------------------------------------------------------------------------------------------------------
# the case list
# --------------------------------------------------------------------------------------------------------------------------
CASES_TXT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'native', 'conv_gemm_cases.txt')

Case = collections.namedtuple('Case', 'index dir G N H W Cin Cout stride flags text plan BM BN ut S planS ncls')


def load_cases():
  """The cases of tests/native/conv_gemm_cases.txt with the variant recorded beside each (tests/test_conv_cover_cpu.py holds that
  text against what conv_plan / conv_gemm_grid give)."""
  cases = []
  for line in open(CASES_TXT):
    line = line.strip()
    if not line or line.startswith('#'):
      continue
    text, plan = (s.strip() for s in line.split('|'))
    f = text.split()
    kv = dict(t.split('=') for t in plan.split()[2:])
    bm, bn = (int(v) for v in plan.split()[1].split('x'))
    assert plan.split()[0] == f[0], line
    cases.append(Case(len(cases), f[0], *(int(v) for v in f[1:8]), frozenset(f[8:]), text, plan, bm, bn, kv['ut'] == '1',
                      int(kv['S']), int(kv['planS']), int(kv['ncls'])))
  return cases


def case_id(c):
  return c.text.replace(' ', '-')


def kernel_name(c):
  """The name launch_cfg notes for the case's tile: 2 x 2 waves for the 64-, 96- and 128-wide tiles, 4 x 1 for the narrow ones."""
  wm, wn = (2, 2) if c.BN >= 64 else (4, 1)
  return 'conv_gemm_kernel<%d, %d, 16, %d, %d, %s>' % (c.BM, c.BN, wm, wn, 'true' if c.ut else 'false')


def out_hw(c):
  return same_pad(c.H, c.stride)[0], same_pad(c.W, c.stride)[0]


def case_inputs(c):
  """Seeded float32 operands of a case, per group.
  Forward: x ~ N(0, 1), w ~ N(0, 1 / (9 Cin)) (pre-activations of unit variance), bias of magnitude 2..4 and either sign: a bias
  near zero would put the pre-activations of its channel around zero, where the sign of a float32 sum is not determined and the
  element has to be left out; with this bias the negative channels are mostly cut by the ReLU and the left-out share stays under
  0.1 % up to the 2304-term sums (tests/test_conv_refs_cpu.py checks every case).
  Input gradient: dz ~ N(0, 1), w ~ N(0, 1 / (9 Cout)), mask ~ N(0, 1) with three tenths exact zeros: positive, zero and negative
  entries (the kernel's test is mask > 0)."""
  r = np.random.default_rng(1000 + c.index)
  G, N, H, W, Cin, Cout = c.G, c.N, c.H, c.W, c.Cin, c.Cout
  Ho, Wo = out_hw(c)
  f = lambda a: a.astype(np.float32)
  if c.dir == 'fwd':
    x = f(r.standard_normal((G, N, H, W, Cin)))
    w = f(r.standard_normal((G, 3, 3, Cin, Cout)) / math.sqrt(9 * Cin))
    b = f(np.sign(r.standard_normal((G, Cout))) * r.uniform(2.0, 4.0, (G, Cout))) if 'bias' in c.flags else None
    return dict(x=x, w=w, b=b)
  dz = f(r.standard_normal((G, N, Ho, Wo, Cout)))
  w = f(r.standard_normal((G, 3, 3, Cin, Cout)) / math.sqrt(9 * Cout))
  mask = None
  if 'mask' in c.flags:
    mask = r.standard_normal((G, N, H, W, Cin))
    mask[r.uniform(size=mask.shape) < 0.3] = 0.0
    mask = f(mask)
  return dict(dz=dz, w=w, mask=mask)


def case_expect(c):
  """(inputs, ref, bound, keep, pre, mag), the last five [G][...].  Not cached: every case is one test's, and the large ones
  hold some hundred megabytes in float64."""
  inp = case_inputs(c)
  out = []
  for g in range(c.G):
    if c.dir == 'fwd':
      _, mag, pre = conv_fwd_ref(inp['x'][g], inp['w'][g], None if inp['b'] is None else inp['b'][g], c.stride, False)
      out.append(conv_expect(pre, mag, 9 * c.Cin, c.S, relu='relu' in c.flags) + (pre, mag))
    else:
      m = None if inp['mask'] is None else inp['mask'][g]
      _, mag, pre = conv_dgrad_ref(inp['dz'][g], inp['w'][g], (c.H, c.W), c.stride, None)
      out.append(conv_expect(pre, mag, dgrad_terms((c.H, c.W), c.stride, c.Cout), c.S, mask=m) + (pre, mag))
  return (inp,) + tuple(np.stack([o[i] for o in out]) for i in range(5))


# --------------------------------------------------------------------------------------------------------------------------
# filter gradient (geeco_conv3x3_wgrad): reference, bound, case list
# --------------------------------------------------------------------------------------------------------------------------
def _wgrad(x, dz, stride):
  N, H, W, Cin = x.shape
  _, Ho, Wo, Cout = dz.shape
  ho, pt, pb = same_pad(H, stride)
  wo, pl, pr = same_pad(W, stride)
  assert (ho, wo) == (Ho, Wo), (x.shape, dz.shape, stride)
  xp = np.zeros((N, H + pt + pb, W + pl + pr, Cin))
  xp[:, pt:pt + H, pl:pl + W] = x
  flat = dz.reshape(N * Ho * Wo, Cout)
  dw = np.zeros((3, 3, Cin, Cout))
  for ky in range(3):
    for kx in range(3):
      # y[i][j] = sum xp[s i + ky][s j + kx] . w[ky][kx], so w[ky][kx][ci][co] receives xp[s i + ky][s j + kx][ci] dz[i][j][co]
      win = xp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride]
      dw[ky, kx] = _mm(win.reshape(N * Ho * Wo, Cin).T, flat)
  return dw, flat.sum(0)


def conv_wgrad_ref(x, dz, stride):
  """x [N][H][W][Cin], dz [N][Ho][Wo][Cout] -> (dw [3][3][Cin][Cout], db [Cout], mag_dw, mag_db): the gradients of
  sum(conv(x, w) + b) . dz with respect to w and b, and the same sums over |x|, |dz|: per element, the sum of the magnitudes of
  its terms."""
  x, dz = np.asarray(x, np.float64), np.asarray(dz, np.float64)
  dw, db = _wgrad(x, dz, stride)
  mag_dw, mag_db = _wgrad(np.abs(x), np.abs(dz), stride)
  return dw, db, mag_dw, mag_db


def wgrad_bound(mag, slice_px, S):
  """(slice_px + S + 8) U mag per element, U = 2**-24, for an element of dw or db: a sum over all output pixels, computed in
  float32 in S slices of at most ``slice_px`` pixels each (one slab per slice) and a slab sum.
    products: each is rounded once, alone or inside a fused multiply-add (db: none)           -> U mag in all;
    inside a slice: a sum of n <= slice_px terms takes n - 1 additions in whatever order (MFMA accumulation chains, the order
         of the tiles); each moves the result by at most U times a partial sum of magnitudes    -> (slice_px - 1) U mag;
    the kernels that keep four waves' partial tiles of one slice (conv1's, the 32 -> 48 halo kernel) combine them through LDS:
         at most 3 further additions                                                            -> 3 U mag;
    slab sum: S - 1 additions of partial sums, in whatever grouping (the split form adds four waves' shares)  -> (S - 1) U mag;
    in all (slice_px + S + 3) U mag to first order.  The remaining 5 U mag hold the second-order terms,
    (1 + U)^n - 1 - n U < n^2 U^2: 0.05 U at n = 128 + 768 + 3, the longest chain of the case list.
  The bound is worst case; a real float32 sum uses about 1 / sqrt(terms) of it.  It cannot see one dropped pixel once
  slice_px + S passes a few thousand -- for that the device test has its exact pass (small integers: any order of float32
  additions gives the float64 result) and keeps this one for what integers cannot show: a product path of reduced precision."""
  return (float(slice_px) + S + 8.0) * U * mag


WGRAD_CASES_TXT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'native', 'conv_wgrad_cases.txt')

WgradCase = collections.namedtuple('WgradCase', 'index G N H W Cin Cout stride flags text plan family inst S reduce slice_px remainder '
                                   'unreached')
_WGRAD_PLAN = re.compile(r'^(halo|conv1|lds|generic) (.+) S=(\d+) reduce=(split|plain|none) slice_px=(\d+)( remainder)?( unreached)?$')


def load_wgrad_cases():
  """The cases of tests/native/conv_wgrad_cases.txt with the plan recorded beside each (tests/test_conv_wgrad_cover_cpu.py holds
  that text against what geeco_amd/csrc/conv_wgrad_plan.h gives)."""
  cases = []
  for line in open(WGRAD_CASES_TXT):
    line = line.strip()
    if not line or line.startswith('#'):
      continue
    text, plan = (s.strip() for s in line.split('|'))
    f = text.split()
    m = _WGRAD_PLAN.match(plan)
    assert m and set(f[7:]) <= {'nodb'}, line
    cases.append(WgradCase(len(cases), *(int(v) for v in f[:7]), frozenset(f[7:]), text, plan, m.group(1), m.group(2),
                           int(m.group(3)), m.group(4), int(m.group(5)), bool(m.group(6)), bool(m.group(7))))
  return cases


def wgrad_key(c):
  """The key tests/native/conv_wgrad_cover.cpp prints for the sweep's launches."""
  return '%s %s reduce=%s %s %s' % (c.family, c.inst, c.reduce, 'S>1' if c.S > 1 else 'S=1', 'remainder' if c.remainder else 'regular')


def wgrad_kernel_names(c):
  """What ops.kernel_trace records for the case: the instantiation, and the slab-sum kernel unless the kernel wrote dw itself."""
  return [c.inst] + ({'split': ['wgrad_reduce_kernel<true>'], 'plain': ['wgrad_reduce_kernel<false>'], 'none': []}[c.reduce])


def wgrad_out_hw(c):
  return same_pad(c.H, c.stride)[0], same_pad(c.W, c.stride)[0]


def wgrad_pixels(c):
  """M: output pixels per group, the number of terms of every element of dw and db."""
  Ho, Wo = wgrad_out_hw(c)
  return c.N * Ho * Wo


def wgrad_case_inputs(c, exact):
  """Seeded float32 x [G][N][H][W][Cin] and dz [G][N][Ho][Wo][Cout].  exact: integers in [-2, 2] -- every product and every
  partial sum of at most M of them is an integer of magnitude <= 4 M < 2**24, which float32 holds exactly, so any order of
  float32 additions, through any MFMA, slab split or slab-sum order, gives exactly the float64 result.  Otherwise N(0, 1)."""
  r = np.random.default_rng(2000 + 2 * c.index + (1 if exact else 0))
  Ho, Wo = wgrad_out_hw(c)
  sx, sz = (c.G, c.N, c.H, c.W, c.Cin), (c.G, c.N, Ho, Wo, c.Cout)
  if exact:
    assert 4 * wgrad_pixels(c) < 2 ** 24
    return r.integers(-2, 3, sx).astype(np.float32), r.integers(-2, 3, sz).astype(np.float32)
  return r.standard_normal(sx).astype(np.float32), r.standard_normal(sz).astype(np.float32)


def wgrad_case_expect(c, exact):
  """(x, dz, dw, db, bound_dw, bound_db): the inputs and, per group, the float64 gradients and their bounds (zero in the exact
  pass: the comparison is equality)."""
  x, dz = wgrad_case_inputs(c, exact)
  out = [conv_wgrad_ref(x[g], dz[g], c.stride) for g in range(c.G)]
  dw, db, mw, mb = (np.stack([o[i] for o in out]) for i in range(4))
  if exact:
    return x, dz, dw, db, np.zeros_like(dw), np.zeros_like(db)
  return x, dz, dw, db, wgrad_bound(mw, c.slice_px, c.S), wgrad_bound(mb, c.slice_px, c.S)


# --------------------------------------------------------------------------------------------------------------------------
# LDS-halo and LDS-staged forwards and input gradients: case list, sign-field packers, seeded inputs, expectations
# --------------------------------------------------------------------------------------------------------------------------
HALO_CASES_TXT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'native', 'conv_halo_cases.txt')

HaloCase = collections.namedtuple('HaloCase', 'index dir G N H W Cin Cout stride flags reserved text plan family inst items blocks '
                                  'rounds cross empty')
_HALO_PLAN = re.compile(r'^(lds|halo|conv1) (.+) items=(\d+) blocks=(\d+) rounds=(\d+) cross=(\S+) empty=(\d+)$')
_HALO_FLAGS = {'dgrad': {'mask', 'fields', 'hostonly'}, 'fwd': {'relu', 'bias', 'fields', 'bits', 'rgb', 'hostonly'}}


def load_halo_cases(device_only=False):
  """The cases of tests/native/conv_halo_cases.txt with the plan recorded beside each (tests/test_conv_halo_cover_cpu.py holds that
  text against what geeco_amd/csrc/conv_halo_plan.h gives).  device_only: without the lines the cover alone holds."""
  cases = []
  for line in open(HALO_CASES_TXT):
    line = line.strip()
    if not line or line.startswith('#'):
      continue
    text, plan = (s.strip() for s in line.split('|'))
    f = text.split()
    flags = frozenset(t for t in f[8:] if not t.startswith('reserved='))
    reserved = [int(t.split('=')[1]) for t in f[8:] if t.startswith('reserved=')]
    assert f[0] in _HALO_FLAGS and flags <= _HALO_FLAGS[f[0]] and len(reserved) <= 1 and not {'fields', 'mask'} <= flags, line
    m = _HALO_PLAN.match(plan)
    assert m or plan == 'gemm', line
    fam = (m.group(1), m.group(2), int(m.group(3)), int(m.group(4)), int(m.group(5)), frozenset(m.group(6).split('+')) - {'none'},
           int(m.group(7))) if m else ('gemm', '', 0, 0, 0, frozenset(), 0)
    c = HaloCase(len(cases), f[0], *(int(v) for v in f[1:8]), flags, reserved[0] if reserved else 0, text, plan, *fam)
    assert (c.family == 'gemm') <= ('hostonly' in flags), line      # a declined shape is the gather GEMM's: not a case of the device list
    cases.append(c)
  return [c for c in cases if not (device_only and 'hostonly' in c.flags)]


def halo_form(c):
  """The mask form of a case: none / mask / fields for a gradient, plain / fields / bits for a forward."""
  if c.dir == 'dgrad':
    return 'fields' if 'fields' in c.flags else 'mask' if 'mask' in c.flags else 'none'
  return 'fields' if 'fields' in c.flags else 'bits' if 'bits' in c.flags else 'plain'


def halo_key(c):
  """The key tests/native/conv_halo_cover.cpp prints for the sweep's launches."""
  return '%s %s %s %s' % (c.family, c.inst, 'several' if c.rounds > 1 else 'one', halo_form(c))


def halo_out_hw(c):
  return same_pad(c.H, c.stride)[0], same_pad(c.W, c.stride)[0]


def halo_terms(c):
  """Products per output element: forward 9 Cin (27 through the RGB kernel variable: the pad channel has no kernel rows); input
  gradient: dgrad_terms."""
  if c.dir == 'fwd':
    return 27.0 if 'rgb' in c.flags else 9.0 * c.Cin
  return dgrad_terms((c.H, c.W), c.stride, c.Cout)


# ---- sign fields and words, packed from the definitions in include/geeco_hip.h ---------------------------------------------
def pack_fields16(pos):
  """pos [..., C] bool, C = 16 n <= 64 -> uint16 [..., 4]: field q, bit 4 i + j set iff channel 16 i + 4 q + j is positive."""
  C = pos.shape[-1]
  assert C % 16 == 0 and C <= 64
  out = np.zeros(pos.shape[:-1] + (4,), np.uint16)
  for ch in range(C):
    i, q, j = ch // 16, (ch % 16) // 4, ch % 4
    out[..., q] |= pos[..., ch].astype(np.uint16) << np.uint16(4 * i + j)
  return out


def pack_fields8(pos):
  """pos [..., C] bool, C = 32 n -> uint8 [..., C / 8]: byte (T >> 1) * 4 + q, bit 4 (T & 1) + j set iff channel 16 T + 4 q + j is
  positive (T = 16-channel tile, q = channel quad inside it)."""
  C = pos.shape[-1]
  assert C % 32 == 0
  out = np.zeros(pos.shape[:-1] + (C // 8,), np.uint8)
  for ch in range(C):
    T, q, j = ch // 16, (ch % 16) // 4, ch % 4
    out[..., (T >> 1) * 4 + q] |= pos[..., ch].astype(np.uint8) << np.uint8(4 * (T & 1) + j)
  return out


def pack_bits32(pos):
  """pos [..., 32] bool -> uint32 [...]: bit (c & 3) * 8 + (c >> 2) set iff channel c is positive (conv1's ReLU sign words)."""
  assert pos.shape[-1] == 32
  out = np.zeros(pos.shape[:-1], np.uint32)
  for ch in range(32):
    out |= pos[..., ch].astype(np.uint32) << np.uint32((ch & 3) * 8 + (ch >> 2))
  return out


def pad_planes(a, Hp, Wp, fill):
  """a [G][N][H][W][...] -> [G][N][Hp][Wp][...] with ``fill`` outside the image (the padded planes of the uint16 fields and of
  conv1's words: whole 8 x 64 tiles)."""
  out = np.full(a.shape[:2] + (Hp, Wp) + a.shape[4:], fill, a.dtype)
  out[:, :, :a.shape[2], :a.shape[3]] = a
  return out


def tiles_8x64(H, W):
  return (H + 7) // 8 * 8, (W + 63) // 64 * 64


# ---- seeded inputs and the float64 expectation -----------------------------------------------------------------------------
def _halo_shape_key(c):
  return (c.dir, c.G, c.N, c.H, c.W, c.Cin, c.Cout, c.stride, 'rgb' in c.flags)


def _halo_seed(key, exact):
  return [3000 + (1 if exact else 0)] + [int(v) for v in key[1:]] + [0 if key[0] == 'fwd' else 1]


@functools.lru_cache(maxsize=1)
def _halo_shape_expect(key, exact):
  """Inputs, pre and mag of a shape: shared by the cases of the list that differ only in their mask form (one is kept: the
  largest holds some hundred megabytes in float64).  Callers leave the arrays unchanged."""
  d, G, N, H, W, Cin, Cout, s, rgb = key
  r = np.random.default_rng(_halo_seed(key, exact))
  Ho, Wo = same_pad(H, s)[0], same_pad(W, s)[0]
  f = lambda a: a.astype(np.float32)
  ints = lambda lo, hi, shape: f(r.integers(lo, hi + 1, shape))
  if d == 'fwd':
    wc = 3 if rgb else Cin
    if exact:
      x, w, b = ints(-2, 2, (G, N, H, W, Cin)), ints(-2, 2, (G, 3, 3, wc, Cout)), ints(-3, 3, (G, Cout))
    else:
      x = f(r.standard_normal((G, N, H, W, Cin)))
      w = f(r.standard_normal((G, 3, 3, wc, Cout)) / math.sqrt(9 * wc))
      b = f(np.sign(r.standard_normal((G, Cout))) * r.uniform(2.0, 4.0, (G, Cout)))
    out = [conv_fwd_ref(x[g][..., :wc], w[g], b[g], s, False) for g in range(G)]
    inp = dict(x=x, w=w, b=b)
  else:
    if exact:
      dz, w = ints(-2, 2, (G, N, Ho, Wo, Cout)), ints(-2, 2, (G, 3, 3, Cin, Cout))
      mask = ints(-1, 1, (G, N, H, W, Cin))
    else:
      dz = f(r.standard_normal((G, N, Ho, Wo, Cout)))
      w = f(r.standard_normal((G, 3, 3, Cin, Cout)) / math.sqrt(9 * Cout))
      mask = r.standard_normal((G, N, H, W, Cin), dtype=np.float32)
      mask[r.random(mask.shape, dtype=np.float32) < 0.3] = 0.0
    out = [conv_dgrad_ref(dz[g], w[g], (H, W), s, None) for g in range(G)]
    inp = dict(dz=dz, w=w, mask=mask)
  pre, mag = np.stack([o[2] for o in out]), np.stack([o[1] for o in out])
  for a in (pre, mag):      # (the operands go to torch.from_numpy, which wants them writable: the device test checks them unchanged)
    a.setflags(write=False)
  return inp, pre, mag


def halo_case_expect(c, exact):
  """-> (inputs, ref, bound, keep) of a case, the last three [G][...].
  exact: integers (operands in [-2, 2], bias in [-3, 3], mask in {-1, 0, 1}): every partial sum is an integer of magnitude at most
  16 Cout + 3 (gradient: at most four taps reach a pixel) or 36 Cin + 3 (forward), far below 2**24, so float32 in any order gives the
  float64 result: bound 0 everywhere, nothing left out.
  Otherwise case_inputs' distributions under conv_bound(mag, halo_terms, S = 1).
  The gradient's inputs always hold the float mask; the case's form decides what the launch is given (halo_form)."""
  inp, pre, mag = _halo_shape_expect(_halo_shape_key(c), bool(exact))
  if c.dir == 'fwd':
    relu = 'relu' in c.flags
    if exact:
      ref = np.maximum(pre, 0.0) if relu else pre
      return inp, ref, np.zeros_like(ref), np.ones(ref.shape, bool)
    return (inp,) + conv_expect(pre, mag, halo_terms(c), 1, relu=relu)
  mask = inp['mask'] if halo_form(c) != 'none' else None
  if exact:
    ref = pre if mask is None else np.where(mask > 0, pre, 0.0)
    return inp, ref, np.zeros_like(ref), np.ones(ref.shape, bool)
  return (inp,) + conv_expect(pre, mag, halo_terms(c)[None, None], 1, mask=mask)


def halo_compare(c, exact, got, inp, ref, bound, keep):
  """The comparisons of one pass of tests/test_conv_halo_variants_gpu.py on an output ``got`` [G][...] float32 -> (worst share of
  the rounding bound, problems): what the device test asserts empty and tests/test_conv_halo_refs_cpu.py holds against emulated
  kernels with one mistake each.
    no NaN; exact pass: equality with the float64 result; rounding pass: assert_within's test, and equality where the bound is 0
    (cut by the ReLU, masked off); a masked gradient: the elements masked off are +0.0 bit for bit."""
  problems, worst = [], 0.0
  if np.isnan(got).any():
    problems.append('NaN in %d elements' % int(np.isnan(got).sum()))
  g64 = got.astype(np.float64)
  if exact:
    bad = ~(g64 == ref)
    if bad.any():
      problems.append('exact: %d of %d elements differ from the float64 result, the first at %s' % (
          int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0])))
  else:
    err = np.abs(g64 - ref)
    bad = ~(err <= bound) & keep
    live = keep & (bound > 0)
    if live.any():
      with np.errstate(invalid='ignore'):
        worst = float(np.nanmax(err[live] / bound[live]))
    if bad.any():
      at = tuple(np.argwhere(bad)[0])
      problems.append('rounding: %d of %d elements out of bound, the first at %s: got %.9g, reference %.9g (bound %.3e)' % (
          int(bad.sum()), bad.size, at, got[at], ref[at], bound[at]))
  if c.dir == 'dgrad' and halo_form(c) != 'none':
    off = ~(inp['mask'] > 0)
    n = int(np.count_nonzero(np.ascontiguousarray(got).view(np.uint32)[off]))
    if n:
      problems.append('bits: %d masked elements are not +0.0' % n)
  return worst, problems


# --------------------------------------------------------------------------------------------------------------------------
# fused encoder-bottom backward (conv2_dgrad_conv1_wgrad_kernel<CREAL, BITS>): case list, reference, seeded inputs, bounds
# --------------------------------------------------------------------------------------------------------------------------
BOTTOM_CASES_TXT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'native', 'conv_bottom_cases.txt')

BottomCase = collections.namedtuple('BottomCase', 'index G N H W C flags reserved text plan inst tiles blocks S per slice_px remainder '
                                    'cross empty')
_BOTTOM_PLAN = re.compile(r'^(conv2_dgrad_conv1_wgrad_kernel<([34]), (true|false)>) tiles=(\d+) blocks=(\d+) S=(\d+) per=(\d+) '
                          r'slice_px=(\d+) (remainder|regular) cross=(\S+) empty=(\d+)$')
_BOTTOM_FLAGS = {'mask', 'bits', 'dz1', 'pending'}


def load_bottom_cases():
  """The cases of tests/native/conv_bottom_cases.txt with the plan recorded beside each (tests/test_conv_bottom_cover_cpu.py holds
  that text against what fused_bottom_launch_plan of geeco_amd/csrc/conv_wgrad_plan.h gives)."""
  cases = []
  for line in open(BOTTOM_CASES_TXT):
    line = line.strip()
    if not line or line.startswith('#'):
      continue
    text, plan = (s.strip() for s in line.split('|'))
    f = text.split()
    flags = frozenset(t for t in f[5:] if not t.startswith('reserved='))
    reserved = [int(t.split('=')[1]) for t in f[5:] if t.startswith('reserved=')]
    m = _BOTTOM_PLAN.match(plan)
    assert m and flags <= _BOTTOM_FLAGS and len(reserved) <= 1, line
    c = BottomCase(len(cases), *(int(v) for v in f[:5]), flags, reserved[0] if reserved else 0, text, plan, m.group(1),
                   *(int(m.group(i)) for i in range(4, 9)), m.group(9) == 'remainder', frozenset(m.group(10).split('+')) - {'none'},
                   int(m.group(11)))
    # one mask form, and it is the instantiation's; dz1 is stored by the float-mask forms only; reserved CUs need the deferred form
    assert ('mask' in flags) != ('bits' in flags) and ('bits' in flags) == (m.group(3) == 'true') and int(m.group(2)) == c.C, line
    assert not {'dz1', 'bits'} <= flags and (not c.reserved or 'pending' in flags), line
    cases.append(c)
  return cases


def bottom_key(c):
  """The key tests/native/conv_bottom_cover.cpp prints for the sweep's launches."""
  return '%s %s cross=%s' % ('bits' if 'bits' in c.flags else 'mask', 'remainder' if c.remainder else 'regular',
                             '+'.join(k for k in ('frame', 'enc') if k in c.cross) or 'none')


def bottom_kernel_names(c):
  """What ops.kernel_trace records for the entry point: the instantiation and the slab sum (85 or more slabs of 1184 floats: the
  split form), unless that is deferred -- ops.slab_reduce_batch then launches wgrad_reduce_batch_kernel."""
  return [c.inst] + ([] if 'pending' in c.flags else ['wgrad_reduce_kernel<true>'])


def bottom_pixels(c):
  return c.N * c.H * c.W


def bottom_ranges(c):
  """[(encoder, slab, first tile, end tile)] of every block (the remainder block: one entry per encoder), from the recorded plan:
  regular block b of S0 = S - remainder per encoder walks [b per, min(b per + per, tiles)), the remainder block [S0 per, tiles)
  of every encoder into slab S0."""
  S0 = c.S - (1 if c.remainder else 0)
  out = [(g, b, b * c.per, max(b * c.per, min(b * c.per + c.per, c.tiles))) for g in range(c.G) for b in range(S0)]
  if c.remainder:
    out += [(g, S0, S0 * c.per, c.tiles) for g in range(c.G)]
  return out


BOTTOM_EXACT_MAX = 4 * 48 * 2      # |dz1| in the exact pass: at most 4 taps reach a pixel, 48 channels, |dz2| <= 2, |w2| <= 1


def bottom_slab_bound(mag, slice_px, S):
  """wgrad_bound with the fused kernel's block reduction: its eight waves each keep partial tiles of the block's slice and are
  summed through LDS in seven additions where wgrad_bound allows three -> (slice_px + S + 12) U mag.  The second-order terms,
  n^2 U^2 at n = 6144 + 43 + 7, the longest chain of the case list, are 2.3 U: inside the 5 U wgrad_bound keeps for them."""
  return wgrad_bound(mag, slice_px, S) + 4.0 * U * mag


def _bottom_shape_key(c):
  return (c.G, c.N, c.H, c.W, c.C)


@functools.lru_cache(maxsize=2)
def _bottom_shape_expect(key, exact):
  """Inputs and the float64 results of a shape, shared by the cases that differ in mask form, entry point or CUs.
  x [G][N][H][W][4] (C = 3: the pad channel holds data too -- it has no column in dw1 and must not reach it), w2 [G][3][3][32][48],
  dz2 [G][N][H/2][W/2][48], mask [G][N][H][W][32]: about half of it is not > 0, with exact zeros and negative values.
    exact: x, w2, mask in {-1, 0, 1} (mask: a quarter -1, a quarter 0), dz2 integers in [-2, 2];  otherwise N(0, 1), a tenth of
    the mask set to exactly 0.
  Per encoder, from the definitions (conv2: stride 2, conv1: stride 1, TF SAME):
    dz1 = on * conv2_dgrad(dz2, w2), on = mask > 0 (data, not a computed sign);
    dw1[tap][c][co] = sum_p x[p + tap][c] dz1[p][co] over the C real channels;   db1 = sum_p dz1[p].
  e1: dz1's own rounding bound, conv_bound(mag, taps * 48, S = 1) where the mask is on and 0 where it is off (exact: 0);
  ew, eb: what e1 can move dw1 / db1 by, sum_p |x| e1;  mw, mb: the magnitudes sum_p |x| (|dz1| + e1) of the filter gradient's terms.
  Callers leave the arrays unchanged."""
  G, N, H, W, C = key
  r = np.random.default_rng([4000 + (1 if exact else 0), G, N, H, W, C])
  f = lambda a: a.astype(np.float32)
  sx, sw, sz, sm = (G, N, H, W, 4), (G, 3, 3, 32, 48), (G, N, H // 2, W // 2, 48), (G, N, H, W, 32)
  if exact:
    x, w2, dz2 = f(r.integers(-1, 2, sx)), f(r.integers(-1, 2, sw)), f(r.integers(-2, 3, sz))
    mask = f(r.choice(np.array([-1, 0, 1, 1]), sm))
  else:
    x, w2, dz2 = f(r.standard_normal(sx)), f(r.standard_normal(sw)), f(r.standard_normal(sz))
    mask = r.standard_normal(sm, dtype=np.float32)
    mask[r.random(sm, dtype=np.float32) < 0.1] = 0.0
  on = mask > 0
  out = collections.defaultdict(list)
  terms = dgrad_terms((H, W), 2, 48)[None]
  for g in range(G):
    z64, w64 = dz2[g].astype(np.float64), w2[g].astype(np.float64)
    pre = _dgrad(z64, w64, (H, W), 2)
    dz1 = np.where(on[g], pre, 0.0)
    e1 = np.zeros_like(dz1) if exact else np.where(on[g], conv_bound(_dgrad(np.abs(z64), np.abs(w64), (H, W), 2), terms, 1), 0.0)
    xr = x[g][..., :C].astype(np.float64)
    dw, db = _wgrad(xr, dz1, 1)
    ew, eb = _wgrad(np.abs(xr), e1, 1)
    eb = e1.reshape(-1, 32).sum(0)
    mw, _ = _wgrad(np.abs(xr), np.abs(dz1) + e1, 1)
    mb = (np.abs(dz1) + e1).reshape(-1, 32).sum(0)
    for k, v in dict(dz1=dz1, e1=e1, dw=dw, db=db, ew=ew, eb=eb, mw=mw, mb=mb).items():
      out[k].append(v)
  res = {k: np.stack(v) for k, v in out.items()}
  for a in res.values():      # (the operands go to torch.from_numpy, which wants them writable: the device test checks them unchanged)
    a.setflags(write=False)
  res.update(x=x, w2=w2, dz2=dz2, mask=mask)
  return res


def bottom_case_expect(c, exact):
  """-> dict: the inputs (x, w2, dz2, mask), the float64 results (dw [G][3][3][C][32], db [G][32], dz1 [G][N][H][W][32]) and their
  bounds (bw, bb, e1).
  exact: every dz1 is an integer of magnitude <= 384 and every partial sum of dw1 / db1 an integer of magnitude <= 384 N H W < 2**24
  (asserted), which float32 holds exactly, so any order of float32 additions through any MFMA, tile walk, LDS reduction or slab
  sum gives the float64 result: all bounds are 0 and the comparison is equality.
  Otherwise dz1 is held under e1, and dw1 under
      sum_p |x| e1  +  bottom_slab_bound(sum_p |x| (|dz1| + e1), slice_px, S)
  -- the filter gradient of the float64 dz1 moved by dz1's own error, plus the rounding of a float32 filter gradient whose terms
  are at most |x| (|dz1| + e1), in S slabs of at most slice_px pixels (the case's recorded plan) -- and db1 under the same with
  |x| = 1.  No element is left out: where the mask is off, dz1 is 0 with bound 0."""
  e = dict(_bottom_shape_expect(_bottom_shape_key(c), bool(exact)))
  if exact:
    assert BOTTOM_EXACT_MAX * bottom_pixels(c) < 2 ** 24, c.text
    e['bw'], e['bb'] = np.zeros_like(e['dw']), np.zeros_like(e['db'])
  else:
    e['bw'] = e['ew'] + bottom_slab_bound(e['mw'], c.slice_px, c.S)
    e['bb'] = e['eb'] + bottom_slab_bound(e['mb'], c.slice_px, c.S)
  return e


def bottom_bits_planes(c, mask):
  """The signs of ``mask`` [G][N][H][W][32] as the sign-word entry point wants them, packed on the host: uint32 [G][N][Hp][Wp],
  whole 8 x 64 tiles, zero outside the image (the entry point's contract)."""
  return pad_planes(pack_bits32(np.asarray(mask) > 0), *tiles_8x64(c.H, c.W), np.uint32(0))


def bottom_compare(c, exact, got, e):
  """The comparisons of one pass of tests/test_conv_bottom_variants_gpu.py on ``got`` = dict(dw, db[, dz1]) float32 [G][...] against
  bottom_case_expect's ``e`` -> (worst share of a rounding bound per output, problems): what the device test asserts empty and
  tests/test_conv_bottom_refs_cpu.py holds against emulated kernels with one mistake each.  Every element of every output is
  compared: none is NaN, exact pass: equality with the float64 result; rounding pass: within its bound (0 where the mask is off)."""
  problems, worst = [], {}
  for name, ref, bound in (('dw', e['dw'], e['bw']), ('db', e['db'], e['bb']), ('dz1', e['dz1'], e['e1'])):
    if name not in got:
      continue
    worst[name] = 0.0
    g64 = np.asarray(got[name]).astype(np.float64)
    assert g64.shape == ref.shape == bound.shape and np.isfinite(bound).all(), (name, g64.shape, ref.shape)
    if np.isnan(g64).any():
      problems.append('nan %s: %d elements' % (name, int(np.isnan(g64).sum())))
    if exact:
      bad = ~(g64 == ref)
      if bad.any():
        at = tuple(np.argwhere(bad)[0])
        problems.append('exact %s: %d of %d elements differ from the float64 result, the first at %s: got %.9g, reference %.9g' % (
            name, int(bad.sum()), bad.size, at, g64[at], ref[at]))
    else:
      err = np.abs(g64 - ref)
      bad = ~(err <= bound)
      live = bound > 0
      ratio = err[live] / bound[live]
      ratio = ratio[~np.isnan(ratio)]
      if ratio.size:
        worst[name] = float(ratio.max())
      if bad.any():
        at = tuple(np.argwhere(bad)[0])
        problems.append('rounding %s: %d of %d elements out of bound, the first at %s: got %.9g, reference %.9g (bound %.3e)' % (
            name, int(bad.sum()), bad.size, at, g64[at], ref[at], bound[at]))
  return worst, problems
