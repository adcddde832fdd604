"""Every instantiation and launch form of the predictor I/O kernels (csrc/predict_io.hip) -- the frame range check, the dense and
ring window pushes, the newest-frame pack, the feature push and the output pack -- against the host models of _predict_io_ref,
bit for bit: these kernels move values or decide, none of them rounds, so no case has a tolerance.

tests/test_batched_predictor_gpu.py and tests/test_incremental_predictor_gpu.py hold this code at 8x12, 6x10 and 5x5 frames (one
block of pixels), J = 7, B <= 32, aligned bases, finite untied logits and two out-of-range values.  The case tables below add
what those shapes cannot reach: a second, ragged block in every grid; the grid-stride loop of the range check past its first
pass and under its 64-block cap; the bounds themselves and one ulp outside, -0.0 and the infinities; the depth exemption of both
range-check forms; the one-pixel / one-float / 4-byte instances chosen by a base one element off a 16-byte boundary (a supported
path); the uint8 one-pixel push; K = 1 and K = PIO_MAXK; J = 257; the ring's advance kernel at B = 65; feature heads outside
0..K-1; every loop of the feature push past 1024 units; np.argmax's rule on ties, signed zeros, infinities and NaN; the control
words once B + 1 leaves one block; the image slots.  The tables are plain data: tests/test_predict_io_ref_cpu.py imports them
and shows that the instance names they expect are exactly the instantiations predict_io.hip launches.

Each case: every tensor a kernel writes is a view inside a larger allocation poisoned with NaN (integers: bytes 0xA5), MARGIN
elements (more than any block of these kernels covers) on both sides; the margins hold their bits afterwards; the inputs of the
misaligned cases sit in such allocations too, so a read past a frame meets NaN; ops.kernel_trace names exactly the instance the
case is there for; with the any-env word set, a push leaves every bit of its state alone.

On an MI355X all 79 cases pass and the file takes 3 s.  One-line changes of predict_io.hip tried against it, each caught: `v >= bv`
in the argmax and the argmax loop without its stop at a NaN (test_pack), `b < B` in the control-word copy (test_pack), the image
slot never advanced (test_pack, both images), `i % C < 4` in the scalar range check (scalar-c4-by-alignment), v.w checked for
C == 4 (depth-exempt), `v.w < hi` and `v.z > lo` for C == 3 (the three float4 RGB cases), push_jnt without its second pass (the
J = 257 dense cases), one block of ring_advance_kernel and no mirror store (test_push_ring), x * (1 / 255) in the uint8 one-pixel
load (the pix1 u8 cases of the dense push and the newest-frame pack), an out-of-range head sent to K - 1 (test_push_features).
"""
import os
import re

import numpy as np
import pytest
import torch

import _predict_io_ref as R
from _predict_io_ref import WindowModel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _define(rel, name):
  return int(re.search(r'#define %s (\d+)' % name, open(os.path.join(ROOT, rel)).read()).group(1))


PIO_MAXK = _define('geeco_amd/csrc/dynimg_internal.h', 'DYN_MAXK')      # predict_io.hip: #define PIO_MAXK DYN_MAXK
MAXSEG = _define('include/geeco_hip.h', 'GEECO_PREDICT_PACK_MAXSEG')
MARGIN = 4096      # elements of poison on each side of a view: the widest block here covers 1024 threads x 4 floats (16-byte steps)


# ---- the case tables (plain data) -----------------------------------------------------------------------------------------------
def _tf(b):
  return 'true' if b else 'false'


# off = 1: the frames start one float (4 bytes) behind a 16-byte boundary; B: envs per launch (None: every env in one launch)
RANGE_CASES = [
    dict(id='one-block-three-float4', HW=4, C=3, off=0, B=None, names=('range_check_kernel<3>',)),
    dict(id='two-blocks-ragged-three-passes', HW=1368, C=3, off=0, B=None, names=('range_check_kernel<3>',)),
    dict(id='64-block-cap', HW=296 * 296, C=3, off=0, B=2, names=('range_check_kernel<3>',)),
    dict(id='depth-exempt', HW=8 * 12, C=4, off=0, B=None, names=('range_check_kernel<4>',)),
    dict(id='scalar-c3', HW=5 * 5, C=3, off=0, B=None, names=('range_check_scalar_kernel<3>',)),
    dict(id='scalar-c3-by-alignment', HW=8 * 12, C=3, off=1, B=None, names=('range_check_scalar_kernel<3>',)),
    dict(id='scalar-c4-by-alignment', HW=8 * 12, C=4, off=1, B=None, names=('range_check_scalar_kernel<4>',)),
]

FRAME_KINDS = ((3, False), (4, False), (3, True))      # (C, uint8 frames)


def _dense_cases():
  cases = []
  # HW = 1028: 257 four-pixel units, a second pixel block with one live thread; HW = 257: the same for the one-pixel instances
  for pix, HW in ((4, 1028), (1, 257)):
    for C, u8 in FRAME_KINDS:
      for K in (1, 2, PIO_MAXK):
        cases.append(dict(id='pix%d-c%d-%s-K%d' % (pix, C, 'u8' if u8 else 'f32', K), HW=HW, C=C, u8=u8, K=K,
                          J=257 if K == 2 else 7, off=None, names=('push_dense_kernel<%d, %d, %s>' % (pix, C, _tf(u8)),)))
  # HW % 4 == 0, one pixel per thread only because a base is one element off
  for C, u8 in FRAME_KINDS:
    cases.append(dict(id='pix1-c%d-%s-frames-off' % (C, 'u8' if u8 else 'f32'), HW=96, C=C, u8=u8, K=2, J=7, off='frames',
                      names=('push_dense_kernel<1, %d, %s>' % (C, _tf(u8)),)))
  cases.append(dict(id='pix1-c3-f32-rgb-off', HW=96, C=3, u8=False, K=2, J=7, off='rgb', names=('push_dense_kernel<1, 3, false>',)))
  return cases


DENSE_CASES = _dense_cases()

# HW = 1376: 4128 bytes = 258 16-byte units; HW = 344: 1032 bytes, no multiple of 16, 258 words; HW = 16: 48 bytes, the ring 4 bytes off
RING_CASES = [dict(id='%s-HW%d-K%d' % (v, HW, K), HW=HW, K=K, off=off, names=('push_ring_kernel<%s>' % v, 'ring_advance_kernel'))
              for v, HW, off in (('u32x4', 1376, 0), ('unsigned', 344, 0), ('unsigned', 16, 4)) for K in (1, 3)]

NEWEST_CASES = (
    [dict(id='pix%d-c%d-%s' % (pix, C, 'u8' if u8 else 'f32'), HW=HW, C=C, u8=u8, off=0,
          names=('pack_newest_kernel<%d, %d, %s>' % (pix, C, _tf(u8)),))
     for pix, HW in ((4, 1028), (1, 257)) for C, u8 in FRAME_KINDS] +
    [dict(id='pix1-c%d-%s-frames-off' % (C, 'u8' if u8 else 'f32'), HW=96, C=C, u8=u8, off=1,
          names=('pack_newest_kernel<1, %d, %s>' % (C, _tf(u8)),)) for C, u8 in FRAME_KINDS])

# ch = 64, K = 3.  cells = 22: the smallest with cells * ch / 4 * K = 1056 > 1024 four-float units, the ring write after a reset
# and the feature gather pass the block twice; cells = 49: K * cells * J = 1029, the joint-state gather does too
FEATURE_CASES = [dict(id='%s-%s' % (tag, mode), mode=mode, cells=cells, ch=64, K=3, off=off, names=('push_features_kernel<%d>' % v,))
                 for tag, cells, off, v in (('feat-off', 4, 1, 1), ('cells22', 22, 0, 4), ('cells49', 49, 0, 4))
                 for mode in ('plain', 'constant', 'residual')]

# P = 11 columns.  (src, len, argmax): a copy and an argmax that share column 2, argmax over 1, 3 and 5 logits, copies behind them
PACK_P = 11
SEGS = ((0, 3, 0), (2, 3, 1), (5, 1, 1), (6, 5, 1), (4, 2, 0), (10, 1, 0))
SEGS_MAX = SEGS + ((0, 11, 0), (0, 5, 1))
assert len(SEGS_MAX) == MAXSEG


def _pack_names(imgs):
  return ('pack_preds_kernel',) + ('pack_image_kernel',) * sum(imgs)


PACK_CASES = (
    # B = 255: B + 1 fills one block; 256: the any-env word is all the second block does; 300: envs in the second block too
    [dict(id='B%d-%dseg' % (B, len(segs)), B=B, segs=segs, HW=0, C=0, imgs=(0, 0), names=_pack_names((0, 0)))
     for B in (1, 255, 256, 300) for segs in (SEGS, SEGS_MAX)] +
    [dict(id='img-HW%d-c%d-%d%d' % (HW, C, imgs[0], imgs[1]), B=3, segs=SEGS, HW=HW, C=C, imgs=imgs, names=_pack_names(imgs))
     for HW in (1, 255, 257) for C in (3, 4) for imgs in ((1, 0), (0, 1), (1, 1))])

ALL_CASES = dict(range_check=RANGE_CASES, push_dense=DENSE_CASES, push_ring=RING_CASES, pack_newest=NEWEST_CASES,
                 push_features=FEATURE_CASES, pack=PACK_CASES)


def expected_instances():
  """Every instance name some case expects in its trace."""
  return {n for cases in ALL_CASES.values() for c in cases for n in c['names']}


def _ids(cases):
  return [c['id'] for c in cases]


# ---- inputs (host side; no GPU needed) --------------------------------------------------------------------------------------------
def range_geometry(HW, C, off):
  """(elements one pass of the range check's grid covers, float4 path) for a frame of HW * C floats at float offset ``off``."""
  n = HW * C
  vec = n % 4 == 0 and off % 4 == 0
  unit = 4 if vec else 1
  nblk = min(-(-(n // unit) // 1024), 64)
  return nblk * 256 * unit, vec


def range_positions(HW, C, off):
  """{tag: element} of one env's frame where a bad value has to be seen; channel 3 of an RGB-D frame is never among them."""
  n = HW * C
  per_pass, _ = range_geometry(HW, C, off)
  chk = lambda e: e if e % C < 3 else e - 1          # the checked element at or before e
  pos = {'first': 0, 'last': chk(n - 1)}
  q = 4 * ((n // 4) // 2)                            # the four lanes of one 16-byte unit in the middle of the frame
  for lane in range(4):
    if (q + lane) % C < 3:
      pos['lane%d' % lane] = q + lane
  if per_pass < n:
    pos['pass0-last'] = chk(per_pass - 1)
    pos['pass1-first'] = per_pass
    last = (n - 1) // per_pass * per_pass
    if last > per_pass:
      pos['last-pass-first'] = last                    # a multiple of 256 * 4 (C == 4) or any element (C == 3): a checked one
  return pos


def range_envs(c, lo, hi, seed=0):
  """The envs of a range-check case -> (frames [E][HW * C] float32, must_flag [E] bool, tags).  One planted value per flagged
  env; the controls and the depth envs (C == 4) must stay clean."""
  HW, C = c['HW'], c['C']
  n = HW * C
  r = np.random.default_rng(seed)
  lo32, hi32 = np.float32(lo), np.float32(hi)
  values = {'nan': np.float32(np.nan), '+inf': np.float32(np.inf), '-inf': np.float32(-np.inf),
            'above-hi': np.nextafter(hi32, np.float32(np.inf)), 'below-lo': np.nextafter(lo32, np.float32(-np.inf))}
  pos = range_positions(HW, C, c['off'])
  clean = lambda: r.random(n, dtype=np.float32)
  frames, flag, tags = [], [], []
  if c['B'] is None:
    plants = [(pt, vt) for pt in pos for vt in values]
  else:                                               # a frame of a megabyte: every position once, the values in turn
    plants = [(pt, list(values)[i % len(values)]) for i, pt in enumerate(pos)]
  for pt, vt in plants:
    f = clean()
    f[pos[pt]] = values[vt]
    frames.append(f), flag.append(True), tags.append('%s@%s' % (vt, pt))
  controls = {'all-hi': np.full(n, hi32), 'all-lo': np.full(n, lo32), 'neg-zero': np.full(n, np.float32(-0.0)), 'clean': clean()}
  if C == 4:
    d7 = clean()
    d7[3::4] = 7.0
    dn = clean()
    dn[4 * (HW // 2) + 3] = np.nan
    dl = clean()
    dl[n - 1] = np.inf
    d0 = clean()
    d0[3] = -np.inf
    controls.update({'depth-all-7': d7, 'depth-nan': dn, 'depth-last-inf': dl, 'depth-first-ninf': d0})
  for tag, f in controls.items():
    frames.append(f.astype(np.float32)), flag.append(False), tags.append(tag)
  while c['B'] and len(frames) % c['B']:              # whole launches of B envs
    frames.append(clean()), flag.append(False), tags.append('clean')
  return np.stack(frames), np.array(flag), tags


def argmax_patterns(n):
  """Logit rows of length n that pin np.argmax's rule: ties (the first maximum), -0.0 == +0.0, infinities, and NaN (the first NaN
  wins, whatever follows it)."""
  nan, inf = float('nan'), float('inf')
  if n == 1:
    return [[0.5], [nan], [inf], [-inf], [-0.0]]
  three = [[1, 1, 0], [0, 1, 1], [1, 0, 1], [2, 2, 2], [-0.0, 0.0, -1], [0.0, -0.0, -1], [-1, 0.0, -0.0], [1, inf, inf],
           [-inf, -inf, -inf], [-inf, 0, inf], [inf, -inf, inf], [nan, 5, 1], [1, nan, 5], [1, 5, nan], [0, nan, 9], [nan, nan, 7],
           [3, 2, 1], [1, 3, 2], [1, 2, 3]]
  pad = n - 3
  rows = [[-5.0] * (pad // 2) + p + [-5.0] * (pad - pad // 2) for p in three]
  if pad:
    rows += [[7.0] * n, [-5.0] * (n - 1) + [nan], [-5.0] * (n - 1) + [-5.0]]
  return rows


def pack_rows(B, segs, seed=0):
  """preds [B][PACK_P]: random normals; the leading rows hold, argmax segment after argmax segment, its argmax_patterns."""
  r = np.random.default_rng(seed)
  preds = r.standard_normal((B, PACK_P)).astype(np.float32)
  row = 0
  for src, n, am in segs:
    if not am:
      continue
    for p in argmax_patterns(n):
      if row < B:
        preds[row, src:src + n] = np.array(p, np.float32)
      row += 1
  return preds


# ---- device buffers --------------------------------------------------------------------------------------------------------------
def same_bits(got, want, msg=''):
  got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
  assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape, msg)
  u = {1: np.uint8, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
  np.testing.assert_array_equal(got.view(u), want.view(u), err_msg=msg)


class Buf:
  """A tensor of ``shape`` inside one poisoned allocation, MARGIN + ``off`` elements from its (16-byte aligned) start and MARGIN
  from its end; ``values`` or poison inside."""

  def __init__(self, dev, shape, dtype=torch.float32, off=0, values=None):
    n = int(np.prod(shape))
    self.raw = torch.empty(2 * MARGIN + off + n, dtype=dtype, device=dev)
    assert self.raw.data_ptr() % 16 == 0
    if dtype == torch.float32:
      self.raw.fill_(float('nan'))
    else:
      self.raw.view(torch.uint8).fill_(0xA5)
    self.isz, self.lo, self.n = self.raw.element_size(), MARGIN + off, n
    self.t = self.raw[self.lo:self.lo + n].view(*shape)
    assert self.t.data_ptr() % 16 == (off * self.isz) % 16
    if values is not None:
      v = torch.from_numpy(np.ascontiguousarray(values))
      assert v.dtype == dtype and tuple(v.shape) == tuple(shape), (v.dtype, dtype, v.shape, shape)
      self.t.copy_(v)
    self.before = self.bytes().clone()

  def bytes(self):
    return self.raw.view(torch.uint8)

  def margins_intact(self):
    b, a, z = self.bytes(), self.lo * self.isz, (self.lo + self.n) * self.isz
    return torch.equal(b[:a], self.before[:a]) and torch.equal(b[z:], self.before[z:])

  def mark(self):
    """Remembers the bits held now; unchanged() compares against them."""
    self.marked = self.bytes().clone()

  def unchanged(self):
    return torch.equal(self.bytes(), self.marked)

  def numpy(self):
    return self.t.cpu().numpy()


def _i32(dev, a):
  return torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)


# ---- 1. range check --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', RANGE_CASES, ids=_ids(RANGE_CASES))
def test_range_check(dev, c):
  """ctl equals range_flags over envs with one planted value each (first and last element, the lanes of a 16-byte unit, both sides
  of the grid's first pass, the start of its last; NaN, the infinities, one ulp outside each bound) and over envs that must stay
  clean (all-hi, all-lo, -0.0, in-range noise, any depth); a word set before the launch stays set."""
  from geeco_amd import ops
  from geeco_amd.batched_predictor import range_bounds
  lo, hi = range_bounds()
  HW, C = c['HW'], c['C']
  frames, must, tags = range_envs(c, lo, hi)
  per = c['B'] or len(frames)
  assert len(frames) % per == 0
  for e0 in range(0, len(frames), per):
    f, m, tg = frames[e0:e0 + per], must[e0:e0 + per], tags[e0:e0 + per]
    B = len(f)
    prev = np.zeros(B + 1, np.int32)
    if 'clean' in tg:                                    # the in-range noise env (not a control at a bound: its word must be
      prev[tg.index('clean')] = 1                        # earned): set by an earlier check, never cleared
    want = R.range_flags(f.reshape(B, HW, C), C, lo, hi, ctl=prev)
    assert (want[:B] == (m | (prev[:B] == 1))).all(), tg          # the model flags what was planted and nothing else
    fb = Buf(dev, (B, HW, C), off=c['off'], values=f.reshape(B, HW, C))
    ctl = Buf(dev, (B + 1,), torch.int32, values=prev)
    names = ops.kernel_trace(lambda: ops.predict_range_check_into(ctl.t, fb.t, B, HW, C, lo, hi))
    got = ctl.numpy()
    assert tuple(names) == c['names'], names
    assert got.tolist() == want.tolist(), [(t, int(g), int(w)) for t, g, w in zip(tg + ['any'], got, want) if g != w]
    assert ctl.margins_intact()


# ---- 2. dense push ---------------------------------------------------------------------------------------------------------------
def _frames(r, B, HW, C, u8):
  """(what the kernel is given, the float32 values it stands for)"""
  if u8:
    f = r.integers(0, 256, (B, HW, 3), dtype=np.uint8)
    f.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)         # every byte value
    return f, f.astype(np.float32) / np.float32(255.0)
  f = r.random((B, HW, C), dtype=np.float32)
  return f, f


@pytest.mark.parametrize('c', DENSE_CASES, ids=_ids(DENSE_CASES))
def test_push_dense(dev, c):
  """Twelve calls with random resets (the first resets every env): rgb, depth and the joint window equal WindowModel; a call
  with the any-env word set keeps every bit of the three."""
  from geeco_amd import ops
  B, HW, C, u8, K, J = 3, c['HW'], c['C'], c['u8'], c['K'], c['J']
  r = np.random.default_rng(HW * 100 + K)
  rgb = Buf(dev, (B, K, HW, 3), off=1 if c['off'] == 'rgb' else 0)
  depth = Buf(dev, (B, K, HW)) if C == 4 else None
  jw = Buf(dev, (B, K, J))
  state = [x for x in (rgb, depth, jw) if x is not None]
  wm_rgb, wm_dep, wm_j = WindowModel(B, K, (HW, 3)), WindowModel(B, K, (HW,)), WindowModel(B, K, (J,))
  ctl = torch.zeros(B + 1, dtype=torch.int32, device=dev)
  for call in range(12):
    reset = (r.random(B) < 0.25) | (call == 0)
    f, fval = _frames(r, B, HW, C, u8)
    j = r.standard_normal((B, J)).astype(np.float32)
    fd = Buf(dev, (B, HW, C), torch.uint8 if u8 else torch.float32, off=1 if c['off'] == 'frames' else 0, values=f)
    jd, rd = torch.from_numpy(j).to(dev), _i32(dev, reset)
    push = lambda: ops.predict_push_dense_into(rgb.t, depth.t if depth else None, jw.t, fd.t, jd, rd, ctl, B, K, HW, C, J)
    if call == 6:                                        # a frame failed the range check: nothing moves
      for x in state:
        x.mark()
      ctl[B] = 1
      assert tuple(ops.kernel_trace(push)) == c['names']
      ctl[B] = 0
      torch.cuda.synchronize()
      assert all(x.unchanged() for x in state)
    names = ops.kernel_trace(push)
    assert tuple(names) == c['names'], names
    wm_rgb.push(fval[..., :3], reset)
    wm_j.push(j, reset)
    same_bits(rgb.numpy(), wm_rgb.dense, 'rgb call %d' % call)
    if C == 4:
      wm_dep.push(fval[..., 3], reset)
      same_bits(depth.numpy(), wm_dep.dense, 'depth call %d' % call)
    same_bits(jw.numpy(), wm_j.dense, 'jnt call %d' % call)
    assert all(x.margins_intact() for x in state), call
  assert int(ctl.abs().sum()) == 0


# ---- 3. ring push ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', RING_CASES, ids=_ids(RING_CASES))
def test_push_ring(dev, c):
  """B = 65 (a second block of the advance kernel), eight calls with random resets: the mirrored ring, the heads, the window the
  address table points at and the joint window equal the ring WindowModel; with the any-env word set none of the four changes."""
  from geeco_amd import ops
  B, HW, K, J = 65, c['HW'], c['K'], 7
  FB = HW * 3
  r = np.random.default_rng(HW + K)
  ring = Buf(dev, (B, 2 * K, FB), torch.uint8, off=c['off'])
  heads = Buf(dev, (B,), torch.int32, values=np.zeros(B, np.int32))
  table = Buf(dev, (B,), torch.int64)
  jw = Buf(dev, (B, K, J))
  state = (ring, heads, table, jw)
  wm, wm_j = WindowModel(B, K, (FB,), np.uint8), WindowModel(B, K, (J,))
  ctl = torch.zeros(B + 1, dtype=torch.int32, device=dev)
  base = ring.t.data_ptr()
  for call in range(8):
    reset = (r.random(B) < 0.25) | (call == 0)
    f = r.integers(0, 256, (B, FB), dtype=np.uint8)
    j = r.standard_normal((B, J)).astype(np.float32)
    fd, jd, rd = torch.from_numpy(f).to(dev), torch.from_numpy(j).to(dev), _i32(dev, reset)
    assert fd.data_ptr() % 16 == 0
    push = lambda: ops.predict_push_ring_into(ring.t, heads.t, table.t, jw.t, fd, jd, rd, ctl, B, K, HW, J)
    if call == 4:
      for x in state:
        x.mark()
      ctl[B] = 1
      assert tuple(ops.kernel_trace(push)) == c['names']
      ctl[B] = 0
      torch.cuda.synchronize()
      assert all(x.unchanged() for x in state)
    names = ops.kernel_trace(push)
    assert tuple(names) == c['names'], names
    wm.push(f, reset)
    wm_j.push(j, reset)
    rb, tb = ring.numpy(), table.numpy()
    same_bits(heads.numpy(), wm.heads.astype(np.int32), 'heads call %d' % call)
    same_bits(jw.numpy(), wm_j.dense, 'jnt call %d' % call)
    off = tb - base - np.arange(B, dtype=np.int64) * (2 * K * FB)
    assert (off % FB == 0).all() and (off // FB == wm.start).all(), call
    same_bits(rb, wm.ring, 'ring call %d' % call)       # the first call fills every slot, so the whole ring is the model's
    for b in range(B):
      s = int(off[b] // FB)
      same_bits(rb[b, s:s + K], wm.ring_window(b), 'window env %d call %d' % (b, call))
    assert all(x.margins_intact() for x in state), call


# ---- 3b. newest-frame pack -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', NEWEST_CASES, ids=_ids(NEWEST_CASES))
def test_pack_newest(dev, c):
  from geeco_amd import ops
  B, HW, C, u8 = 3, c['HW'], c['C'], c['u8']
  f, _ = _frames(np.random.default_rng(HW + C), B, HW, C, u8)
  if u8:
    assert len(np.unique(f)) == 256
  fd = Buf(dev, (B, HW, C), torch.uint8 if u8 else torch.float32, off=c['off'], values=f)
  x = Buf(dev, (B, HW, 4))
  names = ops.kernel_trace(lambda: ops.predict_pack_newest_into(x.t, fd.t, B, HW, C))
  assert tuple(names) == c['names'], names
  same_bits(x.numpy(), R.newest_input(f, C))
  assert x.margins_intact()


# ---- 3c. feature push ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', FEATURE_CASES, ids=_ids(FEATURE_CASES))
def test_push_features(dev, c):
  """Eight calls: rings, heads and the gathered states equal FeatureRingModel.  Before the third call two heads are set to K and
  to -1 and no env resets: both behave as 0.  With the any-env word set nothing changes."""
  from geeco_amd import ops
  from test_incremental_predictor_cpu import FeatureRingModel
  mode, cells, ch, K = c['mode'], c['cells'], c['ch'], c['K']
  B, J = 3, 7
  r = np.random.default_rng(cells * 10 + len(mode))
  rm = FeatureRingModel(B, K, cells, ch, J, mode)
  D = cells * rm.Ctot
  stride = D + 5                                         # a row pitch wider than the row: the pad keeps its NaN
  states = Buf(dev, (K, B, stride))
  fring = Buf(dev, (B, K, cells, ch))
  jring = Buf(dev, (B, K, J))
  heads = Buf(dev, (B,), torch.int32, values=np.zeros(B, np.int32))
  state = (states, fring, jring, heads)
  ctl = torch.zeros(B + 1, dtype=torch.int32, device=dev)
  tgt = r.standard_normal((B, cells, ch)).astype(np.float32)
  td = Buf(dev, (B, cells, ch), values=tgt).t if mode != 'plain' else None
  for call in range(8):
    reset = (r.random(B) < 0.25) | (call == 0)
    if call == 2:
      reset[:] = False
      heads.t.copy_(_i32(dev, [K, -1, int(rm.heads[2])]))
      rm.heads[:2] = 0
    f = r.standard_normal((B, cells, ch)).astype(np.float32)
    j = r.standard_normal((B, J)).astype(np.float32)
    fd = Buf(dev, (B, cells, ch), off=c['off'], values=f)
    jd, rd = torch.from_numpy(j).to(dev), _i32(dev, reset)
    push = lambda: ops.predict_push_features_into(states.t, fring.t, jring.t, heads.t, fd.t, jd, rd, ctl, mode, B, K, cells, ch, J,
                                                  stride, tgt_feat=td)
    if call == 5:
      for x in state:
        x.mark()
      ctl[B] = 1
      assert tuple(ops.kernel_trace(push)) == c['names']
      ctl[B] = 0
      torch.cuda.synchronize()
      assert all(x.unchanged() for x in state)
    names = ops.kernel_trace(push)
    assert tuple(names) == c['names'], names
    want = np.full((K, B, stride), np.nan, np.float32)
    want[..., :D] = rm.push(f, j, reset, tgt)
    same_bits(states.numpy(), want, 'states call %d' % call)
    same_bits(fring.numpy(), rm.feat, 'ring call %d' % call)
    same_bits(jring.numpy(), rm.jnt, 'jnt ring call %d' % call)
    same_bits(heads.numpy(), rm.heads.astype(np.int32), 'heads call %d' % call)
    assert all(x.margins_intact() for x in state), call


# ---- 4. output pack --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', PACK_CASES, ids=_ids(PACK_CASES))
def test_pack(dev, c):
  """out equals pack_preds over rows that hold ties, signed zeros, infinities and NaN in every argmax segment; ctl_out is the old
  ctl (a random 0/1 pattern with the any-env word set), ctl is zero over exactly B + 1 words; the images land in the slots of the
  ones given, in their order."""
  from geeco_amd import ops
  B, segs, HW, C = c['B'], c['segs'], c['HW'], c['C']
  r = np.random.default_rng(B + HW)
  preds = pack_rows(B, segs)
  F = R.pack_width(segs)
  old = r.integers(0, 2, B + 1).astype(np.int32)
  old[B] = old[B - 1] = 1
  pd = torch.from_numpy(preds).to(dev)
  out = Buf(dev, (B, F))
  ctl = Buf(dev, (B + 1,), torch.int32, values=old)
  ctl_out = Buf(dev, (B + 1,), torch.int32)
  imgs = [r.standard_normal((B, HW, 4)).astype(np.float32) if on else None for on in c['imgs']]
  given = [torch.from_numpy(im).to(dev) if im is not None else None for im in imgs]
  n = sum(c['imgs'])
  img_out = Buf(dev, (n, B, HW, C)) if n else None
  names = ops.kernel_trace(lambda: ops.predict_pack_into(out.t, ctl_out.t, pd, ctl.t, B, segs, imgs=given, HW=HW, C=C,
                                                         img_out=img_out.t if n else None))
  assert tuple(names) == c['names'], names
  same_bits(out.numpy(), R.pack_preds(preds, segs))
  assert ctl_out.numpy().tolist() == old.tolist()
  assert not ctl.numpy().any()
  assert out.margins_intact() and ctl.margins_intact() and ctl_out.margins_intact()
  if n:
    same_bits(img_out.numpy(), R.pack_images(imgs, C))
    assert img_out.margins_intact()
