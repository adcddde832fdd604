"""The input stage (csrc/dynimg.hip, csrc/dynimg_goal.hip) as plain data and plain numpy: the case table of
tests/test_input_stage_variants_gpu.py, the inputs of every case, their float64 reference with a per-element error bound, and a
float32 emulation of the stage (per-block min / max into slots, fold, normalise) that tests/test_input_stage_refs_cpu.py runs
right and wrong.  Nothing here needs a GPU.

Why the inputs are built and not drawn: the rank-pooling weights sum to 0, so D = sum_t alpha_t x_t of random frames has both
signs in every sample and 0 lies strictly inside [min D, max D] -- whatever leaks a zero into the min / max (the pad channel, a
dead lane's accumulators, a fold that starts at 0, an unwritten slot of the zero-filled workspace) changes nothing.  And with a
depth in [0.5, 3] beside an RGB in [0, 1] both extrema always sit in the depth channel.  The recipes:

  pos / neg      every element ramps in time (up / down) and the target lies above / below the current frame: every D of both images
                 has one sign, |D| >= 1 for float32 frames (uint8 frames cannot reach 1 at K = 2, where |D| <= 0.5: there
                 |D| >= 0.12 x range), so a leaked 0 moves the minimum (maximum) by more than a ninth of the range.  The
                 steepest and the flattest ramp sit at named elements.  A target far below the current frame puts the whole window
                 high, and sum |alpha x| -- the bound -- with it: neg stops at K = 6 (bytes, which cannot be scaled: K = 3), longer
                 windows of its turn are pos.
  planted-*      a narrow background (D within a few hundredths of 0) and the sample's min and max of each image planted at ONE
                 named element each, 0.29 x c_K away (c_K = sum alpha_t t / (K - 1) >= 0.5): missing one moves the whole image.
                 -rgb: all four in R, G, B; -depth: all four in the depth; -mix: the buffer image's in the depth, the pair image's
                 in RGB; swap: the elements of min and max change places.
  strided        float32 frames and depth as views with sample / frame strides wider than dense, NaN in every gap.

The named elements are chosen per case from the launch geometry (candidates()): unit 0, the frame's last unit and last float4,
lanes 0 and 63 of waves 1, 2, 3 and 15, the first and the last block of a sample, block 64, slot j = 1 of the two-unit form; the
samples of a case walk through them, so a two-sample block's second sample and the unpaired last sample of an odd count get theirs.

The bound (_norm64).  u = 2^-24, gamma_k = k u / (1 - k u).  The kernel's D^ is K products and K additions in t order, fused or not:
  |D^ - D| <= e := gamma_{K+1} sum_t |alpha_t x_t|          (Higham, Accuracy and Stability, section 3.1; the inputs are exact)
and E := max e over the sample.  min and max select among values each off by <= E: |m^ - m| <= E, |M^ - M| <= E.  The range
r^ = fl(fl(M^ - m^) + c), c = float32(1e-6), against r = M - m + 1e-6:
  |r^ - r| <= Er := 2E + |c - 1e-6| + gamma_2 (r + 2E)
The numerator n^ = fl(D^ - m^) against n = D - m = q r, 0 <= q <= 1:  |n^ - n| <= En := (e + E)(1 + u) + u n.
The IEEE division: q^ = (n^ / r^)(1 + d), |d| <= u, and |n^ / r^ - n / r| <= (En + q Er) / (r - Er), so
  |q^ - q| <= ((En + q Er) / (r - Er)) (1 + u) + u q
The tests compare under min(bound, CAP); the CPU module asserts bound <= CAP for every element of every case."""
import functools
import zlib

import numpy as np

CAP = 5e-6            # what tests/test_kernels_gpu.py::test_goal_dynimgs_one_pass allows
RANGE_FLOOR = 0.25    # float64 max D - min D of every sample of every case (K = 1: the pair image; the buffer image is 0 there)
U32 = 2.0 ** -24
F32 = np.float32


def _tf(b):
  return 'true' if b else 'false'


def alpha(K):
  """The kernel's own float32 weights."""
  from geeco_amd import ops
  return np.array(ops.dynimg_alpha(K), F32)


# ---- launch geometry, restated from goal_onepass_dispatch / geeco_dynimg_fwd ------------------------------------------------------
def cdiv(a, b):
  return -(-a // b)


def geometry(c):
  """What the launcher does with this case: the instances it notes, threads per block, units per thread, blocks per sample, the
  register layout ('flat': float4 number (j * 3 + ch) * T + tid of the block's stretch; 'unit': 4-pixel units), the ring depth."""
  N, HW, Cc = c['N'], c['HW'], c['C']
  U = HW // 4
  if c['entry'] in ('goal', 'goal_u8'):
    depth, u8 = Cc == 4, c['entry'] == 'goal_u8'
    if N * cdiv(U, 2048) >= 192:
      if u8:
        return dict(names=['dynimg_goal_onepass_kernel<%s, true, 1024, 2>' % _tf(depth)], T=1024, UPT=2, bps=cdiv(U, 2048),
                    layout='unit', UNR=2 if depth else 3, half=None)
      return dict(names=['dynimg_goal_onepass2_kernel<%s, false, 1024>' % _tf(depth)], T=1024, UPT=1, bps=cdiv(U, 1024),
                  layout='flat', UNR=3 if depth else 4, half=(N + 1) // 2)
    return dict(names=['dynimg_goal_onepass_kernel<%s, %s, 256, 1>' % (_tf(depth), _tf(u8))], T=256, UPT=1, bps=cdiv(U, 256),
                layout='unit' if u8 else 'flat', UNR=2 if depth else 3, half=None)
  if c['entry'] == 'rgbd':
    return dict(names=['dynimg_wsum3_kernel<true>', 'dynimg_norm_kernel'], T=256, UPT=1, bps=cdiv(U, 256), layout='unit', UNR=None, half=None)
  aligned = c['sample_stride'] % 4 == 0 and c['frame_stride'] % 4 == 0
  if c['Cin'] == 3 and c['Cpad'] == 4 and HW % 4 == 0 and aligned:
    return dict(names=['dynimg_wsum3_kernel<false>', 'dynimg_norm_kernel'], T=256, UPT=1, bps=cdiv(U, 256), layout='unit', UNR=None, half=None)
  return dict(names=['dynimg_wsum_generic_kernel', 'dynimg_norm_kernel'], T=256, UPT=1, bps=cdiv(HW, 256), layout='pixel', UNR=None, half=None)


@functools.lru_cache(maxsize=8)
def _element_map(layout, T, UPT, HW, Cc):
  """(block, slot j, thread) of every element [HW][Cc] of a frame in the min / max pass."""
  p, ch = np.meshgrid(np.arange(HW, dtype=np.int64), np.arange(Cc, dtype=np.int64), indexing='ij')
  if layout == 'pixel':
    return (p // T).astype(np.int32), np.zeros_like(p, np.int32), (p % T).astype(np.int32)
  u = p // 4
  per = T * UPT
  b, j, tid = u // per, (u % per) // T, u % T                  # the unit layout, and the depth of both layouts
  if layout == 'flat':
    f = (3 * p + ch) // 4                                     # float4 number in the RGB frame
    r = f % (3 * per)
    rgb = ch < 3
    b = np.where(rgb, f // (3 * per), b)
    j = np.where(rgb, r // T // 3, j)
    tid = np.where(rgb, r % T, tid)
  return b.astype(np.int32), j.astype(np.int32), tid.astype(np.int32)


def element_map(c):
  g = geometry(c)
  return _element_map(g['layout'], g['T'], g['UPT'], c['HW'], c['C'])


def candidates(c, chans):
  """[(tag, pixel, channel)] of the named places this case's geometry has, among the channels ``chans``; interleaved so that
  neighbours in the list lie in different blocks where there are several."""
  g = geometry(c)
  HW, Cc = c['HW'], c['C']
  b, j, tid = element_map(c)
  ok = np.zeros((HW, Cc), bool)
  ok[:, list(chans)] = True
  pix = np.arange(HW)[:, None]
  out = []

  def add(tag, mask, which=0):
    idx = np.flatnonzero((mask & ok).ravel())
    if len(idx):
      e = int(idx[which % len(idx)])
      out.append((tag, e // Cc, e % Cc))

  last = g['bps'] - 1
  add('unit0', (pix < 4) & (b >= 0), c['N'])
  add('last-f4', (pix == HW - 1) & (b >= 0), -1)             # its last element: the B (the depth) of the last pixel
  for w in (1, 2, 3, 15):
    if w * 64 < g['T']:
      add('w%d-l0' % w, (b == 0) & (j == 0) & (tid == 64 * w), w)
      add('w%d-l63' % w, (b == last) & (j == 0) & (tid == 64 * w + 63), w) if last else None
      add('w%d-l63' % w, (b == 0) & (j == 0) & (tid == 64 * w + 63), w + 1)
  add('last-unit', (pix >= HW - 4) & (b >= 0), 1)
  if last:
    add('block0', b == 0, 5)
    add('last-block', b == last, 0)
    add('block0', b == 0, -1)
    add('last-block', b == last, -1)
  if last >= 64:
    add('block64', b == 64, 7)
    add('block0', b == 0, 11)
    add('block64+', b == last, 3)
  for k in range(6):                                           # (and unnamed ones, for the frames with fewer than four named)
    add('other', b >= 0, 1 + k * max(1, HW * len(chans) // 6))
  if g['UPT'] == 2:
    add('slot1', j == 1, 0)
    add('slot1', j == 1, -1)
    add('slot1', (j == 1) & (b == last), 2)
  return out


def tags_of(c, p, ch):
  g = geometry(c)
  b, j, tid = (int(a[p, ch]) for a in element_map(c))
  t = {'wave%d' % (tid // 64)}
  if tid % 64 in (0, 63):
    t.add('lane%d' % (tid % 64))
  if p < 4:
    t.add('unit0')
  if p >= c['HW'] - 4:
    t.add('last-unit')
  if p == c['HW'] - 1 and ch == c['C'] - 1:
    t.add('last-f4')
  if g['bps'] > 1:
    t.add('block0' if b == 0 else 'last-block' if b == g['bps'] - 1 else 'mid-block')
  if b >= 64:
    t.add('block64+')
  if j == 1:
    t.add('slot1')
  t.add('depth' if c['entry'] != 'dynimg' and ch == 3 else 'RGB'[ch] if ch < 3 else 'c%d' % ch)
  return t


# ---- the case table ------------------------------------------------------------------------------------------------------------------
def _case(entry, N, K, HW, C, recipe, strided=None, swap=False, Cin=None, Cpad=None, two_frame=False, tag=''):
  hw = '%dx%d' % HW if isinstance(HW, tuple) else str(HW)
  HWn = HW[0] * HW[1] if isinstance(HW, tuple) else HW
  c = dict(entry=entry, N=N, K=K, HW=HWn, C=C, recipe=recipe, strided=strided, swap=swap, Cin=Cin or C, Cpad=Cpad or max(C, 4),
           two_frame=two_frame)
  if entry == 'dynimg':
    c['Cpad'] = Cpad or C
  # strides in floats (dense unless strided); the two-frame forms read frame 0 with frame_stride 0 and frame 1 from frames2
  fs = HWn * c['Cin'] + (0 if strided is None else 4 if strided == 'wide' else 3)
  c['frame_stride'] = 0 if two_frame else fs
  c['sample_stride'] = (1 if two_frame else K) * fs + (0 if strided is None else 8 if strided == 'wide' else 5)
  c['dframe_stride'] = 0 if two_frame else HWn + (4 if strided else 0)
  c['dsample_stride'] = (1 if two_frame else K) * (HWn + (4 if strided else 0)) + (12 if strided else 0)
  c['id'] = '-'.join(x for x in (entry, 'c%d' % c['Cin'] + ('p%d' % c['Cpad'] if entry == 'dynimg' else ''), 'N%d' % N, 'K%d' % K,
                                'HW' + hw, recipe, 'swap' if swap else '', strided or '', '2f' if two_frame else '', tag) if x)
  return c


def _recipes(depth):
  return ['pos', 'neg', 'planted-rgb'] + (['planted-depth', 'planted-mix'] if depth else [])


NEG_MAXK = {False: 6, True: 3}      # the longest window of a 'neg' case, by uint8


def _goal_cases():
  cs = []
  for u8 in (False, True):
    entry = 'goal_u8' if u8 else 'goal'
    for depth in (False, True):
      C = 4 if depth else 3
      rec = _recipes(depth)

      def pick(i, K=0):
        # (bytes cannot be scaled: a target 150 levels below the current frame puts the whole window high, and the bound with it)
        recipe = rec[i % len(rec)]
        return dict(recipe='pos' if recipe == 'neg' and K > NEG_MAXK[u8] else recipe, swap=(i // len(rec)) % 2 == 1)
      i = 0
      # --- onepass<D, U8, 256, 1>: the frame loop at HW = 1028 (two blocks, one live thread in the second) ...
      unr = 2 if depth else 3
      for km in sorted({0, 1, unr - 1, unr, unr + 1, 2 * unr + 1}):
        cs.append(_case(entry, 2, km + 1, 1028, C, **pick(i, km + 1)))
        i += 1
      # ... and the shapes: one live thread, one wave, one exact block, a ragged third block; N = 3
      for HW in (4, (8, 8), (32, 32), 1028, (36, 40)):
        for k in range(2 if HW in (4, 1028) else 1):
          cs.append(_case(entry, 3, 2 + i % 3, HW, C, **pick(i, 2 + i % 3)))
          i += 1
      for k in range(len(rec)):                                 # every recipe once more at the ragged three-block shape
        cs.append(_case(entry, 2, 3, (36, 40), C, **pick(i + k), tag='b'))
      i += len(rec)
      for sw in (False, True):                                  # 65 blocks per sample: the collect's second trip
        cs.append(_case(entry, 1, 2, 65540, C, 'planted-mix' if depth and sw else 'planted-rgb', swap=sw))
      cs.append(_case(entry, 1, 2, 65540, C, 'pos'))
      if not u8:
        cs.append(_case(entry, 2, 3, 1028, C, 'planted-rgb', strided='wide'))
        cs.append(_case(entry, 3, 4, (36, 40), C, 'neg', strided='wide'))
      # --- the big grid: onepass2<D, false, 1024> / onepass<D, true, 1024, 2>, from N * ceil(U / 2048) = 192 on
      unr = (2 if depth else 3) if u8 else (3 if depth else 4)
      kms = {0, 1, unr - 1, unr, unr + 1, 2 * unr + 1}
      if not u8:
        kms |= {3 * unr, 3 * unr + 1}                           # three ring rounds: mid() inside the steady loop
      for km in sorted(kms):
        cs.append(_case(entry, 192, km + 1, (8, 8), C, **pick(i, km + 1)))
        i += 1
      if u8:
        shapes = [(192, (72, 72)), (192, 4000), (192, 8192), (193, (72, 72))]
      else:
        shapes = [(192, (72, 72)), (193, (72, 72)), (192, 4096)]
      for N, HW in shapes:
        for k in range(2):
          K = 2 if HW == 8192 else 3 + k
          cs.append(_case(entry, N, K, HW, C, **pick(i, K)))
          i += 1
      if not u8:
        cs.append(_case(entry, 193, 3, (72, 72), C, 'planted-rgb', strided='wide'))
      Nbig, HWbig = (3, 524304) if u8 else (6, 262160)          # 65 blocks per sample / per group
      cs.append(_case(entry, Nbig, 2, HWbig, C, 'planted-rgb', swap=depth))
      cs.append(_case(entry, Nbig, 2, HWbig, C, 'planted-mix' if depth else 'neg', swap=not depth))
  return cs


def _dynimg_cases():
  cs = []
  i = 0
  for entry, C in (('dynimg', 3), ('rgbd', 4)):
    rec = ['pos', 'neg', 'planted-rgb'] + (['planted-depth', 'planted-mix'] if entry == 'rgbd' else [])
    kw = dict(Cin=3, Cpad=4) if entry == 'dynimg' else {}
    for HW, N, K in ((4, 2, 2), (4, 3, 1), (1028, 2, 3), (1028, 2, 5), (1028, 3, 6), ((36, 40), 2, 4), ((36, 40), 3, 9)):
      for k in range(2 if HW == 1028 else 1):
        cs.append(_case(entry, N, K, HW, C, rec[i % len(rec)], swap=(i // len(rec)) % 2 == 1, **kw))
        i += 1
    for r in rec:                                               # the two-frame form: frame 0 at frame_stride 0, frame 1 = frames2
      cs.append(_case(entry, 2, 2, 1028, C, r, two_frame=True, **kw))
    cs.append(_case(entry, 2, 2, (36, 40), C, 'planted-rgb', swap=True, two_frame=True, strided='wide', **kw))
    cs.append(_case(entry, 2, 3, 1028, C, 'planted-rgb', strided='wide', **kw))
    cs.append(_case(entry, 3, 4, (36, 40), C, 'pos', strided='wide', **kw))
    cs.append(_case(entry, 1, 2, 262160, C, 'planted-rgb', **kw))      # 257 partials per sample: the fold's second trip
    cs.append(_case(entry, 1, 2, 262160, C, 'neg', swap=True, **kw))
  # the generic kernel: C = 4 (one float4 per frame), and the scalar channel loop at (C, Cpad)
  gen = [(4, 4, 257, 2), (4, 4, 1028, 2), (4, 8, 300, 2), (1, 1, 257, 2), (1, 1, 260, 3), (3, 3, 256, 2), (3, 3, 7, 2), (3, 4, 7, 2),
         (3, 4, 257, 3), (5, 8, 257, 2), (5, 8, 3, 2), (8, 8, 300, 2), (2, 3, 5, 2), (1, 1, 65540, 1)]
  for k, (C, Cpad, HW, N) in enumerate(gen):
    for K in ((2, 5) if HW < 1000 else (2,)):
      cs.append(_case('dynimg', N, K, HW, C, ['pos', 'planted-rgb', 'neg'][(k + K) % 3], swap=k % 2 == 1, Cin=C, Cpad=Cpad))
  cs.append(_case('dynimg', 2, 3, 1028, 3, 'planted-rgb', strided='odd', Cin=3, Cpad=4))      # 4-byte aligned frames: not wsum3
  cs.append(_case('dynimg', 2, 2, 7, 3, 'pos', two_frame=True, Cin=3, Cpad=3))
  cs.append(_case('dynimg', 2, 2, 257, 5, 'planted-rgb', two_frame=True, strided='odd', Cin=5, Cpad=8))
  return cs


GOAL_CASES = _goal_cases()
DYNIMG_CASES = _dynimg_cases()
CASES = GOAL_CASES + DYNIMG_CASES


BY_ENTRY = {e: [c for c in CASES if c['entry'] == e] for e in ('dynimg', 'rgbd', 'goal', 'goal_u8')}


def expected_instances():
  return {n for c in CASES for n in geometry(c)['names']}


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
BASE, NOISE, DELTA, DELTA2 = 12.0, 5.0, 150.0, 70.0      # planted: background levels BASE .. BASE + NOISE of 255; the buffer image's
# plants ramp over DELTA levels, the pair image's lie DELTA2 apart (its range: DELTA2 / 255 = 0.27)


def _assign_plants():
  """c['plants'] = {(n, image, 'min' | 'max'): (pixel, channel)} for every case, in table order: each plant goes to the named place
  that its instantiation has used least so far for that extremum (then to the least used channel), the second extremum of an image
  into another block than the first where the sample has several -- so the cases of an instantiation together put min and max at
  every named place, and both ways round across the first and the last block."""
  used_tag, used_ch = {}, {}
  for c in CASES:
    name = geometry(c)['names'][0]
    has_depth = c['entry'] != 'dynimg' and c['C'] == 4
    rgb = tuple(range(min(c['C'], 3))) if c['entry'] != 'dynimg' else tuple(range(c['C']))
    where = (rgb, rgb)
    if has_depth:
      where = {'planted-depth': ((3,), (3,)), 'planted-mix': ((3,), rgb), 'planted-rgb': (rgb, rgb)}.get(c['recipe'], ((0, 1, 2, 3),) * 2)
    cand = [candidates(c, where[0]), candidates(c, where[1])]
    blk = element_map(c)[0]
    c['plants'] = {}
    for n in range(c['N']):
      taken = set()
      for img in (0, 1):
        first_block = None
        for ext in (('max', 'min') if c['swap'] else ('min', 'max')):
          best = None
          for k, (tag, p, ch) in enumerate(cand[img]):
            if (p, ch) in taken:
              continue
            score = (1000 * (first_block == int(blk[p, ch])) + 10 * used_tag.get((name, tag, ext), 0) + used_ch.get((name, ch, ext), 0), k)
            if best is None or score < best[0]:
              best = (score, tag, p, ch)
          assert best is not None, 'fewer than four distinct named elements'
          _, tag, p, ch = best
          taken.add((p, ch))
          first_block = int(blk[p, ch])
          if not (img == 0 and c['K'] == 1) and not (img == 1 and c['entry'] in ('dynimg', 'rgbd')):      # (images that exist)
            used_tag[(name, tag, ext)] = used_tag.get((name, tag, ext), 0) + 1
            used_ch[(name, ch, ext)] = used_ch.get((name, ch, ext), 0) + 1
          c['plants'][(n, img, ext)] = (p, ch)


def _levels(c):
  """Levels in 0..255 (real-valued) of the frames [N][K][HW][C] and of the target [N][HW][C], and the plants
  {(n, image, 'min' | 'max'): (pixel, channel)}; image 0 = buffer image, 1 = pair image."""
  N, K, HW, C, recipe = c['N'], c['K'], c['HW'], c['C'], c['recipe']
  r = np.random.default_rng(zlib.crc32(c['id'].encode()))
  u8 = c['entry'] == 'goal_u8'
  plants = c['plants']
  t = (np.arange(K, dtype=np.float64) / max(K - 1, 1)).reshape(1, K, 1, 1)
  if recipe in ('pos', 'neg'):
    # s1: what an element gains (pos) / loses (neg) over the window; s2: how far the target lies above / below the current frame.
    # Both span smin..smax (the pair image's range is 0.5 (smax - smin) / 255 >= 0.25 for bytes), s1 + s2 <= 250 of 255 levels.
    smin, smax, m = 20.0, 150.0, 15.0
    lo = r.random((N, 1, HW, C)) * 3
    s1 = smin + m + r.random((N, 1, HW, C)) * (smax - smin - 2 * m)
    # (float32 frames are scaled by 26, so their pair image has its range from 20 levels; the lower the levels, the smaller
    # sum |alpha x| and with it the bound)
    smax2, m2 = (smax, m) if u8 or recipe == 'pos' else (50.0, 5.0)
    top = np.minimum(smax2, 250.0 - s1[:, 0])
    s2 = smin + m2 + r.random((N, HW, C)) * (top - smin - 2 * m2)
    for (n, img, ext), (p, ch) in plants.items():
      first = (ext == 'min') == (recipe == 'pos')                 # (neg: the flattest ramp is the maximum)
      lo[n, 0, p, ch] = 0.0
      if img == 0:
        s1[n, 0, p, ch] = smin if first else smax
        s2[n, p, ch] = min(s2[n, p, ch], 250.0 - s1[n, 0, p, ch] - m)
      else:
        s2[n, p, ch] = smin if first else smax2
        s1[n, 0, p, ch] = min(s1[n, 0, p, ch], 250.0 - s2[n, p, ch] - m)
    if K == 1:
      t = t + 1.0
    if recipe == 'pos':
      X = lo + s1 * t
      if u8:
        X = np.rint(X)
      T = X[:, K - 1] + s2
    else:
      if u8:
        lo, s2 = np.rint(lo), np.rint(s2)
      T = lo[:, 0]
      X = lo + s2[:, None] + s1 * (1.0 - t if K > 1 else 0.0 * t)
  else:
    X = BASE + r.random((N, K, HW, C)) * NOISE
    T = BASE + r.random((N, HW, C)) * NOISE
    for (n, img, ext), (p, ch) in plants.items():
      if img == 0 and K > 1:
        X[n, :, p, ch] = BASE + DELTA * (t[0, :, 0, 0] if ext == 'max' else 1.0 - t[0, :, 0, 0])
        T[n, p, ch] = X[n, K - 1, p, ch]
      elif img == 1 and ext == 'max':
        T[n, p, ch] = BASE + DELTA2
      elif img == 1:
        X[n, :, p, ch] = BASE + DELTA2
        T[n, p, ch] = BASE
  return X, T, plants


class Inputs:
  """The float32 values the kernels read: x [N][K][HW][C], tgt [N][HW][C] (depth = channel 3 of the RGB-D entries), the bytes
  behind them for the uint8 entry, and the plants."""

  def __init__(self, c):
    X, T, self.plants = _levels(c)
    u8 = c['entry'] == 'goal_u8'
    scale = 26.0 if (c['recipe'] in ('pos', 'neg') and not u8) else 1.0      # 20 / 255 x 0.5 x 26 > 1
    self.x = (X / 255.0 * scale).astype(F32)
    self.tgt = (T / 255.0 * scale).astype(F32)
    self.bytes = self.tgt_bytes = None
    if u8:
      self.bytes, self.tgt_bytes = np.rint(X[..., :3]).astype(np.uint8), np.rint(T[..., :3]).astype(np.uint8)
      assert (np.rint(X[..., :3]) >= 0).all() and (np.rint(T[..., :3]) <= 255).all() and (np.rint(X[..., :3]) <= 255).all()
      self.x[..., :3] = self.bytes.astype(F32) / F32(255.0)
      self.tgt[..., :3] = self.tgt_bytes.astype(F32) / F32(255.0)


@functools.lru_cache(maxsize=2)
def inputs(cid):
  return Inputs(CASE_BY_ID[cid])


CASE_BY_ID = {c['id']: c for c in CASES}
assert len(CASE_BY_ID) == len(CASES), 'duplicate case ids'
_assign_plants()


# ---- the float64 reference and its bound ---------------------------------------------------------------------------------------------
def gamma(k):
  return k * U32 / (1.0 - k * U32)


def _norm64(D, S, K):
  """D, S = sum |alpha x| [N][HW][C] float64 -> (normalised image, bound, range [N])."""
  N = D.shape[0]
  ax = (1, 2)
  m, M = D.min(axis=ax, keepdims=True), D.max(axis=ax, keepdims=True)
  r = M - m + 1e-6
  q = (D - m) / r
  e = gamma(K + 1) * S
  E = e.max(axis=ax, keepdims=True)
  Er = 2 * E + abs(float(F32(1e-6)) - 1e-6) + gamma(2) * (r + 2 * E)
  En = (e + E) * (1 + U32) + U32 * (D - m)
  bound = (En + q * Er) / (r - Er) * (1 + U32) + U32 * q
  return q, bound, (M - m).reshape(N), m.reshape(N), M.reshape(N)


class Reference:
  """cur [N][HW][C] float32 (compared by equality); per image (buffer, pair): the float64 image, its bound, D itself, the range."""

  def __init__(self, c, inp):
    K = c['K']
    x, tg = inp.x.astype(np.float64), inp.tgt.astype(np.float64)
    a = alpha(K).astype(np.float64).reshape(1, K, 1, 1)
    a2 = alpha(2).astype(np.float64)
    self.cur = inp.x[:, K - 1]
    self.D = [(a * x).sum(axis=1), a2[0] * x[:, K - 1] + a2[1] * tg]
    self.S = [np.abs(a * x).sum(axis=1), np.abs(a2[0] * x[:, K - 1]) + np.abs(a2[1] * tg)]
    self.img, self.bound, self.range, self.min, self.max = [], [], [], [], []
    for D, S, k in zip(self.D, self.S, (K, 2)):
      q, b, rg, m, M = _norm64(D, S, k)
      self.img.append(q), self.bound.append(b), self.range.append(rg), self.min.append(m), self.max.append(M)

  def images(self, c):
    """The images this case's entry point writes: goal entries both, a two-frame form none but the pair image of frame 0 and
    frames2 -- which the inputs hold as x[:, 0], x[:, 1] with K = 2, i.e. as the buffer image."""
    return (0, 1) if c['entry'] in ('goal', 'goal_u8') else (0,)


@functools.lru_cache(maxsize=2)
def reference(cid):
  return Reference(CASE_BY_ID[cid], inputs(cid))


def check_recipe(c, inp, ref):
  """The effect each recipe claims on the float64 extrema."""
  N, K, HW, C = c['N'], c['K'], c['HW'], c['C']
  u8 = c['entry'] == 'goal_u8'
  for img in ref.images(c):
    D = ref.D[img].reshape(N, -1)
    if img == 0 and K == 1:
      assert not D.any()                                        # alpha(1) = [0]: the buffer image is 0 / 1e-6 = 0, exactly
      continue
    assert (ref.range[img] >= RANGE_FLOOR).all(), (c['id'], img, ref.range[img].min())
    assert float(ref.bound[img].max()) <= CAP, (c['id'], img, float(ref.bound[img].max()))
    for n in range(N):
      for ext, arg in (('min', D[n].argmin()), ('max', D[n].argmax())):
        p, ch = inp.plants[(n, img, ext)]
        assert arg == p * C + ch, (c['id'], n, img, ext, divmod(int(arg), C), (p, ch))
    if c['recipe'] in ('pos', 'neg'):
      sgn = 1.0 if c['recipe'] == 'pos' else -1.0
      assert (sgn * D > 0).all(), c['id']
      near = np.abs(D).min(axis=1)
      assert (near >= (0.12 * ref.range[img] if u8 else 1.0)).all(), (c['id'], img, near.min(), ref.range[img].max())
    else:
      # planted: without its plant the extremum falls back into the background, several background spreads away
      for n in range(N):
        d = np.sort(D[n])
        spread = d[-2] - d[1]
        assert d[-1] - d[-2] > 3 * spread and d[1] - d[0] > 3 * spread, (c['id'], n, img, d[0], d[1], d[-2], d[-1])
  if c['entry'] in ('goal', 'goal_u8'):
    for n in range(N):
      assert len({inp.plants[(n, i, e)] for i in (0, 1) for e in ('min', 'max')}) == 4
    if C == 4 and c['recipe'] in ('planted-rgb', 'planted-depth', 'planted-mix'):
      chans = [[inp.plants[(n, i, e)][1] for n in range(N) for e in ('min', 'max')] for i in (0, 1)]
      want = {'planted-rgb': (False, False), 'planted-depth': (True, True), 'planted-mix': (True, False)}[c['recipe']]
      for i in (0, 1):
        assert all((ch == 3) == want[i] for ch in chans[i]), c['id']


# ---- the float32 emulation, right and wrong ------------------------------------------------------------------------------------------
MUTATIONS = ('fold-from-0', 'pad-joins', 'depth-only', 'rgb-only', 'live-for-flive', 'last-slot-dropped', 'slots-from-64-dropped',
             'slot1-dropped', 'second-sample-first-range', 'pair-with-buffer-norm', 'alpha2-swapped', 'remainder-alpha-off-by-one',
             'range-without-1e-6')


def _fma32(acc, w, x, fused):
  if fused:                                                    # the float32 product is exact in float64; one rounding to float32
    return (acc.astype(np.float64) + np.float64(w) * x.astype(np.float64)).astype(F32)
  return (acc + (F32(w) * x).astype(F32)).astype(F32)


@functools.lru_cache(maxsize=4)
def _order(layout, T, UPT, HW, Cc):
  b, j, tid = _element_map(layout, T, UPT, HW, Cc)
  key = b.ravel().astype(np.int64)
  order = np.argsort(key, kind='stable')
  starts = np.flatnonzero(np.r_[True, np.diff(key[order]) != 0])
  return order, starts, key[order][starts]


def emulate(c, inp, fused=True, mut=None):
  """(cur, [buffer image, pair image]) in float32 as the stage computes them: accumulation in t order, per-block min / max into
  slots, the fold, (D - min) / range.  ``mut``: one of MUTATIONS, a wrong kernel.  Returns None when the mutation does not touch
  this case's form."""
  g = geometry(c)
  N, K, HW, C = c['N'], c['K'], c['HW'], c['C']
  goal = c['entry'] in ('goal', 'goal_u8')
  has_depth = c['entry'] != 'dynimg' and C == 4
  a, a2 = alpha(K), alpha(2)
  idx = list(range(K))
  if mut == 'remainder-alpha-off-by-one':
    if not goal or (K - 1) % g['UNR'] == 0:
      return None
    for t in range((K - 1) // g['UNR'] * g['UNR'], K - 1):
      idx[t] = t + 1
  if mut == 'alpha2-swapped':
    if not goal:
      return None
    a2 = a2[::-1]
  applies = {'pad-joins': not has_depth and c['Cpad'] > c['Cin'], 'depth-only': has_depth, 'rgb-only': has_depth,
             'live-for-flive': g['layout'] == 'flat', 'last-slot-dropped': g['bps'] > 1, 'slots-from-64-dropped': g['bps'] > 64,
             'slot1-dropped': g['UPT'] == 2, 'second-sample-first-range': g['half'] is not None, 'pair-with-buffer-norm': goal}
  if mut in applies and not applies[mut]:
    return None
  x = inp.x
  D1 = np.zeros((N, HW, C), F32)
  for t in range(K):
    D1 = _fma32(D1, a[idx[t]], x[:, t], fused)
  Ds = [D1]
  if goal:
    D2 = _fma32(np.zeros((N, HW, C), F32), a2[0], x[:, K - 1], fused)
    Ds.append(_fma32(D2, a2[1], inp.tgt, fused))
  # which elements enter the min / max
  b, j, tid = element_map(c)
  inc = np.ones((HW, C), bool)
  if mut == 'depth-only':
    inc[:, :3] = False
  if mut == 'rgb-only':
    inc[:, 3] = False
  if mut == 'slot1-dropped':
    inc &= j != 1
  if mut == 'live-for-flive':
    U = HW // 4
    livecount = np.clip(U - (b.astype(np.int64) * g['T'] * g['UPT'] + j.astype(np.int64) * g['T']), 0, g['T'])
    inc &= (tid < livecount) | (np.arange(C)[None, :] == 3)
  order, starts, blocks = _order(g['layout'], g['T'], g['UPT'], HW, C)
  keep = np.ones(len(blocks), bool)
  if mut == 'last-slot-dropped':
    keep &= blocks != g['bps'] - 1
  if mut == 'slots-from-64-dropped':
    keep &= blocks < 64
  norms = []
  for D in Ds:
    lo = np.where(inc, D, F32(np.inf)).reshape(N, -1)[:, order]
    hi = np.where(inc, D, F32(-np.inf)).reshape(N, -1)[:, order]
    smn, smx = np.minimum.reduceat(lo, starts, axis=1), np.maximum.reduceat(hi, starts, axis=1)      # the slots [N][bps]
    m, M = smn[:, keep].min(axis=1), smx[:, keep].max(axis=1)
    if mut == 'fold-from-0' or mut == 'pad-joins':
      m, M = np.minimum(m, F32(0)), np.maximum(M, F32(0))
    r = (M - m).astype(F32)
    if mut != 'range-without-1e-6':
      r = (r + F32(1e-6)).astype(F32)
    norms.append((m.astype(F32), r))
  if mut == 'pair-with-buffer-norm':
    norms[1] = norms[0]
  if mut == 'second-sample-first-range':
    h = g['half']
    for i, (m, r) in enumerate(norms):
      m, r = m.copy(), r.copy()
      m[h:], r[h:] = m[:N - h], r[:N - h]
      norms[i] = (m, r)
  out = []
  with np.errstate(divide='ignore', invalid='ignore'):
    for D, (m, r) in zip(Ds, norms):
      out.append(((D - m.reshape(N, 1, 1)).astype(F32) / r.reshape(N, 1, 1)).astype(F32))
  return x[:, K - 1], out


def accepts(c, ref, got_cur, got_imgs):
  """Whether outputs pass what the GPU test asserts; the worst excess over the bound otherwise."""
  if not np.array_equal(got_cur.view(np.uint32), ref.cur.view(np.uint32)):
    return False
  for img in ref.images(c):
    err = np.abs(got_imgs[img].astype(np.float64) - ref.img[img])
    if not (err <= np.minimum(ref.bound[img], CAP)).all():      # (a NaN fails too)
      return False
  return True
