"""The launch-variant table of the kernels that build the decoder's inputs from frame tables -- csrc/replay.hip, replay_dynimg.hip and
shared_frames.hip -- with pure-Python mirrors of their launch rules and the host models the device test compares against.

CASES holds one record per case: the entry point, its arguments, the alignment offsets of its tensors (in floats behind a 16-byte
boundary) and the row pitch.  ``plan(c)`` gives, from the mirrors alone, the traced kernel names the case must show and, per loop of
the kernels it runs, (trips, ragged): the largest number of trips any thread (or block) makes and whether the last trip is a partial
one.  tests/test_table_builders_cover_cpu.py proves on the host that the table reaches every instantiation and every loop's second
trip; tests/test_table_builders_variants_gpu.py launches exactly this table.

Host models: the states come from _replay_ref.states_ref / _replay_dynimg_ref.states_pair_ref, the shared-frame gather and its float64
scatter-sum are here (tests/test_shared_frames_gpu.py imports the scatter-sum back), the image stage is a float64 restatement with
the bound below, and its planted pixels are computed bitwise in float32.

The image bound (replay_images, buffer and pair image).  Inputs are float32 values x_k (a byte / 255 correctly rounded, or the
float32 frame) and float32 coefficients alpha_k, so the float64 restatement starts from the same numbers.  The raw image is a chain
of K steps acc <- acc + alpha_k x_k; fused or not, a step commits at most two roundings of relative size u = 2^-24, so
  |D^ - D| <= E = g(2 K) A,   A = sum_k |alpha_k x_k|,   g(m) = m u / (1 - m u).
The extrema of the computed image are those of perturbed values: |mn^ - mn|, |mx^ - mx| <= Emax = the largest E of the window.
The stored value is fl(fl(D^ - mn^) / fl(fl(mx^ - mn^) + 1e-6f)); with inv = 1 / (mx - mn + 1e-6) and y the exact value in [0, 1]
  numerator:    |N^ - N| <= E + Emax + u N            denominator: |r^ - r| <= 2 Emax + 2 u r
  |y^ - y| <= (E + Emax) inv + 2 y Emax inv + 4 u y   to first order; the test allows 1.01 times that for the higher orders.
With planted extrema every window's range is at least 0.5, so inv <= 2."""
import collections

import numpy as np

import _replay_dynimg_ref as D
import _replay_ref as R

RP_THREADS, RP_MAX_BLOCKS = 256, 2048          # csrc/replay_internal.h
SF_THREADS, SF_MAX_POSITIONS = 256, 1024       # csrc/shared_frames.hip
U = 2.0 ** -24
MODES = ('plain', 'constant', 'residual')

Case = collections.namedtuple('Case', 'id entry a')


def cdiv(a, b):
  return -(-a // b)


def trips(units, step):
  """(trips of the busiest thread or block, whether the last trip is partial) of ``for (u = first; u < units; u += step)``."""
  return cdiv(units, step), units % step != 0


# ---- mirrors of the launch rules ---------------------------------------------------------------------------------------------
def replay_states_launch(widths, src_offs, J, stride, states_off, K, n, cells):
  """launch_replay_states: ``widths`` the table widths (one or two), ``src_offs`` the offsets in floats of every source pointer that
  enters the alignment test (the tables and, where there is one, the constant target row)."""
  vec = all(w % 4 == 0 for w in widths) and all(o % 4 == 0 for o in src_offs)
  vst = vec and J % 4 == 0 and stride % 4 == 0 and states_off % 4 == 0
  V = 4 if vec else 1
  per = max(cells * max(widths) // V, cells * J)
  grid = min(cdiv(K * n * per, RP_THREADS), RP_MAX_BLOCKS)
  step = grid * RP_THREADS
  loops = {'table%d' % s: trips(K * n * (cells * w // V), step) for s, w in enumerate(widths)}
  loops['joint'] = trips(K * n * cells * J, step)
  return dict(vec=vec, vst=vst, V=V, per=per, grid=grid, loops=loops,
              names=['replay_states_kernel<%d, %s>' % (V, 'true' if vst else 'false')])


def replay_images_launch(HW, n, u8, buf):
  """geeco_replay_images: blocks per window, the capped grid, both kernels' item loop and the emit kernel's fold of the partials."""
  bpw = cdiv(HW // 4, RP_THREADS)
  grid = min(n * bpw, RP_MAX_BLOCKS)
  tmpl = '<%s, %s>' % ('true' if u8 else 'false', 'true' if buf else 'false')
  return dict(bpw=bpw, grid=grid, loops={'items': trips(n * bpw, grid), 'fold': trips(bpw, RP_THREADS)},
              names=['replay_images_minmax_kernel' + tmpl, 'replay_images_emit_kernel' + tmpl])


def shared_vec(ch, *offs):
  """The rule of geeco_window_states_fwd (feat) and geeco_window_states_bwd (feat | dfeat): 16-byte loads of the feature rows."""
  return ch % 4 == 0 and all(o % 4 == 0 for o in offs)


def pack_frames_launch(HW, u8, slot_offs):
  """geeco_pack_frames_by_address: grid.x covers the frame on the path the launch is sized for (4 pixels per thread when HW % 4 == 0);
  a block whose slot is unused (offset None) or misaligned for that path walks the frame one pixel per thread WITH THE SAME GRID,
  so only there px += step runs again.  ``slot_offs``: per slot the frame's offset in bytes behind a 16-byte boundary."""
  quad = HW % 4 == 0
  gx = cdiv(HW // 4 if quad else HW, SF_THREADS)
  step = gx * SF_THREADS
  loops = {}
  for o in slot_offs:
    if quad and o is not None and o % (4 if u8 else 16) == 0:
      loops['quad'] = trips(HW // 4, step)
    elif o is None:
      loops['zero'] = trips(HW, step)
    else:
      loops['pixel'] = trips(HW, step)
  sized = 'quad' if quad else 'pixel'
  return dict(grid_x=gx, sized=sized, last_block_ragged=(HW // 4 if quad else HW) % SF_THREADS != 0, loops=loops,
              names=['pack_frames_kernel<%s>' % ('true' if u8 else 'false')])


def state_width(mode, cells, ch, J):
  return R.state_width(mode, cells, ch, J)


def plan(c):
  """The names the case's trace must show and {loop: (trips, ragged)} for every loop of the kernels it launches."""
  a = c.a
  if c.entry == 'replay_states':
    offs = [a['feat_off']] + ([a['tgt_off']] if a['mode'] != 'plain' else [])
    D_ = state_width(a['mode'], a['cells'], a['ch'], a['J'])
    p = replay_states_launch([a['ch']], offs, a['J'], D_ + a['pad'], a['states_off'], a['K'], a['t1'] - a['t0'], a['cells'])
  elif c.entry == 'replay_states_pair':
    D_ = a['cells'] * (a['ch'] + a['J'] + a['ch_t'])
    p = replay_states_launch([a['ch'], a['ch_t']], [a['feat_off'], a['tgt_off']], a['J'], D_ + a['pad'], a['states_off'], a['K'],
                             a['t1'] - a['t0'], a['cells'])
  elif c.entry == 'replay_errors':
    nh = len(a['heads'])
    p = dict(names=['replay_errors_frame_kernel', 'replay_errors_episode_kernel'], blocks=cdiv(a['T'] * nh, RP_THREADS),
             loops={'frame_blocks': trips(a['T'] * nh, RP_THREADS), 'episode': trips(a['T'], RP_THREADS)})
  elif c.entry == 'replay_images':
    p = replay_images_launch(a['HW'], a['t1'] - a['t0'], a['u8'], a['buf'])
  elif c.entry == 'pack_frames':
    p = pack_frames_launch(a['HW'], a['u8'], a['slot_offs'])
  elif c.entry == 'window_states_fwd':
    V = 4 if shared_vec(a['ch'], a['feat_off']) else 1
    p = dict(V=V, names=['window_states_fwd_kernel<%d>' % V],
             loops={'units': trips(a['cells'] * a['ch'] // V, SF_THREADS), 'joint': trips(a['cells'] * a['J'], SF_THREADS)})
  elif c.entry == 'window_states_bwd':
    V = 4 if shared_vec(a['ch'], a['feat_off'], a['dfeat_off']) else 1
    loops = {'units': trips(a['cells'] * a['ch'] // V, SF_THREADS), 'positions': trips(a['N'] * a['K'], 64)}
    if a['mode'] != 'plain':
      loops['targets'] = trips(a['N'], 64)
    p = dict(V=V, names=['window_states_bwd_kernel<%d>' % V], loops=loops)
  else:
    raise ValueError(c.entry)
  return p


# ---- the table ---------------------------------------------------------------------------------------------------------------
def _cases():
  out = []
  add = lambda id, entry, **a: out.append(Case(id, entry, a))
  # replay_states: K * n * cells * cw / V and K * n * cells * J both above 2048 * 256 = 524 288.  (ch, J, pad): <4, true> / <4, false>
  # (J = 7) / <1, false> (ch = 9); T = 133 frames, the windows [3, 133): the first 60 of them still show frame 0 in their oldest slots
  big = dict(K=64, T=133, t0=3, t1=133, cells=10, feat_off=0, tgt_off=0, states_off=0)
  for tag, ch, J, pad in (('v4-vs', 32, 8, 4), ('v4', 32, 7, 5), ('v1', 9, 7, 3)):
    for mode in MODES:
      add('states-%s-%s-two-trips' % (tag, mode), 'replay_states', mode=mode, ch=ch, J=J, pad=pad, **big)
  # ... the instantiation an ALIGNMENT decides, small: the table, the target row or the states one float off a 16-byte boundary
  small = dict(K=4, T=7, t0=1, t1=6, cells=4, ch=8, J=8, pad=4)
  add('states-feat-misaligned', 'replay_states', mode='residual', feat_off=1, tgt_off=0, states_off=0, **small)
  add('states-tgt-misaligned', 'replay_states', mode='constant', feat_off=0, tgt_off=1, states_off=0, **small)
  add('states-out-misaligned', 'replay_states', mode='plain', feat_off=0, tgt_off=0, states_off=1, **small)
  # replay_states_pair: both tables past the cap, ch != ch_t
  for tag, ch, ch_t, J, pad in (('v4-vs', 32, 36, 8, 4), ('v4', 32, 36, 7, 5), ('v1', 9, 10, 7, 3)):
    add('pair-%s-two-trips' % tag, 'replay_states_pair', ch=ch, ch_t=ch_t, J=J, pad=pad, **big)
  add('pair-tgt-misaligned', 'replay_states_pair', feat_off=0, tgt_off=1, states_off=0, ch_t=4, **small)
  # replay_errors: T * nheads = 514 / 771 > 256 with a ragged last block, T = 257 > 256 for the episode kernel
  add('errors-squared', 'replay_errors', T=257, heads=[(0, 3, 0), (3, 7, 0)], seed=1)
  add('errors-class-hit', 'replay_errors', T=257, heads=[(0, 3, 1), (3, 2, 1), (5, 3, 0)], seed=2)
  # replay_images.  'items': n * bpw > 2048 (bpw = 1: HW = 128; bpw = 3: HW = 2208, the third block ragged); 'fold': bpw = 257 > 256
  hw3 = 4 * (2 * 256 + 40)
  for u8, buf, K, HW, n in ((True, True, 16, 128, 3000), (False, True, 4, hw3, 700), (True, False, 3, hw3, 700), (False, False, 1, 128, 3000)):
    t0 = 1 if buf else 0
    add('images-%s-%s-items-bpw%d' % ('u8' if u8 else 'f32', 'buf' if buf else 'nobuf', cdiv(HW // 4, 256)), 'replay_images', u8=u8, buf=buf,
        K=K, HW=HW, T=t0 + n, t0=t0, t1=t0 + n, plant='items')
  for u8 in (True, False):
    for buf in (True, False):
      add('images-%s-%s-fold' % ('u8' if u8 else 'f32', 'buf' if buf else 'nobuf'), 'replay_images', u8=u8, buf=buf, K=2, HW=4 * 256 * 257,
          T=3, t0=1, t1=3, plant='fold')
  # pack_frames_by_address: slot offsets in bytes behind a 16-byte boundary (None: an unused slot).  HW = 1200: two blocks of 4-pixel
  # units, the second ragged, and one slot misaligned for that path (three trips of px += step under the grid of the 4-pixel path);
  # HW = 1201: five blocks of single pixels, the last ragged
  for u8 in (True, False):
    add('pack-%s-quad' % ('u8' if u8 else 'f32'), 'pack_frames', u8=u8, HW=1200, slot_offs=[0, None, 1 if u8 else 4, 0])
    add('pack-%s-pixel' % ('u8' if u8 else 'f32'), 'pack_frames', u8=u8, HW=1201, slot_offs=[0, None, 1 if u8 else 4, 0])
  # window_states_fwd: cells * ch / V = 280 (V = 4) and 1080 (V = 1) units, cells * J = 280 joint elements
  wide = dict(cells=40, J=7, pad=3, feat_off=0, out_of_range=False)
  for V, ch in ((4, 28), (1, 27)):
    for mode in MODES:
      add('fwd-v%d-%s-two-trips' % (V, mode), 'window_states_fwd', mode=mode, ch=ch, N=3, K=2, F=5, **wide)
  add('fwd-v1-by-alignment', 'window_states_fwd', mode='constant', ch=8, N=3, K=2, F=5, cells=4, J=7, pad=3, feat_off=1, out_of_range=False)
  for V, ch in ((4, 8), (1, 6)):
    for mode in ('constant', 'residual'):
      add('fwd-v%d-%s-out-of-range' % (V, mode), 'window_states_fwd', mode=mode, ch=ch, N=4, K=3, F=5, cells=4, J=7, pad=3, feat_off=0,
          out_of_range=True)
  # window_states_bwd: the same unit counts; N = 65 windows: two 64-lane trips over the targets, three over the 130 positions
  bwide = dict(cells=40, J=7, pad=3, feat_off=0, dfeat_off=0, kind='disjoint')
  for V, ch in ((4, 28), (1, 27)):
    for mode in MODES:
      add('bwd-v%d-%s-two-trips' % (V, mode), 'window_states_bwd', mode=mode, ch=ch, N=65, K=2, **bwide)
  add('bwd-v1-by-alignment', 'window_states_bwd', mode='residual', ch=8, N=4, K=3, cells=4, J=7, pad=3, feat_off=0, dfeat_off=1, kind='disjoint')
  for mode in ('constant', 'residual'):
    add('bwd-%s-full-list' % mode, 'window_states_bwd', mode=mode, ch=8, N=64, K=16, cells=4, J=7, pad=3, feat_off=0, dfeat_off=0, kind='full')
    add('bwd-%s-out-of-range' % mode, 'window_states_bwd', mode=mode, ch=8, N=4, K=3, cells=4, J=7, pad=3, feat_off=0, dfeat_off=0,
        kind='out_of_range')
  return out


CASES = _cases()
ENTRIES = ('replay_states', 'replay_states_pair', 'replay_errors', 'replay_images', 'pack_frames', 'window_states_fwd', 'window_states_bwd')


def cases(entry):
  return [c for c in CASES if c.entry == entry]


# ---- inputs and host models: states --------------------------------------------------------------------------------------------
def distinct_tables(T, cells, widths, J):
  """float32 tables whose every value is a different small integer: feature tables [T][cells][w] per width, jnt [T][J] and a constant
  target row [cells][widths[0]] above every table's values and in steps of 2, so tgt - feat is exact and distinct per (frame, cell,
  column) too."""
  out, base = [], 1
  for w in widths:
    out.append((base + np.arange(T * cells * w)).reshape(T, cells, w).astype(np.float32))
    base += T * cells * w
  jnt = (base + np.arange(T * J)).reshape(T, J).astype(np.float32)
  base += T * J
  tgt = (2 * base + 2 * np.arange(cells * widths[0])).reshape(cells, widths[0]).astype(np.float32)
  assert 2 * base + 2 * cells * widths[0] < 2 ** 24
  diff = (tgt[None] - out[0]).ravel()
  assert len(np.unique(diff)) == diff.size and diff.min() > base
  return out, jnt, tgt


# ---- inputs and host models: shared frames -----------------------------------------------------------------------------------
def shared_indices(a):
  """(F, idx [N][K], tgt [N]) int32 of a shared-frame case.  'disjoint': windows draw from the first slots, targets from slots of their
  own behind them, the last slot referenced by nothing; 'full': every position names slot 0 and every target slot 1; 'out_of_range':
  'disjoint' with entries of -1 and F in both lists."""
  N, K = a['N'], a['K']
  kind = a.get('kind', 'disjoint')
  r = np.random.default_rng(N * K + a['ch'])
  if kind == 'full':
    return 3, np.zeros((N, K), np.int32), np.ones(N, np.int32)
  if 'F' in a:
    F = a['F']
    nw = F - 2
    tgt = np.full(N, F - 2, np.int32)
  else:
    nw = max(1, (N * K) // 2 + 1)
    nt = (N + 1) // 2
    F = nw + nt + 1
    tgt = (nw + np.arange(N) // 2).astype(np.int32)
  idx = r.integers(0, nw, (N, K)).astype(np.int32)
  if kind == 'out_of_range' or a.get('out_of_range'):
    idx[0, 0], idx[1, K - 1], idx[N - 1, 1] = -1, F, F
    tgt[0], tgt[N - 1] = F, -1
  return F, idx, tgt


def window_states_fwd_ref(feat, idx, jnt, tgt_idx, mode):
  """float32 [K][N][cells * Ctot] of feat [F][cells][ch], idx [N][K], jnt [N][K][J], tgt_idx [N]: the columns of _replay_ref.states_ref;
  a slot outside [0, F) reads nothing and gives zeros."""
  F, cells, ch = feat.shape
  N, K = idx.shape
  J = jnt.shape[2]
  padded = np.concatenate([feat, np.zeros((1, cells, ch), np.float32)])
  at = lambda i: padded[np.where((i >= 0) & (i < F), i, F)]
  Ctot = state_width(mode, 1, ch, J)
  out = np.zeros((K, N, cells, Ctot), np.float32)
  for t in range(K):
    f = at(idx[:, t])
    out[t, :, :, :ch] = (at(tgt_idx) - f) if mode == 'residual' else f
    out[t, :, :, ch:ch + J] = jnt[:, t][:, None, :]
    if mode == 'constant':
      out[t, :, :, ch + J:] = at(tgt_idx)
  return out.reshape(K, N, cells * Ctot)


def window_states_bwd_ref(dst, feat, idx, tgt, mode, J):
  """The float64 scatter-sum of geeco_window_states_bwd: dst [K][N][cells * Ctot] (float32 or float64), feat [F][cells][ch], idx [N][K],
  tgt [N] -> (ref, mag), both [F][cells][ch]: per slot the signed sum of the columns that reference it, masked by feat > 0 (the
  ReluGrad of the encoder's last layer), and the sum of their magnitudes.  An index outside [0, F) contributes to no slot."""
  F, cells, ch = feat.shape
  N, K = idx.shape
  Ctot = state_width(mode, 1, ch, J)
  d4 = dst.astype(np.float64).reshape(K, N, cells, Ctot)
  ref, mag = np.zeros([F, cells, ch]), np.zeros([F, cells, ch])
  sign = -1.0 if mode == 'residual' else 1.0
  for n in range(N):
    for t in range(K):
      if 0 <= idx[n, t] < F:
        ref[idx[n, t]] += sign * d4[t, n, :, :ch]
        mag[idx[n, t]] += np.abs(d4[t, n, :, :ch])
      if mode != 'plain' and 0 <= tgt[n] < F:
        cols = d4[t, n, :, ch + J:] if mode == 'constant' else d4[t, n, :, :ch]
        ref[tgt[n]] += cols
        mag[tgt[n]] += np.abs(cols)
  ref *= feat > 0
  mag *= feat > 0
  return ref, mag


# ---- inputs and host models: the image stage ---------------------------------------------------------------------------------
def unit_block(pixel):
  """The 256-unit block of a window that holds ``pixel`` (a unit = 4 pixels)."""
  return (pixel // 4) // RP_THREADS


def planted_episode(a):
  """uint8 frames [T][HW][3], a goal [HW][3] and the planted pixels of an image case.  Everything else is a narrow random band
  (bytes 124 .. 131).  Returns (frames, goal, binary, pair_binary): ``binary`` the pixels whose frames hold the bytes 0 and 255 alone
  (the buffer image is bitwise computable there), ``pair_binary`` those of them whose goal byte is 0 or 255 as well.

  'items' (any K, bpw = 1 or 3).  2 K phase pixels, phase q in unit block q % bpw: a square wave of period 2 K over the frames, 255
  while (f + q) % 2K < K.  A K-frame window sees of every phase one step up or one step down at one of its K slots, so its buffer
  image has one largest value (the step up where the coefficients' suffix sum peaks) and one smallest (the same step down), K
  frames later at the phase the window before saw: the two extrema walk through the phases, hence through the blocks, as t grows.
  Two constant pixels give the pair image its extrema: frames 0 under goal 255 in block 0 (+1/2), frames 255 under goal 0 in the last
  block (-1/2); the phase pixels' goal is 128, so they stay at +-1/4 there.

  'fold' (K = 2, T = 3, windows 1 and 2, bpw = 257).  Block 0 holds a (0, 255, 0), c (255, 255, 0 | goal 255), e (255, 255, 0 | goal 0);
  block 256 holds b (255, 0, 255), d (0, 0, 255 | goal 0), f (0, 0, 255 | goal 255).  Buffer image 1/2 (x_t - x_t-1): window 1 has its
  maximum at a (block 0) and its minimum at b (block 256); window 2 has them swapped (minimum in block 0: a, c, e; maximum in block
  256: b, d, f).  Pair image 1/2 (goal - x_t): window 2 has its maximum at c (block 0) and its minimum at d (block 256), window 1 its
  minimum at e (block 0) and its maximum at f (block 256)."""
  T, HW, K = a['T'], a['HW'], a['K']
  r = np.random.default_rng(HW + 10 * K + a['u8'])
  frames = r.integers(124, 132, (T, HW, 3), dtype=np.uint8)
  goal = r.integers(124, 132, (HW, 3), dtype=np.uint8)
  f = np.arange(T)
  if a['plant'] == 'items':
    bpw = cdiv(HW // 4, RP_THREADS)
    binary = []
    for q in range(2 * K):
      p = 4 * RP_THREADS * (q % bpw) + 4 * q + 1
      frames[:, p] = np.where((f + q) % (2 * K) < K, 255, 0)[:, None]
      goal[p] = 128
      binary.append(p)
    hi, lo = 3, HW - 2
    assert unit_block(hi) == 0 and unit_block(lo) == bpw - 1 and hi not in binary and lo not in binary
    frames[:, hi], goal[hi] = 0, 255
    frames[:, lo], goal[lo] = 255, 0
    return frames, goal, binary + [hi, lo], [hi, lo]
  assert a['plant'] == 'fold' and K == 2 and T == 3
  far = 4 * RP_THREADS * 256
  pix = dict(a=5, c=9, e=13, b=far + 5, d=far + 9, f=far + 13)
  assert HW > pix['f'] and unit_block(pix['e']) == 0 and unit_block(pix['b']) == 256
  for k, (x, g) in dict(a=((0, 255, 0), 128), c=((255, 255, 0), 255), e=((255, 255, 0), 0), b=((255, 0, 255), 128), d=((0, 0, 255), 0),
                        f=((0, 0, 255), 255)).items():
    frames[:, pix[k]] = np.asarray(x, np.uint8)[:, None]
    goal[pix[k]] = g
  return frames, goal, sorted(pix.values()), sorted(pix[k] for k in 'cdef')


def as_unit(a):
  """uint8 -> the float32 the kernels convert it to (byte / 255, correctly rounded)."""
  return a.astype(np.float32) / np.float32(255)


def images_f64(frames, goal, K, t0, t1, buf):
  """The float64 restatement of geeco_replay_images for float32 ``frames`` [T][HW][3] and ``goal`` [HW][3]: per image ('buf', 'diff')
  a dict of raw [n][HW][3], A = sum |alpha_k x_k|, mn / mx [n] and the normalised values y [n][HW][3]."""
  n = t1 - t0
  idx = R.window_index(frames.shape[0], K)[t0:t1]
  f64, g64 = frames.astype(np.float64), goal.astype(np.float64)
  eps = np.float64(np.float32(1e-6))

  def image(terms):
    raw, A = np.zeros((n,) + goal.shape), np.zeros((n,) + goal.shape)
    for w, x in terms:
      raw += np.float64(w) * x
      A += np.abs(np.float64(w) * x)
    mn, mx = raw.reshape(n, -1).min(1), raw.reshape(n, -1).max(1)
    return dict(raw=raw, A=A, mn=mn, mx=mx, y=(raw - mn[:, None, None]) / (mx - mn + eps)[:, None, None], steps=len(terms))
  a2 = D.alpha(2)
  out = {'diff': image([(a2[0], f64[t0:t1]), (a2[1], g64[None])])}
  if buf:
    ak = D.alpha(K)
    out['buf'] = image([(ak[k], f64[idx[:, k]]) for k in range(K)])
  return out


def image_bound(im):
  """The module docstring's bound on |y^ - y|, [n][HW][3], from the float64 restatement ``im`` of one image."""
  m = 2 * im['steps']
  g = m * U / (1 - m * U)
  E = g * im['A']
  Emax = E.reshape(E.shape[0], -1).max(1)[:, None, None]
  inv = 1.0 / (im['mx'] - im['mn'] + np.float64(np.float32(1e-6)))[:, None, None]
  return 1.01 * ((E + Emax) * inv + 2 * im['y'] * Emax * inv + 4 * U * im['y'])


def planted_f32(frames, goal, K, t0, t1, pixels, which):
  """Bitwise what geeco_replay_images stores at ``pixels`` (whose bytes are 0 and 255 alone: every product is by 0.0 or 1.0, exact with
  or without contraction) when the image's extrema lie among them: float32 [n][len(pixels)][3].  The raw values are summed in frame
  order; the minimum stores 0.0 and the maximum fl(fl(max - min) / fl(fl(max - min) + 1e-6f))."""
  x = as_unit(frames[:, pixels]) if frames.dtype == np.uint8 else frames[:, pixels]
  g = as_unit(goal[pixels]) if goal.dtype == np.uint8 else goal[pixels]
  assert np.isin(x, (0.0, 1.0)).all() and (which == 'buf' or np.isin(g, (0.0, 1.0)).all())
  idx = R.window_index(frames.shape[0], K)[t0:t1]
  n = t1 - t0
  acc = np.zeros((n,) + g.shape, np.float32)
  if which == 'buf':
    ak = D.alpha(K)
    for k in range(K):
      acc = (acc + ak[k] * x[idx[:, k]]).astype(np.float32)
  else:
    a2 = D.alpha(2)
    acc = (acc + a2[0] * x[t0:t1]).astype(np.float32)
    acc = (acc + a2[1] * g[None]).astype(np.float32)
  mn, mx = acc.reshape(n, -1).min(1)[:, None, None], acc.reshape(n, -1).max(1)[:, None, None]
  r = ((mx - mn).astype(np.float32) + np.float32(1e-6)).astype(np.float32)
  return ((acc - mn).astype(np.float32) / r).astype(np.float32), mn[:, 0, 0], mx[:, 0, 0]


def check_planted(a, frames, goal, binary, pair_binary):
  """Proves the planting in float64 on the host and returns, per image, {'range': the smallest range of a window, 'max_blocks' /
  'min_blocks': per window the unit block of its one largest / smallest value}.  Asserts for every window: the range is at least
  0.5; the extrema lie among the pixels that are computed bitwise, and every other pixel stays clear of them by more than the raw
  images' rounding (so the float32 extrema are theirs too); the largest and the smallest value are each held by ONE unit block."""
  t0, t1, K = a['t0'], a['t1'], a['K']
  im = images_f64(as_unit(frames), as_unit(goal), K, t0, t1, a['buf'])
  out = {}
  for name, d in im.items():
    exact = np.asarray(binary if name == 'buf' else pair_binary)
    raw = d['raw']
    n = raw.shape[0]
    assert (d['mx'] - d['mn'] >= 0.5).all(), (name, (d['mx'] - d['mn']).min())
    others = np.ones(raw.shape[1], bool)
    others[exact] = False
    Emax = (2 * d['steps'] * U / (1 - 2 * d['steps'] * U)) * d['A'].reshape(n, -1).max(1)
    assert (raw[:, others].reshape(n, -1).max(1) < d['mx'] - 4 * Emax).all() and (raw[:, others].reshape(n, -1).min(1) > d['mn'] + 4 * Emax).all(), name
    blocks = unit_block(np.arange(raw.shape[1]))
    mxb, mnb = [], []
    for w in range(n):
      top = np.unique(blocks[np.nonzero((raw[w] >= d['mx'][w] - 4 * Emax[w]).any(1))[0]])
      low = np.unique(blocks[np.nonzero((raw[w] <= d['mn'][w] + 4 * Emax[w]).any(1))[0]])
      assert len(top) == 1 and len(low) == 1, (name, w + t0, top, low)
      mxb.append(int(top[0]))
      mnb.append(int(low[0]))
    out[name] = dict(range=float((d['mx'] - d['mn']).min()), max_blocks=np.asarray(mxb), min_blocks=np.asarray(mnb))
  return out
