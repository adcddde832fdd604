"""The two comparisons of tests/test_conv_bottom_variants_gpu.py reject wrong kernels, shown without a GPU: a float32 numpy emulation
of the fused encoder-bottom backward that sums in the kernel's grouping (per 8 x 64 tile, per block's range into one slab, then the
slabs), with one mistake each, at cases of tests/native/conv_bottom_cases.txt, judged by the very function the device test asserts
on (_conv_refs.bottom_compare).

Per mistake the test states which pass sees it: 'exact' (integers, equality), 'rounding' (N(0, 1) under the derived bound), 'nan'
(either pass: an output element that is NaN).  The emulation without a mistake passes both on every case: that measures the
reference and its bound, never the kernel.
"""
import numpy as np
import pytest

import _conv_refs as R

CASES = R.load_bottom_cases()


def case(text):
  return next(c for c in CASES if c.text == text)


def bf16(a):
  """float32 -> the nearest bfloat16 (round to nearest even), as float32."""
  u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
  u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
  return u.astype(np.uint32).view(np.float32)


def emu_dgrad(dz2, w2, Hc, Wc, mistake):
  """conv2's input gradient of one encoder in float32 on a canvas of whole tiles [N][Hc][Wc][32] (stride 2, even sizes: no padding
  in front), tap by tap in the kernel's order.  The canvas holds what the kernel's accumulators hold for the out-of-image pixels
  of a ragged tile as well: dz2's last row and column reach one pixel past the image."""
  N, Ho, Wo, _ = dz2.shape
  canvas = np.zeros((N, max(Hc, 2 * Ho + 2), max(Wc, 2 * Wo + 2), 32), np.float32)
  flat = dz2.reshape(-1, 48)
  for tap in (4, 3, 5, 1, 7, 0, 2, 6, 8):
    if mistake == 'drop_tap' and tap == 5:
      continue
    src = {1: 7, 7: 1}.get(tap, tap) if mistake == 'swap_taps' else tap
    ky, kx = divmod(tap, 3)
    z, wk = flat, w2[src // 3, src % 3]
    if mistake == 'bf16':
      z, wk = bf16(z), bf16(wk)
    canvas[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2] += (z @ wk.T).reshape(N, Ho, Wo, 32)
  return canvas[:, :Hc, :Wc]


def emu_bottom(c, e, mistake=None):
  """-> dict(dw, db, dz1) float32 [G][...]: every block's range tile by tile into that block's slab, the slabs summed in order."""
  G, N, H, W, C = c.G, c.N, c.H, c.W, c.C
  Hc, Wc = R.tiles_8x64(H, W)
  tx_n, ty_n = Wc // 64, Hc // 8
  cols = 4 if mistake == 'pad_column' else C      # pad_column: the (tap, channel) columns taken at pitch 4, the pad channel among them
  dw, db, dz1_out = [], [], []
  ranges = R.bottom_ranges(c)
  for g in range(G):
    on = e['mask'][g] > 0
    if mistake == 'mask_shift':        # the mask of the pixel to the left
      on = np.concatenate([on[:, :, :1], on[:, :, :-1]], 2)
    if mistake == 'bit_neighbour':     # channel 5's bit taken from channel 4
      on = on.copy()
      on[..., 5] = on[..., 4]
    onc = np.zeros((N, Hc, Wc, 32), bool)
    onc[:, :H, :W] = on
    acc = emu_dgrad(e['dz2'][g], e['w2'][g], Hc, Wc, mistake)
    dz1 = np.where(onc, acc, np.float32(0))
    dz1_db = dz1
    if mistake == 'oob_db':            # out-of-image pixels of a ragged tile pass the mask on their way into db1 (dw1: left alone)
      onc[:, H:] = True
      onc[:, :, W:] = True
      dz1_db = np.where(onc, acc, np.float32(0))
    xp = np.zeros((N, Hc + 2, Wc + 2, 4), np.float32)
    xp[:, 1:H + 1, 1:W + 1] = e['x'][g]
    slabs_w = np.full((c.S, 9 * cols, 32), np.nan, np.float32)      # the workspace starts as NaN: every slab has to be written
    slabs_b = np.full((c.S, 32), np.nan, np.float32)
    for gg, slab, first, end in ranges:
      if gg != g:
        continue
      if mistake == 'skip_segment' and c.remainder and slab == c.S - 1 and g == 1:
        slabs_w[slab], slabs_b[slab] = 0, 0      # the slab the previous segment left in LDS is not this encoder's: here, nothing
        continue
      if mistake == 'garbage_empty' and first == end:
        continue
      aw, ab = np.zeros((9 * cols, 32), np.float32), np.zeros(32, np.float32)
      n_first = first // (tx_n * ty_n)
      for t in range(first, end):
        n, rem = divmod(t, tx_n * ty_n)
        ty, tx = divmod(rem, tx_n)
        nx = n_first if mistake == 'prev_frame_x' and t > first else n      # the x halo of a later tile of the range: the first tile's frame
        d = dz1[n, 8 * ty:8 * ty + 8, 64 * tx:64 * tx + 64].reshape(512, 32)
        win = np.stack([xp[nx, 8 * ty + ky:8 * ty + ky + 8, 64 * tx + kx:64 * tx + kx + 64, :cols].reshape(512, cols)
                        for ky in range(3) for kx in range(3)], 1).reshape(512, 9 * cols)
        aw += win.T @ d
        ab += dz1_db[n, 8 * ty:8 * ty + 8, 64 * tx:64 * tx + 64].reshape(512, 32).sum(0, dtype=np.float32)
      slabs_w[slab], slabs_b[slab] = aw, ab
    sw, sb = slabs_w[0].copy(), slabs_b[0].copy()
    for k in range(1, c.S):
      sw += slabs_w[k]
      sb += slabs_b[k]
    sw = sw.reshape(-1)[:9 * C * 32].reshape(3, 3, C, 32).copy()      # the slab's first 9 C rows are dw1 (pad_column: rows at pitch 4 read at pitch C)
    if mistake == 'last_column':      # row 9 C - 1 = (tap 8, the last real channel) is never stored
      sw[2, 2, C - 1] = 0
    dw.append(sw); db.append(sb); dz1_out.append(dz1[:, :H, :W])
  return dict(dw=np.stack(dw), db=np.stack(db), dz1=np.stack(dz1_out))


def seen(problems):
  return {p.split(' ')[0] for p in problems}


def run(c, exact, mistake=None):
  e = R.bottom_case_expect(c, exact)
  got = emu_bottom(c, e, mistake)
  if 'dz1' not in c.flags:
    del got['dz1']
  return R.bottom_compare(c, exact, got, e)


EXACT_RGB = '1 2 16 64 3 mask'
EXACT_RGBD = '1 2 16 64 4 mask dz1'
RAGGED_BITS = '3 3 10 66 3 bits'
RAGGED_DZ1 = '3 3 10 66 3 mask dz1'
FRAMES = '3 40 2 130 3 bits'
REMAINDER = '3 64 10 66 3 bits pending'

# mistake -> (case meant to catch it, {exact pass: seen, rounding pass: seen})
BOTH = {True: {'exact'}, False: {'rounding'}}
MISTAKES = {
    'drop_tap': (RAGGED_DZ1, BOTH),
    'swap_taps': (RAGGED_DZ1, BOTH),
    'pad_column': (EXACT_RGB, BOTH),
    'last_column': (EXACT_RGB, BOTH),
    'last_column_rgbd': (EXACT_RGBD, BOTH),
    'mask_shift': (RAGGED_DZ1, BOTH),
    'bit_neighbour': (RAGGED_BITS, BOTH),
    'oob_db': (RAGGED_BITS, BOTH),
    'prev_frame_x': (FRAMES, BOTH),
    'skip_segment': (REMAINDER, BOTH),
    'garbage_empty': (EXACT_RGB, {True: {'exact', 'nan'}, False: {'rounding', 'nan'}}),
    # small integers are exact in bf16: only the rounding pass sees a product path of reduced precision
    'bf16': (RAGGED_DZ1, {True: set(), False: {'rounding'}}),
    'bf16_unstored': (RAGGED_BITS, {True: set(), False: {'rounding'}}),      # dz1 stays on chip: seen through dw1 / db1 alone
}


@pytest.mark.parametrize('name', sorted(MISTAKES))
def test_mistake_is_seen(name):
  text, want = MISTAKES[name]
  c = case(text)
  for exact in (True, False):
    _, problems = run(c, exact, name.replace('_rgbd', '').replace('_unstored', ''))
    assert seen(problems) == want[exact], (name, exact, problems)


def test_the_mistakes_touch_what_they_are_meant_to():
  """The cases behind MISTAKES have what each mistake needs: data in the pad channel, ragged tiles, a range across frames, a
  remainder segment of encoder 1, empty blocks -- and oob_db moves db1 alone."""
  c = case(EXACT_RGB)
  assert c.C == 3 and c.empty and np.abs(R.bottom_case_expect(c, True)['x'][..., 3]).max() > 0
  c = case(RAGGED_BITS)
  assert c.H % 8 and c.W % 64
  _, problems = run(c, True, 'oob_db')
  assert len(problems) == 1 and problems[0].startswith('exact db'), problems
  c = case(FRAMES)
  assert 'frame' in c.cross and c.per == 2
  c = case(REMAINDER)
  assert c.remainder and c.G == 3
  for exact in (True, False):
    m = R.bottom_case_expect(case(RAGGED_DZ1), exact)['mask']
    assert 0.4 < np.mean(m > 0) < 0.6 and (m == 0).any() and (m < 0).any()


@pytest.mark.parametrize('c', CASES, ids=lambda c: c.text.replace(' ', '-'))
def test_float32_in_the_kernel_s_grouping_stays_inside_the_bounds(c):
  """Every case: the emulation without a mistake equals the float64 reference in the exact pass (so does the reference itself) and
  stays inside the rounding bound, with dz1 compared whether the case stores it or not."""
  for exact in (True, False):
    e = R.bottom_case_expect(c, exact)
    if exact:
      ref = dict(dw=e['dw'].astype(np.float32), db=e['db'].astype(np.float32), dz1=e['dz1'].astype(np.float32))
      assert R.bottom_compare(c, True, ref, e) == (dict(dw=0.0, db=0.0, dz1=0.0), [])
      assert np.abs(e['dz1']).max() <= R.BOTTOM_EXACT_MAX and np.array_equal(e['dz1'], np.rint(e['dz1']))
    worst, problems = R.bottom_compare(c, exact, emu_bottom(c, e), e)
    assert not problems, problems
    assert exact or min(worst.values()) > 0, worst
    if not exact:
      print('%s: float32 in the kernel\'s grouping uses %s of its bounds' % (c.text, ', '.join('%s %.4f' % kv for kv in worst.items())))


def test_the_bound_counts_what_the_kernel_adds():
  """bottom_slab_bound against its own derivation, and dz1's bound is 0 exactly where the mask is off."""
  assert R.bottom_slab_bound(1.0, 512, 85) == (512 + 85 + 12) * R.U
  c = case(RAGGED_DZ1)
  e = R.bottom_case_expect(c, False)
  off = ~(e['mask'] > 0)
  assert (e['e1'][off] == 0).all() and (e['dz1'][off] == 0).all() and (e['e1'][~off] > 0).all()
  assert (e['bw'] > 0).all() and (e['bb'] > 0).all()
