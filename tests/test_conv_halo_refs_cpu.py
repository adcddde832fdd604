"""The two comparisons of tests/test_conv_halo_variants_gpu.py reject wrong kernels, shown without a GPU: float32 numpy emulations
of the kernels' arithmetic with one mistake each, at the small cases of tests/native/conv_halo_cases.txt, judged by the very
function the device test asserts on (_conv_refs.halo_compare) and by the host packers of the sign fields.

Per mistake the test states which pass sees it: 'exact' (integers, equality), 'rounding' (N(0, 1) under conv_bound), and 'bits'
(the check, part of both passes, that masked elements are +0.0 bit for bit).  An emulation with no mistake, summed in a shuffled
order, passes both.  Also held here, for every case: the forward's left-out share with the seeded inputs and the size of the exact
pass's sums, the conditions the device test relies on.
"""
import numpy as np
import pytest

import _conv_refs as R

CASES = R.load_halo_cases(device_only=True)


def case(text):
  return next(c for c in CASES if c.text == text)


def bf16(a):
  """float32 -> the nearest bfloat16 (round to nearest even), as float32."""
  u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
  u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
  return u.astype(np.uint32).view(np.float32)


def emu_dgrad(dz, w, H, W, rng, TH=None, mistake=None):
  """One group's input gradient in float32 (stride 2, even sizes: pad_before = 0): taps and 16-channel chunks in a shuffled order,
  each chunk one float32 matrix product.  TH: class-pixel rows of a tile (the -1 halo row of an interior tile boundary)."""
  N, Ho, Wo, Cout = dz.shape
  Cin = w.shape[2]
  dxp = np.zeros((N, H + 2, W + 2, Cin), np.float32)
  chunks = [(t, k) for t in range(9) for k in range(Cout // 16 - (1 if mistake == 'drop_chunk' else 0))]
  for i in rng.permutation(len(chunks)):
    (tap, k), sl = chunks[i], slice(16 * chunks[i][1], 16 * chunks[i][1] + 16)
    ky, kx = divmod(tap, 3)
    z, wk = dz[..., sl], w[ky, kx][:, sl]
    if mistake == 'bf16':
      z, wk = bf16(z), bf16(wk)
    if ky == 2 and mistake in ('halo_zero', 'prev_frame'):
      z = z.copy()
      if mistake == 'halo_zero':       # output row i feeds class row i + 1 through ky = 2: that tile's -1 halo row
        z[:, [i for i in range(Ho - 1) if (i + 1) % TH == 0]] = 0
    part = (z.reshape(-1, 16) @ wk.T).reshape(N, Ho, Wo, Cin)
    dxp[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2] += part
    if ky == 2 and mistake == 'prev_frame':      # class row 0 of frame n takes the last dz row of frame n - 1 as its -1 halo row
      prev = (dz[:-1, Ho - 1][..., sl].reshape(-1, 16) @ wk.T).reshape(N - 1, Wo, Cin)
      dxp[1:, 0, kx:kx + 2 * Wo:2] += prev
  return dxp[:, :H, :W]      # (pad_before = 0: padded row 0 is input row 0, which the -1 halo row feeds)


def emu_fwd(x, w, b, stride, relu, rng, mistake=None):
  """One group's forward in float32, taps in a shuffled order."""
  N, H, W, Cin = x.shape
  wc, Cout = w.shape[2], w.shape[3]
  Ho, pt, pb = R.same_pad(H, stride)
  Wo, pl, pr = R.same_pad(W, stride)
  xp = np.zeros((N, H + pt + pb, W + pl + pr, Cin), np.float32)
  xp[:, pt:pt + H, pl:pl + W] = x
  y = np.zeros((N * Ho * Wo, Cout), np.float32)
  win = lambda ky, kx: xp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride].reshape(N * Ho * Wo, Cin)
  for tap in rng.permutation(9):
    ky, kx = divmod(int(tap), 3)
    a, wk = win(ky, kx)[:, :wc], w[ky, kx]
    if mistake == 'bf16':
      a, wk = bf16(a), bf16(wk)
    y += a @ wk
  if mistake == 'rgb_pad':      # the pad channel of x times tap 0's first kernel row
    y += win(0, 0)[:, 3:4] * w[0, 0, 0][None, :]
  y = (y + b).reshape(N, Ho, Wo, Cout)
  return np.maximum(y, np.float32(0)) if relu else y


def masked(v, pos, neg_zero=False):
  return np.where(pos, v, np.float32(-0.0 if neg_zero else 0.0)).astype(np.float32)


def unpack_fields8(f, C, swap=None):
  """The LDS-staged kernel's reading of the byte fields; swap: 'jq' / 'T' read another bit."""
  pos = np.zeros(f.shape[:-1] + (C,), bool)
  for ch in range(C):
    T, q, j = ch // 16, (ch % 16) // 4, ch % 4
    if swap == 'jq':
      q, j = j, q
    byte, bit = ((T & 1) * 4 + q, 4 * (T >> 1) + j) if swap == 'T' else ((T >> 1) * 4 + q, 4 * (T & 1) + j)
    pos[..., ch] = (f[..., byte % f.shape[-1]] >> np.uint8(bit % 8)) & 1
  return pos


def unpack_fields16(f, C, swap=None):
  pos = np.zeros(f.shape[:-1] + (C,), bool)
  for ch in range(C):
    i, q, j = ch // 16, (ch % 16) // 4, ch % 4
    if swap == 'jq':
      q, j = j, q
    pos[..., ch] = (f[..., q] >> np.uint16(4 * i + j)) & 1
  return pos


def run_dgrad(c, exact, mistake=None, seed=7):
  """The emulated launch of a gradient case -> halo_compare's problems."""
  inp, ref, bound, keep = R.halo_case_expect(c, exact)
  rng = np.random.default_rng(seed)
  form = R.halo_form(c)
  TH = 4 if c.family == 'halo' else 8
  got = np.stack([emu_dgrad(inp['dz'][g], inp['w'][g], c.H, c.W, rng, TH,
                            mistake if mistake in ('drop_chunk', 'bf16', 'halo_zero', 'prev_frame') else None) for g in range(c.G)])
  if mistake == 'second_item':
    # block b's second item (item b + blocks) computed with the ci block and the encoder's kernel of its first (item b)
    n_cib = c.items // (c.G * c.N)      # one-frame tiles: tiles_per_group = N
    cib_w = c.Cin // n_cib
    for it in range(c.blocks, c.items):
      g, r = divmod(it, n_cib * c.N)
      cib, n = divmod(r, c.N)
      g0, r0 = divmod(it - c.blocks, n_cib * c.N)
      cib0 = r0 // c.N
      wrong = emu_dgrad(inp['dz'][g][n:n + 1], inp['w'][g0][:, :, cib0 * cib_w:(cib0 + 1) * cib_w], c.H, c.W, rng)
      got[g, n, :, :, cib * cib_w:(cib + 1) * cib_w] = wrong[0]
  pos = inp['mask'] > 0
  if form == 'mask' and mistake == 'mask_stride':
    # the mask read at the dz group stride: groups packed at stride |dx| + 28 inside NaN, read at g * (|dz| + 20)
    size, gs = pos[0].size, pos[0].size + 28
    flat = np.full(c.G * gs, np.nan, np.float32)
    for g in range(c.G):
      flat[g * gs:g * gs + size] = inp['mask'][g].reshape(-1)
    gs_dz = inp['dz'][0].size + 20
    pos = np.stack([(flat[g * gs_dz:g * gs_dz + size] > 0).reshape(pos.shape[1:]) for g in range(c.G)])
  if form == 'fields':
    if c.family == 'halo':
      Hp, Wp = R.tiles_8x64(c.H, c.W)
      planes = R.pad_planes(R.pack_fields16(pos), Hp, Wp, 0xFFFF)
      if mistake == 'pad_as_data':      # the planes addressed with the image's pitch instead of the padded one
        flat = planes.reshape(c.G, -1, 4)
        idx = (np.arange(c.N)[:, None, None] * c.H + np.arange(c.H)[None, :, None]) * c.W + np.arange(c.W)[None, None, :]
        f = flat[:, idx]
      else:
        f = planes[:, :, :c.H, :c.W]
      pos = unpack_fields16(f, c.Cin, 'jq' if mistake == 'swap_jq' else None)
    else:
      pos = unpack_fields8(R.pack_fields8(pos), c.Cin, {'swap_jq': 'jq', 'swap_T': 'T'}.get(mistake))
  if form != 'none':
    got = masked(got, pos, neg_zero=mistake == 'neg_zero')
  return R.halo_compare(c, exact, got, inp, ref, bound, keep)[1]


def run_fwd(c, exact, mistake=None, seed=7):
  inp, ref, bound, keep = R.halo_case_expect(c, exact)
  rng = np.random.default_rng(seed)
  got = np.stack([emu_fwd(inp['x'][g], inp['w'][g], inp['b'][g], c.stride, 'relu' in c.flags, rng, mistake) for g in range(c.G)])
  return R.halo_compare(c, exact, got, inp, ref, bound, keep)[1]


def seen(problems):
  return {p.split(':')[0] for p in problems}


LDS_2X2 = 'dgrad 1 3 32 64 64 32 2'            # 2 x 2 tiles per frame: an interior tile boundary
LDS_FRAME_ROUNDS = 'dgrad 3 130 16 16 64 32 2'      # 780 items on 768 blocks
HALO_SMALL = 'dgrad 1 2 16 64 48 64 2'
HALO_RAGGED = 'dgrad 3 53 10 66 48 64 2'
FWD_SMALL = 'fwd 1 2 16 64 48 64 2 relu bias'
RGB_SMALL = 'fwd 1 2 16 64 4 32 1 relu bias bits rgb'

# mistake -> (case, the passes that see it: 'exact' / 'rounding' name halo_compare's value comparison of that pass, 'bits' its
# check of the masked elements, which both passes run)
MISTAKES = {
    'halo_zero': (LDS_2X2, {True: {'exact'}, False: {'rounding'}}),
    'prev_frame': (LDS_2X2, {True: {'exact'}, False: {'rounding'}}),
    'drop_chunk': (LDS_2X2, {True: {'exact'}, False: {'rounding'}}),
    'second_item': (LDS_FRAME_ROUNDS, {True: {'exact'}, False: {'rounding'}}),
    'mask_stride': (LDS_FRAME_ROUNDS + ' mask', {True: {'exact', 'bits'}, False: {'rounding', 'bits'}}),
    'swap_jq': (LDS_2X2 + ' fields', {True: {'exact', 'bits'}, False: {'rounding', 'bits'}}),
    'swap_T': (LDS_2X2 + ' fields', {True: {'exact', 'bits'}, False: {'rounding', 'bits'}}),
    'swap_jq16': (HALO_SMALL + ' fields', {True: {'exact', 'bits'}, False: {'rounding', 'bits'}}),
    'pad_as_data': (HALO_RAGGED + ' fields', {True: {'exact', 'bits'}, False: {'rounding', 'bits'}}),
    # small integers are exact in bf16: only the rounding pass sees a product path of reduced precision
    'bf16': (LDS_2X2, {True: set(), False: {'rounding'}}),
    # -0.0 == 0.0: the value comparisons pass, the bit check of both passes sees it
    'neg_zero': (LDS_2X2 + ' mask', {True: {'bits'}, False: {'bits'}}),
}


@pytest.mark.parametrize('name', sorted(MISTAKES))
def test_gradient_mistake_is_seen(name):
  text, want = MISTAKES[name]
  c = case(text)
  for exact in (True, False):
    got = seen(run_dgrad(c, exact, 'swap_jq' if name == 'swap_jq16' else name))
    assert got == want[exact], (name, exact, got)


@pytest.mark.parametrize('text', [LDS_2X2, LDS_2X2 + ' mask', LDS_2X2 + ' fields', HALO_SMALL + ' fields', HALO_RAGGED + ' fields',
                                  LDS_FRAME_ROUNDS + ' mask'])
def test_gradient_without_mistake_passes(text):
  for exact in (True, False):
    assert run_dgrad(case(text), exact, None, seed=11) == []


def test_forward_mistakes_are_seen():
  c = case(FWD_SMALL)
  assert seen(run_fwd(c, True, 'bf16')) == set() and seen(run_fwd(c, False, 'bf16')) == {'rounding'}
  # the RGB kernel variable: the input's pad channel is random data and must not reach y
  c = case(RGB_SMALL)
  assert np.abs(R.halo_case_expect(c, True)[0]['x'][..., 3]).max() > 0
  assert seen(run_fwd(c, True, 'rgb_pad')) == {'exact'} and seen(run_fwd(c, False, 'rgb_pad')) == {'rounding'}
  for text in (FWD_SMALL, RGB_SMALL, 'fwd 1 2 16 64 4 32 1 bias'):
    for exact in (True, False):
      assert run_fwd(case(text), exact, None, seed=11) == []


def test_packers_are_inverted_by_the_documented_layouts():
  """pack_fields8 / pack_fields16 / pack_bits32 against a bit-by-bit reading of the definitions, and a swapped reading differs."""
  r = np.random.default_rng(5)
  pos = r.random((3, 5, 64)) < 0.5
  assert np.array_equal(unpack_fields8(R.pack_fields8(pos), 64), pos)
  assert not np.array_equal(unpack_fields8(R.pack_fields8(pos), 64, 'jq'), pos)
  assert not np.array_equal(unpack_fields8(R.pack_fields8(pos), 64, 'T'), pos)
  p48 = pos[..., :48]
  assert np.array_equal(unpack_fields16(R.pack_fields16(p48), 48), p48)
  words = R.pack_bits32(pos[..., :32])
  for ch in range(32):
    assert np.array_equal((words >> np.uint32((ch & 3) * 8 + (ch >> 2))) & 1, pos[..., ch].astype(np.uint32))


def test_the_device_test_s_conditions_hold_for_every_case():
  """Forward with ReLU: the share left out around zero stays below LEFT_OUT_MAX with the seeded inputs.  Exact pass: every sum, and
  the sum of the magnitudes of its terms, is an integer below 2**24."""
  done = set()
  for c in CASES:
    key = (R._halo_shape_key(c), 'relu' in c.flags)
    if key in done:
      continue
    done.add(key)
    inp, ref, bound, keep = R.halo_case_expect(c, False)
    assert R.left_out(keep) < R.LEFT_OUT_MAX, (c.text, R.left_out(keep))
    _, pre, mag = R._halo_shape_expect(R._halo_shape_key(c), True)
    assert np.array_equal(pre, np.rint(pre)) and mag.max() <= (16 * c.Cout + 3 if c.dir == 'dgrad' else 36 * c.Cin + 3) < 2 ** 24, c.text
