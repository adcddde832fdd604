"""The filter-gradient reference of tests/_conv_refs.py against the oracle, and the two comparisons of
tests/test_conv_wgrad_variants_gpu.py against wrong kernels (no GPU).

Three parts.  (1) conv_wgrad_ref restates what autograd through oracle.conv2d_same states, and agrees with it in float64.  (2) A
float32 evaluation in a shuffled pixel order, in the case's own number of slices, is bit-exact on the integer inputs of the exact
pass and uses less than half of wgrad_bound on the normal inputs of the rounding pass.  (3) Each of ten mistakes a filter-gradient
kernel could make, emulated in float64 on a case of tests/native/conv_wgrad_cases.txt and rounded to float32 like a kernel's output,
is rejected with at least four elements out of bound -- by both passes, except products rounded to bf16, which only the rounding
pass can see (small integers are exact in bf16): that is why both passes are kept.
"""
import numpy as np
import pytest
import torch

import _conv_refs as R
from oracle import geeco_oracle as O

CASES = R.load_wgrad_cases()
BY_TEXT = {c.text: c for c in CASES}
f32 = lambda a: np.asarray(a, np.float64).astype(np.float32)
t64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)


# --------------------------------------------------------------------------------------------------------------------------
# (1) the reference agrees with the oracle
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('stride', [1, 2, 3, 4])
@pytest.mark.parametrize('H,W', [(9, 7), (8, 10), (5, 6), (1, 7), (1, 1), (2, 2), (13, 4)])
def test_wgrad_ref_is_autograd_through_the_oracle(H, W, stride):
  r = np.random.default_rng(H * 100 + W * 10 + stride)
  Cin, Cout = 3, 5
  Ho, Wo = R.same_pad(H, stride)[0], R.same_pad(W, stride)[0]
  x, dz = r.standard_normal((2, H, W, Cin)), r.standard_normal((2, Ho, Wo, Cout))

  def autograd(x, dz):
    w = torch.zeros(3, 3, Cin, Cout, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(Cout, dtype=torch.float64, requires_grad=True)
    O.conv2d_same(t64(x), w, b, stride, relu=False).backward(t64(dz))
    return w.grad.numpy(), b.grad.numpy()

  dw, db, mag_dw, mag_db = R.conv_wgrad_ref(x, dz, stride)
  for got, want in zip((dw, db), autograd(x, dz)):
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
  for got, want in zip((mag_dw, mag_db), autograd(np.abs(x), np.abs(dz))):
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
  assert np.all(np.abs(dw) <= mag_dw * (1 + 1e-12)) and np.all(np.abs(db) <= mag_db * (1 + 1e-12))


def test_every_case_keeps_the_exact_pass_exact():
  """|x|, |dz| <= 2: a partial sum of at most M products is an integer of magnitude <= 4 M, below 2**24 for every case."""
  for c in CASES:
    assert 4 * R.wgrad_pixels(c) < 2 ** 24, c.text
    x, dz = R.wgrad_case_inputs(c._replace(G=1, N=1), True)
    assert x.dtype == np.float32 and set(np.unique(x)) <= {-2, -1, 0, 1, 2} and set(np.unique(dz)) <= {-2, -1, 0, 1, 2}
    if x.size >= 500:
      assert set(np.unique(x)) == {-2, -1, 0, 1, 2}


# --------------------------------------------------------------------------------------------------------------------------
# (2) float32 in any order passes
# --------------------------------------------------------------------------------------------------------------------------
def _columns(x, dz, stride, pad=None, dtype=np.float64):
  """The sum's terms as matrices: A [M][9 Cin] (the input pixel of every (output pixel, tap), zero in the padding) and Z [M][Cout],
  so that dw = A^T Z and db = the column sums of Z.  pad = (top, left) replaces TF SAME's."""
  N, H, W, Cin = x.shape
  _, Ho, Wo, Cout = dz.shape
  _, pt, _ = R.same_pad(H, stride)
  _, pl, _ = R.same_pad(W, stride)
  if pad is not None:
    pt, pl = pad
  xp = np.zeros((N, max(pt + H, (Ho - 1) * stride + 3), max(pl + W, (Wo - 1) * stride + 3), Cin), dtype)
  xp[:, pt:pt + H, pl:pl + W] = x
  A = np.concatenate([xp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride].reshape(N * Ho * Wo, Cin)
                      for ky in range(3) for kx in range(3)], axis=1)
  return A, dz.reshape(N * Ho * Wo, Cout).astype(dtype)


def _shape(c, dw_flat):
  return dw_flat.reshape(3, 3, c.Cin, c.Cout)


@pytest.mark.parametrize('text', ['1 2 33 31 16 128 1', '3 1 96 96 16 64 1', '1 3 10 36 48 64 2', '1 2 10 20 4 32 1',
                                  '2 33 12 36 32 48 2', '1 11 16 16 192 256 2', '1 2 9 7 16 64 2'])
def test_float32_in_a_shuffled_order_passes_both_comparisons(text):
  c = BY_TEXT[text]
  for exact in (True, False):
    x, dz, dw_ref, db_ref, dw_bound, db_bound = R.wgrad_case_expect(c, exact)
    A, Z = _columns(x[0], dz[0], c.stride, dtype=np.float32)
    r = np.random.default_rng(7)
    dw = db = None
    for px in np.array_split(r.permutation(A.shape[0]), c.S):     # the case's own number of slices, pixels in a shuffled order
      pw, pb = A[px].T @ Z[px], Z[px].sum(0, dtype=np.float32)
      dw, db = (pw, pb) if dw is None else (dw + pw, db + pb)
    assert dw.dtype == np.float32 and db.dtype == np.float32
    dw = _shape(c, dw)
    if exact:
      assert np.array_equal(dw.astype(np.float64), dw_ref[0]) and np.array_equal(db.astype(np.float64), db_ref[0])
    else:
      ratio = max(R.worst_ratio(dw, dw_ref[0], dw_bound[0]), R.worst_ratio(db, db_ref[0], db_bound[0]))
      print('%s: float32 in %d slices uses %.3f of the bound' % (text, c.S, ratio))
      assert ratio < 0.5        # a worst-case bound: a real float32 sum stays far inside it


# --------------------------------------------------------------------------------------------------------------------------
# (3) wrong kernels are rejected.  A mistake: (c, x, dz) -> (dw [G][3][3][Cin][Cout], db [G][Cout]) in float64; only the group it
# names is compared.
# --------------------------------------------------------------------------------------------------------------------------
def _right(c, x, dz, g):
  dw, db, _, _ = R.conv_wgrad_ref(x[g], dz[g], c.stride)
  return dw, db


def _pixels_dropped(c, x, dz, g, drop):
  """The gradient without the output pixels drop [M] (bool)."""
  A, Z = _columns(x[g], dz[g], c.stride)
  return _shape(c, A[~drop].T @ Z[~drop]), Z[~drop].sum(0)


def _last_chunk_of_a_ragged_slice_dropped(c, x, dz):
  """Generic kernel: M = 2046 in slices of 704; the last slice holds 638 pixels = 19 chunks of MK = 32 and one of 30."""
  M = R.wgrad_pixels(c)
  assert c.family == 'generic' and M % c.slice_px % 32 != 0
  drop = np.zeros(M, bool)
  drop[M - M % 32:] = True
  return _pixels_dropped(c, x, dz, 0, drop)


def _slab(c, x, dz, s, factor):
  """Slice s of the generic kernel (pixels [s slice_px, (s + 1) slice_px)) counted `factor` times."""
  A, Z = _columns(x[0], dz[0], c.stride)
  sel = slice(s * c.slice_px, (s + 1) * c.slice_px)
  dw, db = _right(c, x, dz, 0)
  return dw + (factor - 1) * _shape(c, A[sel].T @ Z[sel]), db + (factor - 1) * Z[sel].sum(0)


def _one_slab_dropped(c, x, dz):
  return _slab(c, x, dz, 1, 0)


def _one_slab_added_twice(c, x, dz):
  return _slab(c, x, dz, c.S - 1, 2)


def _symmetric_padding(c, x, dz):
  """Even sizes at stride 2: TF SAME pads only the bottom and the right; here one row on top and one column on the left."""
  assert c.stride == 2 and R.same_pad(c.H, 2)[1:] == (0, 1) and R.same_pad(c.W, 2)[1:] == (0, 1)
  A, Z = _columns(x[0], dz[0], c.stride, pad=(1, 1))
  return _shape(c, A.T @ Z), Z.sum(0)


def _flat_extra(c, x, dz, g, TH, TW, rows, cols):
  """What a tile adds when its DMA does not test the image edges: the tile grid's pixels (oy, ox) past the image, with
  `rows` / `cols` choosing the direction, read from memory as it lies -- dz at flat pixel (n Ho + oy) Wo + ox, x at flat pixel
  (n H + iy) W + ix, zero past the end of the group's tensor."""
  N, H, W, Cin, Cout = c.N, c.H, c.W, c.Cin, c.Cout
  Ho, Wo = R.wgrad_out_hw(c)
  xf = np.concatenate([x[g].reshape(-1, Cin).astype(np.float64), np.zeros((4 * H * W, Cin))])
  zf = np.concatenate([dz[g].reshape(-1, Cout).astype(np.float64), np.zeros((4 * Ho * Wo, Cout))])
  dw, db = np.zeros((3, 3, Cin, Cout)), np.zeros(Cout)
  oys = [oy for oy in range(-(-Ho // TH) * TH) if (oy >= Ho) == rows and (not rows or oy % TH >= TH // 2)]
  oxs = [ox for ox in range(-(-Wo // TW) * TW) if (ox >= Wo) == cols]
  for n in range(N):
    for oy in oys:
      zi = np.array([(n * Ho + oy) * Wo + ox for ox in oxs])
      db += zf[zi].sum(0)
      for ky in range(3):
        for kx in range(3):
          xi = np.array([(n * H + 2 * oy + ky) * W + 2 * ox + kx for ox in oxs])
          dw[ky, kx] += xf[xi].T @ zf[zi]
  return dw, db


def _last_tile_rows_second_half_summed(c, x, dz):
  """LDS kernel, 4 x 8 tiles, Ho = 5: the last tile row holds rows 4..7; rows 6 and 7 (past Ho) are summed as memory holds them."""
  assert c.family == 'lds' and R.wgrad_out_hw(c)[0] % 4 == 1
  dw, db = _right(c, x, dz, 0)
  ew, eb = _flat_extra(c, x, dz, 0, 4, 8, rows=True, cols=False)
  return dw + ew, db + eb


def _ragged_tile_column_reads_the_next_row(c, x, dz):
  """LDS kernel, 4 x 8 tiles, Wo = 18: the third tile column holds columns 16..23; 18..23 wrap into the next row's pixels."""
  assert c.family == 'lds' and R.wgrad_out_hw(c)[1] % 8 == 2
  dw, db = _right(c, x, dz, 0)
  ew, eb = _flat_extra(c, x, dz, 0, 4, 8, rows=False, cols=True)
  return dw + ew, db + eb


def _group1_fed_group0s_dz(c, x, dz):
  dw, db, _, _ = R.conv_wgrad_ref(x[1], dz[0], c.stride)
  return dw, db


def _db_over_xs_pixel_count(c, x, dz):
  """The bias gradient summed over N H W rows of dz instead of N Ho Wo: at stride 2 four times as many, read on into the next
  groups' dz (to the end of the tensor)."""
  assert c.stride == 2 and c.G > 1
  dw, _ = _right(c, x, dz, 0)
  return dw, dz.reshape(-1, c.Cout).astype(np.float64)[:c.N * c.H * c.W].sum(0)


def _column_tile1_written_over_tile0(c, x, dz):
  assert c.family == 'generic' and c.Cout == 128
  dw, db = _right(c, x, dz, 0)
  dw, db = dw.copy(), db.copy()
  dw[..., :64] = dw[..., 64:]
  db[:64] = db[64:]
  return dw, db


def _bf16(a):
  """float64 -> the nearest bfloat16 (ties to even), as float64."""
  b = np.asarray(a, np.float64).astype(np.float32).view(np.uint32).astype(np.uint64)
  b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
  return b.astype(np.uint32).view(np.float32).astype(np.float64)


def _products_rounded_to_bf16(c, x, dz):
  A, Z = _columns(x[0], dz[0], c.stride)
  assert A.shape[0] * A.shape[1] * Z.shape[1] < 10 ** 7
  dw = _bf16(A[:, :, None] * Z[:, None, :]).sum(0)
  return _shape(c, dw), Z.sum(0)


MISTAKES = [
    # name, case, group compared, emulation, seen by the exact pass
    ('last MK chunk of a ragged slice dropped', '1 2 33 31 16 128 1', 0, _last_chunk_of_a_ragged_slice_dropped, True),
    ('one slab dropped', '1 2 33 31 16 128 1', 0, _one_slab_dropped, True),
    ('one slab added twice', '1 2 33 31 16 128 1', 0, _one_slab_added_twice, True),
    ('symmetric padding where SAME pads bottom and right', '1 2 10 40 32 48 2', 0, _symmetric_padding, True),
    ('second half of the last tile row summed past Ho', '1 3 10 36 48 64 2', 0, _last_tile_rows_second_half_summed, True),
    ('ragged tile column reads the next row', '1 3 10 36 48 64 2', 0, _ragged_tile_column_reads_the_next_row, True),
    ('group 1 fed the dz of group 0', '3 23 6 40 48 64 2', 1, _group1_fed_group0s_dz, True),
    ('db summed over the pixel count of x', '3 2 10 40 32 48 2 nodb', 0, _db_over_xs_pixel_count, True),
    ('column tile 1 written over column tile 0', '1 2 33 31 16 128 1', 0, _column_tile1_written_over_tile0, True),
    ('products rounded to bf16', '1 2 9 7 16 64 2', 0, _products_rounded_to_bf16, False),
]


def _out_of_bound(c, g, emulate, exact):
  """Elements of (dw, db) the device test's comparison of this pass rejects: for the rounded reference (must be none) and for
  the mistake."""
  c_db = c._replace(flags=c.flags - {'nodb'})
  x, dz, dw_ref, db_ref, dw_bound, db_bound = R.wgrad_case_expect(c_db, exact)
  ref = np.concatenate([dw_ref[g].reshape(-1), db_ref[g]])
  bound = np.concatenate([dw_bound[g].reshape(-1), db_bound[g]])
  dw, db = emulate(c, x, dz)
  got = np.concatenate([f32(dw).reshape(-1), f32(db)]).astype(np.float64)
  assert got.shape == ref.shape
  right = f32(ref).astype(np.float64)
  return int((~(np.abs(right - ref) <= bound)).sum()), int((~(np.abs(got - ref) <= bound)).sum()), ref.size


@pytest.mark.parametrize('name,text,g,emulate,exact_sees', MISTAKES, ids=[m[0] for m in MISTAKES])
def test_comparisons_reject(name, text, g, emulate, exact_sees):
  c = BY_TEXT[text]
  right_r, bad_r, n = _out_of_bound(c, g, emulate, exact=False)
  right_e, bad_e, _ = _out_of_bound(c, g, emulate, exact=True)
  print('%-52s %-22s out of bound: %d (rounding pass), %d (exact pass) of %d elements' % (name, text, bad_r, bad_e, n))
  assert right_r == 0 and right_e == 0       # the rounded reference itself passes both
  assert bad_r >= 4                          # no mistake hangs on a single lucky element
  if exact_sees:
    assert bad_e >= 4
  else:
    assert bad_e == 0                        # integers in [-2, 2] and their products are exact in bf16: only the rounding pass sees it
