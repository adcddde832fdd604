"""The references of tests/_conv_refs.py against the oracle, and their bound against wrong kernels (no GPU).

Three parts.  (1) conv_fwd_ref / conv_dgrad_ref restate what oracle.conv2d_same and its autograd state, and agree with them in
float64.  (2) The seeded inputs of every case of tests/native/conv_gemm_cases.txt leave fewer than 0.1 % of the ReLU outputs with a
pre-activation inside its own bound (those are left out of the device comparison).  (3) conv_bound, as
tests/test_conv_gemm_variants_gpu.py applies it, accepts a float32 evaluation in a shuffled order and 13 slabs, and rejects each of
ten mistakes a gather GEMM could make, each emulated in float64 on a case of the list and rounded to float32 like a kernel's output.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _conv_refs as R
from oracle import geeco_oracle as O

CASES = R.load_cases()
BY_TEXT = {c.text: c for c in CASES}
f32 = lambda a: np.asarray(a, np.float64).astype(np.float32)
t64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)


# --------------------------------------------------------------------------------------------------------------------------
# (1) the references agree with the oracle
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('stride', [1, 2, 3, 4])
@pytest.mark.parametrize('H,W', [(9, 7), (8, 10), (5, 6), (1, 7), (1, 1), (2, 2), (13, 4)])
@pytest.mark.parametrize('relu', [True, False])
def test_fwd_ref_is_the_oracles_conv(H, W, stride, relu):
  r = np.random.default_rng(H * 100 + W * 10 + stride)
  x, w, b = r.standard_normal((2, H, W, 3)), r.standard_normal((3, 3, 3, 5)), r.standard_normal(5)
  y, mag, pre = R.conv_fwd_ref(x, w, b, stride, relu)
  np.testing.assert_allclose(y, O.conv2d_same(t64(x), t64(w), t64(b), stride, relu=relu).numpy(), rtol=1e-12, atol=1e-12)
  np.testing.assert_allclose(pre, O.conv2d_same(t64(x), t64(w), t64(b), stride, relu=False).numpy(), rtol=1e-12, atol=1e-12)
  np.testing.assert_allclose(mag, O.conv2d_same(t64(np.abs(x)), t64(np.abs(w)), t64(np.abs(b)), stride, relu=False).numpy(),
                             rtol=1e-12, atol=1e-12)
  assert np.all(np.abs(pre) <= mag * (1 + 1e-12))


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('H,W', [(9, 7), (8, 10), (5, 6), (1, 7), (1, 1), (2, 2), (13, 4)])
@pytest.mark.parametrize('with_mask', [True, False])
def test_dgrad_ref_is_autograd_through_the_oracle(H, W, stride, with_mask):
  r = np.random.default_rng(H * 100 + W * 10 + stride)
  Cin, Cout = 3, 5
  Ho, Wo = R.same_pad(H, stride)[0], R.same_pad(W, stride)[0]
  dz, w = r.standard_normal((2, Ho, Wo, Cout)), r.standard_normal((3, 3, Cin, Cout))
  mask = r.standard_normal((2, H, W, Cin)) * (r.uniform(size=(2, H, W, Cin)) > 0.3) if with_mask else None

  def autograd(dz, w):
    x = torch.zeros(2, H, W, Cin, dtype=torch.float64, requires_grad=True)
    O.conv2d_same(x, t64(w), torch.zeros(Cout, dtype=torch.float64), stride, relu=False).backward(t64(dz))
    return x.grad.numpy()

  dx, mag, pre = R.conv_dgrad_ref(dz, w, (H, W), stride, mask)
  np.testing.assert_allclose(pre, autograd(dz, w), rtol=1e-12, atol=1e-12)
  np.testing.assert_allclose(mag, autograd(np.abs(dz), np.abs(w)), rtol=1e-12, atol=1e-12)
  np.testing.assert_allclose(dx, pre * (mask > 0) if with_mask else pre, rtol=0, atol=0)
  # the tap counts of the bound: an all-ones problem counts the products of every element; only the border has fewer
  ones = autograd(np.ones_like(dz), np.ones_like(w))
  terms = np.broadcast_to(R.dgrad_terms((H, W), stride, Cout), ones.shape[1:])
  assert np.all(ones <= terms[None])
  if H >= 5 and W >= 5:
    np.testing.assert_array_equal(ones[:, 1:-1, 1:-1], np.broadcast_to(terms[1:-1, 1:-1], ones[:, 1:-1, 1:-1].shape))
    if stride == 2:
      assert sorted(set(terms[1:-1, 1:-1, 0].reshape(-1))) == [Cout, 2 * Cout, 4 * Cout]


def test_same_pad_puts_the_smaller_half_first():
  assert R.same_pad(8, 2) == (4, 0, 1) and R.same_pad(9, 2) == (5, 1, 1) and R.same_pad(22, 4) == (6, 0, 1)
  assert R.same_pad(1, 2) == (1, 1, 1) and R.same_pad(22, 3) == (8, 1, 1) and R.same_pad(7, 1) == (7, 1, 1)
  for size in range(1, 40):
    for s in (1, 2, 3, 4):
      assert R.same_pad(size, s) == O.same_pad(size, 3, s)


# --------------------------------------------------------------------------------------------------------------------------
# (2) the seeds
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [c for c in CASES if 'relu' in c.flags], ids=R.case_id)
def test_left_out_share_of_the_seeded_inputs(c):
  """Depends on the reference and the bound alone, so it is settled here: under 0.1 % of a case's elements have a pre-activation
  within the bound of zero; and the ReLU cuts a real share of the rest (the bound-0 elements are a check of their own)."""
  _, ref, bound, keep, pre, _ = R.case_expect(c)
  assert R.left_out(keep) < R.LEFT_OUT_MAX, R.left_out(keep)
  assert R.within(f32(ref)[keep], ref[keep], bound[keep])      # the rounded reference itself passes
  cut = float(np.mean(pre < 0))
  assert 0.2 < cut < 0.8, cut


def test_masks_of_the_seeded_inputs_have_all_three_signs():
  c = BY_TEXT['dgrad 1 2 21 19 32 16 2 mask ws w wt']
  m = R.case_inputs(c)['mask']
  assert 0.2 < np.mean(m == 0) < 0.4 and np.mean(m > 0) > 0.25 and np.mean(m < 0) > 0.25


# --------------------------------------------------------------------------------------------------------------------------
# (3) the bound accepts float32 and rejects wrong kernels
# --------------------------------------------------------------------------------------------------------------------------
def _fp32_slabs(c, g, S, seed):
  """The case's group g in float32: the channels dealt to S slabs, each slab summed over the taps in a shuffled order in float32
  (float32 matrix products), the slabs added in float32, then bias / ReLU / mask."""
  inp = R.case_inputs(c)
  r = np.random.default_rng(seed)
  w = inp['w'][g]
  C = c.Cin if c.dir == 'fwd' else c.Cout
  chunks = np.array_split(r.permutation(C), S)
  taps = [(ky, kx) for ky in range(3) for kx in range(3)]
  total = None
  for ch in chunks:
    part = None
    for i in r.permutation(9):
      ky, kx = taps[i]
      wt = np.zeros_like(w)
      if c.dir == 'fwd':
        wt[ky, kx, ch, :] = w[ky, kx, ch, :]
        term = _f32_conv(inp['x'][g], wt, c.stride)
      else:
        wt[ky, kx, :, ch] = w[ky, kx, :, ch]
        term = _f32_dgrad(inp['dz'][g], wt, (c.H, c.W), c.stride)
      part = term if part is None else part + term
    total = part if total is None else total + part
  assert total.dtype == np.float32
  if c.dir == 'fwd':
    total = total + inp['b'][g]
    return np.maximum(total, np.float32(0)) if 'relu' in c.flags else total
  return np.where(inp['mask'][g] > 0, total, np.float32(0))


def _f32_conv(x, w, stride):
  N, H, W, Cin = x.shape
  Ho, pt, pb = R.same_pad(H, stride)
  Wo, pl, pr = R.same_pad(W, stride)
  xp = np.zeros((N, H + pt + pb, W + pl + pr, Cin), np.float32)
  xp[:, pt:pt + H, pl:pl + W] = x
  y = np.zeros((N, Ho, Wo, w.shape[3]), np.float32)
  for ky in range(3):
    for kx in range(3):
      if w[ky, kx].any():
        y += xp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride] @ w[ky, kx]
  return y


def _f32_dgrad(dz, w, in_hw, stride):
  N, Ho, Wo, Cout = dz.shape
  H, W = in_hw
  _, pt, pb = R.same_pad(H, stride)
  _, pl, pr = R.same_pad(W, stride)
  dxp = np.zeros((N, H + pt + pb, W + pl + pr, w.shape[2]), np.float32)
  for ky in range(3):
    for kx in range(3):
      if w[ky, kx].any():
        dxp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride] += dz @ w[ky, kx].T
  return dxp[:, pt:pt + H, pl:pl + W]


@pytest.mark.parametrize('text', ['fwd 3 5 9 9 192 256 2 relu bias ws', 'fwd 1 2 21 19 20 64 1 relu bias ws',
                                  'fwd 1 2 21 19 16 32 2 bias ws', 'dgrad 3 5 9 9 192 256 2 mask ws w wt',
                                  'dgrad 1 2 21 19 16 20 2 mask ws w wt'])
def test_float32_in_a_shuffled_order_and_13_slabs_is_accepted(text):
  c = BY_TEXT[text]
  _, ref, bound, keep, pre, mag = R.case_expect(c._replace(S=13))
  got = _fp32_slabs(c, 0, 13, 5)
  assert got.dtype == np.float32 and got.shape == ref[0].shape
  ratio = R.worst_ratio(got[keep[0]], ref[0][keep[0]], np.maximum(bound[0][keep[0]], 1e-300))
  print('%s: float32 in 13 slabs uses %.3f of the bound' % (text, ratio))
  assert R.within(got[keep[0]], ref[0][keep[0]], bound[0][keep[0]])
  assert R.left_out(keep) < R.LEFT_OUT_MAX
  assert ratio < 0.5        # a worst-case bound: a real float32 sum stays far inside it


def _fwd_pre(c, inp, g, x=None, w=None, b=None):
  """conv + bias in float64 of group g with operands replaced."""
  x = inp['x'][g] if x is None else x
  w = inp['w'][g] if w is None else w
  b = inp['b'][g] if b is None else b
  return R.conv_fwd_ref(x, w, b, c.stride, False)[2]


def _only(w, sel):
  z = np.zeros_like(w)
  z[sel] = w[sel]
  return z


def _symmetric_padding(c, inp):
  """Padding 1 on top / left where TF SAME puts pad_total = 1 at the bottom / right (W = 16 at stride 2; H = 15 has pad_total = 2)."""
  assert R.same_pad(c.W, c.stride)[1:] == (0, 1) and R.same_pad(c.H, c.stride)[1:] == (1, 1)
  x = F.pad(t64(inp['x'][0]).permute(0, 3, 1, 2), (1, 0, 1, 1))
  y = F.conv2d(x, t64(inp['w'][0]).permute(3, 2, 0, 1), t64(inp['b'][0]), stride=c.stride).permute(0, 2, 3, 1).numpy()
  return np.maximum(y, 0)


def _tap_dropped_in_one_class(c, inp):
  """Tap (2, 0) missing: at stride 2 it reaches only the pixels of one parity class, which loses one of its four taps."""
  pre = R.conv_dgrad_ref(inp['dz'][0], inp['w'][0], (c.H, c.W), c.stride, None)[2]
  lost = R.conv_dgrad_ref(inp['dz'][0], _only(inp['w'][0], (2, 0)), (c.H, c.W), c.stride, None)[2]
  classes = {(y % 2, x % 2) for y, x in zip(*np.nonzero(np.abs(lost).sum(axis=(0, 3))))}
  assert len(classes) == 1, classes
  return np.where(inp['mask'][0] > 0, pre - lost, 0)


def _last_kstep_dropped(c, inp):
  """Cin = 20: 180 (tap, channel) pairs are eleven K-steps of 16 and a twelfth of 4: channels 16..19 of the last tap."""
  assert (9 * c.Cin) % 16 == 4
  return np.maximum(_fwd_pre(c, inp, 0) - _fwd_pre(c, inp, 0, w=_only(inp['w'][0], (2, 2, slice(16, 20))), b=np.zeros(c.Cout)), 0)


def _bias_per_slab(c, inp):
  return np.maximum(_fwd_pre(c, inp, 0) + (c.S - 1) * inp['b'][0].astype(np.float64), 0)


def _relu_per_slab(c, inp):
  """The slabs as the kernel deals them: the (tap, channel) axis in c.S contiguous runs of whole K-steps."""
  K = 9 * c.Cin
  per = -(-(K // 16) // c.S) * 16
  total = 0.0
  for s in range(c.S):
    sel = np.zeros(K, bool)
    sel[s * per:(s + 1) * per] = True
    ws = np.where(sel.reshape(3, 3, c.Cin, 1), inp['w'][0], 0)
    total = total + np.maximum(_fwd_pre(c, inp, 0, w=ws, b=np.zeros(c.Cout)), 0)
  return np.maximum(total + inp['b'][0], 0)


def _mask_ge(c, inp):
  pre = R.conv_dgrad_ref(inp['dz'][0], inp['w'][0], (c.H, c.W), c.stride, None)[2]
  return np.where(inp['mask'][0] >= 0, pre, 0)


def _ragged_tile_unwritten(fill):
  def mistake(c, inp):
    y = np.maximum(_fwd_pre(c, inp, 0), 0)
    rows = y.reshape(-1, c.Cout)      # a view
    assert rows.shape[0] % c.BM != 0
    rows[rows.shape[0] // c.BM * c.BM:] = fill
    return y
  return mistake


def _class_to_neighbour_parity(c, inp):
  """The rows of the class of odd columns written to the even columns beside them."""
  dx = R.conv_dgrad_ref(inp['dz'][0], inp['w'][0], (c.H, c.W), c.stride, inp['mask'][0])[0].copy()
  odd = dx[:, :, 1::2].copy()
  dx[:, :, 0:2 * odd.shape[2]:2] = odd
  return dx


def _group1_with_group0s_kernel(c, inp):
  return np.maximum(_fwd_pre(c, inp, 1, w=inp['w'][0]), 0)


def _ntile_columns_wrap(c, inp):
  y = np.maximum(_fwd_pre(c, inp, 0), 0)
  y[..., 128:] = y[..., :c.Cout - 128].copy()
  return y


MISTAKES = [
    # name, case, group compared, emulation
    ('symmetric padding where pad_total is odd', 'fwd 1 2 15 16 16 48 2 relu bias ws', 0, _symmetric_padding),
    ('one tap dropped in one parity class', 'dgrad 1 2 21 19 48 16 2 mask ws w wt', 0, _tap_dropped_in_one_class),
    ('last K-step dropped (C % 16 != 0)', 'fwd 1 2 21 19 20 64 1 relu bias ws', 0, _last_kstep_dropped),
    ('bias added once per slab', 'fwd 3 5 9 9 192 256 2 relu bias ws', 0, _bias_per_slab),
    ('ReLU per slab before the sum', 'fwd 3 5 9 9 192 256 2 relu bias ws', 0, _relu_per_slab),
    ('mask >= 0', 'dgrad 1 2 21 19 32 16 2 mask ws w wt', 0, _mask_ge),
    ('ragged last M tile left unwritten (NaN)', 'fwd 1 2 21 19 64 48 2 relu bias ws', 0, _ragged_tile_unwritten(np.nan)),
    ('ragged last M tile left unwritten (zeros)', 'fwd 1 2 21 19 64 48 2 relu bias ws', 0, _ragged_tile_unwritten(0.0)),
    ('a class written to the neighbouring parity', 'dgrad 1 2 21 19 48 16 2 mask ws w wt', 0, _class_to_neighbour_parity),
    ('group 1 with the kernel of group 0', 'fwd 3 5 17 17 128 192 2 relu bias ws', 1, _group1_with_group0s_kernel),
    ('N-tile columns 128.. taken from 0..', 'fwd 3 5 9 9 192 256 2 relu bias ws', 0, _ntile_columns_wrap),
]


@pytest.mark.parametrize('name,text,g,emulate', MISTAKES, ids=[m[0] for m in MISTAKES])
def test_bound_rejects(name, text, g, emulate):
  c = BY_TEXT[text]
  inp, ref, bound, keep, _, _ = R.case_expect(c)
  ref, bound, keep = ref[g], bound[g], keep[g]
  # the comparison of the device test: accepted for the rounded reference ...
  right = f32(ref)
  assert R.within(right[keep], ref[keep], bound[keep])
  # ... and rejected for the mistake
  got = f32(emulate(c, inp))
  assert got.shape == ref.shape
  bad = ~(np.abs(got.astype(np.float64) - ref) <= bound) & keep
  print('%-45s %-42s rejected: %d of %d elements out of bound' % (name, text, int(bad.sum()), bad.size))
  assert not R.within(got[keep], ref[keep], bound[keep])
  assert bad.sum() >= 4       # no mistake hangs on a single lucky element
