"""Every instantiation and launch form of the fused encoder-bottom backward (conv2_dgrad_conv1_wgrad_kernel<CREAL, BITS>: conv2's
input gradient, ReluGrad and conv1's filter / bias gradient in one kernel) against float64, one small case each.

tests/test_kernels_gpu.py and tests/test_bench_shapes_gpu.py hold this kernel on dense tensors under atol = 2e-5 sqrt(N H W), far
above one dropped pixel or tap, and the sign-word kernels only bitwise against the float-mask kernels of the same template.  The
cases here come from tests/native/conv_bottom_cases.txt: all four instantiations at exact tiles and at tiles ragged in both
directions; ranges of two and three tiles across frames; one, two and three encoders; blocks with an empty range; the
remainder-block form with one, two and four tiles per segment, also reached through reserved CUs; the plain, the deferred and the
sign-word entry points; dz1 stored or not.  tests/test_conv_bottom_cover_cpu.py shows on the host that each case runs the form
recorded beside it and that the list holds every form the 136 / 144 / 256 models reach; tests/test_conv_bottom_refs_cpu.py that
the two comparisons used here reject wrong kernels.

Each case runs twice.  Exact pass: x, w2 and the mask in {-1, 0, 1}, dz2 integers in [-2, 2]: |dz1| <= 384 and every partial sum of
dw1 / db1 is an integer below 2**24, so float32 in any order gives the float64 result and the comparison of dw1, db1 and dz1 is
equality: a dropped or misplaced tap, pixel, column, sign bit, tile, segment or slab shows at any size.  The sign-word and the
float-mask form of one shape share their inputs, so both equal the same reference.  Rounding pass: N(0, 1) operands under
_conv_refs.bottom_case_expect's bound: a product path of reduced precision shows here (small integers are exact in bf16 too).
The mask is data with about half its entries not > 0, and the sign words are packed from it on the host: no element is left out.

dz2, w2, x, dw1, db1, dz1 and the workspace live inside larger allocations of NaN: slack before the first group, between the
groups (padded, distinct strides; y1 and dz1 share one, as in the entry point) and behind the last; the workspace is exactly
conv2_dgrad_conv1_wgrad_ws_bytes and starts as NaN, as do dw1, db1 and dz1.  A NaN in the mask would compare false and hide a
stray read: the slack around y1 is 1e30.  The sign words are zero in the padding of their planes (the entry point's contract) and
the byte 0xA5 around the planes.  A read past a tensor turns up as a NaN (or a wrong sign) in the output, a write past a ragged
tile or one slab too many as slack that is no longer what it was, a slab of an empty block that was left unwritten as a NaN in dw1.

Measured on an MI355X (recorded, not asserted): the worst share of a rounding bound over the list is 0.082, on dz1 (48- to 192-term
sums) of case 3 64 10 66 3 mask dz1; dw1 uses at most 0.0005 and db1 0.0003 of theirs (sums of thousands of terms under a worst-case
count: what holds dw1 / db1 to the pixel is the exact pass).  Every case passes both passes; the whole file takes 5.1 s.
"""
import numpy as np
import pytest
import torch

import _conv_refs as R
from test_conv_gemm_variants_gpu import IntSlab, Slab

pytestmark = pytest.mark.gpu

CASES = R.load_bottom_cases()
# the largest err / bound any case of the list printed on an MI355X (rounding pass, dw1, db1 and dz1, every group); recorded, not
# asserted: the assertion is the bound itself
WORST_RATIO_MEASURED = 0.082      # case 3 64 10 66 3 mask dz1 (dz1); dw1 at most 0.0005 (1 2 16 64 4 ...), db1 at most 0.0003
WALL_TIME_MEASURED = 5.1          # seconds for the whole file (20 cases, two passes and four launches each)


class MaskSlab(Slab):
  """Slab whose slack is a large positive value: a stray read of it turns a ReluGrad on where NaN would turn it off unseen."""
  SLACK = 1e30

  def __init__(self, dev, G, size, values, gap):
    super().__init__(dev, G, size, values, gap=gap)
    self.buf[~self.inside] = self.SLACK

  def slack_untouched(self):
    return bool((self.buf[~self.inside] == self.SLACK).all())


def _launch(c, dev, e):
  """One launch of the case into fresh buffers -> (kernel names, slabs)."""
  from geeco_amd import ops
  G, N, H, W, C = c.G, c.N, c.H, c.W, c.C
  ws_bytes = ops.conv2_dgrad_conv1_wgrad_ws_bytes(G)
  # slabs of 9 C 32 + 32 floats in a workspace sized for C = 4 and every CU
  assert ws_bytes >= G * c.S * (9 * 4 * 32 + 32) * 4 and ws_bytes % 16 == 0, ws_bytes
  slabs = dict(dz2=Slab(dev, G, N * (H // 2) * (W // 2) * 48, e['dz2'], gap=20), w2=Slab(dev, G, 9 * 32 * 48, e['w2'], gap=12),
               x=Slab(dev, G, N * H * W * 4, e['x'], gap=28), dw=Slab(dev, G, 9 * C * 32, gap=36), db=Slab(dev, G, 32, gap=4),
               ws=Slab(dev, 1, ws_bytes // 4))
  dz2, w2, x, dw, db, ws = (slabs[k] for k in ('dz2', 'w2', 'x', 'dw', 'db', 'ws'))
  pending = [] if 'pending' in c.flags else None
  if 'bits' in c.flags:
    Hp, Wp = ops.relu_bits_rows(H), ops.relu_bits_pitch(W)
    assert (Hp, Wp) == R.tiles_8x64(H, W)
    planes = R.bottom_bits_planes(c, e['mask'])
    bits = slabs['bits'] = IntSlab(dev, G, N * Hp * Wp, torch.int32, planes, gap=52)
    run = lambda: ops.conv2_dgrad_conv1_wgrad_bits_into(dw.first, db.first, dz2.first, w2.first, bits.first, x.first, G, dz2.gs, w2.gs,
                                                        bits.gs, x.gs, dw.gs, db.gs, N, H, W, ws.first, real_channels=C,
                                                        pending=pending, reserved_cus=c.reserved)
  else:
    # y1 and dz1 share one group stride (gs_y1 in the entry point)
    y1 = slabs['y1'] = MaskSlab(dev, G, N * H * W * 32, e['mask'], gap=44)
    dz1 = slabs['dz1'] = Slab(dev, G, N * H * W * 32, gap=44) if 'dz1' in c.flags else None
    run = lambda: ops.conv2_dgrad_conv1_wgrad_into(dw.first, db.first, dz2.first, w2.first, y1.first, x.first, G, dz2.gs, w2.gs, y1.gs,
                                                   x.gs, dw.gs, db.gs, N, H, W, ws.first, dz1=dz1.first if dz1 else None,
                                                   real_channels=C, pending=pending, reserved_cus=c.reserved)
  names = ops.kernel_trace(run)
  torch.cuda.synchronize()
  if pending is not None:
    # the deferred form: one slab sum recorded, dw1 / db1 not written yet; ops.slab_reduce_batch finishes it
    assert len(pending) == 1 and pending[0].S == c.S, (len(pending), c.S)
    assert bool(torch.isnan(dw.buf).all()) and bool(torch.isnan(db.buf).all()), 'the deferred form wrote dw1 / db1 itself'
    names_sum = ops.kernel_trace(lambda: ops.slab_reduce_batch(pending))
    torch.cuda.synchronize()
    assert names_sum == ['wgrad_reduce_batch_kernel'], names_sum
  return names, slabs


def _groups(c, slab, shape):
  return np.stack([slab.group(g).cpu().numpy().reshape(shape) for g in range(c.G)])


def _pass(c, dev, exact):
  e = R.bottom_case_expect(c, exact)
  names, slabs = _launch(c, dev, e)
  # the launch is the instantiation the list records, under its exact name, and the slab sum behind it
  assert names == R.bottom_kernel_names(c), (names, R.bottom_kernel_names(c))
  got = dict(dw=_groups(c, slabs['dw'], (3, 3, c.C, 32)), db=_groups(c, slabs['db'], (32,)))
  if slabs.get('dz1') is not None:
    got['dz1'] = _groups(c, slabs['dz1'], (c.N, c.H, c.W, 32))
  # no NaN (every output and the workspace start as NaN); equality (exact pass) or the bound, on every element: bottom_compare,
  # which tests/test_conv_bottom_refs_cpu.py holds against emulated wrong kernels
  worst, problems = R.bottom_compare(c, exact, got, e)
  what = '%s: %s, %s pass' % (c.text, names[0], 'exact' if exact else 'rounding')
  if not exact:
    print('%s: %s of its bounds (slice_px = %d, S = %d)' % (what, ', '.join('%s %.4f' % kv for kv in worst.items()), c.slice_px, c.S))
  assert not problems, what + ': ' + '; '.join(problems)
  for name, slab in slabs.items():
    assert slab is None or slab.slack_untouched(), 'the slack around %s is no longer what it was' % name
  # the operands themselves are unchanged
  for name, src in (('dz2', e['dz2']), ('w2', e['w2']), ('x', e['x']), ('y1', e['mask'])):
    if slabs.get(name) is not None:
      for g in range(c.G):
        assert np.array_equal(slabs[name].group(g).cpu().numpy(), np.ascontiguousarray(src[g]).reshape(-1)), name
  if 'bits' in slabs:
    planes = R.bottom_bits_planes(c, e['mask'])
    for g in range(c.G):
      assert np.array_equal(slabs['bits'].group(g).cpu().numpy().view(np.uint32), planes[g].reshape(-1)), 'bits'
  # run to run: a second launch into fresh buffers gives the same bits
  names2, slabs2 = _launch(c, dev, e)
  assert names2 == names
  for name in ('dw', 'db', 'dz1'):
    assert slabs.get(name) is None or torch.equal(slabs[name].bits(), slabs2[name].bits()), name
  return worst


@pytest.mark.parametrize('c', CASES, ids=lambda c: c.text.replace(' ', '-'))
def test_bottom_variant(dev, c):
  _pass(c, dev, exact=True)
  worst = _pass(c, dev, exact=False)
  print('%s: worst share of a rounding bound %.4f' % (c.text, max(worst.values())))
