"""Every launch variant of the filter gradient (geeco_conv3x3_wgrad) against float64, one small case each.

tests/test_kernels_gpu.py holds this entry point at the models' shapes under atol = 2e-5 sqrt(M), dense tensors, mostly one group.
The cases here come from tests/native/conv_wgrad_cases.txt: the six instantiations of the LDS-staged kernel with one encoder and with
three, the four tiles of the generic kernel with one slab (written straight to dw / db), a few and 18, conv1's kernel with fewer and
with more tiles than slices, the 32 -> 48 halo kernel with one, two and three encoders and in its remainder-block form, both slab-sum
kernels, ragged tiles and slices, db = NULL.  tests/test_conv_wgrad_cover_cpu.py shows on the host that each case runs the variant
recorded beside it and that the list holds every variant the 136 / 144 / 256 models reach and every instantiation the dispatcher
can choose; tests/test_conv_wgrad_refs_cpu.py that the two comparisons used here reject wrong kernels.

Each case runs twice.  Exact pass: x and dz are integers in [-2, 2], every partial sum is an integer below 2**24, so float32 in any
order gives the float64 result and the comparison is equality: a dropped, doubled or misplaced pixel, tap, channel or slab shows at
any M.  Rounding pass: x, dz ~ N(0, 1) under _conv_refs.wgrad_bound, (slice_px + S + 8) U mag: a product path of reduced precision
shows here (small integers are exact in bf16 too).

x, dz, dw, db and the workspace live inside larger allocations of NaN: slack before the first group, between the groups (strides
padded by an odd multiple of 4 floats) and behind the last; the workspace is exactly conv3x3_wgrad_ws_bytes.  A read past a tensor
that enters a product turns up as a NaN in the output, a write past a tensor or one slab too many as slack that is no longer NaN.

Worst share of the rounding bound over the list on an MI355X: see WORST_RATIO_MEASURED below.
"""
import numpy as np
import pytest
import torch

import _conv_refs as R
from test_conv_gemm_variants_gpu import Slab

pytestmark = pytest.mark.gpu

CASES = R.load_wgrad_cases()
# the largest err / bound any case of the list printed on an MI355X (rounding pass, dw and db, every group); recorded, not asserted:
# the assertion is the bound itself
WORST_RATIO_MEASURED = 0.048      # case 1 2 10 20 64 64 2 (dw); the mean over the list is 0.01


def _launch(c, dev, x, dz):
  """One launch of the case into fresh NaN-filled buffers -> (kernel names, slabs)."""
  from geeco_amd import ops
  G, N, H, W, Cin, Cout, s = c.G, c.N, c.H, c.W, c.Cin, c.Cout, c.stride
  Ho, Wo = R.wgrad_out_hw(c)
  ws_bytes = ops.conv3x3_wgrad_ws_bytes(G, N, H, W, Cin, Cout, s)
  assert ws_bytes >= G * c.S * (9 * Cin * Cout + Cout) * 4 and ws_bytes % 16 == 0, ws_bytes
  slabs = dict(x=Slab(dev, G, N * H * W * Cin, x, gap=20), dz=Slab(dev, G, N * Ho * Wo * Cout, dz, gap=12),
               dw=Slab(dev, G, 9 * Cin * Cout, gap=28), db=None if 'nodb' in c.flags else Slab(dev, G, Cout, gap=4),
               ws=Slab(dev, 1, ws_bytes // 4))
  db = slabs['db']
  names = ops.kernel_trace(lambda: ops.conv3x3_wgrad_into(
      slabs['dw'].first, db.first if db else None, slabs['x'].first, slabs['dz'].first, G, slabs['x'].gs, slabs['dz'].gs,
      slabs['dw'].gs, db.gs if db else 0, N, H, W, Cin, Cout, s, slabs['ws'].first))
  torch.cuda.synchronize()
  return names, slabs


def _pass(c, dev, exact):
  x, dz, dw_ref, db_ref, dw_bound, db_bound = R.wgrad_case_expect(c, exact)
  names, slabs = _launch(c, dev, x, dz)
  # the launch is the variant the list records
  assert names == R.wgrad_kernel_names(c), (names, R.wgrad_kernel_names(c))
  outs = [('dw', slabs['dw'], dw_ref, dw_bound)] + ([('db', slabs['db'], db_ref, db_bound)] if slabs['db'] else [])
  worst = 0.0
  for name, slab, ref, bound in outs:
    got = np.stack([slab.group(g).cpu().numpy().reshape(ref.shape[1:]) for g in range(c.G)])
    assert not np.isnan(got).any(), 'NaN in %d elements of %s' % (int(np.isnan(got).sum()), name)
    for g in range(c.G):
      what = '%s: %s, %s of group %d, %s pass' % (c.text, names[0], name, g, 'exact' if exact else 'rounding')
      if exact:
        bad = got[g].astype(np.float64) != ref[g]
        assert not bad.any(), '%s: %d of %d elements differ from the float64 result, the first at %s' % (
            what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]))
      else:
        ratio = R.worst_ratio(got[g], ref[g], bound[g])
        worst = max(worst, ratio)
        print('%s: %.3f of its bound (slice_px = %d, S = %d)' % (what, ratio, c.slice_px, c.S))
        R.assert_within(got[g], ref[g], bound[g], what)
  for name, slab in slabs.items():
    assert slab is None or slab.slack_untouched(), 'the slack around %s is no longer NaN' % name
  for name, src in (('x', x), ('dz', dz)):      # the operands themselves are unchanged
    for g in range(c.G):
      assert np.array_equal(slabs[name].group(g).cpu().numpy(), src[g].reshape(-1)), name
  # run to run: a second launch into fresh NaN-filled buffers gives the same bits
  names2, slabs2 = _launch(c, dev, x, dz)
  assert names2 == names
  for name in ('dw', 'db'):
    assert slabs[name] is None or torch.equal(slabs[name].bits(), slabs2[name].bits()), name
  return worst


@pytest.mark.parametrize('c', CASES, ids=lambda c: c.text.replace(' ', '-'))
def test_wgrad_variant(dev, c):
  _pass(c, dev, exact=True)
  worst = _pass(c, dev, exact=False)
  print('%s: worst share of the rounding bound %.3f' % (c.text, worst))
