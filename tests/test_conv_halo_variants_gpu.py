"""Every launch variant of the LDS-staged input gradient (conv_dgrad_lds.hip), the LDS-halo input gradients (conv_halo_s2_bwd.hip)
and the LDS-halo forwards (conv_halo_s2_fwd.hip, conv_halo_conv1.hip) against float64, one small case each.

tests/test_kernels_gpu.py and tests/test_bench_shapes_gpu.py hold these kernels under rtol = atol = 2e-5 on dense tensors, mostly
with one group, check the launched kernel by its name's prefix and the sign-field paths only against the float-mask path of the same
kernel.  The cases here come from tests/native/conv_halo_cases.txt: all ten instantiations; the three LDS-staged gradients with one
round and with blocks that take a second item across a ci-block and an encoder boundary; the halo kernels with exact and ragged
tiles, ranges across frames and encoders, blocks with an empty range and reserved CUs; every mask form (float mask, uint16 / byte
sign fields packed on the host, none; forward: plain, sign fields, conv1's sign words, the RGB kernel variable).
tests/test_conv_halo_cover_cpu.py shows on the host that each case runs the variant recorded beside it and that the list holds every
variant the 136 / 144 / 256 models reach; tests/test_conv_halo_refs_cpu.py that the two comparisons used here reject wrong kernels.

Each case runs twice.  Exact pass: operands are integers in [-2, 2] (bias [-3, 3], mask {-1, 0, 1}), every sum is an integer of at
most 4099, so float32 in any order gives the float64 result and the comparison is equality: a dropped or misplaced tap, pixel,
channel, chunk or item shows at any size.  Rounding pass: N(0, 1) inputs under _conv_refs.conv_bound(mag, terms, S = 1): a product
path of reduced precision shows here (small integers are exact in bf16 too).

Operands, output, mask, fields and words live inside larger allocations: NaN (integers: the byte 0xA5) before the first group,
between the groups (padded, distinct strides) and behind the last; the padded planes of the uint16 fields hold set bits outside the
image.  A read past a tensor that enters a product turns up as a NaN in the output, a write past a ragged tile as slack that is no
longer what it was.

Worst share of the rounding bound over the list on an MI355X: see WORST_RATIO_MEASURED below.
"""
import numpy as np
import pytest
import torch

import _conv_refs as R
from test_conv_gemm_variants_gpu import IntSlab, Slab

pytestmark = pytest.mark.gpu

CASES = R.load_halo_cases(device_only=True)
# the largest err / bound any case of the list printed on an MI355X (rounding pass, every group); recorded, not asserted: the
# assertion is the bound itself
WORST_RATIO_MEASURED = 0.153      # case dgrad 3 130 16 16 64 32 2 (one-tap class, 32-term sums); the mean over the list is 0.07


def _field_values(c, pos):
  """The sign fields of a gradient case's mask tensor as the entry point wants them, packed on the host: uint16 planes padded to
  whole 8 x 64 tiles with every bit set outside the image (a read of the padding that reached dx would show), or byte fields."""
  if c.family == 'halo':
    Hp, Wp = R.tiles_8x64(c.H, c.W)
    return R.pad_planes(R.pack_fields16(pos), Hp, Wp, 0xFFFF)
  return R.pack_fields8(pos)


def _launch(c, dev, inp, form):
  """One launch of the case into fresh buffers -> (kernel names, slabs)."""
  from geeco_amd import ops
  G, N, H, W, Cin, Cout, s = c.G, c.N, c.H, c.W, c.Cin, c.Cout, c.stride
  Ho, Wo = R.halo_out_hw(c)
  w = Slab(dev, G, inp['w'][0].size, inp['w'])
  slabs = {'w': w}
  if c.dir == 'dgrad':
    dz = Slab(dev, G, N * Ho * Wo * Cout, inp['dz'], gap=20)
    dx = Slab(dev, G, N * H * W * Cin, gap=28)
    slabs.update(dz=dz, out=dx)
    if form == 'fields':
      vals = _field_values(c, inp['mask'] > 0)
      if c.family == 'halo':
        assert vals[0].size == ops.relu_fields_elems(N, H, W)
        f = IntSlab(dev, G, vals[0].size, torch.int16, vals, gap=20)
        run = lambda: ops.conv3_dgrad_relu_fields_into(dx.first, dz.first, w.first, f.first, G, dz.gs, w.gs, f.gs, dx.gs, N, H, W,
                                                       reserved_cus=c.reserved)
      else:
        assert ops.conv3x3_dgrad_relu_fields_supported(H, W, Cin, Cout, s)
        f = IntSlab(dev, G, vals[0].size, torch.uint8, vals, gap=20)
        run = lambda: ops.conv3x3_dgrad_relu_fields_into(dx.first, dz.first, w.first, f.first, G, dz.gs, w.gs, f.gs, dx.gs, N, H, W,
                                                         Cin, Cout, s)
      slabs.update(fields=f)
    else:
      # the float mask shares the output's group stride (one gs_dx in the entry point)
      mask = Slab(dev, G, N * H * W * Cin, inp['mask'], gap=28) if form == 'mask' else None
      assert not ops.conv3x3_dgrad_needs_wt(H, W, Cin, Cout, s)
      slabs.update(mask=mask)
      run = lambda: ops.conv3x3_dgrad_into(dx.first, dz.first, None, mask.first if mask else None, G, dz.gs, 0, dx.gs, N, H, W, Cin,
                                           Cout, s, ws=None, w=w.first, gs_w=w.gs)
  else:
    x = Slab(dev, G, N * H * W * Cin, inp['x'], gap=20)
    b = Slab(dev, G, Cout, inp['b'], gap=4)
    y = Slab(dev, G, N * Ho * Wo * Cout, gap=28)
    slabs.update(x=x, b=b, out=y)
    args = (x.first, w.first, b.first, G, x.gs, w.gs, b.gs, y.gs)
    if form == 'plain':
      run = lambda: ops.conv3x3_fwd_into(y.first, x.first, w.first, b.first, G, x.gs, w.gs, b.gs, y.gs, N, H, W, Cin, Cout, s,
                                         relu='relu' in c.flags, ws=None)
    elif form == 'bits':
      f = IntSlab(dev, G, N * ops.relu_bits_rows(H) * ops.relu_bits_pitch(W), torch.int32, gap=20)
      fn = ops.conv1_fwd_relu_bits_rgb_into if 'rgb' in c.flags else ops.conv1_fwd_relu_bits_into
      run = lambda: fn(y.first, f.first, *args, f.gs, N, H, W)
      slabs.update(fields=f)
    elif Cin == 32:
      f = IntSlab(dev, G, ops.relu_fields_elems(N, Ho, Wo), torch.int16, gap=20)
      run = lambda: ops.conv2_fwd_relu_fields_into(y.first, f.first, *args, f.gs, N, H, W)
      slabs.update(fields=f)
    else:
      f = IntSlab(dev, G, N * Ho * Wo * (Cout // 8), torch.uint8, gap=20)
      run = lambda: ops.conv3_fwd_relu_fields_into(y.first, f.first, *args, f.gs, N, H, W)
      slabs.update(fields=f)
  names = ops.kernel_trace(run)
  torch.cuda.synchronize()
  return names, slabs


def _out(c, slabs, shape):
  return np.stack([slabs['out'].group(g).cpu().numpy().reshape(shape) for g in range(c.G)])


def _fwd_fields_expected(c, pos, fill):
  """What the forward's field / word slab holds for the signs ``pos`` [G][N][Ho][Wo][Cout]: only real pixels are written, the
  padding of the planes keeps the slab's pattern."""
  Ho, Wo = R.halo_out_hw(c)
  if R.halo_form(c) == 'bits':
    return R.pad_planes(R.pack_bits32(pos), *R.tiles_8x64(Ho, Wo), np.uint32(fill & 0xFFFFFFFF))
  if c.Cin == 32:
    return R.pad_planes(R.pack_fields16(pos), *R.tiles_8x64(Ho, Wo), np.uint16(fill & 0xFFFF))
  return R.pack_fields8(pos)


def _pass(c, dev, exact):
  form = R.halo_form(c)
  inp, ref, bound, keep = R.halo_case_expect(c, exact)
  if c.dir == 'fwd' and 'relu' in c.flags:
    assert R.left_out(keep) < R.LEFT_OUT_MAX, R.left_out(keep)
  names, slabs = _launch(c, dev, inp, form)
  # the launch is the variant the list records, under its exact name
  assert names == [c.inst], (names, c.inst)
  got = _out(c, slabs, ref.shape[1:])
  # no NaN (every output starts as NaN); equality (exact pass) or the bound; masked elements +0.0 bit for bit: halo_compare, which
  # tests/test_conv_halo_refs_cpu.py holds against emulated wrong kernels
  worst, problems = R.halo_compare(c, exact, got, inp, ref, bound, keep)
  what = '%s: %s, %s pass' % (c.text, names[0], 'exact' if exact else 'rounding')
  if not exact:
    print('%s: %.3f of its bound (%.4f %% left out)' % (what, worst, 100 * R.left_out(keep)))
  assert not problems, what + ': ' + '; '.join(problems)
  if c.dir == 'fwd' and 'fields' in slabs:
    f = slabs['fields']
    have = np.stack([f.group(g).cpu().numpy() for g in range(c.G)])
    have = have.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[have.itemsize])
    # the packed signs of the device's own y everywhere (and the slab's pattern in the planes' padding) ...
    own = _fwd_fields_expected(c, got > 0, f.fill).reshape(c.G, -1)
    assert np.array_equal(have, own), '%s: %d fields / words differ from the signs of y' % (c.text, int((have != own).sum()))
    # ... and the reference's sign wherever that is determined
    assert np.array_equal((got > 0)[keep], (ref > 0)[keep]), c.text
  for name, slab in slabs.items():
    assert slab is None or slab.slack_untouched(), 'the slack around %s is no longer what it was' % name
  for name in ('x', 'w', 'b', 'dz', 'mask'):      # the operands themselves are unchanged
    if slabs.get(name) is not None:
      for g in range(c.G):
        assert np.array_equal(slabs[name].group(g).cpu().numpy(), np.ascontiguousarray(inp[name][g]).reshape(-1)), name
  if c.dir == 'dgrad' and form == 'fields':
    vals = _field_values(c, inp['mask'] > 0)
    for g in range(c.G):
      assert np.array_equal(slabs['fields'].group(g).cpu().numpy().view(vals.dtype), vals[g].reshape(-1)), 'fields'
    # the mask path of the same kernel family stores the same bits as the fields path, on the whole output
    names_m, slabs_m = _launch(c, dev, inp, 'mask')
    assert len(names_m) == 1 and names_m[0].split('<')[0] == c.inst.split('<')[0], names_m
    assert torch.equal(slabs['out'].bits(), slabs_m['out'].bits()), '%s: the fields and the mask path differ' % c.text
  # run to run: a second launch into fresh buffers gives the same bits
  names2, slabs2 = _launch(c, dev, inp, form)
  assert names2 == names
  assert torch.equal(slabs['out'].bits(), slabs2['out'].bits())
  if c.dir == 'fwd' and 'fields' in slabs:
    assert torch.equal(slabs['fields'].bits(), slabs2['fields'].bits())
  return worst


@pytest.mark.parametrize('c', CASES, ids=lambda c: c.text.replace(' ', '-'))
def test_halo_variant(dev, c):
  _pass(c, dev, exact=True)
  worst = _pass(c, dev, exact=False)
  print('%s: worst share of the rounding bound %.3f' % (c.text, worst))
