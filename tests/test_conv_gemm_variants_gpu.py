"""Every launch variant of the gather GEMM (geeco_amd/csrc/conv_gemm.hip) against float64, one small case each.

tests/test_kernels_gpu.py reaches this kernel only through ops.conv3x3 / ops.conv3x3_dgrad (one group, dense tensors) and runs the
64 x 64, 128 x 16 and one 64 x 96 tile there.  The cases here come from tests/native/conv_gemm_cases.txt: all seven tile
instantiations forward and with four parity classes, UT true and false, split factors 2..18, the HWIO and the transposed B operand,
rotated and unrotated class order, strides 3 and 4, G > 1 with padded group strides, the missing-workspace fallback, H = 1 and
W = 1.  tests/test_conv_cover_cpu.py shows on the host that each case runs the variant recorded beside it and that the list holds
every variant the 136 / 144 / 256 models reach; tests/test_conv_refs_cpu.py that the bound used here rejects wrong kernels.

Every operand, the output and the workspace live inside a larger allocation of NaN: slack before the first group, between the
groups and behind the last.  A read past a tensor that enters a product turns up as a NaN in the output, a write past a ragged
tile or one slab too many as slack that is no longer the NaN it was.
"""
import numpy as np
import pytest
import torch

import _conv_refs as R

pytestmark = pytest.mark.gpu

CASES = R.load_cases()
NAN_BITS = int(np.array([np.nan], np.float32).view(np.int32)[0])
LEAD, TAIL = 12, 20      # floats of slack before the first group and behind the last (16-byte steps: the kernel's float4 accesses)


class Slab:
  """[G] tensors of ``size`` floats each at group stride size + an odd multiple of 4 floats, inside one NaN-filled allocation."""

  def __init__(self, dev, G, size, values=None, gap=12):
    assert size % 4 == 0 and gap % 8 == 4
    self.G, self.size, self.gs = G, size, size + gap
    self.buf = torch.full((LEAD + G * self.gs - gap + TAIL,), float('nan'), dtype=torch.float32, device=dev)
    self.first = self.buf[LEAD:]      # what the entry point is given
    self.inside = torch.zeros(self.buf.numel(), dtype=torch.bool, device=dev)
    for g in range(G):
      self.inside[LEAD + g * self.gs:LEAD + g * self.gs + size] = True
      if values is not None:
        self.group(g).copy_(torch.from_numpy(np.ascontiguousarray(values[g]).reshape(-1)))

  def group(self, g):
    return self.buf[LEAD + g * self.gs:LEAD + g * self.gs + self.size]

  def slack_untouched(self):
    return bool((self.buf.view(torch.int32)[~self.inside] == NAN_BITS).all())

  def bits(self):
    return self.buf.view(torch.int32)


class IntSlab:
  """Slab for sign fields and sign words (uint8 as torch.uint8, uint16 as torch.int16, uint32 as torch.int32): [G] tensors of
  ``size`` elements each at group stride size + gap.  There is no NaN for integers: the slack, and every element a launch has not
  written, is the byte pattern 0xA5."""
  FILL = 0xA5

  def __init__(self, dev, G, size, dtype, values=None, gap=12):
    self.G, self.size, self.gs = G, size, size + gap
    self.buf = torch.empty(LEAD + G * self.gs - gap + TAIL, dtype=dtype, device=dev)
    self.buf.view(torch.uint8).fill_(self.FILL)
    self.fill = int(self.buf[0])      # the pattern as one element of dtype
    self.first = self.buf[LEAD:]
    self.inside = torch.zeros(self.buf.numel(), dtype=torch.bool, device=dev)
    for g in range(G):
      self.inside[LEAD + g * self.gs:LEAD + g * self.gs + size] = True
      if values is not None:
        v = np.ascontiguousarray(values[g]).reshape(-1)
        self.group(g).copy_(torch.from_numpy(v.view({1: np.uint8, 2: np.int16, 4: np.int32}[v.itemsize])))

  def group(self, g):
    return self.buf[LEAD + g * self.gs:LEAD + g * self.gs + self.size]

  def slack_untouched(self):
    return bool((self.buf[~self.inside] == self.fill).all())

  def bits(self):
    return self.buf


def _launch(c, dev, inp):
  """One launch of the case into fresh NaN-filled buffers -> (kernel names, output slab, every slab, workspace bytes asked for)."""
  from geeco_amd import ops
  G, N, H, W, Cin, Cout, s = c.G, c.N, c.H, c.W, c.Cin, c.Cout, c.stride
  Ho, Wo = R.out_hw(c)
  dims = (G, N, H, W, Cin, Cout, s)
  ws_bytes = (ops.conv3x3_fwd_ws_bytes if c.dir == 'fwd' else ops.conv3x3_dgrad_ws_bytes)(*dims)
  ws = Slab(dev, 1, ws_bytes // 4) if 'ws' in c.flags and ws_bytes else None
  w = Slab(dev, G, 9 * Cin * Cout, inp['w'])
  slabs = {'w': w, 'ws': ws}
  if c.dir == 'fwd':
    x = Slab(dev, G, N * H * W * Cin, inp['x'], gap=20)
    b = Slab(dev, G, Cout, inp['b'], gap=4) if inp['b'] is not None else None
    y = Slab(dev, G, N * Ho * Wo * Cout, gap=28)
    slabs.update(x=x, b=b, out=y)
    run = lambda: ops.conv3x3_fwd_into(y.first, x.first, w.first, b.first if b else None, G, x.gs, w.gs, b.gs if b else 0, y.gs,
                                       N, H, W, Cin, Cout, s, relu='relu' in c.flags, ws=ws.first if ws else None)
  else:
    dz = Slab(dev, G, N * Ho * Wo * Cout, inp['dz'], gap=20)
    dx = Slab(dev, G, N * H * W * Cin, gap=28)
    # the mask shares the output's group stride (one gs_dx in the entry point)
    mask = Slab(dev, G, N * H * W * Cin, inp['mask'], gap=28) if inp['mask'] is not None else None
    # the per-tap transposed copy [3][3][Cout][Cin], made on the host
    wt = Slab(dev, G, 9 * Cin * Cout, inp['w'].transpose(0, 1, 2, 4, 3), gap=4) if 'wt' in c.flags else None
    slabs.update(dz=dz, out=dx, mask=mask, wt=wt)
    hwio = 'w' in c.flags
    run = lambda: ops.conv3x3_dgrad_into(dx.first, dz.first, wt.first if wt else None, mask.first if mask else None, G, dz.gs,
                                         wt.gs if wt else 0, dx.gs, N, H, W, Cin, Cout, s, ws=ws.first if ws else None,
                                         w=w.first if hwio else None, gs_w=w.gs if hwio else 0)
  names = ops.kernel_trace(run)
  torch.cuda.synchronize()
  return names, slabs['out'], slabs, ws_bytes


@pytest.mark.parametrize('c', CASES, ids=R.case_id)
def test_gather_gemm_variant(dev, c):
  from geeco_amd import ops
  if c.dir == 'dgrad' and c.Cout % 16 != 0:
    assert ops.conv3x3_dgrad_needs_wt(c.H, c.W, c.Cin, c.Cout, c.stride)
  inp, ref, bound, keep, _, _ = R.case_expect(c)
  assert R.left_out(keep) < R.LEFT_OUT_MAX, R.left_out(keep)
  Ho, Wo = R.out_hw(c)
  Hd, Wd, Nout = (Ho, Wo, c.Cout) if c.dir == 'fwd' else (c.H, c.W, c.Cin)

  names, out, slabs, ws_bytes = _launch(c, dev, inp)
  # the launch is the variant the list records
  want = [R.kernel_name(c)] + (['conv_splitk_epilogue_kernel'] if c.S > 1 else [])
  assert names == want, (names, want)
  assert ('ws' in c.flags) or c.S == 1
  assert ws_bytes == (c.planS * c.G * c.N * Hd * Wd * Nout * 4 if c.planS > 1 else 0), ws_bytes

  got = np.stack([out.group(g).cpu().numpy().reshape(ref.shape[1:]) for g in range(c.G)])
  assert not np.isnan(got).any(), 'NaN in %d elements' % int(np.isnan(got).sum())
  for g in range(c.G):
    k = keep[g]
    what = '%s: %s group %d' % (c.text, names[0], g)
    print('%s: %.3f of its bound (S = %d, %.4f %% left out)' % (
        what, R.worst_ratio(got[g][k], ref[g][k], np.where(bound[g][k] > 0, bound[g][k], 1e-300)), c.S, 100 * R.left_out(k)))
    R.assert_within(got[g][k], ref[g][k], bound[g][k], what)
  for name, slab in slabs.items():
    assert slab is None or slab.slack_untouched(), 'the slack around %s is no longer NaN' % name
  for name in ('x', 'w', 'b', 'dz', 'mask', 'wt'):      # the operands themselves are unchanged
    slab = slabs.get(name)
    if slab is not None:
      src = inp['w'].transpose(0, 1, 2, 4, 3) if name == 'wt' else inp[name]
      for g in range(c.G):
        assert np.array_equal(slab.group(g).cpu().numpy(), np.ascontiguousarray(src[g]).reshape(-1)), name

  # run to run: a second launch into fresh NaN-filled buffers gives the same bits
  names2, out2, _, _ = _launch(c, dev, inp)
  assert names2 == names
  assert torch.equal(out.bits(), out2.bits())
