"""Every instantiation and launch form of the decoder tail -- fc1, the heads, the losses and their gradients: heads_loss_kernel<SHAPED>,
heads_sample_kernel<FUSE, G, SHAPED>, the finish roles as heads_finish_kernel and as the first blocks of lstm_step_bwd_heads_kernel --
against float64, one small case each.

tests/test_kernels_gpu.py::test_heads_loss, ::test_lstm_step_heads_one_launch_per_sample and tests/test_loss_shaping_gpu.py hold
this code at H = Hfc = 128 (the fused form at no other shape), N <= 64, dense targets, unit-stride weights, N(0, 1) inputs and one
tolerance per tensor.  The cases here come from _tail_refs.CASES: Hfc 64 and 128 with H in {1, 100, 127, 128}; the single-workgroup
kernel at H = 129 and Hfc = 96; N over the 32-sample chunk edges of the finish roles and past 1024 (the second trip of every N
loop and of shaped_counts), up to the 4096 the entry points accept; OT = 32 with a head of 16, OT = 1, a kind-1 head in third
place, two kind-1 heads; the four fused instantiations at H = 128 and 100, finished here or deferred into geeco_lstm_step_bwd,
forward only, with 1, 5 and 18 slabs of the gate product; the models' strided target views and sample weights at stride 3, with
NaN in every column and gap the kernels have no business reading.  tests/test_tail_refs_cpu.py shows on the host that the table
holds these edges, that the inputs are what _tail_refs says and that the comparison used here rejects wrong kernels.

Each case: every output (predictions, losses, every gradient, z / c / h / gates / dz, the workspaces) lives inside a larger
allocation of NaN and starts as NaN; the heads workspace is exactly heads_ws_bytes.  After the launch the slack and the unused
slots of losses[8] hold the bits they held, and so does every input; ops.kernel_trace gives exactly the launch names the case
records; _tail_refs.tail_compare finds no NaN, equality where it asks for equality and every other element under its own bound; a
fused case equals the separate entry points bit for bit; with the batch sums deferred, geeco_lstm_step_bwd's own outputs equal
those of the call without them; a second launch into fresh buffers gives the same bits.

Measured on an MI355X (recorded, not asserted: the assertion is the bound): the worst share of a bound over the list is 0.305, on
the gates of the fused case step_heads-N33-H100-F64-OT12k2102-shaped-D1152-model (expf and the division under the allowances of
_primitive_refs); over the tail's own outputs it is 0.211, on the gradient of the first head kernel of
heads-N1-H128-F128-OT18k20200-shaped-model; the losses use at most 0.099 of theirs, and every lattice prediction is equal.  All
50 cases pass; the whole file takes 2.8 s.
"""
import numpy as np
import pytest
import torch

import _tail_refs as R

pytestmark = pytest.mark.gpu

CASES = R.CASES
# the largest err / bound any case of the list printed on an MI355X, and the file's wall time; recorded, not asserted
WORST_SHARE_MEASURED = 0.305      # gates of step_heads-N33-H100-F64-OT12k2102-shaped-D1152-model; the tail's own outputs: 0.211
WALL_TIME_MEASURED = 2.8          # seconds for the whole file (50 cases, two or three launches of the case each)

LEAD, TAIL = 12, 20      # floats of NaN before and behind every tensor (16-byte steps: the kernels' float4 accesses)
_inputs = {}


def inputs(c):
  if c.index not in _inputs:
    _inputs[c.index] = R.tail_inputs(c)
  return _inputs[c.index]


class Buf:
  """``n`` floats inside one NaN-filled allocation; ``values`` (which may hold NaN themselves) or NaN inside."""

  def __init__(self, dev, n, values=None):
    self.n = n
    self.buf = torch.full((LEAD + n + TAIL,), float('nan'), dtype=torch.float32, device=dev)
    self.t = self.buf[LEAD:LEAD + n]
    if values is not None:
      self.t.copy_(torch.from_numpy(np.ascontiguousarray(values, np.float32).reshape(-1)))
    self.before = self.bits().clone()

  def bits(self):
    return self.buf.view(torch.int32)

  def slack_untouched(self):
    b = self.bits()
    return torch.equal(b[:LEAD], self.before[:LEAD]) and torch.equal(b[LEAD + self.n:], self.before[LEAD + self.n:])

  def unchanged(self):
    return torch.equal(self.bits(), self.before)

  def numpy(self, *shape):
    return self.t.cpu().numpy().reshape(shape)


def _launch(c, dev, separate=False):
  """One launch of the case into fresh buffers -> (launch names, inputs {name: Buf}, outputs {name: Buf}).  ``separate`` (fused
  cases): the entry points the fused form stands for -- geeco_lstm_input_step_fwd, geeco_heads_loss(_shaped)_fwd_bwd,
  geeco_lstm_gates_bwd -- in its place."""
  from geeco_amd import _native, ops
  inp = inputs(c)
  N, H, F = c.N, c.H, c.F
  sizes, kinds, wts = [sz for sz, _, _ in c.heads], [k for _, k, _ in c.heads], [w for _, _, w in c.heads]
  nh, OT = len(sizes), sum(sizes)
  fused = c.entry == 'step_heads'
  ins = dict(w1=Buf(dev, H * F, inp['w1']), b1=Buf(dev, F, inp['b1']))
  for i in range(nh):
    ins['hw%d' % i], ins['hb%d' % i] = Buf(dev, F * sizes[i], inp['hw'][i]), Buf(dev, sizes[i], inp['hb'][i])
  targets, strides = [], []
  for i in range(nh):
    flat, col, stride = R.target_layout(c, inp, i)
    ins['tg%d' % i] = Buf(dev, flat.size, flat)
    targets.append(ins['tg%d' % i].t[col:])
    strides.append(stride)
  shaping = None
  if c.shaping:
    if inp['sw'] is not None:
      ins['sw'] = Buf(dev, (N - 1) * c.sw_stride + 1, R.sample_weight_layout(c, inp))
    if inp['cw'] is not None:
      ins['cw'] = Buf(dev, 3, inp['cw'])
    sw = ins['sw'].t[::c.sw_stride] if 'sw' in ins else None
    assert sw is None or (sw.numel() == N and sw.stride(0) == c.sw_stride)
    shaping = ops.loss_shaping(sw, ins['cw'].t if 'cw' in ins else None, c.shaping['smooth'], [R.DELTA if k == R.HUBER else 0.0 for k in kinds])
  ws_bytes = ops.heads_ws_bytes(N, H, F)
  assert ws_bytes % 16 == 0
  outs = dict(preds=Buf(dev, N * OT), losses=Buf(dev, 8), ws=Buf(dev, ws_bytes // 4))
  grads = {}
  if c.backward:
    outs.update(dw1=Buf(dev, H * F), db1=Buf(dev, F))
    for i in range(nh):
      outs['dhw%d' % i], outs['dhb%d' % i] = Buf(dev, F * sizes[i]), Buf(dev, sizes[i])
    grads = dict(d_fc1_w=outs['dw1'].t, d_fc1_b=outs['db1'].t, d_heads_w=[outs['dhw%d' % i].t for i in range(nh)],
                 d_heads_b=[outs['dhb%d' % i].t for i in range(nh)])
  head_args = ([ins['hw%d' % i].t for i in range(nh)], [ins['hb%d' % i].t for i in range(nh)], sizes, kinds, wts, targets, strides)
  if not fused:
    ins['h'] = Buf(dev, N * H, inp['h'])
    if c.backward:
      outs['dh'] = Buf(dev, N * H)
      grads['dh'] = outs['dh'].t
    names = ops.kernel_trace(lambda: ops.heads_loss_into(outs['preds'].t, outs['losses'].t, ins['h'].t, ins['w1'].t, ins['b1'].t, *head_args,
                                                         1.0, N, H, F, outs['ws'].t, shaping=shaping, **grads))
    torch.cuda.synchronize()
    return names, ins, outs
  D = c.D
  ins.update(x=Buf(dev, N * D, inp['x']), wx=Buf(dev, D * 4 * H, inp['wx']), bias=Buf(dev, 4 * H, inp['bias']))
  gws_bytes = ops.gemm_ws_bytes(N, 4 * H, D)
  assert gws_bytes == (c.S * N * 4 * H * 4 if c.S > 1 else 16), (gws_bytes, c.S)      # the slab count the case records
  outs.update(z=Buf(dev, N * 4 * H), c=Buf(dev, N * H), h=Buf(dev, N * H), gates=Buf(dev, N * 4 * H), gws=Buf(dev, gws_bytes // 4))
  if c.backward:
    outs['dz'] = Buf(dev, N * 4 * H)
  cell = (outs['z'].t, outs['c'].t, outs['h'].t, outs['gates'].t, ins['x'].t, ins['wx'].t, ins['bias'].t, N, H, D, D, 4 * H, outs['gws'].t)
  if separate:
    ops.lstm_input_step_fwd_into(*cell)
    dh = Buf(dev, N * H) if c.backward else None
    ops.heads_loss_into(outs['preds'].t, outs['losses'].t, outs['h'].t, ins['w1'].t, ins['b1'].t, *head_args, 1.0, N, H, F, outs['ws'].t,
                        shaping=shaping, **(dict(grads, dh=dh.t) if c.backward else {}))
    if c.backward:
      ops.lstm_gates_bwd_into(outs['dz'].t, None, outs['gates'].t, None, outs['c'].t, dh.t, None, N, H)
    torch.cuda.synchronize()
    assert dh is None or dh.slack_untouched()
    return [], ins, outs
  pend = _native.HeadsFinish() if c.deferred else None
  names = ops.kernel_trace(lambda: ops.lstm_step_heads_into(
      *cell, outs['preds'].t, outs['losses'].t, ins['w1'].t, ins['b1'].t, *head_args, 1.0, F, outs['ws'].t,
      dz=outs['dz'].t if c.backward else None, pending=pend, shaping=shaping,
      **{k: v for k, v in grads.items()}))
  if c.deferred:
    # the batch sums ride in geeco_lstm_step_bwd's first grid; its own outputs are those of the call without them
    bws = ops.lstm_step_bwd_ws_bytes(N, D, 4 * H)

    def step(tag, pending):
      outs.update({tag + 'dwx': Buf(dev, D * 4 * H), tag + 'dbx': Buf(dev, 4 * H), tag + 'dx': Buf(dev, N * D), tag + 'bws': Buf(dev, bws // 4)})
      return ops.kernel_trace(lambda: ops.lstm_step_bwd_into(outs[tag + 'dwx'].t, outs[tag + 'dbx'].t, outs[tag + 'dx'].t, ins['x'].t,
                                                            outs['dz'].t, ins['wx'].t, N, D, 4 * H, 4 * H, outs[tag + 'bws'].t, pending=pending))
    names = names + step('', pend)
    assert step('plain_', None) == []
    torch.cuda.synchronize()
    for k in ('dwx', 'dbx', 'dx'):
      assert not torch.isnan(outs[k].t).any() and torch.equal(outs[k].bits(), outs['plain_' + k].bits()), k
  torch.cuda.synchronize()
  return names, ins, outs


def _got(c, outs):
  N, H, F = c.N, c.H, c.F
  sizes = [sz for sz, _, _ in c.heads]
  nh, OT = len(sizes), sum(sizes)
  got = dict(preds=outs['preds'].numpy(N, OT), losses=outs['losses'].numpy(8)[:1 + nh])
  if c.backward:
    got.update(dw1=outs['dw1'].numpy(H, F), db1=outs['db1'].numpy(F))
    for i in range(nh):
      got['dhw%d' % i], got['dhb%d' % i] = outs['dhw%d' % i].numpy(F, sizes[i]), outs['dhb%d' % i].numpy(sizes[i])
    if 'dh' in outs:
      got['dh'] = outs['dh'].numpy(N, H)
  if c.entry == 'step_heads':
    got.update(z=outs['z'].numpy(N, 4 * H), c=outs['c'].numpy(N, H), h=outs['h'].numpy(N, H), gates=outs['gates'].numpy(N, 4 * H))
    if c.backward:
      got['dz'] = outs['dz'].numpy(N, 4 * H)
  return got


@pytest.mark.parametrize('c', CASES, ids=lambda c: c.id)
def test_tail_variant(dev, c):
  inp = inputs(c)
  names, ins, outs = _launch(c, dev)
  # the launches are the instantiations the case records, under their exact names
  assert names == c.names, (names, c.names)
  got = _got(c, outs)
  fused = c.entry == 'step_heads'
  ref = R.tail_reference(c, inp, z=got['z'], h=got['h']) if fused else R.tail_reference(c, inp)
  assert set(ref) == set(got), (sorted(ref), sorted(got))
  worst, problems = R.tail_compare(c, got, ref)
  print('%s: %s: worst share of a bound %.4f (%s)' % (c.id, ', '.join(names), max(worst.values()), ', '.join('%s %.3f' % kv for kv in worst.items())))
  assert not problems, c.id + ': ' + '; '.join(problems)
  # nothing written outside the outputs, the unused slots of losses[8] included; the inputs are what they were
  for name, b in outs.items():
    assert b.slack_untouched(), 'the slack around %s is no longer what it was' % name
  nh = len(c.heads)
  lb = outs['losses']
  assert torch.equal(lb.bits()[LEAD + 1 + nh:LEAD + 8], lb.before[LEAD + 1 + nh:LEAD + 8]), 'an unused slot of losses[8] was written'
  for name, b in ins.items():
    assert b.unchanged(), 'the input %s was written' % name
  # the fused form is the separate entry points, bit for bit
  if fused:
    _, _, sep = _launch(c, dev, separate=True)
    for k in got:
      assert torch.equal(outs[k].bits(), sep[k].bits()), 'fused and separate entry points differ in %s' % k
  # run to run: a second launch into fresh buffers gives the same bits
  names2, _, outs2 = _launch(c, dev)
  assert names2 == names
  for k in list(got) + [k for k in ('dwx', 'dbx', 'dx') if k in outs]:
    assert torch.equal(outs[k].bits(), outs2[k].bits()), 'two launches differ in %s' % k
