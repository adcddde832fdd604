"""Every instantiation and launch form of the input-gradient pass (csrc/input_grad.hip: conv1_dgrad_kernel<3 | 4>,
pack_pixels_bwd_kernel, dynimg_bwd_reduce_kernel<4 | 1> / dynimg_bwd_apply_kernel<4 | 1>) against float64, one small case each, and
the chunk loop of ConvEncoderStack.input_gradient.

tests/test_input_grad_gpu.py holds this code at dense, 16-byte aligned layouts whose HW * C is a multiple of 4 (so only <4> of the
dynimg kernels), with ``rel_max`` / ``rel_l2`` relative to the largest element (the two extremum elements of a sample, tens of times
an ordinary one) and at the default chunk of 96 frames against at most 6.  The cases here come from _input_grad_ref.CASES: conv1 over
the 8 x 32 tile's edges with padded, shared and zero group strides and a small-integer case; the pack adjoint over (C1, C2, Cpad),
the 256-pixel block edge, null outputs and the four accumulate combinations; the dynimg adjoint in <1> for every reason on its own
(the same values through <4> as well), 1 / 2 / 5 blocks per sample, extrema planted in named blocks, ties inside and across blocks,
the flat sample, K in {1, 2, 3, 4, 16, 64}, (C, Cpad) up to (4, 8), N = 3, and the two-frame form with either output null.
tests/test_input_grad_cover_cpu.py shows on the host that the table holds these edges and that the comparison rejects wrong kernels.

Each case: every output lives inside a larger allocation of NaN (gaps of a strided layout included); overwriting outputs start as
NaN, accumulating ones from random values; the dynimg workspace is exactly geeco_dynimg_bwd_ws_bytes.  After the launch the slack,
the gaps, the workspace past its N * nblk * 8 records and every input hold the bits they held; _input_grad_ref.input_grad_compare
finds no NaN, equality where it asks for it and every other element under its own derived bound; a second launch into fresh buffers
gives the same bits; an accumulating launch is start + the overwriting result, one float32 addition, bitwise; a sample of an N = 3
launch is bitwise what it is when launched alone.

The recomputed extrema.  input_grad.hip promises that "the positions of min / max are the forward's": the records left in the
workspace give the backward's mn / mx per sample, and they equal -- bitwise -- the extrema of D formed on the host with the forward's
chain.  That chain is FUSED: dynimg.hip's ``acc += w * v`` and input_grad.hip's ``D += w * v`` are both compiled under hipcc's default
-ffp-contract=fast into v_fma_f32 / v_fmac_f32 / v_pk_fma_f32 (no v_mul_f32 + v_add_f32 pair in either accumulation loop), i.e.
acc = 0; acc = fma(alpha_t, x_t, acc).  Checked in every dynimg case, the two with nothing planted included.

The chunked pass: conv2's input gradient at these shapes is the LDS-halo kernel (one tile of one frame per output pixel, no split
over K), and where it declines, the gather GEMM whose plan (conv_gemm_plan.h: conv_plan) splits K only at nk >= 16 K-steps -- conv2's
input gradient has at most 4 taps x 48 channels = 12 -- so no launch parameter that touches a sum depends on the chunk's frame
count, and geeco_conv1_dgrad gives one block per tile per frame.  Chunked results are therefore asserted BITWISE equal to the
one-chunk result, besides passing the oracle comparison of test_input_gradients_whole_graph at its tolerance.

Measured on an MI355X (recorded, not asserted: the assertion is the bound): the worst share of a bound over the table is 0.260, on
dynimg-v4-5blocks-ragged-min-in-last; every dynimg case with K = 4 sits near 0.25 (the ordinary elements: one correctly rounded
division and one product against the DIV_U + 1 = 6 U allowed, plus r's share), the two-frame cases near 0.15, K = 64 at 0.04 (r's own
gamma(K) term dominates its bound); conv1 uses at most 0.015 of its worst-case chain bound; the pack adjoint and the integer cases are
equal.  All 75 cases and the six whole-graph tests pass; the whole file takes 3.4 s (tests/test_input_grad_gpu.py: 3.8 s).
"""
import numpy as np
import pytest
import torch

import _input_grad_ref as R
import _relu_taps as T
import test_input_grad_gpu as G
from oracle import geeco_oracle as O

pytestmark = pytest.mark.gpu

CONV = [c for c in R.CASES if c.entry == 'conv1']
PACK = [c for c in R.CASES if c.entry == 'pack']
DYN = [c for c in R.CASES if c.entry == 'dynimg']
# the largest err / bound any case of the table printed on an MI355X, and the file's wall time; recorded, not asserted
WORST_SHARE_MEASURED = 0.2598     # dynimg-v4-5blocks-ragged-min-in-last; conv1: 0.0145 (conv1-17x65-cin4-F2-shared_w); pack: equal
WALL_TIME_MEASURED = 3.4          # seconds for the whole file (81 tests; tests/test_input_grad_gpu.py alone: 3.8 s in the same run)

LEAD, TAIL = 12, 20      # floats of NaN before and behind every tensor (16-byte steps: the kernels' float4 accesses)
_inputs = {}


def inputs(c):
  if c.index not in _inputs:
    _inputs[c.index] = R.input_grad_inputs(c)
  return _inputs[c.index]


class Buf:
  """``n`` floats inside one NaN-filled allocation; ``values`` (which may hold NaN themselves: the gaps of a layout) or NaN inside."""

  def __init__(self, dev, n, values=None):
    self.n = n
    self.buf = torch.full((LEAD + n + TAIL,), float('nan'), dtype=torch.float32, device=dev)
    self.t = self.buf[LEAD:LEAD + n]
    assert self.t.data_ptr() % 16 == 0
    if values is not None:
      self.t.copy_(torch.from_numpy(np.ascontiguousarray(values, np.float32).reshape(-1)))
    self.before = self.bits().clone()

  def bits(self):
    return self.buf.view(torch.int32)

  def unchanged(self):
    return torch.equal(self.bits(), self.before)

  def unchanged_outside(self, written):
    """Everything but the elements ``written`` (indices into the n floats) holds the bits it held: slack and gaps."""
    keep = torch.ones(self.buf.numel(), dtype=torch.bool, device=self.buf.device)
    keep[torch.as_tensor(np.asarray(written).reshape(-1) + LEAD, device=self.buf.device)] = False
    return torch.equal(self.bits()[keep], self.before[keep])

  def numpy(self):
    return self.t.cpu().numpy()


def _report(c, kernels, worst, problems):
  print('%s: %s: worst share of a bound %.4f' % (c.id, ', '.join(kernels), max(worst.values()) if worst else float('nan')))
  assert not problems, c.id + ': ' + '; '.join(problems)


# ---- geeco_conv1_dgrad -----------------------------------------------------------------------------------------------------
def _strided(parts, stride, n):
  """parts[g] flat at g * stride inside NaN."""
  flat = np.full((len(parts) - 1) * stride + n, np.nan, np.float32)
  for g, p in enumerate(parts):
    flat[g * stride:g * stride + n] = p.reshape(-1)
  return flat


def _launch_conv1(c, dev):
  from geeco_amd import ops
  inp, geo = inputs(c), R.conv1_geometry(c)
  ins = dict(dz=Buf(dev, geo['len_dz'], _strided(inp['dz'], geo['gs_dz'], geo['n_dz'])),
             w=Buf(dev, geo['len_w'], _strided(inp['w'], geo['gs_w'], geo['n_w'])))
  out = Buf(dev, geo['len_dx'])
  names = ops.kernel_trace(lambda: ops.conv1_dgrad_into(out.t, ins['dz'].t, ins['w'].t, geo['G'], geo['gs_dz'], geo['gs_w'], geo['gs_dx'],
                                                        c.F, c.H, c.W, c.Cin))
  torch.cuda.synchronize()
  written = np.concatenate([g * geo['gs_dx'] + np.arange(geo['n_dx']) for g in range(geo['G'])])
  return names, ins, out, written


@pytest.mark.parametrize('c', CONV, ids=lambda c: c.id)
def test_conv1_dgrad_variant(dev, c):
  geo = R.conv1_geometry(c)
  names, ins, out, written = _launch_conv1(c, dev)
  assert names == [geo['kernel']], names
  got = out.numpy()[written].reshape(geo['G'], c.F, c.H, c.W, 4)
  worst, problems = R.input_grad_compare(c, dict(dx=got), R.input_grad_reference(c, inputs(c)))
  _report(c, names + ['%d x %d tiles' % (geo['tiles_y'], geo['tiles_x'])], worst, problems)
  assert not np.signbit(got[..., c.Cin:]).any()      # channel 3 of an RGB layer: +0
  assert out.unchanged_outside(written), 'slack or a gap between the groups of dx was written'
  for k, b in ins.items():
    assert b.unchanged(), k
  _, _, out2, _ = _launch_conv1(c, dev)
  assert torch.equal(out.bits(), out2.bits())


# ---- geeco_pack_pixels_bwd -------------------------------------------------------------------------------------------------
def _launch_pack(c, dev):
  from geeco_amd import ops
  inp = inputs(c)
  N, K, HW, C1, C2, t = c.N, c.K, c.HW, c.C1, c.C2, c.t
  a0, b0 = inp['a0'].copy(), inp['b0'].copy()
  if c.form != 'src2' and not c.acc[0]:
    a0[:, t] = np.nan                     # an overwriting output starts as NaN
  if c.form in ('both', 'src2') and not c.acc[1]:
    b0[:, t] = np.nan
  g, a, b = Buf(dev, inp['g'].size, inp['g']), Buf(dev, a0.size, a0), Buf(dev, b0.size, b0)
  d_src = a.t.view(N, K, HW, C1)[:, t] if c.form != 'src2' else None
  d_src2 = b.t.view(N, K, HW, b0.shape[-1])[:, t] if c.form in ('both', 'src2') else None
  ops.pack_pixels_bwd_into(d_src, g.t, K * HW * C1, N, HW, C1, c.Cpad, accumulate=bool(c.acc[0]), d_src2=d_src2,
                           src2_sample_stride=K * HW * C2, C2=C2, accumulate2=bool(c.acc[1]))
  torch.cuda.synchronize()
  return g, a, b


@pytest.mark.parametrize('c', PACK, ids=lambda c: c.id)
def test_pack_pixels_bwd_variant(dev, c):
  inp = inputs(c)
  ref = R.input_grad_reference(c, inp)
  g, a, b = _launch_pack(c, dev)
  bufs = dict(d_src=a, d_src2=b)
  got = {k: bufs[k].numpy().reshape(r['val'].shape) for k, r in ref.items()}
  worst, problems = R.input_grad_compare(c, got, ref)      # the whole stacks: equality, the frames beside frame t included
  _report(c, ['pack_pixels_bwd_kernel, %d block(s) per sample' % R.cdiv(c.HW, 256)], worst, problems)
  assert g.unchanged()
  everything = lambda buf: np.arange(buf.n)
  assert a.unchanged_outside(everything(a)) and b.unchanged_outside(everything(b))      # the slack
  if c.form == 'src2':
    assert a.unchanged()
  if c.form in ('src', 'c2_null'):
    assert b.unchanged()
  _, a2, b2 = _launch_pack(c, dev)
  assert torch.equal(a.bits(), a2.bits()) and torch.equal(b.bits(), b2.bits())


# ---- geeco_dynimg_bwd ------------------------------------------------------------------------------------------------------
def _launch_dyn(c, dev, inp, acc):
  """One launch of the case into fresh buffers with the accumulate flags ``acc`` -> (outputs as numpy per dyn_split's names,
  {name: Buf} inputs, {name: (Buf, written indices)} outputs, workspace Buf)."""
  from geeco_amd import ops
  geo = R.dyn_geometry(c)
  N, K, total, Kf = c.N, c.K, geo['total'], geo['Kf']

  def place(vals, idx, off, length):
    flat = np.full(off + length, np.nan, np.float32)
    if vals is not None:
      flat[off + idx.reshape(-1)] = vals.reshape(-1)
    return flat
  dense = (np.arange(N) * total)[:, None] + np.arange(total)
  ins = dict(g=Buf(dev, inp['gp'].size, inp['gp']), frames=Buf(dev, geo['off'] + geo['len_f'], place(inp['frames'][:, :Kf], geo['idx'], geo['off'], geo['len_f'])))
  if c.two:
    ins['frames2'] = Buf(dev, geo['off2'] + N * total, place(inp['frames'][:, 1], dense, geo['off2'], N * total))
  outs = {}
  if geo['has1']:
    start = inp['start'][:, :Kf] if acc[0] else None
    outs['d_frames'] = (Buf(dev, geo['doff'] + geo['len_d'], place(start, geo['didx'], geo['doff'], geo['len_d'])), geo['doff'] + geo['didx'].reshape(-1))
  if geo['has2']:
    start = inp['start'][:, 1] if acc[1] else None
    outs['d_frames2'] = (Buf(dev, geo['doff2'] + N * total, place(start, dense, geo['doff2'], N * total)), geo['doff2'] + dense.reshape(-1))
  assert geo['ws_bytes'] % 4 == 0 and geo['ws_bytes'] == int(ops._lib().geeco_dynimg_bwd_ws_bytes(N, c.HW, c.C))
  ws = Buf(dev, geo['ws_bytes'] // 4)
  tensor = lambda name, off: outs[name][0].t[off:] if name in outs else None
  ops.dynimg_bwd_into(tensor('d_frames', geo['doff']), ins['g'].t, ins['frames'].t[geo['off']:], K, N, c.HW, c.C, c.Cpad, ws.t, geo['ss'], geo['fs'],
                      geo['dss'], geo['dfs'], accumulate=bool(acc[0]), frames2=ins['frames2'].t[geo['off2']:] if c.two else None,
                      d_frames2=tensor('d_frames2', geo['doff2']), accumulate2=bool(acc[1]))
  torch.cuda.synchronize()
  got = {}
  if geo['has1']:
    got['d_frames'] = outs['d_frames'][0].numpy()[outs['d_frames'][1]].reshape(N, Kf, total)
  if geo['has2']:
    got['d_frames2'] = outs['d_frames2'][0].numpy()[outs['d_frames2'][1]].reshape(N, total)
  return got, ins, outs, ws


def _host_D32(frames, K):
  """D in float32 by the forward's chain, acc = 0; acc = fma(alpha_t, x_t, acc) (the product of two float32 is exact in float64)."""
  a = O.dynimg_alpha(K)
  acc = np.zeros(frames.shape[:1] + frames.shape[2:], np.float32)
  for t in range(K):
    acc = (acc.astype(np.float64) + np.float64(a[t]) * frames[:, t].astype(np.float64)).astype(np.float32)
  return acc


def _check_dyn(c, dev, inp):
  """The overwriting launch of ``c`` under every check of this file's docstring -> its outputs."""
  geo = R.dyn_geometry(c)
  got, ins, outs, ws = _launch_dyn(c, dev, inp, (0, 0))
  worst, problems = R.input_grad_compare(c, got, R.input_grad_reference(c, inp))
  _report(c, geo['kernels'] + ['nblk %d' % geo['nblk']], worst, problems)
  for k, (b, written) in outs.items():
    assert b.unchanged_outside(written), 'slack or a gap of %s was written' % k
  for k, b in ins.items():
    assert b.unchanged(), 'the input %s was written' % k
  # the workspace: N * nblk records of 8 floats, nothing behind them; the records hold the forward's extrema
  assert ws.unchanged_outside(np.arange(geo['rec_floats'])), 'the workspace was written past its records'
  rec = ws.numpy()[:geo['rec_floats']].reshape(c.N, geo['nblk'], 8)
  D32 = _host_D32(inp['frames'], c.K)
  assert np.array_equal(rec[:, :, 0].min(1), D32.min(1)) and np.array_equal(rec[:, :, 1].max(1), D32.max(1)), (
      c.id, rec[:, :, 0].min(1), D32.min(1), rec[:, :, 1].max(1), D32.max(1))
  # run to run
  again, _, _, _ = _launch_dyn(c, dev, inp, (0, 0))
  for k in got:
    assert np.array_equal(got[k].view(np.int32), again[k].view(np.int32)), 'two launches differ in %s' % k
  return got


@pytest.mark.parametrize('c', DYN, ids=lambda c: c.id)
def test_dynimg_bwd_variant(dev, c):
  from geeco_amd import ops
  assert np.array_equal(np.array(ops.dynimg_alpha(c.K), np.float32), O.dynimg_alpha(c.K))
  inp, geo = inputs(c), R.dyn_geometry(c)
  plain = _check_dyn(c, dev, inp)
  if any(c.acc):      # start + the overwriting result, ONE float32 addition; an output without its flag: the overwriting result
    got, _, outs, _ = _launch_dyn(c, dev, inp, c.acc)
    starts = dict(d_frames=(inp['start'][:, :geo['Kf']], c.acc[0]))
    if c.two:
      starts['d_frames2'] = (inp['start'][:, 1], c.acc[1])
    for k in plain:
      want = starts[k][0] + plain[k] if starts[k][1] else plain[k]
      assert np.array_equal(got[k].view(np.int32), want.view(np.int32)), 'accumulate: %s is not start + the overwriting result' % k
      assert outs[k][0].unchanged_outside(outs[k][1])
  if c.twin:          # the same values through <4>: held to its own bound (another summation order: not compared bitwise)
    t = R.dense_twin(c)
    _check_dyn(t, dev, inp)
  if c.N == 3:        # a sample does not see its neighbours
    for n in range(c.N):
      one = c.replace(N=1, mins=[c.mins[n]], maxs=[c.maxs[n]], id='%s-sample%d-alone' % (c.id, n))
      alone, _, _, _ = _launch_dyn(one, dev, {k: v[n:n + 1] for k, v in inp.items()}, (0, 0))
      for k in plain:
        assert np.array_equal(alone[k][0].view(np.int32), plain[k][n].view(np.int32)), (k, n)


# ---- the chunked pass and repeated calls --------------------------------------------------------------------------------
def _prepared(dev, cfg_kw, goal, N=2, H=136):
  ocfg, P, feats, labels = G._mk(dict(cfg_kw, lr=1e-3), goal, N, H)
  G._plant(feats, ocfg, goal)
  model = G._build(ocfg, goal, P, feats, labels, dev)
  model.forward(backward_too=True)
  torch.cuda.synchronize()
  masks = T.snapshot_masks(model.enc)
  model.backward()
  torch.cuda.synchronize()
  return ocfg, P, feats, labels, model, masks


def _oracle(model, ocfg, goal, P, feats, labels, masks):
  """Steps one and two of test_input_gradients_whole_graph, once per model: (slots, dx_ref, refs)."""
  C = ocfg.img_channels
  tap, slots = T.device_tap(model, goal, masks, C)
  leaves = {}

  def inputs_fn(scope, call):
    g, f0, n = slots[(scope, call)]
    leaves[(scope, call)] = x = model.enc.x_in[g][f0:f0 + n][..., :C].cpu().double().requires_grad_(True)
    return x
  tap.inputs_fn = inputs_fn
  O.OracleTrainer(ocfg, goal, P, dtype=torch.float64).loss_and_grads(feats, labels, tap=tap)
  T.check_decisions(tap.stats)
  assert sorted(leaves) == sorted(slots)
  dx_ref = {k: x.grad.numpy() for k, x in leaves.items()}
  return slots, dx_ref, G._frame_gradient_refs(model, ocfg, goal, feats, dx_ref)


def _against_oracle(name, dx, grads, slots, dx_ref, refs, C):
  order = sorted(slots)
  got = np.concatenate([dx[slots[k][0]][slots[k][1]:slots[k][1] + slots[k][2]][..., :C].reshape(-1) for k in order])
  G._norms(got, np.concatenate([dx_ref[k].reshape(-1) for k in order]), '%s: dx_in' % name)
  if C == 3:
    assert not dx[..., 3].any()
  assert sorted(grads) == sorted(refs)
  for k, ref in refs.items():
    G._norms(grads[k], ref, '%s: d %s' % (name, k))


CHUNK_CASES = [
    ('e2e_vmc', dict(window_size=3), False, (1, 4, 6, 96)),      # Nf = 6: 1 then 4 regrows dz1_chunk; 4 leaves a ragged chunk of 2
    ('geeco-f', dict(proc_obs='dynimg', proc_tgt='dyndiff', window_size=4), True, (1, 96)),      # G = 3: the multi-encoder loop
]


@pytest.mark.parametrize('name,cfg_kw,goal,chunks', CHUNK_CASES, ids=[c[0] for c in CHUNK_CASES])
def test_chunk_frames(dev, name, cfg_kw, goal, chunks):
  """``input_gradients(chunk_frames=c)`` in this order on ONE model: every call passes the oracle comparison of
  test_input_gradients_whole_graph (same tolerance) and equals the one-chunk call bitwise (frames are independent in both launches and
  no launch parameter that touches a sum depends on the frame count: see the module docstring)."""
  ocfg, P, feats, labels, model, masks = _prepared(dev, cfg_kw, goal)
  slots, dx_ref, refs = _oracle(model, ocfg, goal, P, feats, labels, masks)
  Nf, results = model.enc.Nf, []
  for cf in chunks:
    grads = model.input_gradients(chunk_frames=cf)
    torch.cuda.synchronize()
    assert model.enc.dz1_chunk.shape[0] >= min(cf, Nf)
    results.append((model.enc.dx_in.cpu().numpy(), {k: v.cpu().numpy() for k, v in grads.items()}))
    _against_oracle('%s, chunk_frames=%d (%d trips per encoder)' % (name, cf, R.cdiv(Nf, min(cf, Nf))), *results[-1], slots, dx_ref, refs,
                    ocfg.img_channels)
  assert Nf > 1 and chunks[0] == 1 and chunks[-1] >= Nf
  dx1, g1 = results[-1]
  for cf, (dx, g) in zip(chunks[:-1], results[:-1]):
    assert np.array_equal(dx.view(np.int32), dx1.view(np.int32)), 'dx_in at chunk_frames=%d differs from the one-chunk result' % cf
    for k in g1:
      assert np.array_equal(g[k].view(np.int32), g1[k].view(np.int32)), (cf, k)


REPEAT_CASES = [
    ('dynimg', dict(proc_obs='dynimg', proc_tgt='dyndiff', window_size=2), True),
    ('seq_dyndiff', dict(proc_obs='sequence', proc_tgt='dyndiff', window_size=2), True),
    ('per-frame goal', dict(proc_obs='sequence', proc_tgt='constant', window_size=2), True),
    ('rgbd', dict(proc_obs='dynimg', proc_tgt='dyndiff', window_size=2, img_channels=4, lambda_aux=0.5), True),
]


@pytest.mark.parametrize('name,cfg_kw,goal', REPEAT_CASES, ids=[c[0] for c in REPEAT_CASES])
def test_second_call_gives_the_same_bits(dev, name, cfg_kw, goal):
  """A second ``input_gradients()`` on the same model reuses d_frames / d_tgt (the pair form accumulates into them) and packs
  obs4 / tgt4 again: nothing of the first call may be left in the second's result."""
  ocfg, P, feats, labels = G._mk(dict(cfg_kw, lr=1e-3), goal, 2, 136)
  model = G._build(ocfg, goal, P, feats, labels, dev)
  model.forward(backward_too=True)
  model.backward()
  first = {k: v.clone() for k, v in model.input_gradients().items()}
  dx_first = model.enc.dx_in.clone()
  second = model.input_gradients()
  torch.cuda.synchronize()
  assert sorted(first) == sorted(second) and torch.equal(dx_first.view(torch.int32), model.enc.dx_in.view(torch.int32))
  for k in first:
    assert bool(first[k].any()) and not bool(torch.isnan(first[k]).any()), k
    assert torch.equal(first[k].contiguous().view(torch.int32), second[k].contiguous().view(torch.int32)), k
