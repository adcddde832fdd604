"""Every instantiation of the input stage (csrc/dynimg.hip, csrc/dynimg_goal.hip: eight one-pass goal-stage kernels, the two
three-channel sums, the generic sum, the normalisation) at the smallest shapes that reach each of its paths, against the float64
reference of tests/_input_stage_refs.py under that module's per-element bound (capped at 5e-6), on inputs built so that a wrong
min / max shows: windows whose D has one sign (0 is outside the range, so nothing that leaks a zero can hide) and windows with
the extrema planted at named elements (unit 0, the last float4, lanes 0 and 63 of the later waves, the first and the ragged last
block, block 64, slot 1, a two-sample block's second sample, the unpaired sample of an odd count) in R, G, B and the depth.  The
case table, the recipes and the bound's derivation are in _input_stage_refs.py; tests/test_input_stage_refs_cpu.py shows on the
CPU that the table covers every instantiation and rejects thirteen emulated wrong kernels.

Each case: ops.kernel_trace names exactly the expected instance; every output is a view inside a NaN-filled allocation whose
margins keep their bits; float32 frames and depth of the strided cases are views with NaN in every gap; the current frame is
compared by equality, pad channels are exactly 0.  The goal stage runs three times on one workspace of exactly goal_dynimgs_ws
bytes inside a poisoned allocation: after each call the arrival and departure counters are zero, no wait has expired and the
outputs have the bits of the first call.  The uint8 form has the bits of the float32 form fed float32(b) / float32(255).  No
case touches the wait bound (the expired-wait tests are in tests/test_kernels_gpu.py).

On an MI355X all 214 cases pass and the file takes 19 s; the largest case (6 samples of 262160 pixels with depth) holds 151 MB on
the device.  One-line changes of the two kernel files tried against it on a scratch build, each caught: mn1 / mn2 / mx1 / mx2
initialised to 0 (73 cases, first goal-c3-N2-K1-HW1028-pos), `q < 4` in the min / max under DEPTH = false (45, the same case),
`i < bps - 1` in dyn_collect (all 147 goal cases), live for flive (62, goal-c3-N3-K2-HW4-pos), s_norm[0], s_norm[1] for the pair
image in onepass2's finish (65, goal-c3-N192-K1-HW8x8-neg-swap), dyn_collect without its second trip (the 20 cases of 65 blocks),
wsum3<true> without the depth in its max (8, rgbd-c4-N2-K2-HW4-pos), the norm kernel's fold without its second trip (the five cases
of more than 256 partials)."""
import numpy as np
import pytest
import torch

import _input_stage_refs as R

pytestmark = pytest.mark.gpu

MARGIN = 4096      # floats of NaN on each side of an output: a 1024-thread block stores 16 KiB per float4 slot


def _ids(cases):
  return [c['id'] for c in cases]


class Buf:
  """A float32 (int32: bytes 0xA5) tensor of ``shape`` inside one poisoned allocation, MARGIN elements from either end."""

  def __init__(self, dev, shape, dtype=torch.float32, margin=MARGIN):
    n = int(np.prod(shape))
    self.raw = torch.empty(2 * margin + n, dtype=dtype, device=dev)
    if dtype == torch.float32:
      self.raw.fill_(float('nan'))
    else:
      self.raw.view(torch.uint8).fill_(0xA5)
    self.lo, self.n = margin, n
    self.t = self.raw[margin:margin + n].view(*shape)
    assert self.t.data_ptr() % 64 == 0
    self.before = self.raw.view(torch.uint8).clone()

  def margins_intact(self):
    b, a, z = self.raw.view(torch.uint8), self.lo * 4, (self.lo + self.n) * 4
    return torch.equal(b[:a], self.before[:a]) and torch.equal(b[z:], self.before[z:])

  def numpy(self):
    return self.t.cpu().numpy()


def _strided(dev, values, sample_stride, frame_stride):
  """values [N][K][L] float32 -> a NaN-filled allocation holding frame (n, t) at n * sample_stride + t * frame_stride."""
  N, K, L = values.shape
  raw = torch.full((N * sample_stride + 4,), float('nan'), dtype=torch.float32, device=dev)
  view = raw.as_strided((N, K, L), (sample_stride, frame_stride, 1))
  view.copy_(torch.from_numpy(np.ascontiguousarray(values)))
  if sample_stride > K * L or frame_stride > L:
    assert bool(torch.isnan(raw).any())
  return raw


def _dev(dev, a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _same_bits(a, b, msg):
  np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=msg)


def _check_image(c, ref, img, got, what):
  """got [N][HW][Cpad] against the float64 image under min(bound, CAP); the channels past C are exactly zero."""
  C = c['C']
  assert np.isfinite(got).all(), (c['id'], what)
  err = np.abs(got[..., :C].astype(np.float64) - ref.img[img])
  lim = np.minimum(ref.bound[img], R.CAP)
  worst = np.unravel_index(np.argmax(err - lim), err.shape)
  print('%s %s: max err %.3g, worst (err %.3g, bound %.3g) at %s' % (c['id'], what, err.max(), err[worst], lim[worst], worst))
  assert (err <= lim).all(), (c['id'], what, float(err[worst]), float(lim[worst]), worst)
  if got.shape[-1] > C:
    assert not got[..., C:].any(), (c['id'], what, 'pad channel')


def _current_frame(c, inp):
  """[N][HW][4]: the window's last frame, its 4th channel the depth or 0."""
  cur = np.zeros((c['N'], c['HW'], 4), np.float32)
  cur[..., :c['C']] = inp.x[:, c['K'] - 1]
  return cur


def _goal_run(dev, c, inp, u8):
  """The three outputs of three consecutive calls on one exact-size workspace; the trace of the first."""
  from geeco_amd import ops
  N, K, HW, C = c['N'], c['K'], c['HW'], c['C']
  words = ops.goal_dynimgs_ws(N, HW, dev).numel()
  ws = Buf(dev, (words,), torch.int32, margin=64)
  ws.t.zero_()
  outs = [Buf(dev, (N, HW, 4)) for _ in range(3)]
  kw = {}
  if C == 4:
    kw = dict(depth=_strided(dev, inp.x[..., 3], c['dsample_stride'], c['dframe_stride']), tgt_depth=_dev(dev, inp.tgt[..., 3]),
              dsample_stride=c['dsample_stride'], dframe_stride=c['dframe_stride'])
  if u8:
    frames, tgt = _dev(dev, inp.bytes), _dev(dev, inp.tgt_bytes)
    win = torch.tensor([frames.data_ptr() + n * K * HW * 3 for n in range(N)], dtype=torch.int64, device=dev)
    tpt = torch.tensor([tgt.data_ptr() + n * HW * 3 for n in range(N)], dtype=torch.int64, device=dev)
    run = lambda: ops.goal_dynimgs_u8_into(outs[0].t, outs[1].t, outs[2].t, win, tpt, K, N, HW, ws.t, **kw)
  else:
    frames = _strided(dev, inp.x[..., :3].reshape(N, K, HW * 3), c['sample_stride'], c['frame_stride'])
    tgt = _dev(dev, inp.tgt[..., :3])
    run = lambda: ops.goal_dynimgs_into(outs[0].t, outs[1].t, outs[2].t, frames, tgt, K, N, HW, ws.t, c['sample_stride'],
                                        c['frame_stride'], **kw)
  first = None
  for call in range(3):
    names = ops.kernel_trace(run) if call == 0 else names
    if call:
      run()
    assert ops.goal_dynimgs_timeouts(ws.t, N) == 0, (c['id'], call)        # (synchronises)
    assert not ws.t[:16 * N].view(N, 16)[:, :2].any(), (c['id'], call)     # arrival and departure counters
    got = [o.numpy() for o in outs]
    if first is None:
      first = got
    for a, b, what in zip(got, first, ('current frame', 'buffer image', 'pair image')):
      _same_bits(a, b, '%s call %d' % (what, call))
    assert all(o.margins_intact() for o in outs) and ws.margins_intact(), (c['id'], call)
  return names, first, outs


def _goal_check(c, inp, names, got):
  ref = R.reference(c['id'])
  assert names == R.geometry(c)['names'], names
  _same_bits(got[0], _current_frame(c, inp), 'current frame')
  _check_image(c, ref, 0, got[1], 'buffer image')
  _check_image(c, ref, 1, got[2], 'pair image')


@pytest.mark.parametrize('c', R.BY_ENTRY['goal'], ids=_ids(R.BY_ENTRY['goal']))
def test_goal_dynimgs_fwd(dev, c):
  inp = R.inputs(c['id'])
  names, got, _ = _goal_run(dev, c, inp, False)
  _goal_check(c, inp, names, got)


@pytest.mark.parametrize('c', R.BY_ENTRY['goal_u8'], ids=_ids(R.BY_ENTRY['goal_u8']))
def test_goal_dynimgs_u8_fwd(dev, c):
  from geeco_amd import ops
  inp = R.inputs(c['id'])
  names, got, outs = _goal_run(dev, c, inp, True)
  _goal_check(c, inp, names, got)
  # the float32 form on float32(b) / float32(255), into the same buffers: the same bits
  N, K, HW, C = c['N'], c['K'], c['HW'], c['C']
  np.testing.assert_array_equal(inp.x[..., :3], inp.bytes.astype(np.float32) / np.float32(255.0))
  kw = {}
  if C == 4:
    kw = dict(depth=_dev(dev, inp.x[..., 3]), tgt_depth=_dev(dev, inp.tgt[..., 3]), dsample_stride=K * HW, dframe_stride=HW)
  for o in outs:
    o.t.fill_(float('nan'))
  ws = ops.goal_dynimgs_ws(N, HW, dev)
  ops.goal_dynimgs_into(outs[0].t, outs[1].t, outs[2].t, _dev(dev, inp.x[..., :3]), _dev(dev, inp.tgt[..., :3]), K, N, HW, ws,
                        K * HW * 3, HW * 3, **kw)
  assert ops.goal_dynimgs_timeouts(ws, N) == 0
  for o, g, what in zip(outs, got, ('current frame', 'buffer image', 'pair image')):
    _same_bits(o.numpy(), g, what + ': uint8 form against the float32 form')


def _dynimg_ws(dev, N, hwc):
  from geeco_amd import ops
  return Buf(dev, (ops.dynimg_ws(N, hwc, dev).numel(),), margin=64)


@pytest.mark.parametrize('c', R.BY_ENTRY['dynimg'], ids=_ids(R.BY_ENTRY['dynimg']))
def test_dynimg_fwd(dev, c):
  from geeco_amd import ops
  N, K, HW, C, Cpad = c['N'], c['K'], c['HW'], c['C'], c['Cpad']
  inp, ref = R.inputs(c['id']), R.reference(c['id'])
  out, ws = Buf(dev, (N, HW, Cpad)), _dynimg_ws(dev, N, HW * C)
  x = inp.x.reshape(N, K, HW * C)
  frames2 = None
  if c['two_frame']:
    frames, frames2 = _strided(dev, x[:, :1], c['sample_stride'], 0), _dev(dev, x[:, 1])
  else:
    frames = _strided(dev, x, c['sample_stride'], c['frame_stride'])
  names = ops.kernel_trace(lambda: ops.dynimg_into(out.t, frames, K, N, HW, C, Cpad, ws.t, c['sample_stride'], c['frame_stride'],
                                                   frames2=frames2))
  torch.cuda.synchronize()
  assert names == R.geometry(c)['names'], names
  _check_image(c, ref, 0, out.numpy(), 'image')
  assert out.margins_intact() and ws.margins_intact()


@pytest.mark.parametrize('c', R.BY_ENTRY['rgbd'], ids=_ids(R.BY_ENTRY['rgbd']))
def test_dynimg_rgbd_fwd(dev, c):
  from geeco_amd import ops
  N, K, HW = c['N'], c['K'], c['HW']
  inp, ref = R.inputs(c['id']), R.reference(c['id'])
  out, ws = Buf(dev, (N, HW, 4)), _dynimg_ws(dev, N, HW * 4)
  rgb, dep = inp.x[..., :3].reshape(N, K, HW * 3), inp.x[..., 3]
  rgb2 = depth2 = None
  if c['two_frame']:
    rgb_d, dep_d = _strided(dev, rgb[:, :1], c['sample_stride'], 0), _strided(dev, dep[:, :1], c['dsample_stride'], 0)
    rgb2, depth2 = _dev(dev, rgb[:, 1]), _dev(dev, dep[:, 1])
  else:
    rgb_d = _strided(dev, rgb, c['sample_stride'], c['frame_stride'])
    dep_d = _strided(dev, dep, c['dsample_stride'], c['dframe_stride'])
  names = ops.kernel_trace(lambda: ops.dynimg_rgbd_into(out.t, rgb_d, dep_d, K, N, HW, ws.t, c['sample_stride'], c['frame_stride'],
                                                        c['dsample_stride'], c['dframe_stride'], rgb2=rgb2, depth2=depth2))
  torch.cuda.synchronize()
  assert names == R.geometry(c)['names'], names
  _check_image(c, ref, 0, out.numpy(), 'image')
  assert out.margins_intact() and ws.margins_intact()
