"""Every instantiation of the kernels that build the decoder's inputs from frame tables -- csrc/replay.hip (replay_states_kernel<4, true |
4, false | 1, false> through geeco_replay_states and geeco_replay_states_pair, the two error kernels), csrc/replay_dynimg.hip (the
four minmax / emit pairs) and csrc/shared_frames.hip (pack_frames_kernel<true | false>, window_states_fwd_kernel<4 | 1>,
window_states_bwd_kernel<4 | 1>) -- launched past the first trip of every loop they hold, one case of tests/_table_builder_cases.py
each.  tests/test_table_builders_cover_cpu.py proves on the host that the table reaches them; tests/test_replay_gpu.py,
test_replay_dynimg_gpu.py and test_shared_frames_gpu.py hold the same code at shapes where a block serves one item and a thread one
unit.

Each case: the traced kernel names are exactly those the Python mirror of the launch rule predicts; every output lies inside a larger
NaN-filled allocation (a row pitch wider than the row where the entry point takes one, one spare row behind the last, slack on both
sides) and everything outside the result keeps its bits; two runs are bitwise equal; the values are compared with the host model:

  states, pack, the forward gather, the current frame's copy   bitwise (they move values; the state tables hold a different integer
                                                               per frame, cell and column)
  window_states_bwd                                            the float64 scatter-sum: rtol 1e-6 where nothing cancels, 1e-6 of
                                                               sum |term| where terms are signed (the two rules of
                                                               test_shared_frames_gpu.py); exact +0 for unreferenced slots
  out-of-range slots                                           exact zeros in the forward, no contribution in the backward, with a
                                                               NaN-filled guard slot on either side of the feature table
  replay_errors                                                float64, the bounds of test_replay_errors_against_float64
  replay_images, buffer and pair image                         the float64 restatement under the bound derived in
                                                               _table_builder_cases.py (module docstring) from K, sum |alpha_k x_k|
                                                               and 1 / (max - min + 1e-6); the worst observed / bound ratio is
                                                               printed per case
  replay_images, planted pixels (bytes 0 and 255 alone)        bitwise: the minimum stores 0.0, the maximum
                                                               fl(fl(max - min) / fl(fl(max - min) + 1e-6f)); the extrema sit where
                                                               only a second trip of the item loop, or a partial with index >= 256,
                                                               finds them

Measured on an MI355X (recorded, not asserted: the assertions are the bounds): all 52 cases pass in 4.4 s.  The worst observed / bound
ratio of the image cases is 0.120 (buffer image of the two fold cases with it, K = 2), 0.097 for the pair image of the item-loop
cases, 0.055 and 0.023 for the buffer images at K = 4 and K = 16; window_states_bwd stays within 1.5e-7 of sum |term| everywhere,
6.8e-8 for the 1024-term sums; the regression heads of replay_errors within 3.2 u.
"""
import math

import numpy as np
import pytest
import torch

import _replay_dynimg_ref as D
import _replay_ref as R
import _table_builder_cases as C

pytestmark = pytest.mark.gpu

LEAD, TAIL = 8, 12      # floats of NaN before and behind every float tensor (16-byte steps)
NAN = float('nan')


class Buf:
  """``n`` floats ``off`` floats behind a 16-byte boundary inside one NaN-filled allocation; ``values`` or NaN inside."""

  def __init__(self, dev, n, off=0, values=None):
    self.buf = torch.full((LEAD + off + n + TAIL,), NAN, dtype=torch.float32, device=dev)
    self.lo, self.hi = LEAD + off, LEAD + off + n
    self.t = self.buf[self.lo:self.hi]
    assert self.t.data_ptr() % 16 == (4 * off) % 16
    if values is not None:
      self.t.copy_(torch.from_numpy(np.ascontiguousarray(values, np.float32).reshape(-1)))
    self.before = self.bits().clone()

  def bits(self):
    return self.buf.view(torch.int32)

  def unchanged(self):
    return torch.equal(self.bits(), self.before)

  def slack_unchanged(self):
    return torch.equal(self.bits()[:self.lo], self.before[:self.lo]) and torch.equal(self.bits()[self.hi:], self.before[self.hi:])

  def numpy(self):
    return self.t.cpu().numpy()


def _all_nan(a):
  return bool(np.isnan(a).all())


def _same_bits(a, b):
  a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
  return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def _trace(fn):
  from geeco_amd import ops
  names = ops.kernel_trace(fn)
  torch.cuda.synchronize()
  return names


# ---- geeco_replay_states / geeco_replay_states_pair --------------------------------------------------------------------------------
def _states_case(dev, c, launch, want, width):
  a, p = c.a, C.plan(c)
  n, K = a['t1'] - a['t0'], a['K']
  N, stride = n + 1, width + a['pad']
  runs = []
  for _ in range(2):
    out = Buf(dev, K * N * stride, a['states_off'])
    names = _trace(lambda: launch(out.t.view(K, N, stride)))
    assert names == p['names'], (names, p['names'])
    runs.append(out)
  assert torch.equal(runs[0].bits(), runs[1].bits()), 'two runs differ'
  got = runs[0].numpy().reshape(K, N, stride)
  assert np.array_equal(got[:, :n, :width], want), c.id
  assert _all_nan(got[:, n:]) and _all_nan(got[:, :, width:]) and runs[0].slack_unchanged()
  print('%s: %s, grid %d, trips %s' % (c.id, names[0], p['grid'], p['loops']))


@pytest.mark.parametrize('c', C.cases('replay_states'), ids=lambda c: c.id)
def test_replay_states_variant(dev, c):
  from geeco_amd import ops
  a = c.a
  (feat,), jnt, tgt = C.distinct_tables(a['T'], a['cells'], [a['ch']], a['J'])
  fd, jd = Buf(dev, feat.size, a['feat_off'], feat), Buf(dev, jnt.size, 0, jnt)
  td = Buf(dev, tgt.size, a['tgt_off'], tgt) if a['mode'] != 'plain' else None
  launch = lambda states: ops.replay_states_into(states, fd.t, jd.t, a['mode'], a['T'], a['t0'], a['t1'], a['K'], a['cells'], a['ch'], a['J'],
                                                 tgt_feat=None if td is None else td.t)
  _states_case(dev, c, launch, R.states_ref(feat, jnt, tgt, a['mode'], a['K'], a['t0'], a['t1']),
               C.state_width(a['mode'], a['cells'], a['ch'], a['J']))
  assert fd.unchanged() and jd.unchanged() and (td is None or td.unchanged())


@pytest.mark.parametrize('c', C.cases('replay_states_pair'), ids=lambda c: c.id)
def test_replay_states_pair_variant(dev, c):
  from geeco_amd import ops
  a = c.a
  (feat, tgt), jnt, _ = C.distinct_tables(a['T'], a['cells'], [a['ch'], a['ch_t']], a['J'])
  fd, td, jd = Buf(dev, feat.size, a['feat_off'], feat), Buf(dev, tgt.size, a['tgt_off'], tgt), Buf(dev, jnt.size, 0, jnt)
  launch = lambda states: ops.replay_states_pair_into(states, fd.t, td.t, jd.t, a['T'], a['t0'], a['t1'], a['K'], a['cells'], a['ch'], a['ch_t'],
                                                      a['J'])
  _states_case(dev, c, launch, D.states_pair_ref(feat, tgt, jnt, a['K'], a['t0'], a['t1']), a['cells'] * (a['ch'] + a['J'] + a['ch_t']))
  assert fd.unchanged() and td.unchanged() and jd.unchanged()


# ---- geeco_replay_errors -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', C.cases('replay_errors'), ids=lambda c: c.id)
def test_replay_errors_variant(dev, c):
  """The bounds of test_replay_errors_against_float64: a regression head of n columns within (n + 4) u of the float64 value, class
  hits exact (ties take the first maximum), the episode mean in the documented order and within (ceil(T / 256) + 8) u of the exact
  mean of the per-frame values."""
  from geeco_amd import ops
  a, p = c.a, C.plan(c)
  T, heads = a['T'], a['heads']
  P = sum(h[1] for h in heads)
  r = np.random.default_rng(a['seed'])
  preds = r.standard_normal((T, P)).astype(np.float32)
  labels = r.standard_normal((T, P)).astype(np.float32)
  for off, size, kind in heads:
    if kind == 1:
      labels[:, off] = r.integers(0, size, T)
      preds[T - 1, off:off + size] = 0.5      # all equal, in the last (ragged) block: class 0
      labels[T - 1, off] = 0
  pd, ld = Buf(dev, preds.size, 0, preds), Buf(dev, labels.size, 0, labels)
  runs = []
  for _ in range(2):
    of, oe = Buf(dev, T * len(heads)), Buf(dev, len(heads))
    names = _trace(lambda: ops.replay_errors_into(of.t.view(T, len(heads)), oe.t, pd.t.view(T, P), ld.t.view(T, P), T, heads))
    assert names == p['names'], names
    assert of.slack_unchanged() and oe.slack_unchanged()
    runs.append((of, oe))
  assert torch.equal(runs[0][0].bits(), runs[1][0].bits()) and torch.equal(runs[0][1].bits(), runs[1][1].bits())
  frame, episode = runs[0][0].numpy().reshape(T, len(heads)), runs[0][1].numpy()
  want_f, _ = R.errors_ref(preds, labels, heads)
  chain = math.ceil(T / 256) + 8
  for h, (off, size, kind) in enumerate(heads):
    if kind == 1:
      np.testing.assert_array_equal(frame[:, h], want_f[:, h])
      assert frame[T - 1, h] == 1.0
    else:
      err = np.abs(frame[:, h] - want_f[:, h])
      print('%s head %d (%d columns): worst per-frame error %.3g u' % (c.id, h, size, (err / (C.U * want_f[:, h])).max()))
      assert (err <= (size + 4) * C.U * want_f[:, h]).all()
    assert episode[h] == R.episode_sum_order(frame[:, h])
    exact = frame[:, h].astype(np.float64).mean()
    assert abs(episode[h] - exact) <= chain * C.U * exact
  assert pd.unchanged() and ld.unchanged()


# ---- geeco_replay_images -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', C.cases('replay_images'), ids=lambda c: c.id)
def test_replay_images_variant(dev, c):
  from geeco_amd import ops
  a, p = c.a, C.plan(c)
  T, HW, K, t0, t1, n = a['T'], a['HW'], a['K'], a['t0'], a['t1'], a['t1'] - a['t0']
  fr, gl, binary, pair_binary = C.planted_episode(a)
  C.check_planted(a, fr, gl, binary, pair_binary)      # the planting, proved in float64 on the host
  f32, g32 = C.as_unit(fr), C.as_unit(gl)
  frames, goal = (torch.from_numpy(x).to(dev) for x in ((fr, gl) if a['u8'] else (f32, g32)))
  keep_f, keep_g = frames.clone(), goal.clone()
  addr = torch.from_numpy(frames.data_ptr() + np.arange(T, dtype=np.int64) * HW * 3 * frames.element_size()).to(dev)
  ws = ops.replay_images_ws(n, HW, dev)
  assert ws.numel() == n * p['bpw'] * 4
  runs = []
  for _ in range(2):
    ws.fill_(NAN)      # no zero-fill contract: whatever the workspace holds
    got = [Buf(dev, (n + 1) * HW * 4) for _ in range(3)]
    names = _trace(lambda: ops.replay_images_into(got[0].t, got[1].t if a['buf'] else None, got[2].t, addr, goal, T, t0, t1, K, HW, ws))
    assert names == p['names'], (names, p['names'])
    runs.append(got)
  out = {}
  for i, name in enumerate(('cur', 'buf', 'diff')):
    assert torch.equal(runs[0][i].bits(), runs[1][i].bits()), '%s differs between two runs' % name
    if name == 'buf' and not a['buf']:
      assert runs[0][i].unchanged()
      continue
    assert runs[0][i].slack_unchanged()
    img = runs[0][i].numpy().reshape(n + 1, HW, 4)
    assert _all_nan(img[n]), name      # the spare row
    out[name] = img[:n]
  assert torch.equal(frames, keep_f) and torch.equal(goal, keep_g)
  # the copy: byte / 255 in IEEE float32 (or the float32 frame), R, G, B, 0
  assert _same_bits(out['cur'], D.pad4(f32[t0:t1])), 'cur'
  im = C.images_f64(f32, g32, K, t0, t1, a['buf'])
  for name, d in im.items():
    y = out[name]
    assert not y[..., 3].any() and not np.signbit(y[..., 3]).any() and np.isfinite(y).all(), name
    ratio = np.abs(y[..., :3] - d['y']) / C.image_bound(d)
    at = np.unravel_index(ratio.argmax(), ratio.shape)
    print('%s %s: worst observed / bound = %.4f at window %d pixel %d (bound there %.3g); smallest range %.4f'
          % (c.id, name, ratio.max(), at[0] + t0, at[1], C.image_bound(d)[at], (d['mx'] - d['mn']).min()))
    assert ratio.max() <= 1.0, name
    # the sharp check: the planted pixels, bit for bit
    pix = binary if name == 'buf' else pair_binary
    want, mn, mx = C.planted_f32(fr, gl, K, t0, t1, pix, name)
    assert _same_bits(y[:, pix, :3], want), '%s: planted pixels' % name
    assert (y[..., :3].reshape(n, -1).min(1) == 0.0).all()
    r = (mx - mn).astype(np.float32)
    assert np.array_equal(y[..., :3].reshape(n, -1).max(1), (r / (r + np.float32(1e-6)).astype(np.float32)).astype(np.float32)), name
  print('%s: %s, grid %d, bpw %d, trips %s' % (c.id, names, p['grid'], p['bpw'], p['loops']))


# ---- geeco_pack_frames_by_address ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', C.cases('pack_frames'), ids=lambda c: c.id)
def test_pack_frames_variant(dev, c):
  from geeco_amd import ops
  a, p = c.a, C.plan(c)
  HW, u8, offs = a['HW'], a['u8'], a['slot_offs']
  F = len(offs)
  r = np.random.default_rng(HW + u8)
  esz = 1 if u8 else 4
  host = r.integers(0, 256, (F, HW * 3)).astype(np.uint8) if u8 else r.random((F, HW * 3), dtype=np.float32)
  want = host.astype(np.float32) / np.float32(255) if u8 else host
  store, table = [], []
  for s, o in enumerate(offs):      # every frame in an allocation of its own, ``o`` bytes behind a 16-byte boundary
    if o is None:
      table.append(0)
      continue
    buf = torch.zeros(HW * 3 + 16, dtype=torch.uint8 if u8 else torch.float32, device=dev)
    view = buf[o // esz:o // esz + HW * 3]
    view.copy_(torch.from_numpy(host[s]))
    assert view.data_ptr() % 16 == o
    store.append(buf)
    table.append(view.data_ptr())
  td = torch.tensor(table, dtype=torch.int64, device=dev)
  runs = []
  for _ in range(2):
    x = Buf(dev, (F + 1) * HW * 4)
    names = _trace(lambda: ops.pack_frames_by_address_into(x.t, td, F, HW, u8))
    assert names == p['names'], names
    runs.append(x)
  assert torch.equal(runs[0].bits(), runs[1].bits())
  got = runs[0].numpy().reshape(F + 1, HW, 4)
  exp = np.zeros((F, HW, 4), np.float32)
  for s, o in enumerate(offs):
    if o is not None:
      exp[s, :, :3] = want[s].reshape(HW, 3)
  assert _same_bits(got[:F], exp), c.id
  assert _all_nan(got[F]) and runs[0].slack_unchanged()
  print('%s: %s, grid.x %d, trips %s' % (c.id, names[0], p['grid_x'], p['loops']))


# ---- geeco_window_states_fwd / geeco_window_states_bwd -----------------------------------------------------------------------------
def _guarded(dev, table, off):
  """``table`` [F][cells][ch] with one NaN-filled guard slot in front and one behind -> (Buf of F + 2 slots, the view of the F)."""
  F, FE = table.shape[0], table[0].size
  vals = np.full((F + 2, FE), np.nan, np.float32)
  vals[1:F + 1] = table.reshape(F, FE)
  b = Buf(dev, (F + 2) * FE, off, vals)
  return b, b.t[FE:(F + 1) * FE]


@pytest.mark.parametrize('c', C.cases('window_states_fwd'), ids=lambda c: c.id)
def test_window_states_fwd_variant(dev, c):
  from geeco_amd import ops
  a, p = c.a, C.plan(c)
  N, K, cells, ch, J, mode = a['N'], a['K'], a['cells'], a['ch'], a['J'], a['mode']
  F, idx, tgt = C.shared_indices(a)
  # a different integer per (slot, cell, column) and per joint-state element; odd features below, even joint states above
  feat = (1 + 2 * np.arange(F * cells * ch)).reshape(F, cells, ch).astype(np.float32)
  jnt = (2 * F * cells * ch + 2 * np.arange(N * K * J)).reshape(N, K, J).astype(np.float32)
  width = C.state_width(mode, cells, ch, J)
  stride = width + a['pad']
  fb, fview = _guarded(dev, feat, a['feat_off'])
  assert fview.data_ptr() % 16 == (4 * a['feat_off']) % 16
  jd = Buf(dev, jnt.size, 0, jnt)
  idx_d, tgt_d = torch.from_numpy(idx).to(dev), torch.from_numpy(tgt).to(dev)
  runs = []
  for _ in range(2):
    out = Buf(dev, (K * N + 1) * stride)
    names = _trace(lambda: ops.window_states_fwd_into(out.t, fview, idx_d, jd.t, mode, F, N, K, cells, ch, J, stride,
                                                      tgt_idx=None if mode == 'plain' else tgt_d))
    assert names == p['names'], names
    runs.append(out)
  assert torch.equal(runs[0].bits(), runs[1].bits())
  got = runs[0].numpy().reshape(K * N + 1, stride)
  want = C.window_states_fwd_ref(feat, idx, jnt, tgt, mode)
  assert _same_bits(got[:K * N, :width].reshape(K, N, width), want), c.id
  assert _all_nan(got[K * N]) and _all_nan(got[:, width:]) and runs[0].slack_unchanged() and fb.unchanged() and jd.unchanged()
  if a['out_of_range']:      # exact zeros where a slot is outside [0, F): feature columns of the position, target columns of the window
    g4 = got[:K * N, :width].reshape(K, N, cells, -1)
    for n_, t_ in zip(*np.nonzero((idx < 0) | (idx >= F))):
      if mode == 'constant':
        assert not g4[t_, n_, :, :ch].any() and not np.signbit(g4[t_, n_, :, :ch]).any()
    for n_ in np.nonzero((tgt < 0) | (tgt >= F))[0]:
      if mode == 'constant':
        assert not g4[:, n_, :, ch + J:].any() and not np.signbit(g4[:, n_, :, ch + J:]).any()
    assert np.isfinite(g4).all()
  print('%s: %s, trips %s' % (c.id, names[0], p['loops']))


@pytest.mark.parametrize('c', C.cases('window_states_bwd'), ids=lambda c: c.id)
def test_window_states_bwd_variant(dev, c):
  from geeco_amd import ops
  a, p = c.a, C.plan(c)
  N, K, cells, ch, J, mode, kind = a['N'], a['K'], a['cells'], a['ch'], a['J'], a['mode'], a['kind']
  F, idx, tgt = C.shared_indices(a)
  width = C.state_width(mode, cells, ch, J)
  stride = width + a['pad']
  r = np.random.default_rng(ch + K + N)
  signed = kind == 'full'
  dst = (r.standard_normal([K, N, width]) if signed else 0.5 + r.random([K, N, width])).astype(np.float32)
  feat = r.standard_normal([F, cells, ch]).astype(np.float32)
  ref, mag = C.window_states_bwd_ref(dst, feat, idx, tgt, mode, J)
  rows = np.full((K * N + 1, stride), np.nan, np.float32)      # NaN in the pitch and in the spare row: never read
  rows[:K * N, :width] = dst.reshape(K * N, width)
  dd = Buf(dev, rows.size, 0, rows)
  fb, fview = _guarded(dev, feat, a['feat_off'])
  idx_d, tgt_d = torch.from_numpy(idx).to(dev), torch.from_numpy(tgt).to(dev)
  FE = cells * ch
  runs = []
  for _ in range(2):
    ob = Buf(dev, (F + 2) * FE, a['dfeat_off'])
    oview = ob.t[FE:(F + 1) * FE]
    names = _trace(lambda: ops.window_states_bwd_into(oview, dd.t, stride, idx_d, fview, mode, F, N, K, cells, ch, J,
                                                      tgt_idx=None if mode == 'plain' else tgt_d))
    assert names == p['names'], names
    runs.append(ob)
  assert torch.equal(runs[0].bits(), runs[1].bits())                  # deterministic
  every = runs[0].numpy().reshape(F + 2, cells, ch)
  assert _all_nan(every[0]) and _all_nan(every[F + 1]) and runs[0].slack_unchanged() and fb.unchanged() and dd.unchanged()
  got = every[1:F + 1]
  referenced = np.zeros(F, bool)
  referenced[idx[(idx >= 0) & (idx < F)]] = True
  if mode != 'plain':
    referenced[tgt[(tgt >= 0) & (tgt < F)]] = True
  assert not referenced[F - 1]
  assert not got[~referenced].any() and not np.signbit(got[~referenced]).any()       # exact zeros
  err = np.abs(got - ref)
  print('%s: %s, trips %s: worst |err| / sum|term| = %.2e' % (c.id, names[0], p['loops'], (err / np.maximum(mag, 1e-30)).max()))
  if signed:
    assert (mag[:2] > 0).any() and (err <= 1e-6 * mag).all()
  else:
    assert np.array_equal(mag, np.abs(ref))         # nothing cancels
    np.testing.assert_allclose(got, ref, rtol=1e-6, atol=0)
