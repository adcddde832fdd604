"""Window augmentation on the GPU: geeco_gather_windows_augmented against the float64 restatement of
tests/_augment_ref.py and, bitwise, against the merged by-address gather; its argument checks; the Estimator's 'dense_augmented'
feed for e2e_vmc and geeco-f against the same model fed host-augmented dense windows.

Tolerances.  Kernel against float64: atol 1e-6, no rtol -- at most three float32 roundings (the division by 255, the multiply,
the add; a fused multiply-add has one fewer) of values below 2 in magnitude, each at most 2^-23 = 1.2e-7, so at most 3.6e-7.
Zero fill: exactly 0.0.  Identity parameters and pure shifts: bitwise the by-address gather (moved).  Model against model: the
standing dense-vs-dense bound, rtol 1e-4 and atol 2e-5, on the loss and the predictions of ONE step (the inputs of the two runs
differ in the last bit where the host rounds the float64 tint to float32 once and the kernel rounds twice)."""
import os

import numpy as np
import pytest
import torch

from _augment_ref import augment_windows, in_view, moved

pytestmark = pytest.mark.gpu

T_EP, N, K = 6, 3, 2
PICKS = [(2, 3), (0, 1), (1, 0)]                  # (episode, start) per window
KINDS = {'uint8': (True, True, True), 'float32': (False, False, False), 'mixed': (True, False, True)}
# the vector path (W * C % 4 == 0), the one-element path (75 / 25 elements per frame), rows shorter than a block's 1024 elements
# -- and than a thread's 4 with C = 1 -- and a frame of more than one block (12 * 32 * 3 = 1152)
SHAPES = [(8, 12), (5, 5), (6, 4), (12, 32)]
INT_MAX = 2 ** 31 - 1

_EPISODES = {}


def _episodes(dev, fe, kinds):
  """Three resident episodes [T_EP][fe] (uint8 0..255, or float32 in [0, 1)), built once per case and left unchanged."""
  key = (fe, kinds)
  if key not in _EPISODES:
    r = np.random.default_rng(fe + 7 * sum(kinds))
    _EPISODES[key] = [torch.from_numpy(r.integers(0, 256, [T_EP, fe]).astype(np.uint8) if u8 else r.random([T_EP, fe], dtype=np.float32)).to(dev)
                      for u8 in kinds]
  return _EPISODES[key]


def _shift_tables(H, W):
  """[launches][N][2]: every listed value on either axis alone and paired with another one (mixed signs inside a window and
  between the windows of a launch), and the extremes of int32."""
  vals = [0, 1, -1, 3, -3, W - 1, -(W - 1), W, -W, H + 2, -(H + 2)]
  pairs = [(v, 0) for v in vals] + [(0, v) for v in vals] + [(v, vals[(i + 3) % len(vals)]) for i, v in enumerate(vals)]
  pairs += [(INT_MAX, -INT_MAX - 1), (-INT_MAX - 1, 1), (1, INT_MAX)]
  assert len(pairs) % N == 0
  return np.asarray(pairs, np.int32).reshape(-1, N, 2)


def _colour(C, n=N, seed=0):
  """gain[C] in [0.5, 1.5], bias[C] in [-0.3, 0.3] per window: the upper corner for window 0 (values above 0.47 leave [0, 1] at
  the top), the lower one for window 1 (values below 0.6 leave it at the bottom), random ones for the rest."""
  r = np.random.default_rng(seed)
  col = np.concatenate([r.uniform(0.5, 1.5, (n, C)), r.uniform(-0.3, 0.3, (n, C))], axis=1).astype(np.float32)
  col[0] = [1.5] * C + [0.3] * C
  col[1] = [0.5] * C + [-0.3] * C
  return col


def _plain_values(eps, picks, k, fe):
  """[n][k][fe] float64: the plain windows as real numbers (what the float64 restatement starts from)."""
  out = np.empty((len(picks), k, fe), np.float64)
  for n, (e, st) in enumerate(picks):
    fr = eps[e][st:st + k].cpu().numpy()
    out[n] = fr.astype(np.float64) / 255.0 if fr.dtype == np.uint8 else fr.astype(np.float64)
  return out


def _plain_f32(dev, eps, picks, k, fe):
  """[n][k][fe] float32: the merged by-address gather of the same windows; frames it does not take (fe % 4 != 0) from numpy's
  float32 division, the IEEE division the gathers state."""
  from geeco_amd import ops
  if fe % 4 == 0:
    addr, kind = _table(dev, eps, picks, fe)
    got = torch.full((len(picks), k, fe), float('nan'), device=dev)
    ops.gather_windows_by_address_into(got, addr, kind, len(picks), k, fe)
    torch.cuda.synchronize()
    return got.cpu().numpy()
  out = np.empty((len(picks), k, fe), np.float32)
  for n, (e, st) in enumerate(picks):
    fr = eps[e][st:st + k].cpu().numpy()
    out[n] = fr.astype(np.float32) / np.float32(255.0) if fr.dtype == np.uint8 else fr
  return out


def _table(dev, eps, picks, fe):
  addr = [eps[e].data_ptr() + st * fe * eps[e].element_size() for e, st in picks]
  kind = [0 if eps[e].dtype == torch.uint8 else 1 for e, _ in picks]
  return torch.tensor(addr, dtype=torch.int64, device=dev), torch.tensor(kind, dtype=torch.int32, device=dev)


def _augmented(dev, eps, picks, k, H, W, C, shift, colour):
  """One launch; the tables sit at a non-zero offset of larger buffers, the output starts as NaN."""
  from geeco_amd import ops
  n = len(picks)
  addr, kind = _table(dev, eps, picks, H * W * C)
  big_s = torch.full((n + 5, 2), 1 << 20, dtype=torch.int32, device=dev)
  big_s[3:3 + n] = torch.from_numpy(np.ascontiguousarray(shift, np.int32))
  col = None
  if colour is not None:
    big_c = torch.full((n + 3, 2 * C), float('nan'), device=dev)
    big_c[2:2 + n] = torch.from_numpy(colour)
    col = big_c[2:2 + n]
  got = torch.full((n, k, H, W, C), float('nan'), device=dev)
  ops.gather_windows_augmented_into(got, addr, kind, big_s[3:3 + n], col, n, k, H, W, C)
  torch.cuda.synchronize()
  return got.cpu().numpy()


def _check_against_float64(dev, eps, k, H, W, C, with_colour):
  fe = H * W * C
  values = _plain_values(eps, PICKS, k, fe).reshape(N, k, H, W, C)
  colour = _colour(C) if with_colour else None
  if with_colour:       # both clamps act on some elements
    raw = values * colour[:, None, None, None, :C].astype(np.float64) + colour[:, None, None, None, C:].astype(np.float64)
    assert (raw < 0).any() and (raw > 1).any()
  for shift in _shift_tables(H, W):
    got = _augmented(dev, eps, PICKS, k, H, W, C, shift, colour)
    want = augment_windows(values, shift, colour)
    assert got.dtype == np.float32 and not np.isnan(got).any()              # the poisoned output was overwritten everywhere
    err = np.abs(got.astype(np.float64) - want).max()
    assert err <= 1e-6, (shift.tolist(), err)
    for n in range(N):
      outside = ~in_view(H, W, *shift[n])
      assert not got[n][:, outside].any(), shift[n].tolist()                # exactly 0.0 where zeros move in
    if with_colour and not shift.any():
      assert (got == 0.0).any() and (got == 1.0).any()                      # ... and the kernel's clamps gave the bounds themselves


@pytest.mark.parametrize('with_colour', [False, True], ids=['plain', 'colour'])
@pytest.mark.parametrize('kinds', list(KINDS))
@pytest.mark.parametrize('C', [3, 1])
@pytest.mark.parametrize('hw', SHAPES, ids=lambda hw: '%dx%d' % hw)
def test_augmented_gather_is_the_float64_restatement(dev, hw, C, kinds, with_colour):
  H, W = hw
  _check_against_float64(dev, _episodes(dev, H * W * C, KINDS[kinds]), K, H, W, C, with_colour)


@pytest.mark.parametrize('C', [3, 1])
def test_target_stream_of_single_frames(dev, C):
  """K = 1: the goal model's 'target_rgb' / 'target_depth' stream through the same launch."""
  H, W = 8, 12
  _check_against_float64(dev, _episodes(dev, H * W * C, KINDS['mixed']), 1, H, W, C, C == 3)


def _odd_episodes(dev, fe, u8):
  """[one-ELEMENT-offset view, aligned episode, the view again]: a uint8 episode 1 byte off a 4-byte boundary, a float32 episode
  4 bytes off a 16-byte boundary, next to an aligned episode in the same launch."""
  r = np.random.default_rng(11 + fe)
  host = r.integers(0, 256, [1 + T_EP * fe]).astype(np.uint8) if u8 else r.random([1 + T_EP * fe], dtype=np.float32)
  buf = torch.from_numpy(host).to(dev)
  odd = buf[1:].view(T_EP, fe)
  assert odd.data_ptr() % (4 if u8 else 16) == (1 if u8 else 4)
  return [odd, _episodes(dev, fe, KINDS['uint8' if u8 else 'float32'])[1], odd], buf


@pytest.mark.parametrize('u8', [True, False], ids=['uint8', 'float32'])
@pytest.mark.parametrize('C', [3, 1])
def test_unaligned_windows(dev, C, u8):
  """Frames whose base is not aligned for the vector loads: every shifted source is read narrower, and the narrow reads of the
  first and last group of a frame stay inside it (uint8: no aligned word around them lies in the frame)."""
  H, W = 8, 12
  eps, _keep = _odd_episodes(dev, H * W * C, u8)
  _check_against_float64(dev, eps, K, H, W, C, True)


@pytest.mark.parametrize('kinds', list(KINDS))
@pytest.mark.parametrize('C', [3, 1])
@pytest.mark.parametrize('hw', SHAPES, ids=lambda hw: '%dx%d' % hw)
def test_identity_and_pure_shifts_are_bitwise_the_plain_gather(dev, hw, C, kinds):
  H, W = hw
  fe = H * W * C
  eps = _episodes(dev, fe, KINDS[kinds])
  plain = _plain_f32(dev, eps, PICKS, K, fe).reshape(N, K, H, W, C)
  zeros = np.zeros((N, 2), np.int32)
  identity = np.tile(np.float32([1] * C + [0] * C), (N, 1))
  for colour in (None, identity):
    got = _augmented(dev, eps, PICKS, K, H, W, C, zeros, colour)
    assert np.array_equal(got.view(np.uint32), plain.view(np.uint32)), colour is None
  for shift in _shift_tables(H, W):
    got = _augmented(dev, eps, PICKS, K, H, W, C, shift, None)
    want = np.stack([moved(plain[n], *shift[n]) for n in range(N)])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), shift.tolist()
    # ... and a pure shift under the identity colour is the same move
    got = _augmented(dev, eps, PICKS, K, H, W, C, shift, identity)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), shift.tolist()


def test_unaligned_pure_shifts_are_bitwise(dev):
  H, W, C = 8, 12, 3
  fe = H * W * C
  for u8 in (True, False):
    eps, _keep = _odd_episodes(dev, fe, u8)
    plain = _plain_f32(dev, eps, PICKS, K, fe).reshape(N, K, H, W, C)
    for shift in _shift_tables(H, W):
      got = _augmented(dev, eps, PICKS, K, H, W, C, shift, None)
      want = np.stack([moved(plain[n], *shift[n]) for n in range(N)])
      assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (u8, shift.tolist())


def test_argument_checks_return_the_error_code(dev):
  """Bad arguments return GEECO_EINVAL before anything is launched (the output keeps its poison) and raise through ops."""
  from geeco_amd import _native, ops
  lib = _native.load()
  H, W, C = 6, 4, 3
  fe = H * W * C
  ep = _episodes(dev, fe, KINDS['uint8'])[0]
  addr = torch.tensor([ep.data_ptr(), ep.data_ptr() + fe], dtype=torch.int64, device=dev)
  kind = torch.zeros(2, dtype=torch.int32, device=dev)
  shift = torch.zeros((2, 2), dtype=torch.int32, device=dev)
  col = torch.ones((2, 6), device=dev)
  out = torch.full((2, K, H, W, C), float('nan'), device=dev)
  a, k, s, c, o = (t.data_ptr() for t in (addr, kind, shift, col, out))
  call = lib.geeco_gather_windows_augmented
  for args in ((None, k, s, c, 2, K, H, W, C, o), (a, None, s, c, 2, K, H, W, C, o), (a, k, None, c, 2, K, H, W, C, o),
               (a, k, s, c, 2, K, H, W, C, None), (a, k, s, c, 2, K, H, W, 2, o), (a, k, s, c, 2, K, H, W, 4, o),
               (a, k, s, c, 2, K, H, W, C, o + 4), (a, k, s, c, 0, K, H, W, C, o), (a, k, s, c, 2, 0, H, W, C, o),
               (a, k, s, c, 2, K, 0, W, C, o), (a, k, s, c, 2, K, H, 0, C, o), (a, k, s, c, 65536, K, H, W, C, o),
               (a + 4, k, s, c, 2, K, H, W, C, o), (a, k, s + 2, c, 2, K, H, W, C, o), (a, k, s, c, 2, K, 1 << 16, 1 << 16, 1, o)):
    assert call(*args, None) == _native.GEECO_EINVAL, args
    assert lib.geeco_last_error()
  assert call(a, k, s, c, 2, K, H, W, 2, o, None) == _native.GEECO_EINVAL and b'C=2' in lib.geeco_last_error()
  torch.cuda.synchronize()
  assert torch.isnan(out).all()
  with pytest.raises(_native.GeecoNativeError, match='C=2'):
    ops.gather_windows_augmented_into(out, addr, kind, shift, None, 2, K, H, W, 2)
  with pytest.raises(ValueError, match='tables'):
    ops.gather_windows_augmented_into(out, addr, kind, shift.to(torch.int64), col, 2, K, H, W, C)
  with pytest.raises(ValueError, match='tables'):
    ops.gather_windows_augmented_into(out, addr, kind, shift, col[:1], 2, K, H, W, C)
  with pytest.raises(ValueError, match='output of'):
    ops.gather_windows_augmented_into(out[:1], addr, kind, shift, col, 2, K, H, W, C)
  assert call(a, k, s, None, 2, K, H, W, C, o, None) == 0                 # ... and the good call still runs (colour may be NULL)
  torch.cuda.synchronize()
  assert not torch.isnan(out).any()


# ================================================================================================
# the recorded values of the kernel this entry point launched before the builders shared one body
# ================================================================================================
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'augmented_gather.npz')
# 5 x 5 x 3: rows of 15 elements, the one-element path, and frames of 75 bytes at changing residues; 4 x 8 x 3: the vector path;
# 4 x 8 x 1: the C = 1 instance.  N = 3 windows of K = 3 frames from starts 0, 2, 1 of ONE episode of 5 frames.
GOLDEN_CASES = [(5, 5, 3, 'uint8'), (4, 8, 3, 'uint8'), (4, 8, 3, 'float32'), (4, 8, 1, 'float32'), (4, 8, 1, 'uint8')]
GOLDEN_STARTS = (0, 2, 1)


def golden_shifts(H, W):
  """[2 launches][3 windows][2]: interior, the right and the left edge groups; three ways out of the frame."""
  return np.asarray([[(0, 0), (1, -2), (-1, 3)], [(0, W), (H, 0), (-H - 1, W + 1)]], np.int32)


def golden_offsets(dtype):
  """Elements between a 16-byte aligned address and the episode: byte residues 0..3 (uint8), 16- and 4-byte alignment (float32)."""
  return (0, 1, 2, 3) if dtype == 'uint8' else (0, 1)


def golden_gather(dev, episode, offset, H, W, C, shift, colour, entry='augmented'):
  """[3][3][H][W][C] float32: the GOLDEN_STARTS windows of ``episode`` (host [5][H * W * C]) resident ``offset`` elements behind
  an aligned address, through ONE launch of ``entry``: 'augmented', 'scene' without extras, 'frames' with the consecutive table."""
  from geeco_amd import ops
  fe, n, k = H * W * C, len(GOLDEN_STARTS), 3
  flat = torch.from_numpy(np.ascontiguousarray(episode).ravel())
  buf = torch.zeros(offset + flat.numel(), dtype=flat.dtype, device=dev)
  buf[offset:] = flat.to(dev)
  size = buf.element_size()
  assert buf.data_ptr() % 16 == 0
  addr = np.asarray([buf.data_ptr() + (offset + st * fe) * size for st in GOLDEN_STARTS], np.int64)
  if entry == 'frames':
    addr = addr[:, None] + np.arange(k, dtype=np.int64)[None, :] * fe * size
  addr = torch.from_numpy(addr).to(dev)
  kind = torch.full((n,), 0 if size == 1 else 1, dtype=torch.int32, device=dev)
  shift = torch.from_numpy(np.ascontiguousarray(shift, np.int32)).to(dev)
  col = None if colour is None else torch.from_numpy(np.ascontiguousarray(colour, np.float32)).to(dev)
  got = torch.full((n, k, H, W, C), float('nan'), device=dev)
  if entry == 'augmented':
    ops.gather_windows_augmented_into(got, addr, kind, shift, col, n, k, H, W, C)
  else:
    getattr(ops, 'gather_windows_%s_into' % entry)(got, addr, kind, shift, col, None, None, None, 0.0, 0, n, k, H, W, C)
  torch.cuda.synchronize()
  return got.cpu().numpy()


def test_augmented_gather_reproduces_the_recorded_values(dev):
  """Bitwise the arrays scripts/record_augmented_golden.py recorded from the kernel geeco_gather_windows_augmented launched
  before it took an instance of the shared body -- every case, residue, shift launch, with and without colour -- and the scene
  entry without extras (C = 3) and the frames entry under the consecutive table write the same values."""
  gold = np.load(GOLDEN)
  for i, (H, W, C, dtype) in enumerate(GOLDEN_CASES):
    episode, colour, want = gold['episode%d' % i], gold['colour%d' % i], gold['out%d' % i]
    assert episode.dtype == np.dtype(dtype) and want.dtype == np.float32
    assert want.shape == (len(golden_offsets(dtype)), 2, 2, 3, 3, H, W, C)
    for a, offset in enumerate(golden_offsets(dtype)):
      for b, shift in enumerate(golden_shifts(H, W)):
        for c, col in enumerate((colour, None)):
          for entry in ('augmented', 'frames') + (('scene',) if C == 3 else ()):
            got = golden_gather(dev, episode, offset, H, W, C, shift, col, entry)
            assert np.array_equal(got.view(np.uint32), want[a, b, c].view(np.uint32)), (H, W, C, dtype, offset, b, col is None, entry)


# ================================================================================================
# through the feed and the Estimator
# ================================================================================================
HH = 136
K3 = 3
AUG = dict(shift=9, gain=0.3, bias=0.1)
MODELS = {'e2e_vmc': (False, dict()), 'geeco_f': (True, dict(proc_obs='dynimg', proc_tgt='dyndiff'))}
IMAGES = ('rgb', 'target_rgb', 'depth', 'target_depth')


def _batches(root, device, **kw):
  from geeco_amd import input_fn as I
  kw = dict(dict(window_size=K3, batch_size=4, num_threads=2, seed=3), **kw)
  if device is not None:
    kw = dict(dict(device=device, device_keys=('rgb',), cache=False), **kw)
  return list(I.pickplace_input_fn(root, 'default', 'train', **kw))


def _host_augmented(host, devb):
  """The host pipeline's dense batches with the helper's transform under the draws the device batches carry."""
  out = []
  for (fh, lh), (fd, _) in zip(host, devb):
    for k in ('step', 'goal_state', 'jnt_state'):
      np.testing.assert_array_equal(fd[k], fh[k], err_msg=k)        # the same windows
    aug = fd['rgb'].augment
    f = dict(fh)
    for k in IMAGES:
      if k in fh:
        f[k] = augment_windows(fh[k], aug.shift, aug.colour if fh[k].shape[-1] == 3 else None).astype(np.float32)
    out.append((f, lh))
  return out


@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
  """2 episodes x 8 windows of K = 3 at 136 x 136: four full batches of 4."""
  from geeco_amd import input_fn as I
  root = str(tmp_path_factory.mktemp('augment_ds'))
  I.write_synthetic_dataset(root, 2, episode_length=11, img_hw=(HH, HH), seed=9)
  return root


def _close(got, want, what):
  np.testing.assert_allclose(got, want, rtol=1e-4, atol=2e-5, err_msg=what)


@pytest.mark.parametrize('name', list(MODELS))
def test_estimator_step_matches_host_augmented_windows(dev, dataset, name):
  """One step fed through pickplace_input_fn(device=, augment=) against the same model fed, through load_batch, dense windows the
  helper augmented on the host with the same draws: loss and predictions.  Then three more steps, the last two replayed under
  the hipGraph step: after every feed the model's image inputs are the host-augmented windows of THAT batch."""
  from geeco_amd import estimator as est, graph
  from geeco_amd import input_fn as I
  from geeco_amd.params import create_e2evmc_config
  goal, kw = MODELS[name]
  devb = _batches(dataset, 'cuda', fetch_target=goal, augment=AUG)
  want = _host_augmented(_batches(dataset, None, fetch_target=goal), devb)
  assert len(devb) == 4 and all(len(f['step']) == 4 and f['rgb'].augmented and f['rgb'].is_u8() for f, _ in devb)
  assert any((f['rgb'].augment.shift != 0).any() for f, _ in devb)
  cfg = create_e2evmc_config(dict(kw, window_size=K3, img_height=HH, img_width=HH, batch_size=4))
  e = est.Estimator(est.goal_e2evmc_model_fn if goal else est.e2evmc_model_fn, None, est.RunConfig(init_seed=4, use_hipgraph=True),
                    {'e2evmc_config': cfg, 'log_steps': 10 ** 9})
  ref = (graph.GoalE2EVMC if goal else graph.E2EVMC)(cfg, 4, dev, training=True)
  ref.store.initialize(seed=4)
  image_inputs = ('rgb', 'target_rgb') if goal else ('rgb',)
  for i, ((fd, ld), (fh, lh)) in enumerate(zip(devb, want)):
    spec, fbuf, lbuf = e._get_spec(est.ModeKeys.TRAIN, fd, ld, 4)
    e._feed_step(fbuf, lbuf, fd, ld)
    torch.cuda.synchronize()
    for k in image_inputs:
      slot = fbuf[k]
      assert isinstance(slot, I.WindowFeed) and slot.form == 'dense_augmented' and slot.table is None and not slot.u8, (k, slot.form)
      assert spec.model.inputs[k] is slot.buffer
      got = slot.buffer.cpu().numpy()
      assert got.shape == fh[k].shape and np.abs(got.astype(np.float64) - fh[k]).max() <= 1e-6, (i, k)
    spec.train_op()
    torch.cuda.synchronize()
    loss = float(spec.model.loss)
    assert np.isfinite(loss)
    if i == 0:
      preds = {k: v.detach().cpu().numpy().copy() for k, v in spec.model.predictions().items()}
      ref.load_batch({k: torch.from_numpy(v) for k, v in fh.items()}, {k: torch.from_numpy(v) for k, v in lh.items()})
      ref.train_step()
      torch.cuda.synchronize()
      print('%s: loss %.9g through the augmented feed, %.9g from host-augmented windows' % (name, loss, float(ref.loss)))
      _close(loss, float(ref.loss), 'loss')
      ref_preds = ref.predictions()
      assert set(preds) == set(ref_preds) and preds
      for k in preds:
        _close(preds[k], ref_preds[k].detach().cpu().numpy(), k)
  assert len(e._specs) == 1 and next(iter(e._specs))[-1] == 'augmented'
  runner = spec.train_op.__self__
  assert runner._graphs is not None and runner._calls == 4          # steps 3 and 4 were replays
  assert int(e._store.global_step.item()) == 4
  spec.model.check_device_errors()


def test_shuffled_and_augmented(dev, dataset):
  """shuffle_windows with augment: the slot is 'dense_augmented' (not 'dense_by_address'), the step runs, and the first batch
  is the host pipeline's shuffled batch of the same picks, host-augmented."""
  from geeco_amd import estimator as est
  from geeco_amd.params import create_e2evmc_config
  kw = dict(shuffle_windows=True, shuffle_buffer=8, fetch_target=True)
  devb = _batches(dataset, 'cuda', augment=AUG, **kw)[:1]
  want = _host_augmented(_batches(dataset, None, **kw)[:1], devb)
  assert devb[0][0]['rgb'].scattered and devb[0][0]['rgb'].augmented and len(devb[0][0]['rgb'].segments) > 1
  cfg = create_e2evmc_config(dict(proc_obs='dynimg', proc_tgt='dyndiff', window_size=K3, img_height=HH, img_width=HH, batch_size=4))
  e = est.Estimator(est.goal_e2evmc_model_fn, None, est.RunConfig(init_seed=4), {'e2evmc_config': cfg, 'log_steps': 10 ** 9})
  e.train(input_fn=lambda: iter(devb))
  torch.cuda.synchronize()
  (spec, fbuf, lbuf), = e._specs.values()
  for k in ('rgb', 'target_rgb'):
    assert fbuf[k].form == 'dense_augmented' and fbuf[k].scattered
    got = spec.model.inputs[k].cpu().numpy()
    assert np.abs(got.astype(np.float64) - want[0][0][k]).max() <= 1e-6, k
  assert np.isfinite(float(spec.model.loss)) and int(e._store.global_step.item()) == 1


def test_rgbd_streams_share_the_shift_and_depth_keeps_its_values(dev, dataset):
  """All four image streams of an RGB-D goal batch through the feed alone (one arena block, one launch per stream): 'depth' and
  'target_depth' are moved by the windows' shifts and not tinted; DeviceWindows.numpy() gives the same augmented windows."""
  from geeco_amd import feed
  devb = _batches(dataset, 'cuda', fetch_target=True, augment=AUG, device_keys=('rgb', 'depth'))[:2]
  host = _batches(dataset, None, fetch_target=True)[:2]
  want = _host_augmented(host, devb)
  fbuf, lbuf = feed.build_slots(dev, *devb[0])
  bufs = {k: fbuf[k].dense() for k in IMAGES}
  assert all(fbuf[k].form == 'dense_augmented' for k in IMAGES)
  assert fbuf.arena.has(('features', 'rgb', 'aug_colour')) and not fbuf.arena.has(('features', 'depth', 'aug_colour'))
  fbuf, lbuf = feed.adopted_slots(fbuf, lbuf, {})
  assert set(fbuf) == set(IMAGES)
  for (fd, ld), (fh, _), (plain, _) in zip(devb, want, host):
    feed.feed_step(fbuf, lbuf, fd, ld)
    torch.cuda.synchronize()
    got = {k: bufs[k].cpu().numpy() for k in IMAGES}
    for k in IMAGES:
      assert got[k].shape == fh[k].shape and np.abs(got[k].astype(np.float64) - fh[k]).max() <= 1e-6, k
    shift = fd['rgb'].augment.shift
    for k in ('depth', 'target_depth'):       # moved, bitwise: no arithmetic touches a one-channel stream
      moved_depth = np.stack([moved(plain[k][n], *shift[n]) for n in range(len(shift))])
      assert np.array_equal(got[k].view(np.uint32), moved_depth.view(np.uint32)), k
    assert np.array_equal(fd['rgb'].numpy().view(np.uint32), got['rgb'].view(np.uint32))
    assert np.array_equal(fd['target_depth'].numpy().view(np.uint32), got['target_depth'].view(np.uint32))


def test_shared_frames_refuse_an_augmenting_input(dev, dataset):
  from geeco_amd import estimator as est
  from geeco_amd.params import create_e2evmc_config
  cfg = create_e2evmc_config(dict(window_size=K3, img_height=HH, img_width=HH, batch_size=4))
  e = est.Estimator(est.e2evmc_model_fn, None, est.RunConfig(), {'e2evmc_config': cfg, 'shared_frames': True})
  with pytest.raises(ValueError, match='augmenting input'):
    e.train(input_fn=lambda: iter(_batches(dataset, 'cuda', augment=AUG)), steps=1)
