"""Batched predictor (geeco_amd/batched_predictor.py, csrc/predict_io.hip) without a GPU: the C ABI of its four entries, their
host-side argument checks, the uint8 division it relies on, and the window semantics its kernels are held to on the GPU
(WindowModel below is that specification; tests/test_batched_predictor_gpu.py compares the kernels against it bitwise)."""
import ctypes
import os
import re

import numpy as np

import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('geeco_predict_range_check', 'geeco_predict_push_dense', 'geeco_predict_push_ring', 'geeco_predict_pack')


class WindowModel:
  """B envs' K-frame windows after a sequence of pushes, in both device forms:
  * dense [B][K][...]: reset -> every slot = the frame; else slots shift down by one and slot K-1 = the frame;
  * mirrored ring [B][2K][...] with a head p per env: the frame goes to slots p and p + K (every slot after a reset), the
    window is slots p + 1 .. p + K (``start``), then p = (p + 1) % K."""

  def __init__(self, B, K, frame_shape, dtype=np.float32):
    self.B, self.K = B, K
    self.dense = np.zeros((B, K) + tuple(frame_shape), dtype)
    self.ring = np.zeros((B, 2 * K) + tuple(frame_shape), dtype)
    self.heads = np.zeros(B, np.int64)
    self.start = np.zeros(B, np.int64)

  def push(self, frames, reset):
    K = self.K
    for b in range(self.B):
      if reset[b]:
        self.dense[b][:] = frames[b]
        self.ring[b][:] = frames[b]
      else:
        self.dense[b][:-1] = self.dense[b][1:].copy()
        self.dense[b][-1] = frames[b]
        p = self.heads[b]
        self.ring[b][p] = frames[b]
        self.ring[b][p + K] = frames[b]
      p = self.heads[b]
      self.start[b] = p + 1
      self.heads[b] = (p + 1) % K

  def ring_window(self, b):
    return self.ring[b, self.start[b]:self.start[b] + self.K]


class Batch1Window:
  """The reference's frame buffer (its predictor.py:144-146, 192-200): the newest frame replaces the oldest, the first frame after
  a reset fills the whole window.  The window kernels are tested against it bitwise."""

  def __init__(self, K):
    self.K, self.buf, self.filled = K, None, 0

  def reset(self):
    self.filled = 0

  def feed(self, frame):
    if self.filled == 0:
      self.buf = np.stack([frame] * self.K)
    else:
      self.buf = np.concatenate([self.buf[1:], frame[None]])
    self.filled = min(self.filled + 1, self.K)
    return self.buf


def test_entries_declared_exported_typed_at_abi_7():
  from geeco_amd import _native
  for name in ENTRIES:
    assert name in _abi.functions(), name
    assert name in _native.SIGNATURES, name
  lib = ctypes.CDLL(_native.LIB_PATH)
  for name in ENTRIES:
    assert hasattr(lib, name), name
  assert _abi.define('GEECO_ABI_VERSION') == 7
  assert _native.ABI_VERSION == 7 and _native.load().geeco_abi_version() == 7


def test_every_library_build_compiles_predict_io():
  """Every recipe that builds a libgeeco_hip*.so from csrc (product, variant, stamps) compiles the same product
  sources: a library without predict_io would report ABI 7 yet lack its entries, and _native.load() refuses it.
  The list is spelled once, in csrc/sources.sh; every recipe sources that file and loops over its list, and none spells
  a list of its own."""
  src = open(os.path.join(ROOT, 'geeco_amd/csrc/sources.sh')).read()
  m = re.search(r'^HIP_SOURCES="([a-z0-9_ ]+)"$', src, flags=re.M)
  assert m and len(re.findall(r'HIP_SOURCES=', src)) == 1
  files = m.group(1).split()
  assert 'predict_io' in files and len(set(files)) == len(files)
  for f in files:
    assert os.path.exists(os.path.join(ROOT, 'geeco_amd/csrc', f + '.hip')), f
  for rel in ('geeco_amd/csrc/build.sh', 'scripts/dev/build_variant.sh', 'scripts/dev/build_stamps.sh'):
    text = open(os.path.join(ROOT, rel)).read()
    assert re.search(r'^\. \./sources\.sh\b', text, flags=re.M), rel
    loops = re.findall(r'^for f in (.+); do', text, flags=re.M)
    assert loops == ['$HIP_SOURCES'], (rel, loops)
    assert 'HIP_SOURCES=' not in text and 'predict_io' not in text, rel


def test_argument_checks_need_no_gpu():
  """Every rejection comes back as -1 with its message, before any launch."""
  from geeco_amd import _native
  lib = _native.load()
  one = ctypes.c_void_p(256)
  err = lambda: lib.geeco_last_error()
  # range check: null, B, C
  assert lib.geeco_predict_range_check(None, 2, 64, 3, 0.0, 1.0, one, None) == -1 and b'null pointer' in err()
  assert lib.geeco_predict_range_check(one, 0, 64, 3, 0.0, 1.0, one, None) == -1 and b'B=0' in err()
  assert lib.geeco_predict_range_check(one, 2, 64, 5, 0.0, 1.0, one, None) == -1 and b'C=5' in err()
  # dense push: null, B, K, C, uint8 RGB-D
  dense = lambda fr, u8, B, K, C, depth=one: lib.geeco_predict_push_dense(fr, u8, one, one, one, B, K, 64, C, 7, one, depth,
                                                                           one, None)
  assert dense(None, 0, 2, 3, 3) == -1 and b'null pointer' in err()
  assert dense(one, 0, 2, 3, 4, depth=None) == -1 and b'null pointer' in err()
  assert dense(one, 0, -1, 3, 3) == -1 and b'B=-1' in err()
  assert dense(one, 0, 2, 0, 3) == -1 and b'K=0' in err()
  assert dense(one, 0, 2, 65, 3) == -1 and b'K=65' in err()
  assert dense(one, 0, 2, 3, 2) == -1 and b'C=2' in err()
  assert dense(one, 1, 2, 3, 4) == -1 and b'uint8 frames are RGB' in err()
  # ring push: null, B, K, HW % 4
  ring = lambda fr, B, K, HW: lib.geeco_predict_push_ring(fr, one, one, one, B, K, HW, 7, one, one, one, one, None)
  assert ring(None, 2, 3, 64) == -1 and b'null pointer' in err()
  assert ring(one, 0, 3, 64) == -1 and b'B=0' in err()
  assert ring(one, 2, 65, 64) == -1 and b'K=65' in err()
  assert ring(one, 2, 3, 66) == -1 and b'multiple of 4' in err()
  # pack: null, B, C of the images, segments outside the predictions
  s = (ctypes.c_int * 1)(0)
  n = (ctypes.c_int * 1)(3)
  a = (ctypes.c_int * 1)(0)
  pack = lambda pr, B, P, F, img, C: lib.geeco_predict_pack(pr, P, B, 1, s, n, a, one, F, one, one, img, None, 64, C, one, None)
  assert pack(None, 2, 3, 3, None, 0) == -1 and b'null pointer' in err()
  assert pack(one, 0, 3, 3, None, 0) == -1 and b'B=0' in err()
  assert pack(one, 2, 2, 3, None, 0) == -1 and b'outside' in err()
  assert pack(one, 2, 3, 3, one, 5) == -1 and b'C=5' in err()


def test_uint8_division_is_the_float_path_exhaustively():
  """uint8 mode changes nothing: for all 256 byte values the reference's rgb / 255.0 (float64, then float32) equals the float32
  the device produces, float(u8) / 255.0f with the IEEE division (geeco_gather_windows divisor 255, the dense push, the ring
  form's input kernel)."""
  v = np.arange(256)
  ref = (v / 255.0).astype(np.float32)
  dev = np.arange(256, dtype=np.float32) / np.float32(255.0)
  assert dev.dtype == np.float32
  np.testing.assert_array_equal(ref.view(np.uint32), dev.view(np.uint32))


def test_range_bounds_are_the_batch1_check():
  """The float32 bounds the range-check kernel compares against accept exactly the float32 values the batch-1 check accepts."""
  from geeco_amd.batched_predictor import range_bounds
  from geeco_amd.predictor import TOL_FRAME_RANGE
  lo, hi = range_bounds()
  for b in (lo, hi):
    assert float(np.float32(b)) == b
  ok = lambda x: -TOL_FRAME_RANGE <= float(x) <= 1 + TOL_FRAME_RANGE
  for b, out in ((np.float32(lo), -np.inf), (np.float32(hi), np.inf)):
    assert ok(b) and not ok(np.nextafter(b, np.float32(out)))


def test_window_model_agrees_with_batch1_windows():
  """The B-env window (dense and ring forms) equals B independent batch-1 windows over random call sequences with random
  reset masks (the first call of every env pads its window)."""
  r = np.random.default_rng(0)
  for B, K in ((1, 1), (3, 2), (5, 4), (7, 16)):
    wm = WindowModel(B, K, (2, 3))
    ref = [Batch1Window(K) for _ in range(B)]
    pending = np.ones(B, bool)
    for call in range(40):
      if call and r.random() < 0.5:
        for b in np.flatnonzero(r.random(B) < 0.3):
          pending[b] = True
          ref[b].reset()
      frames = r.standard_normal((B, 2, 3)).astype(np.float32)
      wm.push(frames, pending)
      pending[:] = False
      for b in range(B):
        want = ref[b].feed(frames[b])
        np.testing.assert_array_equal(wm.dense[b], want)
        np.testing.assert_array_equal(wm.ring_window(b), want)
        assert 1 <= wm.start[b] <= K
