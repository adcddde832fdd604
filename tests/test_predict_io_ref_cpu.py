"""The host models of tests/_predict_io_ref.py on hand-written cases, the properties of np.argmax the output pack claims, the
inputs the GPU case tables of tests/test_predict_io_variants_gpu.py build, and the completeness of those tables: every kernel
instantiation predict_io.hip launches is named by a trace note and expected by some case."""
import os
import re

import numpy as np

import _predict_io_ref as R
import test_predict_io_variants_gpu as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float('nan'), float('inf')

# the instantiations predict_io.hip launches, read off its dispatch code: 4 + 6 + 3 + 6 + 2 + 2 = 23
INSTANCES = [
    'range_check_kernel<3>', 'range_check_kernel<4>', 'range_check_scalar_kernel<3>', 'range_check_scalar_kernel<4>',
    'push_dense_kernel<4, 3, true>', 'push_dense_kernel<4, 3, false>', 'push_dense_kernel<4, 4, false>',
    'push_dense_kernel<1, 3, true>', 'push_dense_kernel<1, 3, false>', 'push_dense_kernel<1, 4, false>',
    'push_ring_kernel<u32x4>', 'push_ring_kernel<unsigned>', 'ring_advance_kernel',
    'pack_newest_kernel<4, 3, true>', 'pack_newest_kernel<4, 3, false>', 'pack_newest_kernel<4, 4, false>',
    'pack_newest_kernel<1, 3, true>', 'pack_newest_kernel<1, 3, false>', 'pack_newest_kernel<1, 4, false>',
    'push_features_kernel<4>', 'push_features_kernel<1>',
    'pack_preds_kernel', 'pack_image_kernel',
]


def _argmax1(q):
  return float(R.pack_preds(np.array([q], np.float32), [(0, len(q), 1)])[0, 0])


# ---- np.argmax, the rule the kernel claims ---------------------------------------------------------------------------------------
def test_np_argmax_first_maximum_first_nan_signed_zero():
  assert np.argmax(np.float32([1, 3, 3])) == 1 and np.argmax(np.float32([2, 2, 2])) == 0            # the first maximum
  assert np.argmax(np.float32([1, NAN, 9])) == 1 and np.argmax(np.float32([NAN, 9, NAN])) == 0      # the first NaN wins
  assert np.argmax(np.float32([9, 1, NAN])) == 2
  assert np.argmax(np.float32([-0.0, 0.0])) == 0 and np.argmax(np.float32([0.0, -0.0])) == 0        # -0.0 == +0.0: a tie
  assert np.argmax(np.float32([-INF, -INF])) == 0 and np.argmax(np.float32([1, INF, INF])) == 1


def test_pack_preds_argmax_segments():
  assert _argmax1([3, 2, 1]) == -1.0 and _argmax1([1, 3, 2]) == 0.0 and _argmax1([1, 2, 3]) == 1.0   # first, middle, last
  assert _argmax1([2, 2, 1]) == -1.0 and _argmax1([1, 2, 2]) == 0.0 and _argmax1([2, 2, 2]) == -1.0  # tied
  assert _argmax1([NAN, 5, 1]) == -1.0 and _argmax1([1, NAN, 5]) == 0.0                              # NaN before a larger value
  assert _argmax1([5, 1, NAN]) == 1.0 and _argmax1([0, NAN, 9]) == 0.0                               # and after one
  for v in (0.5, NAN, INF, -INF):
    assert _argmax1([v]) == -1.0                                                                     # a length-1 segment
  assert R.pack_preds(np.zeros((2, 3), np.float32), [(0, 3, 1)]).dtype == np.float32


def test_pack_preds_copies_in_segment_order():
  p = np.arange(22, dtype=np.float32).reshape(2, 11)
  p[0, 4] = -0.0
  p[1, 10] = NAN
  segs = [(9, 2, 0), (2, 3, 1), (0, 3, 0), (4, 1, 0)]          # the argmax segment and the second copy share column 2
  got = R.pack_preds(p, segs)
  assert R.pack_width(segs) == 7 and got.shape == (2, 7)
  want = np.float32([[9, 10, 0, 0, 1, 2, -0.0], [20, NAN, 1, 11, 12, 13, 15]])    # argmax(2, 3, -0.0) - 1, argmax(13, 14, 15) - 1
  np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


def test_pack_images_slots_follow_the_images_given():
  a = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
  b = -a
  assert R.pack_images([None, None], 3) is None
  np.testing.assert_array_equal(R.pack_images([a, None], 3), a[None, :, :, :3])
  np.testing.assert_array_equal(R.pack_images([None, b], 3), b[None, :, :, :3])          # img1 alone lands in slot 0
  both = R.pack_images([a, b], 4)
  assert both.shape == (2, 2, 3, 4)
  np.testing.assert_array_equal(both[0], a)
  np.testing.assert_array_equal(both[1], b)


def test_newest_input():
  f = np.float32([[[0.1, 0.2, 0.3], [0.4, 0.5, 0.6]]])
  np.testing.assert_array_equal(R.newest_input(f, 3), np.float32([[[0.1, 0.2, 0.3, 0], [0.4, 0.5, 0.6, 0]]]))
  d = np.float32([[[0.1, 0.2, 0.3, 7.0]]])
  np.testing.assert_array_equal(R.newest_input(d, 4), d)
  u = np.uint8([[[0, 255, 51]]])
  np.testing.assert_array_equal(R.newest_input(u, 3), np.float32([[[0, 1, np.float32(51) / np.float32(255), 0]]]))


def test_range_flags():
  from geeco_amd.batched_predictor import range_bounds
  lo, hi = range_bounds()
  lo32, hi32 = np.float32(lo), np.float32(hi)
  up, down = np.nextafter(hi32, np.float32(INF)), np.nextafter(lo32, np.float32(-INF))
  f = np.full((8, 2, 3), 0.5, np.float32)
  f[0, 1, 2] = hi32
  f[1, 0, 0] = up
  f[2, 1, 1] = lo32
  f[3, 0, 2] = down
  f[4, 0, 0] = NAN
  f[5, 1, 0] = -0.0
  f[6, 1, 2] = INF
  assert R.range_flags(f, 3, lo, hi).tolist() == [0, 1, 0, 1, 1, 0, 1, 0, 1]
  assert R.range_flags(f[[0, 2, 5, 7]], 3, lo, hi).tolist() == [0, 0, 0, 0, 0]
  # words set by an earlier check stay; the any-env word is set only by a bad env
  assert R.range_flags(f[[0, 2]], 3, lo, hi, ctl=[0, 1, 0]).tolist() == [0, 1, 0]
  assert R.range_flags(f[[0, 1]], 3, lo, hi, ctl=[1, 0, 0]).tolist() == [1, 1, 1]
  # depth (channel 3) is exempt, channels 0..2 are not
  d = np.full((3, 2, 4), 0.5, np.float32)
  d[0, 1, 3] = 7.0
  d[1, 0, 3] = NAN
  d[2, 1, 2] = 1.1
  assert R.range_flags(d, 4, lo, hi).tolist() == [0, 0, 1, 1]


# ---- the inputs of the GPU cases -------------------------------------------------------------------------------------------------
def test_range_case_envs_hold_the_edges():
  from geeco_amd.batched_predictor import range_bounds
  lo, hi = range_bounds()
  for c in V.RANGE_CASES:
    HW, C = c['HW'], c['C']
    n = HW * C
    pos = V.range_positions(HW, C, c['off'])
    per_pass, vec = V.range_geometry(HW, C, c['off'])
    assert vec == ('scalar' not in c['names'][0]), c['id']
    assert all(0 <= e < n and e % C < 3 for e in pos.values()), (c['id'], pos)
    assert pos['first'] == 0 and pos['last'] >= n - 2
    assert len({pos[k] % 4 for k in pos if k.startswith('lane')}) == (4 if C == 3 else 3)
    if 'pass1-first' in pos:
      assert pos['pass0-last'] < per_pass <= pos['pass1-first'] < n
    if HW >= 1024:                                       # the two cases of more than one block
      assert 'pass1-first' in pos and 'last-pass-first' in pos and pos['last-pass-first'] >= 2 * per_pass
    if c['id'] == '64-block-cap':
      assert per_pass == 64 * 256 * 4 and -(-(n // 4) // 1024) > 64 and -(-(295 * 295 * 3 // 4) // 1024) <= 64
      continue                                           # (its frames are a megabyte each: the small cases show the builder)
    frames, must, tags = V.range_envs(c, lo, hi)
    assert frames.dtype == np.float32 and frames.shape == (len(tags), n)
    want = R.range_flags(frames.reshape(-1, HW, C), C, lo, hi)
    assert (want[:-1] == must).all() and want[-1] == 1, c['id']
    assert must.sum() == 5 * len(pos)                    # every position with every value
    for t in ('all-hi', 'all-lo', 'neg-zero', 'clean') + (('depth-all-7', 'depth-nan', 'depth-last-inf') if C == 4 else ()):
      assert not must[tags.index(t)]
    for b in np.flatnonzero(must):                       # exactly one planted value: putting 0.5 there makes the env clean
      bad = ~((frames[b] >= np.float32(lo)) & (frames[b] <= np.float32(hi)))
      assert bad.sum() == 1, tags[b]


def test_pack_case_rows_hold_the_edges():
  for segs in (V.SEGS, V.SEGS_MAX):
    assert all(src + n <= V.PACK_P for src, n, _ in segs)
    lens = sorted(n for _, n, am in segs if am)
    assert lens[:3] == [1, 3, 5] and any(not am for _, _, am in segs)
    p = V.pack_rows(300, segs)
    assert p.shape == (300, V.PACK_P) and p.dtype == np.float32
    src, n, _ = [s for s in segs if s[2]][0]             # the first argmax segment's patterns sit in the first rows
    pats = V.argmax_patterns(n)
    got = p[:len(pats), src:src + n]
    np.testing.assert_array_equal(got.view(np.uint32), np.array(pats, np.float32).view(np.uint32))
    assert sum(len(V.argmax_patterns(n)) for _, n, am in segs if am) < 255
  assert V.PACK_P % 4 and len(V.SEGS_MAX) == V.MAXSEG
  a, b = V.SEGS[0], V.SEGS[1]
  assert a[0] + a[1] > b[0] and not a[2] and b[2]        # two segments overlap in src
  three = V.argmax_patterns(3)
  bits = {np.array(p, np.float32).tobytes() for p in three}
  has = lambda *q: np.array(q, np.float32).tobytes() in bits
  assert has(1, 1, 0) and has(0, 1, 1) and has(1, 0, 1) and has(2, 2, 2)                             # ties, all equal
  assert has(-0.0, 0.0, -1) and has(0.0, -0.0, -1)                                                   # -0.0 against +0.0
  assert has(1, INF, INF) and has(-INF, -INF, -INF)
  assert has(NAN, 5, 1) and has(1, NAN, 5) and has(1, 5, NAN) and has(0, NAN, 9)                     # NaN first, middle, last
  assert {int(np.argmax(np.float32(p))) for p in three} == {0, 1, 2}
  five = np.array(V.argmax_patterns(5), np.float32)
  assert five.shape[1] == 5 and all(np.array(p, np.float32).tobytes() in {r[1:4].tobytes() for r in five} for p in three)
  assert np.isnan(five[:, -1]).any() and (five == five[:, :1]).all(axis=1).any()


# ---- completeness ----------------------------------------------------------------------------------------------------------------
def test_every_launch_is_noted_and_every_instance_has_a_case():
  src = open(os.path.join(ROOT, 'geeco_amd/csrc/predict_io.hip')).read()
  launches, notes = len(re.findall(r'hipLaunchKernelGGL\(', src)), re.findall(r'geeco_note_kernel\("([^"]+)"', src)
  assert launches == len(re.findall(r'geeco_note_kernel\(', src)) == len(notes) == 17
  # every note sits on the line in front of its launch and names the kernel launched there
  for m in re.finditer(r'geeco_note_kernel\("([a-z_]+)[^\n]*\n\s*hipLaunchKernelGGL\(\(?([a-z_]+)', src):
    assert m.group(1) == m.group(2)
  assert len(re.findall(r'geeco_note_kernel\("([a-z_]+)[^\n]*\n\s*hipLaunchKernelGGL\(\(?([a-z_]+)', src)) == launches
  # the notes, with PIX written out, are the list; the list is what the case tables expect
  spelled = set()
  for n in notes:
    spelled |= {n.replace('%d', p) for p in ('1', '4')} if '%d' in n else {n}
  assert len(INSTANCES) == len(set(INSTANCES)) == 23
  assert spelled == set(INSTANCES)
  assert V.expected_instances() == set(INSTANCES)
  for entry, cases in V.ALL_CASES.items():
    ids = [c['id'] for c in cases]
    assert len(set(ids)) == len(ids), entry
