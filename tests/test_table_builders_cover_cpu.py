"""The launch-variant table of the frame-table kernels (tests/_table_builder_cases.py: CASES), on the host: from the Python mirrors of
the launch rules alone it reaches every one of the 19 instantiations of csrc/replay.hip, replay_dynimg.hip and shared_frames.hip and
runs every loop of theirs a second, ragged time; the image cases' extrema are planted where a missed item or partial changes the
result; the host models agree with one another; and tests/test_table_builders_variants_gpu.py launches this table and nothing else.
No GPU needed."""
import numpy as np
import pytest

import _replay_dynimg_ref as D
import _replay_ref as R
import _table_builder_cases as C

PLANS = {c.id: C.plan(c) for c in C.CASES}
IMAGES = C.cases('replay_images')


def _need(what, found):
  """Every instantiation, loop and edge by the id of a case that holds it."""
  assert found, 'no case holds: ' + what
  print('%-86s %s' % (what, found[0].id))
  return found[0]


def _second_trip(c, loop):
  t = PLANS[c.id]['loops'].get(loop)
  return t is not None and t[0] >= 2 and t[1]


def _by_name(entry, name):
  return [c for c in C.cases(entry) if name in PLANS[c.id]['names']]


def test_ids_are_unique_and_entries_known():
  assert len({c.id for c in C.CASES}) == len(C.CASES)
  assert {c.entry for c in C.CASES} == set(C.ENTRIES)
  assert sum(len(C.cases(e)) for e in C.ENTRIES) == len(C.CASES)


STATE_NAMES = ['replay_states_kernel<4, true>', 'replay_states_kernel<4, false>', 'replay_states_kernel<1, false>']
IMAGE_TMPL = ['<%s, %s>' % (u, b) for u in ('true', 'false') for b in ('true', 'false')]


def test_every_instantiation_has_a_case():
  names = set()
  for name in STATE_NAMES:
    for mode in C.MODES:
      _need('%s through replay_states, mode %s' % (name, mode), [c for c in _by_name('replay_states', name) if c.a['mode'] == mode])
    _need('%s through replay_states_pair' % name, _by_name('replay_states_pair', name))
    names.add(name)
  for name in ('replay_errors_frame_kernel', 'replay_errors_episode_kernel'):
    _need(name, _by_name('replay_errors', name))
    names.add(name)
  for kernel in ('replay_images_minmax_kernel', 'replay_images_emit_kernel'):
    for t in IMAGE_TMPL:
      _need(kernel + t, _by_name('replay_images', kernel + t))
      names.add(kernel + t)
  for name, entry in [('pack_frames_kernel<true>', 'pack_frames'), ('pack_frames_kernel<false>', 'pack_frames'),
                      ('window_states_fwd_kernel<4>', 'window_states_fwd'), ('window_states_fwd_kernel<1>', 'window_states_fwd'),
                      ('window_states_bwd_kernel<4>', 'window_states_bwd'), ('window_states_bwd_kernel<1>', 'window_states_bwd')]:
    _need(name, _by_name(entry, name))
    names.add(name)
  assert len(names) == 19
  assert {n for p in PLANS.values() for n in p['names']} == names      # and the table launches nothing else
  # the alignment rules on their own: a width that would take 16-byte accesses, one pointer a float off
  for what, found in [('replay_states: the table misaligned', [c for c in C.cases('replay_states') if c.a['feat_off'] % 4 and c.a['ch'] % 4 == 0]),
                      ('replay_states: the target row misaligned', [c for c in C.cases('replay_states') if c.a['tgt_off'] % 4 and c.a['mode'] != 'plain']),
                      ('replay_states: the states misaligned', [c for c in C.cases('replay_states') if c.a['states_off'] % 4]),
                      ('replay_states_pair: the second table misaligned', [c for c in C.cases('replay_states_pair') if c.a['tgt_off'] % 4]),
                      ('window_states_fwd: the table misaligned', [c for c in C.cases('window_states_fwd') if c.a['feat_off'] % 4 and c.a['ch'] % 4 == 0]),
                      ('window_states_bwd: dfeat misaligned', [c for c in C.cases('window_states_bwd') if c.a['dfeat_off'] % 4 and c.a['ch'] % 4 == 0])]:
    c = _need(what, found)
    assert PLANS[c.id]['names'][0].endswith(('<1, false>', '<4, false>', '<1>')), c.id
  c = [c for c in C.cases('replay_states') if c.a['states_off'] % 4][0]
  assert PLANS[c.id]['names'] == ['replay_states_kernel<4, false>']      # loads stay 16 bytes wide, only the stores give way


def test_replay_states_loops_pass_the_capped_grid():
  cap = C.RP_MAX_BLOCKS * C.RP_THREADS
  for name in STATE_NAMES:
    for entry, loops in (('replay_states', ('table0', 'joint')), ('replay_states_pair', ('table0', 'table1', 'joint'))):
      for loop in loops:
        c = _need('%s via %s: second ragged trip of %s' % (name, entry, loop), [c for c in _by_name(entry, name) if _second_trip(c, loop)])
        p, a = PLANS[c.id], c.a
        assert p['grid'] == C.RP_MAX_BLOCKS
        n = a['t1'] - a['t0']
        units = {'table0': a['K'] * n * a['cells'] * a['ch'] // p['V'], 'joint': a['K'] * n * a['cells'] * a['J']}
        if entry == 'replay_states_pair':
          units['table1'] = a['K'] * n * a['cells'] * a['ch_t'] // p['V']
        assert cap < units[loop] < 2 * cap and p['loops'][loop] == (2, True)      # the issue's conditions, restated
    for mode in C.MODES:      # each mode's own stores (append / subtract) behind the cap
      _need('%s, mode %s: second trip of the table loop' % (name, mode),
            [c for c in _by_name('replay_states', name) if c.a['mode'] == mode and _second_trip(c, 'table0')])
  for c in C.cases('replay_states_pair'):
    assert c.a['ch'] != c.a['ch_t']      # a table read with the other's width gives other values
  # the first-frame padding in a second trip: the windows start before frame K - 1
  for c in C.cases('replay_states') + C.cases('replay_states_pair'):
    assert c.a['t0'] < c.a['K'] - 1 and c.a['t0'] > 0 and c.a['pad'] > 0, c.id


def test_replay_errors_blocks():
  for what, pick in (('squared-error heads alone', lambda ks: ks == {0}), ('class-hit heads', lambda ks: 1 in ks)):
    c = _need('replay_errors with ' + what, [c for c in C.cases('replay_errors') if pick({h[2] for h in c.a['heads']})])
    assert _second_trip(c, 'frame_blocks') and PLANS[c.id]['loops']['episode'][0] >= 2 and c.a['T'] > C.RP_THREADS


def test_replay_images_loops():
  for t in IMAGE_TMPL:
    name = 'replay_images_emit_kernel' + t
    c = _need('%s (and minmax): second ragged trip of the item loop' % name, [c for c in _by_name('replay_images', name) if _second_trip(c, 'items')])
    assert PLANS[c.id]['grid'] == C.RP_MAX_BLOCKS and (c.a['t1'] - c.a['t0']) * PLANS[c.id]['bpw'] > C.RP_MAX_BLOCKS
    c = _need('%s: second ragged trip of the fold over the partials' % name, [c for c in _by_name('replay_images', name) if _second_trip(c, 'fold')])
    assert PLANS[c.id]['bpw'] > C.RP_THREADS
  # one block serves items of different windows AND different block indices in successive trips
  c = _need('item loop at bpw = 3', [c for c in IMAGES if PLANS[c.id]['bpw'] == 3 and _second_trip(c, 'items')])
  assert C.RP_MAX_BLOCKS % 3 != 0 and (c.a['HW'] // 4) % C.RP_THREADS != 0      # ... and the last block of a window is ragged
  _need('item loop at bpw = 1', [c for c in IMAGES if PLANS[c.id]['bpw'] == 1 and _second_trip(c, 'items')])
  for c in IMAGES:
    assert c.a['t1'] == c.a['T'] and (c.a['t0'] >= 1 and c.a['K'] >= 2 if c.a['buf'] else True), c.id      # (window 0's buffer image has no range)


def test_shared_frame_loops():
  for V in (4, 1):
    for entry, loops in (('window_states_fwd', ('units', 'joint')), ('window_states_bwd', ('units', 'positions', 'targets'))):
      name = '%s_kernel<%d>' % (entry, V)
      for loop in loops:
        _need('%s: second ragged trip of %s' % (name, loop), [c for c in _by_name(entry, name) if _second_trip(c, loop)])
      for mode in C.MODES:
        _need('%s, mode %s: second trip of the unit loop' % (name, mode),
              [c for c in _by_name(entry, name) if c.a['mode'] == mode and _second_trip(c, 'units')])
  for c in C.cases('window_states_bwd'):
    if _second_trip(c, 'targets'):
      assert c.a['N'] > 64
  # the LDS position list at its limit, every position naming one slot and every target one other slot
  for mode in ('constant', 'residual'):
    c = _need('N * K = %d positions in one slot, mode %s' % (C.SF_MAX_POSITIONS, mode),
              [c for c in C.cases('window_states_bwd') if c.a['kind'] == 'full' and c.a['mode'] == mode])
    F, idx, tgt = C.shared_indices(c.a)
    assert idx.size == C.SF_MAX_POSITIONS and len(set(idx.ravel())) == 1 and len(set(tgt)) == 1 and idx[0, 0] != tgt[0] and F == 3
  # slots outside [0, F) on both sides, in both lists
  for entry, Vs in (('window_states_fwd', (4, 1)), ('window_states_bwd', (4,))):      # (the forward reads through the index, both widths)
    for V in Vs:
      for mode in ('constant', 'residual'):
        c = _need('%s<%d>, mode %s: slots -1 and F' % (entry, V, mode),
                  [c for c in C.cases(entry) if c.a['mode'] == mode and PLANS[c.id]['V'] == V
                   and (c.a.get('out_of_range') or c.a.get('kind') == 'out_of_range')])
        F, idx, tgt = C.shared_indices(c.a)
        assert {-1, F} <= set(idx.ravel()) and {-1, F} <= set(tgt) and idx.min() == -1 and idx.max() == F
  for c in C.cases('window_states_fwd') + C.cases('window_states_bwd'):
    F, idx, tgt = C.shared_indices(c.a)
    assert c.a['N'] * c.a['K'] <= C.SF_MAX_POSITIONS and c.a['pad'] > 0
    if c.a.get('kind', 'disjoint') == 'disjoint' and not c.a.get('out_of_range'):
      assert F - 1 not in set(idx.ravel()) | set(tgt) and not set(idx.ravel()) & set(tgt), c.id      # an unreferenced slot; goal slots of their own


def test_pack_frames_grid():
  for u8 in (True, False):
    for path in ('quad', 'pixel'):
      c = _need('pack_frames_kernel<%s>: a second, ragged block on the %s path' % ('true' if u8 else 'false', path),
                [c for c in C.cases('pack_frames') if c.a['u8'] == u8 and PLANS[c.id]['sized'] == path and PLANS[c.id]['grid_x'] >= 2
                 and PLANS[c.id]['last_block_ragged']])
      assert path in PLANS[c.id]['loops'] and 'zero' in PLANS[c.id]['loops']
  for c in C.cases('pack_frames'):
    p = PLANS[c.id]
    # the grid covers the frame on the path it is sized for: px += step never runs a second time there (a grid cap would show here)
    assert p['loops'][p['sized']][0] == 1, c.id
    if p['sized'] == 'pixel':
      assert all(t[0] == 1 for t in p['loops'].values()), c.id
  # ... but a slot that leaves the 4-pixel path (misaligned, or unused) walks HW pixels under the grid sized for HW / 4 units
  for u8 in (True, False):
    c = _need('pack_frames_kernel<%s>: px += step runs again for a misaligned slot' % ('true' if u8 else 'false'),
              [c for c in C.cases('pack_frames') if c.a['u8'] == u8 and PLANS[c.id]['sized'] == 'quad' and _second_trip(c, 'pixel')])
    assert _second_trip(c, 'zero')


# ---- the image cases' planting ---------------------------------------------------------------------------------------------
_planted = {}


def planted(c):
  if c.id not in _planted:
    ep = C.planted_episode(c.a)
    _planted[c.id] = ep + (C.check_planted(c.a, *ep),)
  return _planted[c.id]


@pytest.mark.parametrize('c', IMAGES, ids=lambda c: c.id)
def test_image_extrema_are_planted_where_a_missed_item_shows(c):
  a, p = c.a, PLANS[c.id]
  frames, goal, binary, pair_binary, where = planted(c)
  assert set(where) == ({'buf', 'diff'} if a['buf'] else {'diff'})
  print('%s: smallest range %s' % (c.id, {k: round(v['range'], 4) for k, v in where.items()}))
  # the planted pixels hold the bytes 0 and 255 alone
  assert np.isin(frames[:, binary], (0, 255)).all() and np.isin(goal[pair_binary], (0, 255)).all() and set(pair_binary) <= set(binary)
  n, bpw = a['t1'] - a['t0'], p['bpw']
  if a['plant'] == 'fold':
    for name, w in where.items():
      swapped = 1 if name == 'buf' else 0      # (window index within the range: t = 2 for the buffer image, t = 1 for the pair image)
      for i in range(n):
        want = (256, 0) if i == swapped else (0, 256)
        assert (w['max_blocks'][i], w['min_blocks'][i]) == want, (name, i)
    assert bpw == 257
    return
  # 'items': the windows whose items a block reaches in its second trip hold their extrema in just those items
  items = np.arange(n)[:, None] * bpw + np.arange(bpw)[None]      # [window][block] -> item
  second = items >= p['grid']
  assert second.any() and not second.all()
  for name, w in where.items():
    mx2 = second[np.arange(n), w['max_blocks']]
    mn2 = second[np.arange(n), w['min_blocks']]
    assert mx2.any() and mn2.any(), name
    late = second.all(1)      # windows served wholly by second trips
    if bpw > 1 and name == 'buf':
      assert set(w['max_blocks'][late]) == set(range(bpw)) and set(w['min_blocks'][late]) == set(range(bpw))      # the extrema walk the blocks
    if bpw > 1 and name == 'diff':
      assert set(w['max_blocks']) == {0} and set(w['min_blocks']) == {bpw - 1}


@pytest.mark.parametrize('c', IMAGES, ids=lambda c: c.id)
def test_image_host_models_agree(c):
  """The float32 values of the planted pixels lie within the derived bound of the float64 restatement; their minimum is 0.0 and their
  maximum the issue's expression; the restatement is _replay_dynimg_ref.images_ref in float64 on a few windows."""
  a = c.a
  frames, goal, binary, pair_binary, _ = planted(c)
  f32, g32 = C.as_unit(frames), C.as_unit(goal)
  im = C.images_f64(f32, g32, a['K'], a['t0'], a['t1'], a['buf'])
  for name, d in im.items():
    pix = binary if name == 'buf' else pair_binary
    got, mn, mx = C.planted_f32(frames, goal, a['K'], a['t0'], a['t1'], pix, name)
    bound = C.image_bound(d)
    assert (np.abs(got - d['y'][:, pix]) <= bound[:, pix]).all(), name
    assert (got.reshape(len(mn), -1).min(1) == 0.0).all()
    r = (mx - mn).astype(np.float32)
    assert np.array_equal(got.reshape(len(mn), -1).max(1), (r / (r + np.float32(1e-6)).astype(np.float32)).astype(np.float32))
    assert bound.max() < 1e-3 and np.median(bound) < 2e-5, (name, bound.max(), np.median(bound))      # a bound that still means something
  rows = [0, (a['t1'] - a['t0']) // 2, a['t1'] - a['t0'] - 1]
  for i in rows:
    t = a['t0'] + i
    cur, b, diff = D.images_ref(f32[:t + 1], g32, a['K'], t, t + 1, buf=a['buf'], dtype=np.float64)
    np.testing.assert_allclose(im['diff']['y'][i], diff[0][:, :3], rtol=0, atol=1e-9)
    if a['buf']:
      np.testing.assert_allclose(im['buf']['y'][i], b[0][:, :3], rtol=0, atol=1e-9)


# ---- the host models of the states ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', C.MODES)
def test_shared_frame_models_are_the_replay_models(mode):
  """window_states_fwd_ref through the window index rule is states_ref; the scatter-sum is the adjoint of the gather."""
  T, K, cells, ch, J = 6, 3, 2, 4, 3
  r = np.random.default_rng(3)
  feat = r.standard_normal((T + 1, cells, ch)).astype(np.float32)      # slot T: the goal frame
  jnt = r.standard_normal((T, J)).astype(np.float32)
  idx = R.window_index(T, K).astype(np.int32)
  tgt = np.full(T, T, np.int32)
  got = C.window_states_fwd_ref(feat, idx, jnt[idx], tgt, mode)
  np.testing.assert_array_equal(got, R.states_ref(feat[:T], jnt, feat[T], mode, K, 0, T))
  # <d, gather(feat)> == <scatter(d), feat> wherever the ReLU mask is open (feat > 0 everywhere here)
  pos = np.abs(feat) + 0.5
  d = r.standard_normal(got.shape)
  ref, mag = C.window_states_bwd_ref(d, pos, idx, tgt, mode, J)
  lhs = (d * C.window_states_fwd_ref(pos.astype(np.float64), idx, np.zeros((T, K, J)), tgt, mode).astype(np.float64)).sum()
  assert abs(lhs - (ref * pos).sum()) <= 1e-5 * (mag * pos).sum()
  # out of range: nothing read, nothing contributed
  idx2, tgt2 = idx.copy(), tgt.copy()
  idx2[2, 1], tgt2[4] = -1, T + 1
  g2 = C.window_states_fwd_ref(feat, idx2, jnt[idx], tgt2, mode).reshape(K, T, cells, -1)
  assert not g2[1, 2, :, :ch].any() if mode == 'plain' else True
  r2, _ = C.window_states_bwd_ref(d, pos, idx2, tgt2, mode, J)
  assert r2.shape == ref.shape and np.isfinite(r2).all()


def test_distinct_tables_are_distinct():
  (a, b), jnt, tgt = C.distinct_tables(9, 3, [4, 5], 2)
  every = np.concatenate([x.ravel() for x in (a, b, jnt, tgt)])
  assert len(np.unique(every)) == every.size and np.array_equal(every, np.round(every))


# ---- the device test launches this table ---------------------------------------------------------------------------------------
def test_the_device_test_is_parametrised_by_this_table():
  import test_table_builders_variants_gpu as G
  tests = {k: v for k, v in vars(G).items() if k.startswith('test_')}
  seen = []
  for name, fn in tests.items():
    marks = [m for m in getattr(fn, 'pytestmark', []) if m.name == 'parametrize']
    assert len(marks) == 1 and marks[0].args[0] == 'c', name
    cs = list(marks[0].args[1])
    assert cs and len({c.entry for c in cs}) == 1 and cs == C.cases(cs[0].entry), name
    seen += cs
  assert len(tests) == len(C.ENTRIES) and sorted(c.id for c in seen) == sorted(c.id for c in C.CASES)
  assert any(m.name == 'gpu' for m in G.pytestmark) if isinstance(G.pytestmark, list) else G.pytestmark.name == 'gpu'
