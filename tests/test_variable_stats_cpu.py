"""The host side of the opt-in per-variable statistics: the restatement tests/_varstats_ref.py on values classed by
hand, the values ``variable_stats`` takes, the chunk table, ``update_norm`` from fabricated sums, the HistogramProto bytes read back
by the project's own wire reader, and the new entry points as header and binding declare them."""
import importlib.util
import os
import re
import struct

import numpy as np
import pytest

import _varstats_ref as V

import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('geeco_variable_stats', 'geeco_variable_stats_ws_bytes')
CH = 4096


def test_classes_of_hand_picked_values():
  f = np.float32
  below_two = np.nextafter(f(2.0), f(0.0))
  #            value, class (None: in no class), non-finite, zero
  cases = [(f(0.0), None, False, True), (f(1e-45), 0, False, False), (f(2.0) ** f(-33), 0, False, False), (f(2.0) ** f(-32), 0, False, False),
           (np.nextafter(f(2.0) ** f(-31), f(0.0)), 0, False, False), (f(2.0) ** f(-31), 1, False, False), (f(1.0), 32, False, False),
           (below_two, 32, False, False), (f(2.0), 33, False, False), (f(127.9), 38, False, False), (f(128.0), 39, False, False),
           (f(3e38), 39, False, False), (f(np.inf), None, True, False), (f(np.nan), None, True, False)]
  for sign in (1.0, -1.0):
    x = np.array([f(sign) * c[0] for c in cases], np.float32)
    cls, negative, nonfinite, zero = V.classes(x)
    for i, (val, want, nf, z) in enumerate(cases):
      assert cls[i] == (-1 if want is None else want), (sign, val)
      assert bool(nonfinite[i]) == nf and bool(zero[i]) == z, (sign, val)
      if not np.isnan(val):
        assert bool(negative[i]) == (sign < 0), (sign, val)      # -0.0 is negative by its bit and still a zero
    t = V.tensor(x)
    assert t['nonfinite'] == 2 and t['zeros'] == 1
    side, other = (t['pos'], t['neg']) if sign > 0 else (t['neg'], t['pos'])
    assert other.sum() == 0 and side.sum() == len(cases) - 3
    assert side[0] == 4 and side[1] == 1 and side[32] == 2 and side[33] == 1 and side[38] == 1 and side[39] == 2
    finite = np.array([float(sign) * float(c[0]) for c in cases if not c[2]])
    assert t['sum'] == pytest.approx(finite.sum(), rel=1e-12) and t['min'] == finite.min() and t['max'] == finite.max()
  # the product is classed as the float32 it rounds to: 1.5 * 2^-149 * 0.5 is a denormal or zero in float32, never 7.5e-46
  r = V.record(np.array([1e-45, 3.0], np.float32), [True, True], np.ones(2, np.float32), np.zeros(2, np.float32), np.ones(2, np.float32), grad_scale=0.25)
  assert r['grad']['zeros'] == 1 and r['grad']['pos'][31] == 1 and r['grad_covered'] == 2
  # nothing finite: the extrema are the empty ones
  t = V.tensor(np.array([np.nan, np.inf], np.float32))
  assert t['min'] == np.inf and t['max'] == -np.inf and t['sum'] == 0.0 and t['nonfinite'] == 2


def test_update_direction_by_hand():
  u = V.update(np.array([3.0, -8.0, np.nan, 1.0], np.float32), np.array([4.0, 16.0, 1.0, -1.0], np.float32), 0.0)
  assert u['nonfinite'] == 2 and u['max_abs'] == 2.0 and u['sumsq'] == 1.5 ** 2 + 2.0 ** 2


@pytest.mark.parametrize('bad', [0, 1, 2.0, 'yes', 'scalars', 'histogram', [True], {}])
def test_bad_variable_stats_is_refused_by_name(bad):
  from geeco_amd import estimator as est
  from geeco_amd.variables import check_variable_stats
  with pytest.raises(ValueError, match='variable_stats'):
    check_variable_stats(bad)
  with pytest.raises(ValueError, match=r"params\['variable_stats'\]"):
    est.Estimator(est.e2evmc_model_fn, None, est.RunConfig(), {'variable_stats': bad})


def test_variable_stats_off_and_on_values():
  from geeco_amd import estimator as est
  from geeco_amd import graph
  from geeco_amd.params import create_e2evmc_config
  from geeco_amd.variables import check_variable_stats
  assert check_variable_stats(None) is None and check_variable_stats(False) is None
  assert check_variable_stats(True) == 'scalars' and check_variable_stats('histograms') == 'histograms'
  for ok in (None, False, True, 'histograms'):
    est.Estimator(est.e2evmc_model_fn, None, est.RunConfig(), {'variable_stats': ok})
  cfg = create_e2evmc_config(dict(window_size=2, img_height=136, img_width=136))
  with pytest.raises(ValueError, match='variable_stats'):
    graph.E2EVMC(cfg, 2, 'cpu', variable_stats='all')


def test_command_line_flags():
  spec = importlib.util.spec_from_file_location('train_e2evmc_vs', os.path.join(ROOT, 'scripts', 'train_e2evmc.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  base = ['--dataset_dir', 'd', '--split_name', 's', '--model_dir', 'm']
  args = mod.ARGPARSER.parse_args(base)
  assert 'variable_stats' not in mod.estimator_params(args, None)
  assert mod.estimator_params(mod.ARGPARSER.parse_args(base + ['--variable_stats']), None)['variable_stats'] is True
  assert mod.estimator_params(mod.ARGPARSER.parse_args(base + ['--variable_stats_histograms']), None)['variable_stats'] == 'histograms'


def test_the_chunk_table_covers_every_element_once_and_no_pad():
  from geeco_amd import ops
  variables = [(0, 1), (4, 3), (8, CH), (8 + CH, CH + 1), (2 * CH + 16, 3 * CH + 7), (8 * CH, 70001), (8 * CH + 70004, 5)]
  t = ops.variable_stats_table(variables)
  nvar = len(variables)
  nch = (t.size - 2 * nvar) // 2
  assert t.dtype == np.int64 and nch == sum(-(-c // CH) for _, c in variables)
  head, chunks = t[:2 * nvar].reshape(nvar, 2), t[2 * nvar:].reshape(nch, 2)
  size = max(o + c for o, c in variables)
  seen = np.zeros(size, int)
  nxt = 0
  for (off, cnt), (first, n) in zip(variables, head):
    assert first == nxt and n == -(-cnt // CH)
    nxt += n
    for k in range(n):
      o, c = chunks[first + k]
      assert o == off + k * CH and o % 4 == 0 and 1 <= c <= CH and o + c <= off + cnt      # inside ITS variable
      assert c == CH or k == n - 1
      seen[o:o + c] += 1
  inside = np.zeros(size, bool)
  for off, cnt in variables:
    inside[off:off + cnt] = True
  assert (seen[inside] == 1).all() and (seen[~inside] == 0).all() and (~inside).sum() > 0
  for bad in ([(2, 4)], [(0, 0)], [(-4, 4)]):
    with pytest.raises(ValueError):
      ops.variable_stats_table(bad)
  assert ops.variable_stats_ws_bytes(nch) >= nch * (16 + 4 * V.CLASSES) * 4 and ops.variable_stats_ws_bytes(nch) % 16 == 0
  assert ops.variable_stats_ws_bytes(0) == 0


def _rec(count, covered, g_sumsq, p_sumsq, u_sumsq, g_nonfinite=0):
  z = np.zeros(V.CLASSES, np.int64)
  t = lambda ss, nf, n: dict(nonfinite=nf, zeros=1, sum=2.0, sumsq=ss, min=-3.0, max=2.0, neg=z, pos=z + (n > 0))
  return dict(grad_covered=covered, grad=t(g_sumsq, g_nonfinite, covered), param=t(p_sumsq, 0, count), update_nonfinite=0,
              update_sumsq=u_sumsq, update_max_abs=1.0)


def test_update_norm_follows_multiplier_frozen_and_skipped():
  from geeco_amd.variables import variable_stats_scalars
  rec = _rec(10, 10, 16.0, 4.0, 9.0)
  d = variable_stats_scalars(rec, 10, 0.5)
  assert d['update_norm'] == 0.5 * 3.0 and d['weight_norm'] == 2.0 and d['update_ratio'] == 0.75 and d['grad_norm'] == 4.0
  assert d['grad_max_abs'] == 3.0 and d['grad_mean'] == 0.2 and d['grad_zero_fraction'] == 0.1 and d['grad_nonfinite'] == 0
  assert d['weight_max_abs'] == 3.0 and d['weight_nonfinite'] == 0 and 'histograms' not in d
  assert variable_stats_scalars(rec, 10, 0.5, multiplier=0.1)['update_norm'] == pytest.approx(0.1 * d['update_norm'], rel=1e-15)
  skipped = variable_stats_scalars(_rec(10, 10, 16.0, 4.0, 9.0, g_nonfinite=2), 10, 0.5, applied=False)
  assert skipped['update_norm'] == 0.0 and skipped['update_ratio'] == 0.0 and skipped['grad_nonfinite'] == 2 and skipped['grad_mean'] == 0.25
  frozen = variable_stats_scalars(_rec(10, 0, 0.0, 4.0, 9.0), 10, 0.5, multiplier=0.0)
  assert frozen['update_norm'] == 0.0 and frozen['weight_norm'] == 2.0
  assert all(frozen[k] is None for k in ('grad_norm', 'grad_max_abs', 'grad_mean', 'grad_zero_fraction', 'grad_nonfinite'))
  assert variable_stats_scalars(_rec(10, 10, 1.0, 0.0, 9.0), 10, 0.5)['update_ratio'] is None      # weights all zero: no ratio
  h = variable_stats_scalars(rec, 10, 0.5, histograms=True)['histograms']
  assert set(h) == {'gradients', 'weights'} and h['weights']['num'] == 10 and h['gradients']['sum_squares'] == 16.0
  assert set(variable_stats_scalars(_rec(10, 0, 0.0, 4.0, 9.0), 10, 0.5, 0.0, histograms=True)['histograms']) == {'weights'}


def _decode_event(payload):
  from geeco_amd.tfrecord import _fields
  out = {'scalars': {}, 'histograms': {}}
  for fnum, wt, val in _fields(payload):
    if fnum == 2:
      out['step'] = val
    if fnum == 5:
      for f2, _, value in _fields(val):
        assert f2 == 1
        tag, simple, histo = None, None, None
        for f3, w3, x in _fields(value):
          if f3 == 1:
            tag = bytes(x).decode()
          elif f3 == 2 and w3 == 5:
            simple = struct.unpack('<f', bytes(x))[0]
          elif f3 == 5:
            histo = {}
            for f4, w4, y in _fields(x):
              if w4 == 1:
                histo[f4] = struct.unpack('<d', bytes(y))[0]
              else:
                histo[f4] = np.frombuffer(bytes(y), '<f8')
        if histo is not None:
          out['histograms'][tag] = histo
        else:
          out['scalars'][tag] = simple
  return out


def test_histogram_proto_bytes_read_back(tmp_path):
  from geeco_amd import summary
  from geeco_amd.tfrecord import read_records
  edges = summary.histogram_edges()
  assert len(edges) == 2 * V.CLASSES + 2 and all(a < b for a, b in zip(edges, edges[1:]))
  dbl_max = float(np.finfo(np.float64).max)
  assert edges[0] == -dbl_max and edges[-1] == dbl_max and edges[V.CLASSES + 1] == 0.0
  # negative class k (exponent e = k - 32) ends at -2^e, positive class k at 2^(e + 1)
  assert edges[1] == -128.0 and edges[V.CLASSES] == -(2.0 ** -32) and edges[V.CLASSES + 2] == 2.0 ** -31 and edges[V.CLASSES + 2 + 32] == 2.0
  x = np.array([0.0, -0.0, 1.0, 1.5, -3.0, 200.0, -1e-40, np.nan], np.float32)
  t = V.tensor(x)
  h = dict(min=t['min'], max=t['max'], num=x.size - t['nonfinite'], sum=t['sum'], sum_squares=t['sumsq'], zeros=t['zeros'],
           neg=[int(v) for v in t['neg']], pos=[int(v) for v in t['pos']])
  w = summary.EventFileWriter(str(tmp_path / 'h'))
  w.add_scalars({'loss': 0.5}, 3, wall_time=1.0)
  w.add_histograms({'weights/a/kernel': h}, 3, wall_time=1.0)
  w.close()
  records = [bytes(r) for r in read_records(w.path, compression=None)]
  assert len(records) == 3
  ev = _decode_event(records[2])
  got = ev['histograms']['weights/a/kernel']
  assert ev['step'] == 3 and not ev['scalars']
  assert (got[1], got[2], got[3], got[4], got[5]) == (-3.0, 200.0, 7.0, t['sum'], t['sumsq'])
  assert list(got[6]) == edges and got[7].sum() == 7.0
  # every finite value lies in the bucket its edges describe: (previous edge, edge] below zero, [previous edge, edge) above
  want = np.zeros(len(edges))
  for v in x[np.isfinite(x)].astype(np.float64):
    if v == 0:
      want[V.CLASSES + 1] += 1
    elif -(2.0 ** -32) < v < 0:
      want[V.CLASSES] += 1      # the clamped negative class 0 also holds what is smaller in magnitude than its edge
    elif v < 0:
      want[next(i for i, e in enumerate(edges) if v <= e)] += 1
    else:
      want[next(i for i, e in enumerate(edges) if v < e)] += 1
  np.testing.assert_array_equal(got[7], want)
  # a scalar-only event stays byte for byte what it was: Event{wall_time, step, Summary{Value{tag, simple_value}}}
  tag = b'loss'
  value = b'\x0a' + bytes([len(tag)]) + tag + b'\x15' + struct.pack('<f', 0.5)
  summ = b'\x0a' + bytes([len(value)]) + value
  assert records[1] == b'\x09' + struct.pack('<d', 1.0) + b'\x10\x03' + b'\x2a' + bytes([len(summ)]) + summ


def test_header_declares_and_binding_binds():
  from geeco_amd import _native, ops
  added = _abi.added_within(7)
  for name in NEW:
    assert name in added and name in _abi.functions(), name
    assert name in _native.SIGNATURES
  assert len(_native.SIGNATURES['geeco_variable_stats'][1]) == len(_abi.functions()['geeco_variable_stats'][1])
  assert _abi.define('GEECO_VARSTATS_CHUNK') == _native.VARSTATS_CHUNK == CH
  assert _abi.define('GEECO_VARSTATS_CLASSES') == _native.VARSTATS_CLASSES == V.CLASSES
  lib = _native.load()
  assert lib.geeco_variable_stats_ws_bytes(1) * 3 == lib.geeco_variable_stats_ws_bytes(3)
  # the record as numpy reads it is the struct the header declares: 8 + 2 * (16 + 16 + 2 * 40 * 8) + 8 + 8 bytes
  assert ops.VARSTATS_DTYPE.itemsize == 8 + 2 * (32 + 2 * V.CLASSES * 8) + 16
  assert ops.VARSTATS_DTYPE.fields['param'][1] == 8 + 32 + 2 * V.CLASSES * 8 and ops.VARSTATS_DTYPE.fields['update_sumsq'][1] == 1360
  # refusals that need no GPU: nothing is launched for them
  import ctypes
  one = ctypes.c_void_p(64)
  seg = (_native.AdamSegment * 1)()
  seg[0].g, seg[0].p_off, seg[0].count = 64, 0, 8
  off, cnt = (ctypes.c_int64 * 2)(0, 4), (ctypes.c_int64 * 2)(4, 4)
  call = lambda p=one, nseg=1, nvar=2, nch=2, o=off, c=cnt: lib.geeco_variable_stats(p, one, one, seg, nseg, 8, 1.0, 1e-8, o, c, nvar, one, nch, one, one, None)
  assert call(p=None) == -1 and b'null pointer' in lib.geeco_last_error()
  assert call(nvar=0) == -1 and call(nseg=9) == -1 and b'pieces' in lib.geeco_last_error()
  assert call(o=(ctypes.c_int64 * 2)(0, 6)) == -1 and b'multiple of 4' in lib.geeco_last_error()
  assert call(c=(ctypes.c_int64 * 2)(5, 4)) == -1 and b'overlap' in lib.geeco_last_error()
  assert call(nch=3) == -1 and b'chunks' in lib.geeco_last_error()
