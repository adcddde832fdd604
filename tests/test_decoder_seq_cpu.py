"""geeco_lstm_seq_heads_fwd (the one-launch K-step inference decoder) at the ABI boundary, without a GPU: declared, exported,
typed by the binding, additive within ABI 7, and every bad argument is turned away before any launch."""
import ctypes
import os
import re

import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'geeco_lstm_seq_heads_fwd'
ONE = ctypes.c_void_p(16)      # a non-null "device pointer": nothing below may get as far as reading it


def _call(lib, zx=ONE, wh=ONE, bias=ONE, fc1_w=ONE, fc1_b=ONE, heads_w=(16, 16, 16, 16), heads_b=(16, 16, 16, 16),
          sizes=(3, 3, 3, 3), nheads=None, N=2, T=3, H=128, Hfc=128, preds=ONE, ldz=None, ldw=None):
  nh = len(sizes) if nheads is None else nheads
  hw = (ctypes.c_void_p * max(len(heads_w), 1))(*heads_w) if heads_w is not None else None
  hb = (ctypes.c_void_p * max(len(heads_b), 1))(*heads_b) if heads_b is not None else None
  sz = (ctypes.c_int * max(len(sizes), 1))(*sizes) if sizes is not None else None
  rc = lib.geeco_lstm_seq_heads_fwd(zx, 4 * H if ldz is None else ldz, wh, 4 * H if ldw is None else ldw, bias, fc1_w, fc1_b, nh, hw,
                                    hb, sz, N, T, H, Hfc, preds, None, None, None)
  return rc, lib.geeco_last_error() or b''


def test_entry_is_declared_in_the_header():
  assert _abi.functions()[NAME][0] == 'int'


def test_library_exports_it():
  from geeco_amd import _native
  assert hasattr(ctypes.CDLL(_native.LIB_PATH), NAME)


def test_binding_types_it():
  from geeco_amd import _native
  res, args = _native.SIGNATURES[NAME]
  assert res is ctypes.c_int and len(args) == 19
  assert getattr(_native.load(), NAME).argtypes == args


def test_abi_is_still_7_and_the_entry_is_noted_as_additive():
  from geeco_amd import _native
  assert _abi.define('GEECO_ABI_VERSION') == 7
  assert _native.ABI_VERSION == 7 and _native.load().geeco_abi_version() == 7
  assert NAME in _abi.added_within(7)


def test_null_pointers_are_rejected():
  from geeco_amd import _native
  lib = _native.load()
  for kw in (dict(zx=None), dict(wh=None), dict(bias=None), dict(fc1_w=None), dict(fc1_b=None), dict(preds=None),
             dict(heads_w=None), dict(heads_b=None), dict(sizes=None, nheads=4)):
    rc, msg = _call(lib, **kw)
    assert rc == -1 and b'lstm_seq_heads: null pointer' in msg, (kw, rc, msg)
  rc, msg = _call(lib, heads_w=(16, 0, 16, 16))
  assert rc == -1 and b'head 1 null pointer' in msg
  rc, msg = _call(lib, heads_b=(16, 16, 16, 0))
  assert rc == -1 and b'head 3 null pointer' in msg


def test_bad_counts_are_rejected():
  from geeco_amd import _native
  lib = _native.load()
  for N in (0, -3):
    rc, msg = _call(lib, N=N)
    assert rc == -1 and b'N=%d < 1' % N in msg
  for T in (0, 65, -1):
    rc, msg = _call(lib, T=T)
    assert rc == -1 and b'T=%d outside 1..64' % T in msg
  for nh in (0, 6):
    rc, msg = _call(lib, heads_w=(16,) * 6, heads_b=(16,) * 6, sizes=(1,) * 6, nheads=nh)
    assert rc == -1 and b'nheads=%d outside 1..5' % nh in msg
  rc, msg = _call(lib, heads_w=(16,) * 3, heads_b=(16,) * 3, sizes=(16, 16, 1))
  assert rc == -1 and b'33 outputs > 32' in msg
  rc, msg = _call(lib, sizes=(3, 0, 3, 3))
  assert rc == -1 and b'head 1 size 0' in msg
  rc, msg = _call(lib, ldz=511)
  assert rc == -1 and b'bad dims' in msg
  rc, msg = _call(lib, ldw=511)
  assert rc == -1 and b'bad dims' in msg
  # the limits themselves pass the argument checks: what stops these two is the size gate below
  rc, _ = _call(lib, T=64, H=256, heads_w=(16,) * 2, heads_b=(16,) * 2, sizes=(16, 16))
  assert rc == -2
  rc, _ = _call(lib, T=1, N=1, H=256, heads_w=(16,), heads_b=(16,), sizes=(1,))
  assert rc == -2


def test_sizes_outside_the_kernel_return_enosup_and_launch_nothing():
  from geeco_amd import _native
  lib = _native.load()
  assert _native.GEECO_ENOSUP == -2
  rc, _ = _call(lib, H=256)
  assert rc == _native.GEECO_ENOSUP
  for Hfc in (32, 96, 256):
    rc, _ = _call(lib, Hfc=Hfc)
    assert rc == _native.GEECO_ENOSUP, Hfc
  rc, _ = _call(lib, H=129)
  assert rc == _native.GEECO_ENOSUP
