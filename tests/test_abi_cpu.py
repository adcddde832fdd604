"""The C-ABI library must load without a GPU and export every symbol include/geeco_hip.h declares
(no compute calls here)."""
import ctypes
import os
import re

import numpy as np
import pytest

import _abi

ROOT = _abi.ROOT

# The ctypes a C type of the header binds as.  A return or scalar argument binds as exactly this type; ``T*`` as c_void_p or as
# POINTER(this type of T) -- the header cannot say whether a pointer is a host array or a device pointer -- and ``T**`` as
# POINTER(c_void_p) or c_void_p.
SCALARS = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float, 'unsigned': ctypes.c_uint,
           'uint32_t': ctypes.c_uint32, 'uint64_t': ctypes.c_uint64}
RETURNS = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'unsigned': ctypes.c_uint, 'char*': ctypes.c_char_p, 'void': None}
POINTEES = dict(SCALARS, int32_t=ctypes.c_int32, int16_t=ctypes.c_int16, uint16_t=ctypes.c_uint16, uint8_t=ctypes.c_uint8, double=ctypes.c_double,
                **{'unsigned char': ctypes.c_ubyte})


def _structs():
  from geeco_amd import _native
  return {'geeco_slab_reduce': _native.SlabReduce, 'geeco_loss_shaping': _native.LossShaping, 'geeco_adam_segment': _native.AdamSegment,
          'geeco_lr_schedule': _native.LrSchedule, 'geeco_heads_finish': _native.HeadsFinish}


def _bindings(ctype):
  """The ctypes the C type ``ctype`` of an argument or a struct field may bind as."""
  if ctype.endswith('**'):
    return [ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p]
  if ctype.endswith('*'):
    pointee = dict(POINTEES, **_structs()).get(ctype[:-1])
    assert pointee is not None or ctype in ('void*', 'geeco_varstats_record*'), ctype      # (the record is mirrored as a numpy dtype)
    return [ctypes.c_void_p] + ([ctypes.POINTER(pointee)] if pointee is not None else [])
  return [SCALARS[ctype] if ctype in SCALARS else POINTEES[ctype]]


def test_library_exports_every_declared_symbol():
  from geeco_amd import _native
  names = sorted(_abi.functions())
  assert len(names) >= 25
  assert names == sorted(set(re.findall(r'\b(geeco_[a-z0-9_]+)\s*\(', _abi.source())))      # no prototype the reader does not parse
  lib = ctypes.CDLL(_native.LIB_PATH)
  missing = [n for n in names if not hasattr(lib, n)]
  assert not missing, missing
  # the Python binding types exactly the declared set
  assert sorted(_native.SIGNATURES.keys()) == names


@pytest.mark.parametrize('name', sorted(_abi.functions()))
def test_signature_matches_the_header(name):
  """Every entry point: the return type, the number of arguments and the type of each, against include/geeco_hip.h."""
  from geeco_amd import _native
  ret, args = _abi.functions()[name]
  restype, argtypes = _native.SIGNATURES[name]
  assert restype is RETURNS[ret], (name, ret, restype)
  assert len(argtypes) == len(args), (name, len(args), len(argtypes))
  for i, (want, have) in enumerate(zip(args, argtypes)):
    assert any(have is b for b in _bindings(want)), '%s: argument %d is %s in the header, %s in SIGNATURES' % (name, i, want, have)


@pytest.mark.parametrize('name', sorted(_structs()))
def test_struct_matches_the_header(name):
  """Every mirrored Structure field by field: names, order, types and array lengths."""
  struct = _structs()[name]
  fields = _abi.struct_fields(name)
  assert [f[0] for f in struct._fields_] == [f[0] for f in fields]
  for (field, have), (_, ctype, length) in zip(struct._fields_, fields):
    want = _bindings(ctype)
    assert any(have is (b * length if length else b) for b in want), '%s.%s is %s%s in the header, %s in _native' % (
        name, field, ctype, '[%d]' % length if length else '', have)
  assert ctypes.sizeof(_structs()['geeco_lr_schedule']) == 144


def _numpy_dtype(struct):
  """The packed numpy dtype of a header struct of int64_t / float fields and nested structs."""
  kinds = {'int64_t': '<i8', 'float': '<f4'}
  return np.dtype([(field, kinds.get(ctype) or _numpy_dtype(ctype)) + (((length,),) if length else ())
                   for field, ctype, length in _abi.struct_fields(struct)])


def test_varstats_record_matches_the_header():
  from geeco_amd import ops
  assert ops.VARSTATS_DTYPE == _numpy_dtype('geeco_varstats_record')
  assert ops.VARSTATS_DTYPE['grad'] == ops.VARSTATS_DTYPE['param'] == _numpy_dtype('geeco_varstats_tensor')
  assert ops.VARSTATS_DTYPE.itemsize == 1368


def test_mirrored_constants_equal_their_defines():
  """Every constant of the header the package mirrors (geeco_amd/_native.py is their one home) equals its #define."""
  from geeco_amd import _native, ops, summary, train_options
  mirrored = {'GEECO_EINVAL': _native.GEECO_EINVAL, 'GEECO_ENOSUP': _native.GEECO_ENOSUP, 'GEECO_ABI_VERSION': _native.ABI_VERSION,
              'GEECO_ADAM_SEGMENTS_MAX': _native.ADAM_SEGMENTS_MAX, 'GEECO_SLAB_REDUCE_MAX': _native.SLAB_REDUCE_MAX,
              'GEECO_LR_BOUNDARIES_MAX': _native.LR_BOUNDARIES_MAX, 'GEECO_VARSTATS_CHUNK': _native.VARSTATS_CHUNK,
              'GEECO_VARSTATS_CLASSES': _native.VARSTATS_CLASSES, 'GEECO_REPLAY_MAXHEADS': _native.REPLAY_MAXHEADS}
  for name, value in mirrored.items():
    assert _abi.define(name) == value, name
  assert _abi.define('GEECO_PREDICT_PACK_MAXSEG') == 8      # (the package mirrors no such constant)
  assert {'GEECO_PREDICT_FEAT_' + k.upper(): v for k, v in ops.PREDICT_FEAT_MODES.items()} == \
      {n: _abi.define(n) for n in _abi.defines('GEECO_PREDICT_FEAT_')}
  kinds = [n for n in _abi.defines('GEECO_LR_') if n != 'GEECO_LR_BOUNDARIES_MAX']
  assert [(n, _abi.define(n)) for n in kinds] == [('GEECO_LR_' + k.upper(), i) for i, k in enumerate(_native.LR_KINDS)]
  # one home: the other places the names can be imported from hold the same objects
  assert ops.PREDICT_FEAT_MODES is _native.PREDICT_FEAT_MODES and train_options.LR_KINDS is _native.LR_KINDS
  assert train_options.LR_BOUNDARIES_MAX == _native.LR_BOUNDARIES_MAX and summary.CLASSES == _native.VARSTATS_CLASSES
  assert (ops.REPLAY_SQUARED_ERROR, ops.REPLAY_CLASS_HIT) == (_native.REPLAY_SQUARED_ERROR, _native.REPLAY_CLASS_HIT) == (0, 1)


def test_every_addition_within_the_version_is_declared():
  added = _abi.added_within(7)
  assert added and len(added) == len(set(added)) and set(added) <= set(_abi.functions())


def test_binding_loads_and_reports_version():
  from geeco_amd import _native
  lib = _native.load()
  declared = _abi.define('GEECO_ABI_VERSION')
  assert lib.geeco_abi_version() == declared == _native.ABI_VERSION     # header, library and binding agree
  assert lib.geeco_dynimg_ws_bytes(2, 1024) > 0
  assert lib.geeco_conv3x3_wgrad_ws_bytes(3, 2, 64, 64, 32, 48, 2) > 0
  assert lib.geeco_conv3x3_fwd_ws_bytes(3, 32, 256, 256, 4, 32, 1) == 0       # big layers never split K
  assert lib.geeco_conv3x3_fwd_ws_bytes(3, 32, 4, 4, 256, 256, 2) > 0         # conv8 does


def test_host_side_argument_checks_need_no_gpu():
  """Bad arguments are rejected before any launch, with a message (error behaviour of the boundary)."""
  from geeco_amd import _native
  lib = _native.load()
  rc = lib.geeco_conv3x3_fwd(None, None, None, None, 1, 0, 0, 0, 0, 1, 8, 8, 4, 16, 1, 1, None, None)
  assert rc == -1 and b'null pointer' in lib.geeco_last_error()
  one = ctypes.c_void_p(16)
  rc = lib.geeco_conv3x3_fwd(one, one, one, one, 1, 0, 0, 0, 0, 1, 8, 8, 3, 16, 1, 1, None, None)
  assert rc == -1 and b'multiple of 4' in lib.geeco_last_error()
  rc = lib.geeco_dynimg_fwd(one, None, 0, 0, one, 1, 65, 16, 3, 4, one, one, None)
  assert rc == -1 and b'K=65' in lib.geeco_last_error()
  # the batched LSTM-step backward: null operands, a concat description without its arrays, a state narrower than its cells
  rc = lib.geeco_lstm_step_bwd(None, 8, one, 8, one, 8, one, 8, one, one, 8, 2, 8, 8, None, None, None, 0, 0, 0, 0, one, None, None)
  assert rc == -1 and b'null pointer' in lib.geeco_last_error()
  rc = lib.geeco_lstm_step_bwd(one, 8, one, 8, one, 8, one, 8, one, one, 8, 2, 8, 8, None, None, None, 2, 0, 0, 4, one, None, None)
  assert rc == -1 and b'concat description' in lib.geeco_last_error()
  arr = (ctypes.c_void_p * 1)(16)
  chs = (ctypes.c_int * 1)(256)
  rc = lib.geeco_lstm_step_bwd(one, 8, one, 8, one, 8, one, 8, one, one, 8, 2, 8, 8, arr, arr, chs, 1, 1, 7, 4, one, None, None)
  assert rc == -1 and b'exceed the state width' in lib.geeco_last_error()
  assert lib.geeco_lstm_step_bwd_ws_bytes(32, 3100, 512) == lib.geeco_gemm_ws_bytes(32, 3100, 512) > 0


def test_alpha_matches_oracle():
  from geeco_amd import _native
  from oracle import geeco_oracle as O
  lib = _native.load()
  for K in (2, 4, 16, 32):
    buf = (ctypes.c_float * K)()
    lib.geeco_dynimg_alpha(K, ctypes.cast(buf, ctypes.c_void_p))
    assert [float(v) for v in buf] == [float(v) for v in O.dynimg_alpha(K)]    # bit-exact float32


def test_stale_library_is_refused_by_version(tmp_path, monkeypatch):
  """A library of another ABI version (a stale build, or another build picked through GEECO_LIB) must be refused at load
  time with a message that says so -- not load and fail later at the first changed entry point."""
  import subprocess
  import pytest
  from geeco_amd import _native
  src = tmp_path / 'stale.c'
  src.write_text('int geeco_abi_version(void) { return 1; }\n')
  so = tmp_path / 'libstale.so'
  subprocess.check_call(['gcc', '-shared', '-fPIC', '-o', str(so), str(src)])
  monkeypatch.setattr(_native, 'LIB_PATH', str(so))
  monkeypatch.setattr(_native, '_lib', None)
  with pytest.raises(_native.GeecoNativeError, match='ABI version mismatch'):
    _native.load()


def test_dev_switches_are_ignored_without_geeco_dev(monkeypatch):
  """The GEECO_* A/B switches are retired (scripts/dev/SWITCHES.md): the library reads no environment variable at all, and
  the Python side reads only GEECO_DEV / GEECO_LIB, in _native.py, to load another build of the library -- and a GEECO_LIB
  without GEECO_DEV=1 (a stray variable in a production environment) does not change which library is loaded."""
  import glob
  for ext in ('hip', 'cpp', 'h'):
    for path in glob.glob(os.path.join(ROOT, 'geeco_amd', 'csrc', '*.' + ext)):
      assert 'getenv' not in open(path).read(), path
  for path in glob.glob(os.path.join(ROOT, 'geeco_amd', '**', '*.py'), recursive=True):
    src = open(path).read()
    reads = set(re.findall(r"""(?:environ(?:\.get)?|getenv)\s*[\[(]\s*['"](GEECO_[A-Z0-9_]*)""", src))
    allowed = {'GEECO_DEV', 'GEECO_LIB'} if os.path.basename(path) == '_native.py' else set()
    assert reads <= allowed, (path, reads)
  from geeco_amd import _native
  product = os.path.join(ROOT, 'geeco_amd', 'libgeeco_hip.so')
  monkeypatch.setenv('GEECO_LIB', 'libgeeco_hip_other.so')
  monkeypatch.delenv('GEECO_DEV', raising=False)
  assert _native.lib_path() == product
  monkeypatch.setenv('GEECO_DEV', '0')
  assert _native.lib_path() == product
  monkeypatch.setenv('GEECO_DEV', '1')
  assert _native.lib_path() == os.path.join(ROOT, 'geeco_amd', 'libgeeco_hip_other.so')


def test_product_library_holds_no_switches_and_no_development_kernels():
  """the shipped library is the path that runs.  It reports itself as the product build, the name of no
  retired GEECO_* switch occurs in it (nothing reads the environment), and none of the kernels only a switch could select is
  compiled in (they were deleted with the switches)."""
  from geeco_amd import _native
  lib = _native.load()
  assert lib.geeco_has_dev_kernels() == 0
  blob = open(os.path.join(ROOT, 'geeco_amd', 'libgeeco_hip.so'), 'rb').read()
  for name in re.findall(r'`(GEECO_[A-Z0-9_]+)', open(os.path.join(ROOT, 'scripts', 'dev', 'SWITCHES.md')).read()) + ['GEECO_DEV']:
    assert name.encode() not in blob, name
  for kernel in (b'conv1_conv2_fwd_kernel', b'conv_s2_halo_fwd_kernel', b'geeco_conv1_conv2_fwd'):
    assert kernel not in blob, kernel
  assert b'conv_s2_halo_fwd_ws_kernel' in blob
