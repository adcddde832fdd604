"""The one reader of include/geeco_hip.h in tests/: its prototypes, structs, #defines and the "added within 7" list, as plain
data for tests/test_abi_cpu.py and the per-feature tests.  A C type is a string without ``const`` and without spaces before the
stars: 'int', 'int64_t', 'const float* x' -> 'float*', 'float* const* ws' -> 'float**'."""
import functools
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(None)
def raw():
  return open(os.path.join(ROOT, 'include', 'geeco_hip.h')).read()


@functools.lru_cache(None)
def source():
  """The header without its comments."""
  return re.sub(r'/\*.*?\*/', '', raw(), flags=re.S)


def _ctype(decl, named=True):
  """'const float* const* ws' -> 'float**' (``named``: the last word is the parameter's name)."""
  words = re.sub(r'\bconst\b', ' ', decl).replace('*', ' * ').split()
  if named and words[-1] != '*' and len([w for w in words if w != '*']) > 1:
    words = words[:-1]
  return ' '.join(w for w in words if w != '*') + '*' * words.count('*')


@functools.lru_cache(None)
def functions():
  """name -> (return type, [argument types]) for every prototype of the header."""
  out = {}
  for ret, name, args in re.findall(r'^([A-Za-z_][\w \t]*?[\w*][ \t*]*?)\b(geeco_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', source(), flags=re.M):
    args = ' '.join(args.split())
    out[name] = (_ctype(ret, named=False), [] if args in ('', 'void') else [_ctype(a) for a in args.split(',')])
  return out


@functools.lru_cache(None)
def define(name):
  """The value of ``#define name``, an integer expression of literals and earlier #defines."""
  m = re.search(r'^#define[ \t]+%s[ \t]+(.+?)[ \t]*$' % re.escape(name), source(), flags=re.M)
  assert m, name
  return _evaluate(m.group(1))


def _evaluate(expr):
  expr = re.sub(r'\b[A-Z][A-Z0-9_]*\b', lambda m: str(define(m.group(0))), expr)
  assert re.fullmatch(r'[\d\s()+\-*]+', expr), expr
  return int(eval(expr, {'__builtins__': {}}))


def defines(prefix):
  """The names of the header's #defines that start with ``prefix``, in the header's order."""
  return re.findall(r'^#define[ \t]+(%s\w*)[ \t]+\S' % re.escape(prefix), source(), flags=re.M)


@functools.lru_cache(None)
def struct_fields(name):
  """[(field, type, array length or None)] of ``typedef struct name { ... } name;`` in order ('float huber_delta[5]' ->
  ('huber_delta', 'float', 5)); array lengths are evaluated from the header's #defines."""
  m = re.search(r'typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;' % (name, name), source(), flags=re.S)
  assert m, name
  out = []
  for decl in (d.strip() for d in m.group(1).split(';')):
    if not decl:
      continue
    first, *more = [d.strip() for d in decl.split(',')]
    base = _ctype(re.sub(r'\[.*?\]', '', first))
    for item in [first] + more:      # 'int64_t gs_dw, gs_db, KC': the declarators share the first one's type
      field, length = re.search(r'(\w+)\s*(?:\[(.+)\])?$', item).groups()
      out.append((field, base, _evaluate(length) if length else None))
  return out


@functools.lru_cache(None)
def added_within(version):
  """The entry points the header's comment lists as added within ABI ``version``."""
  m = re.search(r'/\* added within %d \([^)]*\):(.*?)\*/' % version, raw(), flags=re.S)
  assert m, version
  return re.findall(r'geeco_[a-z0-9_]+', m.group(1))
