"""What ``geeco_amd.ops`` offers, one line per name of ``dir(ops)``: kind, ``inspect.signature``, sha256 of the source and of the
docstring (12 hex digits each); a value's line is its repr, a class also lists its methods.  Needs no GPU and no built library.
Run from a tree's root: ``python profiles/ops_split/api_record.py > record.txt``."""
import hashlib, inspect, os, sys
sys.path.insert(0, os.getcwd())
from geeco_amd import ops


def sha(text):
  return hashlib.sha256((text or '').encode()).hexdigest()[:12]


def line(name, obj):
  if inspect.ismodule(obj):
    return '%s module %s' % (name, obj.__name__)
  if inspect.isfunction(obj) or inspect.isclass(obj):
    kind = 'class' if inspect.isclass(obj) else 'function'
    try:
      source = sha(inspect.getsource(obj))
    except (OSError, TypeError):
      source = '-'
    return '%s %s %s source %s doc %s' % (name, kind, inspect.signature(obj), source, sha(obj.__doc__))
  return '%s value %r' % (name, obj)


for name in sorted(n for n in dir(ops) if not (n.startswith('__') and n.endswith('__'))):
  obj = getattr(ops, name)
  print(line(name, obj))
  if inspect.isclass(obj) and obj.__module__.startswith('geeco_amd.ops'):
    for m in sorted(vars(obj)):
      if inspect.isfunction(vars(obj)[m]):
        print(line('%s.%s' % (name, m), vars(obj)[m]))
