#!/usr/bin/env python
"""Compares the gfx950 device code of two builds of libgeeco_hip.so function by function (the check of a refactor that
must not change a kernel).  usage: isa_compare.py PARENT.so THIS.so [--diffs N]

Every gfx950 code object is taken from the .hip_fatbin section (uncompressed clang offload bundles), disassembled with
llvm-objdump -d and split per function symbol.  Addresses and encodings are dropped, branch targets become offsets inside
their function, the link-time literal of a pc-relative variable address is masked, and the s_nop run behind a function's
last instruction is dropped: it is the padding up to the next function, and behind the last function of a code object's
.text the 1 KiB prefetch guard the compiler ends every code object with -- which function that is changes with every move
of a kernel between files.  Prints the number of code objects, functions and instructions and every function that differs."""
import difflib, re, struct, subprocess, sys, tempfile, os

BIN = '/opt/rocm/llvm/bin/'
MAGIC = b'__CLANG_OFFLOAD_BUNDLE__'


def code_objects(lib, tmp):
  sec = os.path.join(tmp, 'fatbin')
  subprocess.check_call([BIN + 'llvm-objcopy', '-O', 'binary', '--only-section=.hip_fatbin', lib, sec])
  blob = open(sec, 'rb').read()
  out, at = [], blob.find(MAGIC)
  while at >= 0:
    n, = struct.unpack_from('<Q', blob, at + 24)
    q = at + 32
    for _ in range(n):
      off, size, tl = struct.unpack_from('<QQQ', blob, q)
      triple = blob[q + 24:q + 24 + tl].decode()
      q += 24 + tl
      if 'gfx950' in triple and size:
        out.append(blob[at + off:at + off + size])
    at = blob.find(MAGIC, at + 1)
  return out


def functions(lib):
  """{symbol: [normalised instruction, ...]}, number of code objects"""
  fns = {}
  with tempfile.TemporaryDirectory() as tmp:
    cos = code_objects(lib, tmp)
    for i, co in enumerate(cos):
      path = os.path.join(tmp, 'co%d.o' % i)
      open(path, 'wb').write(co)
      txt = subprocess.check_output([BIN + 'llvm-objdump', '-d', '--no-show-raw-insn', path]).decode()
      name, start = None, 0
      for line in txt.split('\n'):
        m = re.match(r'^([0-9a-f]+) <(.+)>:$', line)
        if m:
          start, name = int(m.group(1), 16), m.group(2)
          assert name not in fns, 'function %s in two code objects' % name
          fns[name] = []
          continue
        if name is None or not line.startswith('\t'):
          continue
        ins = line.split('//')[0].strip()
        # branch targets: absolute address <symbol+0x..> -> offset inside the function
        ins = re.sub(r'\b(\d+) <[^>]*>', lambda t: '@%d' % (int(t.group(1)) - start), ins)
        ins = re.sub(r'\s+', ' ', ins)
        # s_getpc_b64 + s_add_u32 literal = pc-relative address of a __device__ variable: the distance is the linker's
        if fns[name] and fns[name][-1].startswith('s_getpc_b64') and re.match(r's_add_u32 (s\d+), \1, 0x[0-9a-f]+$', ins):
          ins = ins.rsplit(' ', 1)[0] + ' <pcrel>'
        if ins and ins != '...':                 # '...': objdump's elision of the zero padding behind a function
          fns[name].append(ins)
  for ins in fns.values():                     # no function ends in s_nop: what trails its s_endpgm / branch is padding
    while ins and ins[-1] == 's_nop 0':
      ins.pop()
  return fns, len(cos)


def main():
  a, na = functions(sys.argv[1])
  b, nb = functions(sys.argv[2])
  ndiff = int(sys.argv[sys.argv.index('--diffs') + 1]) if '--diffs' in sys.argv else 40
  print('code objects: %d / %d' % (na, nb))
  print('functions: %d / %d, only in the first: %s, only in the second: %s' %
        (len(a), len(b), sorted(set(a) - set(b)), sorted(set(b) - set(a))))
  common = sorted(set(a) & set(b))
  differ = [f for f in common if a[f] != b[f]]
  print('compared %d functions, %d instructions: %d differ' % (len(common), sum(len(a[f]) for f in common), len(differ)))
  print('masked pc-relative literals: %d / %d' % tuple(sum(i.endswith('<pcrel>') for f in common for i in x[f]) for x in (a, b)))
  for f in differ:
    print('--- %s (%d / %d instructions)' % (f, len(a[f]), len(b[f])))
    for l in list(difflib.unified_diff(a[f], b[f], lineterm='', n=2))[2:2 + ndiff]:
      print('   ' + l)
  return 1 if differ or set(a) != set(b) else 0


if __name__ == '__main__':
  sys.exit(main())
