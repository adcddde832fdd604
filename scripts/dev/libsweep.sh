#!/bin/bash
export GEECO_DEV=1   # a GEECO_LIB=... leg loads another library build only under GEECO_DEV=1
# same-box A/B of library builds: libsweep.sh "" _i0 ...  (suffixes of geeco_amd/libgeeco_hip<suffix>.so); prints the
# bench value and the first four rows of the per-layer table, twice per build (alternating)
tmp=$(mktemp -d); trap 'rm -rf "$tmp"' EXIT
for rep in 1 2; do
for v in "$@"; do
  GEECO_LIB=libgeeco_hip$v.so timeout -k 10 200 python bench.py --full --steps 30 --warmup 8 --skip-cpu --skip-other-configs --skip-input-pipeline --skip-inference --skip-dp-one-rank > $tmp/b.json 2>$tmp/b.err
  python - "$v" "$tmp/b.json" <<'PY'
import json, sys
d = json.loads(open(sys.argv[2]).read().strip().splitlines()[-1])
print('[%s]' % sys.argv[1], d['value'], d['step_ms']['median'], [(r['layer'], r['op'], r['us']) for r in d["layers"]])
PY
done
done
