#!/bin/bash
# same-box A/B of library builds / env settings with the WHOLE per-layer table: ab_layers.sh "" "GEECO_LIB=libgeeco_hip_x.so" ...
# prints, per setting, the step median and every conv launch's us (median of 30 x 5 launches)
export GEECO_DEV=1   # a GEECO_LIB=... leg loads another library build only under GEECO_DEV=1
tmp=$(mktemp -d); trap 'rm -rf "$tmp"' EXIT
for e in "$@"; do
  env $e timeout -k 10 200 python bench.py --full --steps 60 --warmup 10 --skip-cpu --skip-other-configs > $tmp/l.json 2>$tmp/l.err || { tail -5 $tmp/l.err; continue; }
  python - "$e" "$tmp/l.json" <<'PY'
import json, sys
d = json.loads(open(sys.argv[2]).read().strip().splitlines()[-1])
print('[%s] step median %.4f ms' % (sys.argv[1], d['step_ms']['median']))
print('   ' + ' '.join('%s:%s=%.1f' % (r['layer'][4:], r['op'][:5], r['us']) for r in d['layers']))
PY
done
