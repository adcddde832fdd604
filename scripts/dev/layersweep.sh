#!/bin/bash
export GEECO_DEV=1   # the product reads GEECO_* switches only under GEECO_DEV=1
# per-layer times under a list of env settings (same box, same build): layersweep.sh "A=1" "B=2" ...; prints rows 0-4 of the layer table
tmp=$(mktemp -d); trap 'rm -rf "$tmp"' EXIT
for e in "" "$@"; do
  env $e timeout -k 10 200 python bench.py --full --steps 20 --warmup 5 --skip-cpu > $tmp/b.json 2>$tmp/b.err
  python - "$e" "$tmp/b.json" <<'PY'
import json, os, sys
d = json.loads(open(sys.argv[2]).read().strip().splitlines()[-1])
print('[%s]' % sys.argv[1], d['value'], d['step_ms']['median'], [(r['layer'], r['op'], r['us']) for r in d["layers"][int(os.environ.get("ROWS0", 4)):int(os.environ.get("ROWS1", 16))]])
PY
done
