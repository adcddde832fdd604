#!/bin/bash
export GEECO_DEV=1   # a GEECO_LIB=... leg loads another library build only under GEECO_DEV=1
# A/B of library builds / runtime env settings of bench.py (skip cpu leg): ab2.sh "" "GEECO_LIB=libgeeco_hip_x.so"
for i in 1 2; do
  for e in "$@"; do
  echo -n "[$e] "; env $e python bench.py --full --steps 30 --warmup 5 --skip-cpu 2>/dev/null | python -c "import json,sys; d=json.loads(sys.stdin.read()); print(d['value'], d['ms_per_step'], d['roofline']['achieved'], d['encoder_forward']['tflops'])"
  done
done
