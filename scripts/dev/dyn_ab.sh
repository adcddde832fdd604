#!/bin/bash
# input stage alone (cold caches), product library and ablation builds of dynimg_goal.hip (build_variant.sh _nosync -DDYN_ABL_NOSYNC ...)
# usage: [REPS=3] [DYN_BENCH_ARGS="--depth --N 1"] dyn_ab.sh _suffix ...   (the legs alternate: product, each variant, product, ...)
set -o pipefail
export GEECO_DEV=1   # a GEECO_LIB=... leg loads another library build only under GEECO_DEV=1
for rep in $(seq ${REPS:-2}); do
for v in "" "$@"; do
  GEECO_LIB=libgeeco_hip$v.so timeout -k 10 120 python scripts/dev/u8_input_bench.py ${DYN_BENCH_ARGS:-} 2>&1 | tail -1 || exit 1
done
done
