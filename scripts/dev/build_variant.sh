#!/bin/bash
# Builds the CURRENT csrc tree as geeco_amd/libgeeco_hip<suffix>.so with extra compiler flags, for same-box A/B runs
# (GEECO_DEV=1 GEECO_LIB=libgeeco_hip<suffix>.so python bench.py ...).  usage: build_variant.sh _noskew -DFB_SKEW=0
# (the PRODUCT kernel set: the only one there is)
set -euo pipefail
SUF=$1; shift
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
cd $ROOT/geeco_amd/csrc
B=build$SUF
rm -rf $B && mkdir -p $B
. ./sources.sh      # HIP_SOURCES, FLAGS, extra_flags
FLAGS="$FLAGS $*"
if [ -n "${PLAIN:-}" ]; then extra_flags() { :; }; fi      # PLAIN=1: no per-file settings (to A/B those settings themselves)
pids=()
for f in $HIP_SOURCES; do
  /opt/rocm/bin/hipcc $FLAGS $(extra_flags $f) -c $f.hip -o $B/$f.o &
  pids+=($!)
done
/opt/rocm/bin/hipcc $FLAGS -x hip -c errors.cpp -o $B/errors.o &
pids+=($!)
for p in "${pids[@]}"; do wait $p; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../libgeeco_hip$SUF.so $B/*.o
rm -rf $B
echo "built geeco_amd/libgeeco_hip$SUF.so ($*)"
