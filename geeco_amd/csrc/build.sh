#!/bin/bash
# Builds the C-ABI shared library for gfx950 in-tree (geeco_amd/libgeeco_hip.so): the only kernel set there is, one measured
# path per stage; the library reads no environment variable (the retired A/B switches: scripts/dev/SWITCHES.md).
set -euo pipefail
cd "$(dirname "$0")"
OUT=../libgeeco_hip.so
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
. ./sources.sh      # HIP_SOURCES, FLAGS, extra_flags
rm -rf build && mkdir -p build
pids=()
for f in $HIP_SOURCES; do
  $HIPCC $FLAGS $(extra_flags $f) -c $f.hip -o build/$f.o &
  pids+=($!)
done
$HIPCC $FLAGS -x hip -c errors.cpp -o build/errors.o &
pids+=($!)
for p in "${pids[@]}"; do wait $p; done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o $OUT build/*.o
g++ -O3 -std=c++17 -Wall -fPIC -shared -o ../libgeeco_host.so host_io.cpp host_inflate.cpp -lz -lpthread
echo "built $(realpath $OUT) and $(realpath ../libgeeco_host.so)"
