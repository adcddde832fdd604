#!/bin/bash
# Builds geeco_amd/libgeeco_hip_stamps.so = the library with -DGEECO_STAMPS (in-kernel s_memtime timelines for
# scripts/dev/stamps.py).  Dev only: the product build never executes a stamp.
set -euo pipefail
cd "$(dirname "$0")/../../geeco_amd/csrc"
. ./sources.sh      # HIP_SOURCES, KERNEL_FLAGS, BASE_FLAGS (extra_flags is not used here)
T=$(mktemp -d)
SFLAGS="$KERNEL_FLAGS -DGEECO_STAMPS ${STAMP_FLAGS:-}"      # the product flags without WARN_FLAGS
pids=()
for f in $HIP_SOURCES; do
  /opt/rocm/bin/hipcc $SFLAGS -c $f.hip -o $T/$f.o &
  pids+=($!)
done
/opt/rocm/bin/hipcc $BASE_FLAGS -x hip -c errors.cpp -o $T/errors.o &
pids+=($!)
for p in "${pids[@]}"; do wait $p; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../libgeeco_hip_stamps.so $T/*.o
rm -rf $T
echo "built $(realpath ../libgeeco_hip_stamps.so)"
