// What csrc/clip.hip and csrc/guard.hip share: the norm from the partial sums of squares.
#pragma once
#include "geeco_common.h"

// ---- the norm: sqrt of the sum of the partials, one fixed order --------------------------------------
// For a 256-thread block: thread t adds the partials t, t + 256, ... in ascending order, then the wave butterfly (6 levels) and the four
// wave sums left to right.  ``sw``: 4 floats of LDS.  The value is returned to thread 0 alone.
__device__ __forceinline__ float clip_norm_of_partials(const float* __restrict__ partials, long long nchunks, float* sw) {
  float acc = 0.f;
  for (long long i = threadIdx.x; i < nchunks; i += 256) acc += partials[i];
  acc = wave_reduce_sum(acc);
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = acc;
  __syncthreads();
  return threadIdx.x == 0 ? sqrtf(((sw[0] + sw[1]) + sw[2]) + sw[3]) : 0.f;
}
