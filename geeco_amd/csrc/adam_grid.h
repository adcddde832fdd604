// The one grid rule of the kernels that walk pieces of the arena (csrc/adam.hip, csrc/grad_accum.hip): every block walks every piece
// with the whole grid's stride, n4 = the longest piece's float4s.
#pragma once
#include "geeco_intmath.h"      // cdiv64

static inline int adam_grid(long long n4) {
  long long blocks = cdiv64(n4, 256);
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}
