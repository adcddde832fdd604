// Integer helpers of the launch code in plain C++ (no HIP): geeco_common.h includes this, and so do the headers a host-only
// program compiles (conv_gemm_plan.h).
#pragma once
#include <stdint.h>

static inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// TF 'SAME' padding: out = ceil(in/s); pad_total = max((out-1)s + k - in, 0); before = total/2.
static inline void same_pad(int size, int k, int s, int* out, int* before) {
  int o = (size + s - 1) / s;
  int tot = (o - 1) * s + k - size;
  if (tot < 0) tot = 0;
  *out = o;
  *before = tot / 2;
}
