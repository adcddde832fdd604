// The counter-based normal generator of the device-side noise: Philox4x32-10 (Salmon et al., SC'11) and Box-Muller on its output
// words.  ONE copy for the scene augmentation's sensor noise (window_gather.hip) and the SmoothGrad path points
// (attribution.hip); tests/_augment_scene_ref.py restates both functions in numpy.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned x[4]) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0, c1 = lo1, c2 = hi0 ^ c3 ^ k1, c3 = lo0;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  x[0] = c0, x[1] = c1, x[2] = c2, x[3] = c3;
}

// Box-Muller on two words: ua = ((xa >> 8) + 0.5) 2^-24 in (0, 1), ub = (xb >> 8) 2^-24;  za, zb = sqrt(-2 ln ua) (cos, sin)(2 pi ub).
// t = 2^25 ua is an odd integer below 2^25: float32 holds it exactly below 2^24 and rounds it to a neighbour above, which next
// to ua = 1 would lose all of ln ua.  The rounding res = t - float(t) is an integer in {-1, 0, 1}, so
// ln ua = ln(float(t) 2^-25) + res / float(t) up to res^2 / (2 t^2) < 2^-49.  2 ub is exact in float32.
__device__ __forceinline__ void philox_normal_pair(unsigned xa, unsigned xb, float& za, float& zb) {
  const unsigned t = ((xa >> 8) << 1) | 1u;
  const float tf = (float)t;
  const float res = (float)((int)t - (int)tf);
  const float ln = logf(tf * 0x1p-25f) + res * __builtin_amdgcn_rcpf(tf);
  const float r = sqrtf(-2.f * ln);
  const float a = (float)(xb >> 8) * 0x1p-23f;
  za = r * cospif(a), zb = r * sinpif(a);
}
