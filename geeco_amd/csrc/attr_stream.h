// What the streaming kernels of the attribution passes share (attribution.hip; perturbation.hip; the
// consolidation: DESIGN 5.31).  Device side: float32 operations that are never contracted into an FMA, four-element accesses on the
// 16-byte and the one-float path, the periodic baseline / fill, and the loop over groups of four elements.  Host side: the pointer
// checks of every entry point, the step from runtime flags and a channel count to template arguments, and the grid of a
// grid-stride launch.
#pragma once
#include <algorithm>
#include <type_traits>

#include "geeco_common.h"
#include "philox_normal.h"      // BEFORE the pragma below, whatever the including file does: the generator keeps the form it has in the gather

// No contraction: hipcc fuses a product into the sum behind it by default, and the __f*_rn intrinsics do not stop it (they are
// inline functions of plain operators that carry the header's contraction flag into the caller).  Contraction is switched off for
// everything behind this header, and every rounded operation goes through these three, which are compiled under that setting.
// The pragma is file-scope and holds to the end of the translation unit: include this header LAST, after every header whose
// inline code must keep the default contraction (philox_normal.h is pulled in above for that reason).
#pragma clang fp contract(off)
__device__ __forceinline__ float at_add(float a, float b) { return a + b; }
__device__ __forceinline__ float at_sub(float a, float b) { return a - b; }
__device__ __forceinline__ float at_mul(float a, float b) { return a * b; }

#define AT_THREADS 256
#define AT_MAX_BLOCKS 2048        // 8 blocks of 256 threads per CU: the grid-stride loop takes the rest

// baseline[(e + j) % period], j = 0..3, for a group that starts at element e (a multiple of 4).  BV: period % 4 == 0 and the
// baseline is 16-byte aligned, so the four lie side by side in one aligned word.  ``small``: n < 2^32, the remainder in 32 bits.
template <bool BV>
__device__ __forceinline__ void attr_baseline4(const float* __restrict__ baseline, long long period, bool small, long long e, int cnt,
                                               float b[4]) {
  b[0] = b[1] = b[2] = b[3] = 0.f;
  if (!baseline) return;
  long long r = small ? (long long)((unsigned)e % (unsigned)period) : e % period;
  if (BV) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(baseline + r);
    b[0] = v.x, b[1] = v.y, b[2] = v.z, b[3] = v.w;
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (j < cnt) b[j] = baseline[r];
    if (++r == period) r = 0;
  }
}

template <bool V>
__device__ __forceinline__ void attr_load4(const float* __restrict__ p, long long e, int cnt, float v[4]) {
  if (V && cnt == 4) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p + e);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = j < cnt ? p[e + j] : 0.f;
}

template <bool V>
__device__ __forceinline__ void attr_store4(float* __restrict__ p, long long e, int cnt, const float v[4]) {
  if (V && cnt == 4) {
    *reinterpret_cast<f32x4*>(p + e) = f32x4{v[0], v[1], v[2], v[3]};
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < cnt) p[e + j] = v[j];
}

// f(e, cnt) for the groups of four consecutive elements of n that one thread of a grid-stride launch (AT_THREADS per block) owns:
// group g starts at element e = 4 g and holds cnt = 4 elements, the last group of n possibly fewer.
template <class F>
__device__ __forceinline__ void attr_for_groups4(long long n, F&& f) {
  const long long groups = (n + 3) >> 2, stride = (long long)gridDim.x * AT_THREADS;
  for (long long g = (long long)blockIdx.x * AT_THREADS + threadIdx.x; g < groups; g += stride) {
    const long long e = g << 2;
    f(e, n - e >= 4 ? 4 : (int)(n - e));
  }
}

// ---- the host side of a launch ---------------------------------------------------------------------------------------------------
// every one of these pointers is A-byte aligned (a null pointer, where the entry point allows one, passes)
template <int A, class... P>
static bool attr_aligned(const P*... p) { return ((reinterpret_cast<uintptr_t>(p) | ...) & (A - 1)) == 0; }
// [a, a + bytes_a) and [b, b + bytes_b) share no byte
static bool attr_apart(const void* a, uintptr_t bytes_a, const void* b, uintptr_t bytes_b) {
  const uintptr_t lo_a = reinterpret_cast<uintptr_t>(a), lo_b = reinterpret_cast<uintptr_t>(b);
  return lo_a + bytes_a <= lo_b || lo_b + bytes_b <= lo_a;
}
static unsigned attr_grid(long long units) { return (unsigned)std::min<long long>(cdiv64(units, AT_THREADS), AT_MAX_BLOCKS); }

// From runtime flags and a channel count to template arguments: attr_select(f, a, b) calls f(A, B) with A, B std::true_type or
// std::false_type objects, attr_channels(C, f) calls f(std::integral_constant<int, C>) for C in 1..4 (checked by the caller).
// Inside the generic lambda ``A()`` is a constant expression; attr_tf spells it as the kernel's name does.
template <class F>
static void attr_select(F&& f) { f(); }
template <class F, class... Rest>
static void attr_select(F&& f, bool flag, Rest... rest) {
  if (flag) attr_select([&](auto... t) { f(std::true_type{}, t...); }, rest...);
  else attr_select([&](auto... t) { f(std::false_type{}, t...); }, rest...);
}
template <class F>
static void attr_channels(int C, F&& f) {
  switch (C) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
  }
}
static const char* attr_tf(bool flag) { return flag ? "true" : "false"; }

// the baseline rule of the path point, the finish and the occluder's fill: NULL = zeros (the period is not looked at), else a
// period >= 1 that divides n
static int check_baseline(const char* who, const float* baseline, int64_t period, int64_t n) {
  if (!baseline) return 0;
  GEECO_CHECK_ARG(period >= 1 && period <= n && n % period == 0, "%s: baseline_period=%lld does not divide n=%lld", who,
                  (long long)period, (long long)n);
  GEECO_CHECK_ARG(attr_aligned<4>(baseline), "%s: the baseline must be 4-byte aligned", who);
  return 0;
}
