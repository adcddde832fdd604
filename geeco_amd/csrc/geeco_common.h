// Shared helpers for the gfx950 kernels (wave = 64 lanes, MFMA f32 16x16x4).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <atomic>

#include "../../include/geeco_hip.h"
#include "geeco_intmath.h"      // cdiv, cdiv64, same_pad

typedef float f32x4 __attribute__((ext_vector_type(4)));

void geeco_set_error(const char* fmt, ...);
// records the name of the kernel a dispatcher is about to launch (no-op unless a trace was begun on this thread)
void geeco_note_kernel(const char* fmt, ...);
// conv_wgrad.hip: while set (per thread), geeco_launch_wgrad_reduce records the slab sum there instead of launching it
void geeco_set_pending_reduce(geeco_slab_reduce* p);

// CUs the persistent bottom-of-the-backward kernels leave free: the `reserved_cus` argument of the entry point being served on this
// thread (errors.cpp; 0 outside such a call)
int geeco_call_reserved_cus(void);
int geeco_enter_reserved_cus(int k);     // GEECO_EINVAL outside 0..128
void geeco_leave_reserved_cus(void);

#define GEECO_CHECK_ARG(cond, ...)              \
  do {                                          \
    if (!(cond)) {                              \
      geeco_set_error(__VA_ARGS__);             \
      return GEECO_EINVAL;                      \
    }                                           \
  } while (0)

#define GEECO_LAUNCH_CHECK()                                         \
  do {                                                               \
    hipError_t e_ = hipGetLastError();                               \
    if (e_ != hipSuccess) {                                          \
      geeco_set_error("launch failed: %s", hipGetErrorString(e_));   \
      return (int)e_;                                                \
    }                                                                \
  } while (0)

// Once-per-kernel opt-in to `lds` bytes of dynamic LDS before the first launch: one flag per kernel instantiation; the
// attribute call is idempotent, racing threads at worst repeat it.  Returns 0 or the HIP error (message set).
template <auto KERNEL>
static int geeco_lds_opt_in(size_t lds) {
  static std::atomic<bool> attr_set{false};
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) {
      geeco_set_error("hipFuncSetAttribute(%zu B LDS) failed: %s", lds, hipGetErrorString(e));
      return (int)e;
    }
    attr_set = true;
  }
  return 0;
}

__device__ __forceinline__ float wave_reduce_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_reduce_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_reduce_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
