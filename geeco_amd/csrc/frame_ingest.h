// The device code every frame-ingest kernel shares: the uint8 -> unit-float conversion (both forms), the dword unpack, the
// 4-pixel RGB load and the V-float vector load.  Device-only inline helpers; not a translation unit of its own.  Users:
// frame_pack.hip, window_gather.hip, predict_io.hip, shared_frames.hip (the division form) and dynimg_goal.hip (the Newton form).
#pragma once
#include "geeco_common.h"

// ---- uint8 -> [0, 1], two forms -------------------------------------------------------------------------------------------
// Both give float(u8) / 255 (_parse_v4, geeco_gym.py:312) correctly rounded, so they agree bitwise for all 256 byte values:
// tests/test_primitives_gpu.py::test_every_u8_ingest_path_is_the_one_conversion plants every byte value in each entry point that
// converts and compares against the float32 division.  Which kernel uses which form is a measured choice, not a free one: the
// Newton form was timed only in the one-pass stage (dynimg_goal.hip); every other kernel takes the division.

// the IEEE division
__device__ __forceinline__ float u8_unit_div(unsigned v) { return (float)v / 255.0f; }

// float(u8) / 255.0f (_parse_v4, geeco_gym.py:312) without the division sequence: one Newton correction of a * (1/255) is the
// correctly rounded quotient for every a in 0..255 (tests/test_kernels_gpu.py::test_goal_dynimgs_from_resident_u8_frames plants
// all 256 byte values and compares bitwise against the division of geeco_gather_windows, frame_pack.hip).
__device__ __forceinline__ float u8_unit(float a) {
  const float r = 1.0f / 255.0f;
  const float q = a * r;
  const float e = __builtin_fmaf(-255.0f, q, a);
  return __builtin_fmaf(e, r, q);
}

__device__ __forceinline__ f32x4 u8x4_unit(unsigned int b) {
  return f32x4{u8_unit((float)(b & 255u)), u8_unit((float)((b >> 8) & 255u)), u8_unit((float)((b >> 16) & 255u)),
               u8_unit((float)(b >> 24))};
}

// one dword = four consecutive bytes, lowest address first -> four floats (division form)
__device__ __forceinline__ void u8x4_unit_div(unsigned x, float* e) {
#pragma unroll
  for (int k = 0; k < 4; ++k) e[k] = u8_unit_div((x >> (8 * k)) & 255u);
}

// ---- 4 pixels of an RGB frame -> 12 floats ----------------------------------------------------------------------------------
// three dwords of a uint8 frame (plain loads)
__device__ __forceinline__ void load_rgb4(const unsigned* w, float (&px)[12]) {
#pragma unroll
  for (int q = 0; q < 3; ++q) u8x4_unit_div(w[q], px + q * 4);
}

// three float4 of a float32 frame (non-temporal: a frame is read once)
__device__ __forceinline__ void load_rgb4(const f32x4* w, float (&px)[12]) {
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const f32x4 x = __builtin_nontemporal_load(w + q);
    px[q * 4 + 0] = x.x;
    px[q * 4 + 1] = x.y;
    px[q * 4 + 2] = x.z;
    px[q * 4 + 3] = x.w;
  }
}

// ---- V floats of a feature row (V = 4: one 16-byte load, p aligned for it; V = 1: one float) ----------------------------------
template <int V>
__device__ __forceinline__ void ld_vec(const float* p, float (&v)[V]) {
  if (V == 4) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(p);
    v[0] = x.x;
    v[1] = x.y;
    v[2] = x.z;
    v[3] = x.w;
  } else {
    v[0] = *p;
  }
}
