// Frame plumbing of the data path: channel packing and the on-device window builder.
#include "geeco_common.h"

// ---- pixel packing: [n][HW][C1] (+ [n][HW][C2]) -> [n][HW][Cpad] ---------------------------------
__global__ __launch_bounds__(256) void pack_pixels_kernel(const float* src, long long s1, const float* src2,
                                                          long long s2, long long HW, int C1, int C2, int Cpad,
                                                          float* dst) {
  const int n = blockIdx.y;
  const long long px = (long long)blockIdx.x * 256 + threadIdx.x;
  if (px >= HW) return;
  const float* a = src + (long long)n * s1 + px * C1;
  const float* b = src2 ? src2 + (long long)n * s2 + px * C2 : nullptr;
  float* o = dst + ((long long)n * HW + px) * Cpad;
  if (Cpad == 4) {
    float e[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) e[c] = c < C1 ? a[c] : (b && c - C1 < C2 ? b[c - C1] : 0.f);
    *reinterpret_cast<f32x4*>(o) = f32x4{e[0], e[1], e[2], e[3]};
  } else {
    for (int c = 0; c < Cpad; ++c) o[c] = c < C1 ? a[c] : (b && c - C1 < C2 ? b[c - C1] : 0.f);
  }
}

extern "C" int geeco_pack_pixels(const float* src, int64_t src_sample_stride, const float* src2,
                                 int64_t src2_sample_stride, int N, int64_t HW, int C1, int C2, int Cpad,
                                 float* dst, void* stream) {
  GEECO_CHECK_ARG(src && dst, "pack_pixels: null pointer");
  GEECO_CHECK_ARG(N >= 1 && HW >= 1 && C1 >= 1 && C1 + (src2 ? C2 : 0) <= Cpad, "pack_pixels: bad dims");
  dim3 grid((unsigned)cdiv64(HW, 256), (unsigned)N);
  hipLaunchKernelGGL(pack_pixels_kernel, grid, dim3(256), 0, (hipStream_t)stream, src, (long long)src_sample_stride,
                     src2, (long long)src2_sample_stride, (long long)HW, C1, C2, Cpad, dst);
  GEECO_LAUNCH_CHECK();
  return 0;
}

// ---- on-device window builder ---------------------------------------------------------------------
// The reference materialises every K-frame window of an episode on the host (_window_v3,
// src/data/geeco_gym.py:615-631) and feeds 12.6 MB per sample over PCIe.  Here an episode's frames
// are uploaded ONCE (RGB as the uint8 values the recorder stored, data_recorder / tfrecord.py:73-74)
// and each batch's windows are gathered in HBM:  out[n][k][:] = conv(src[starts[n] + k][:]),
// conv(u8) = float(u8) / 255.0f  (the division of _parse_v4, geeco_gym.py:312, bit-exact).
template <typename T>
__global__ __launch_bounds__(256) void gather_windows_kernel(const T* __restrict__ src, const int* __restrict__ starts,
                                                             int K, long long frame_elems, float divisor,
                                                             float* __restrict__ out) {
  const int n = blockIdx.z, k = blockIdx.y;
  const long long i4 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i4 >= frame_elems) return;
  const T* s = src + (long long)(starts[n] + k) * frame_elems + i4;
  float* o = out + ((long long)n * K + k) * frame_elems + i4;
  if (i4 + 4 <= frame_elems) {
    float e[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) e[j] = divisor != 1.f ? (float)s[j] / divisor : (float)s[j];
    *reinterpret_cast<f32x4*>(o) = f32x4{e[0], e[1], e[2], e[3]};
  } else {
    for (int j = 0; i4 + j < frame_elems; ++j) o[j] = divisor != 1.f ? (float)s[j] / divisor : (float)s[j];
  }
}

extern "C" int geeco_gather_windows(const void* src, int src_is_u8, const int* starts_dev, int N, int K,
                                    int64_t frame_elems, float divisor, float* out, void* stream) {
  GEECO_CHECK_ARG(src && starts_dev && out, "gather_windows: null pointer");
  GEECO_CHECK_ARG(N >= 1 && K >= 1 && frame_elems >= 4 && frame_elems % 4 == 0, "gather_windows: bad dims");
  GEECO_CHECK_ARG(divisor != 0.f, "gather_windows: divisor == 0");
  dim3 grid((unsigned)cdiv64(frame_elems, 1024), (unsigned)K, (unsigned)N);
  if (src_is_u8)
    hipLaunchKernelGGL(gather_windows_kernel<unsigned char>, grid, dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char*)src, starts_dev, K, (long long)frame_elems, divisor, out);
  else
    hipLaunchKernelGGL(gather_windows_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)src,
                       starts_dev, K, (long long)frame_elems, divisor, out);
  GEECO_LAUNCH_CHECK();
  return 0;
}
