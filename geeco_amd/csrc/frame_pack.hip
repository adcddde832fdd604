// Frame plumbing of the data path: channel packing and the plain on-device window builders (per episode, by address; the builders
// that also shift, tint, occlude and add noise are window_gather.hip).  uint8 frames become floats through frame_ingest.h:
// u8_unit_div per element, u8x4_unit_div per loaded word.
#include "frame_ingest.h"

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
// conv = a division by `divisor`; uint8 frames with divisor 255 give u8_unit_div's values (the division of _parse_v4,
// geeco_gym.py:312, bit-exact), the divisor being a run-time argument here.
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

// ---- window builder by address: one launch for windows of any episode, order or frame kind ----------------------------------
// A batch of SHUFFLED windows (input_fn.pickplace_input_fn(shuffle_windows=True)) holds about one episode per window; the
// builder above takes one episode per launch.  Here the host hands a table instead:  out[n][k][:] = conv(frame k of the K
// consecutive frames at addr[n]),  kind[n] = 0: uint8 frames, conv = u8_unit_div;  kind[n] = 1: float32 frames, a copy.
// blockIdx = (unit, k, n): a block serves one frame of one window, so it never straddles kinds, and takes the vector path when ITS window's address is aligned for it (4 bytes for a uint8
// word, 16 for a float4; frame_elems % 4 == 0 keeps every frame of an aligned window aligned), else one element at a time.
// HBM streaming: 4- / 16-byte non-temporal loads on the vector path (as pack_frames_kernel, shared_frames.hip), 16-byte stores.
__global__ __launch_bounds__(256) void gather_windows_by_address_kernel(const long long* __restrict__ addr,
                                                                        const int* __restrict__ kind, int K,
                                                                        long long frame_elems, float* __restrict__ out) {
  const int n = blockIdx.z, k = blockIdx.y;
  const long long i4 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i4 >= frame_elems) return;          // (frame_elems % 4 == 0: every remaining thread owns four whole elements)
  const unsigned long long base = (unsigned long long)addr[n];
  float* o = out + ((long long)n * K + k) * frame_elems + i4;
  float e[4];
  if (kind[n] == 1) {
    const unsigned long long a = base + ((unsigned long long)k * frame_elems + i4) * 4;
    if ((base & 15u) == 0) {
      const f32x4 x = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a));
      e[0] = x.x, e[1] = x.y, e[2] = x.z, e[3] = x.w;
    } else {
      const float* s = reinterpret_cast<const float*>(a);
#pragma unroll
      for (int j = 0; j < 4; ++j) e[j] = s[j];
    }
  } else {
    const unsigned long long a = base + (unsigned long long)k * frame_elems + i4;
    if ((base & 3u) == 0) {
      const unsigned x = __builtin_nontemporal_load(reinterpret_cast<const unsigned*>(a));
      u8x4_unit_div(x, e);
    } else {
      const unsigned char* s = reinterpret_cast<const unsigned char*>(a);
#pragma unroll
      for (int j = 0; j < 4; ++j) e[j] = u8_unit_div(s[j]);
    }
  }
  *reinterpret_cast<f32x4*>(o) = f32x4{e[0], e[1], e[2], e[3]};
}

extern "C" int geeco_gather_windows_by_address(const int64_t* addr, const int* kind, int N, int K, int64_t frame_elems,
                                               float* out, void* stream) {
  GEECO_CHECK_ARG(addr && kind && out, "gather_windows_by_address: null pointer");
  GEECO_CHECK_ARG(N >= 1 && N <= 65535 && K >= 1 && K <= 65535, "gather_windows_by_address: N=%d, K=%d outside 1..65535", N, K);
  GEECO_CHECK_ARG(frame_elems >= 4 && frame_elems % 4 == 0, "gather_windows_by_address: frame_elems=%lld must be a positive multiple of 4",
                  (long long)frame_elems);
  GEECO_CHECK_ARG(cdiv64(frame_elems, 1024) <= 0x7fffffffLL, "gather_windows_by_address: frame_elems=%lld too large", (long long)frame_elems);
  GEECO_CHECK_ARG((reinterpret_cast<uintptr_t>(out) & 15) == 0, "gather_windows_by_address: out must be 16-byte aligned");
  GEECO_CHECK_ARG((reinterpret_cast<uintptr_t>(addr) & 7) == 0 && (reinterpret_cast<uintptr_t>(kind) & 3) == 0,
                  "gather_windows_by_address: the tables must be aligned for their element types");
  dim3 grid((unsigned)cdiv64(frame_elems, 1024), (unsigned)K, (unsigned)N);
  hipLaunchKernelGGL(gather_windows_by_address_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const long long*)addr, kind, K,
                     (long long)frame_elems, out);
  GEECO_LAUNCH_CHECK();
  return 0;
}
