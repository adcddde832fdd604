// The window builders that follow addresses AND transform what they gather: geeco_gather_windows_augmented (shift and tint,
// DESIGN 5.14), geeco_gather_windows_scene (occluders and sensor noise behind them) and geeco_gather_windows_frames
// (one address per frame).  ONE argument check and ONE instance choice serve the three entry points, and ONE kernel
// body all of their launches but one: one-channel frames of consecutive windows keep the run-time-C kernel they had, which
// measured faster there.  The plain builders (per episode, by address) are frame_pack.hip.
#include "frame_ingest.h"
#include "philox_normal.h"

// ---- the gather: the by-address builder with a per-window shift and colour transform -------------------------------------------
// Training-time image augmentation (input_fn.pickplace_input_fn(augment=...)) where the frames already are: the
// table of gather_windows_by_address plus, per window, shift[n] = (dy, dx) in whole pixels and, for colour streams, colour[n] =
// gain[C], bias[C].
// out[n][k][y][x][c] = tint(conv(frame k of window n at (y - dy, x - dx), channel c)), exactly 0.0f where that source pixel lies
// outside the frame;  tint(v) = min(max(v * gain[c] + bias[c], 0), 1), the identity without `colour`.  One draw serves all K
// frames of a window.  blockIdx = (unit, k, n) and 256 threads x 4 output elements as there.  A row holds RW = W * C elements and
// a shift by whole pixels moves a row's elements by dx * C, so the channel of an element is kept and "inside the frame" is
// 0 <= y - dy < H  and  0 <= r - dx * C < RW  for row offset r: both are tested BEFORE any address is formed, in 64-bit, so no
// shift value reads outside [frame, frame + H * W * C).  RW % 4 == 0: a thread's four elements share a row and are stored as one
// 16-byte word; four sources inside the row are read as one 16-byte (float32) / 4-byte (uint8) non-temporal load when their
// address is aligned for it, else narrower: float32 as four words; uint8 as the two aligned words around them and a byte-align
// when both lie inside the frame, else as bytes.  A group that crosses the left or right edge goes per element.  RW % 4 != 0
// (groups straddle rows, frames are not 16-byte multiples): one element at a time, loads and stores.  HBM streaming: no LDS, no
// atomics, nothing waits for another block.
// tint of channel c; gains / biases as scalars by value (an indexed private array would be promoted to LDS)
__device__ __forceinline__ float aug_tint(float v, unsigned c, bool on, float g0, float g1, float g2, float b0, float b1, float b2) {
  if (!on) return v;
  const float gain = c == 0 ? g0 : (c == 1 ? g1 : g2), bias = c == 0 ? b0 : (c == 1 ? b1 : b2);
  return fminf(fmaxf(v * gain + bias, 0.f), 1.f);
}

__device__ __forceinline__ float aug_load(unsigned long long frame, bool f32, long long e) {
  return f32 ? reinterpret_cast<const float*>(frame)[e] : u8_unit_div(reinterpret_cast<const unsigned char*>(frame)[e]);
}

// ---- scene extras: occluders and per-element sensor noise of RGB streams behind the gather -------------------------------------
// (input_fn.pickplace_input_fn(augment=dict(noise=, occlude=)))  Per element, in this order:  v1 = what the gather
// above gives (shift, zero fill, tint);  v2 = the colour component of the highest-numbered rectangle of window n that holds the
// element's OUTPUT pixel, else v1;  out = min(max(fma(sigma, z, v2), 0), 1) with z ~ N(0, 1) from Philox4x32-10 under the counter
// (e / 4, k, n, tag) for element offset e of the frame: z depends on (key, tag, n, k, e) alone, whatever path or thread made it.
// sigma == 0 skips the noise step (no clamp: the output is v2 itself).  The rectangles and the key are uniform per block (scalar
// loads); no address is formed from a rectangle.  Grid, thread ownership and stores as above; a thread's four elements are
// e = i4 .. i4 + 3 on either path, so ONE Philox call serves them.
// philox4x32_10 and philox_normal_pair (Box-Muller on two of its words): philox_normal.h, shared with attribution.hip.

// One rectangle slot of a window as scalars (an indexed private array would leave the registers): (y0, x0, h, w) and its colour;
// h <= 0 or w <= 0: an empty slot.
struct SceneRect {
  int y0, x0, h, w;
  float r, g, b;
};

__device__ __forceinline__ SceneRect scene_rect(const int* occ_rect, const float* occ_colour, int n, int j) {
  if (!occ_rect) return SceneRect{0, 0, 0, 0, 0.f, 0.f, 0.f};
  const int* rc = occ_rect + ((long long)n * 4 + j) * 4;
  const float* cc = occ_colour + ((long long)n * 4 + j) * 3;
  return SceneRect{rc[0], rc[1], rc[2], rc[3], cc[0], cc[1], cc[2]};
}

// v under one rectangle at output pixel (y, x), channel c.  y, x < 2^31: y >= y0 as int32, then y - y0 lies in [0, 2^32) and is
// compared unsigned with h > 0 -- no overflow for any table content.
__device__ __forceinline__ float scene_occlude(float v, const SceneRect q, unsigned y, unsigned x, unsigned c) {
  const bool in = q.h > 0 && q.w > 0 && (int)y >= q.y0 && y - (unsigned)q.y0 < (unsigned)q.h && (int)x >= q.x0 &&
                  x - (unsigned)q.x0 < (unsigned)q.w;
  return in ? (c == 0 ? q.r : (c == 1 ? q.g : q.b)) : v;
}

// Two sources of a block's frame address: WindowFrames, the K consecutive frames at addr[n] (the augmented and the scene entry),
// and TableFrames, the frame at addr[n][k] (the frames entry).  Everything behind the address is ONE body: conversion, shift test,
// tint, rectangles, Philox / Box-Muller.  Every load-width decision of that body is taken on the element's own address (or on
// RW % 4, a launch constant), never on the window's first frame, so frames of one window may lie at any alignment of their kind.
struct WindowFrames {
  static constexpr bool kTable = false;
  __device__ static unsigned long long frame(const long long* addr, int n, int k, int K, unsigned fe, bool f32) {
    return (unsigned long long)addr[n] + (unsigned long long)k * fe * (f32 ? 4u : 1u);
  }
};
struct TableFrames {
  static constexpr bool kTable = true;
  __device__ static unsigned long long frame(const long long* addr, int n, int k, int K, unsigned fe, bool f32) {
    return (unsigned long long)addr[(long long)n * K + k];
  }
};

// C = 3: the whole chain.  C = 1 (instantiated under TableFrames only): shift and tint of channel 0; no rectangles, no noise (the argument check refuses them).
// ``shift`` may be null under TableFrames alone (no shift).  Extras = false: an instance without the rectangle and noise steps,
// for launches that carry neither -- the tests for them and the registers they hold cost the bare gather a fifth of its time
// (DESIGN 5.26).  <3, WindowFrames, false> is what geeco_gather_windows_augmented launches for an RGB stream.
template <int C, typename Frames, bool Extras>
__global__ __launch_bounds__(256) void window_gather_kernel(const long long* __restrict__ addr, const int* __restrict__ kind,
                                                            const int* __restrict__ shift, const float* __restrict__ colour,
                                                            const int* __restrict__ occ_rect, const float* __restrict__ occ_colour,
                                                            const unsigned* __restrict__ noise_key, float sigma, unsigned tag, int K,
                                                            int H, int W, float* __restrict__ out) {
  const int n = blockIdx.z, k = blockIdx.y;
  const unsigned RW = (unsigned)W * (unsigned)C, fe = RW * (unsigned)H;      // (the entry point checked H * W * C < 2^31)
  const unsigned i4 = (blockIdx.x * 256u + threadIdx.x) * 4u;
  if (i4 >= fe) return;
  const bool f32 = kind[n] == 1;
  const bool shifted = !Frames::kTable || shift != nullptr;
  const long long dy = shifted ? shift[2 * n] : 0, dxe = shifted ? (long long)shift[2 * n + 1] * C : 0;   // the column shift in ELEMENTS of a row
  const unsigned long long frame = Frames::frame(addr, n, k, K, fe, f32);
  float* o = out + ((long long)n * K + k) * fe + i4;
  const bool on = colour != nullptr;
  float g0 = 1.f, g1 = 1.f, g2 = 1.f, b0 = 0.f, b1 = 0.f, b2 = 0.f;
  if (on) {
    const float* col = colour + (long long)n * 2 * C;       // gain[C], bias[C]
    g0 = col[0], b0 = col[C];
    if (C == 3) g1 = col[1], g2 = col[2], b1 = col[4], b2 = col[5];
  }
  auto tint = [=](float v, unsigned c) { return aug_tint(v, c, on, g0, g1, g2, b0, b1, b2); };
  const bool occluded = Extras && C == 3 && occ_rect != nullptr;
  const SceneRect q0 = scene_rect(occ_rect, occ_colour, n, 0), q1 = scene_rect(occ_rect, occ_colour, n, 1),
                  q2 = scene_rect(occ_rect, occ_colour, n, 2), q3 = scene_rect(occ_rect, occ_colour, n, 3);
  float z[4] = {0.f, 0.f, 0.f, 0.f};
  const bool noisy = Extras && C == 3 && sigma != 0.f;
  if (noisy) {
    unsigned x[4];
    philox4x32_10(i4 >> 2, (unsigned)k, (unsigned)n, tag, noise_key[0], noise_key[1], x);
    philox_normal_pair(x[0], x[1], z[0], z[1]);
    philox_normal_pair(x[2], x[3], z[2], z[3]);
  }
  // v1 of element j of this thread at (row y, row offset r) -> the stored value
  auto finish = [&](float v, unsigned y, unsigned r, int j) {
    if (occluded) {       // the highest-numbered slot that holds the pixel wins
      const unsigned x = r / 3u, c = r % 3u;
      v = scene_occlude(scene_occlude(scene_occlude(scene_occlude(v, q0, y, x, c), q1, y, x, c), q2, y, x, c), q3, y, x, c);
    }
    return noisy ? fminf(fmaxf(fmaf(sigma, z[j], v), 0.f), 1.f) : v;
  };
  if (RW % 4u != 0) {       // one element at a time
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (i4 + j >= fe) break;
      const unsigned y = (i4 + j) / RW, r = (i4 + j) - y * RW;
      const long long sy = (long long)y - dy, sr = (long long)r - dxe;
      const bool inside = sy >= 0 && sy < H && sr >= 0 && sr < (long long)RW;
      o[j] = finish(inside ? tint(aug_load(frame, f32, sy * RW + sr), C == 3 ? r % 3u : 0u) : 0.f, y, r, j);
    }
    return;
  }
  const unsigned y = i4 / RW, r = i4 - y * RW;      // r % 4 == 0 and r + 3 < RW: the group lies in row y
  const long long sy = (long long)y - dy, sr = (long long)r - dxe;
  const unsigned c0 = C == 3 ? r % 3u : 0u;
  float e[4] = {0.f, 0.f, 0.f, 0.f};
  if (sy >= 0 && sy < H && sr + 3 >= 0 && sr < (long long)RW) {      // at least one source inside the frame
    const long long s0 = sy * RW + sr;
    if (sr >= 0 && sr + 3 < (long long)RW) {                         // all four
      if (f32) {
        const unsigned long long a = frame + (unsigned long long)s0 * 4;
        if ((a & 15u) == 0) {
          const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a));
          e[0] = v.x, e[1] = v.y, e[2] = v.z, e[3] = v.w;
        } else {
          const float* s = reinterpret_cast<const float*>(a);
#pragma unroll
          for (int j = 0; j < 4; ++j) e[j] = s[j];
        }
      } else {
        const unsigned long long a = frame + (unsigned long long)s0, wa = a & ~3ull;
        if (wa == a || (wa >= frame && wa + 8 <= frame + fe)) {
          unsigned v = __builtin_nontemporal_load(reinterpret_cast<const unsigned*>(wa));
          if (wa != a) v = __builtin_amdgcn_alignbyte(__builtin_nontemporal_load(reinterpret_cast<const unsigned*>(wa + 4)), v, (unsigned)(a & 3u));
          u8x4_unit_div(v, e);
        } else {
          const unsigned char* s = reinterpret_cast<const unsigned char*>(a);
#pragma unroll
          for (int j = 0; j < 4; ++j) e[j] = u8_unit_div(s[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) e[j] = tint(e[j], C == 3 ? (c0 + j) % 3u : 0u);
    } else {                                                         // the group crosses the left or right edge of the image
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (sr + j >= 0 && sr + j < (long long)RW) e[j] = tint(aug_load(frame, f32, s0 + j), C == 3 ? (c0 + j) % 3u : 0u);
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) e[j] = finish(e[j], y, r + j, j);
  *reinterpret_cast<f32x4*>(o) = f32x4{e[0], e[1], e[2], e[3]};
}

// The gather alone with C a run-time argument: the kernel geeco_gather_windows_augmented launched for every stream before it took
// instances of the body above.  It stays for ONE-CHANNEL streams only, where the <1, WindowFrames, false> instance measured 5.8 %
// slower (256 x 256 float32 depth); its values are bitwise that instance's.  A change to the load path above is made
// here too until that is looked into.
__global__ __launch_bounds__(256) void gather_windows_augmented_kernel(const long long* __restrict__ addr,
                                                                       const int* __restrict__ kind,
                                                                       const int* __restrict__ shift,
                                                                       const float* __restrict__ colour, int K, int H, int W,
                                                                       int C, float* __restrict__ out) {
  const int n = blockIdx.z, k = blockIdx.y;
  const unsigned RW = (unsigned)W * (unsigned)C, fe = RW * (unsigned)H;      // (the entry point checked H * W * C < 2^31)
  const unsigned i4 = (blockIdx.x * 256u + threadIdx.x) * 4u;
  if (i4 >= fe) return;
  const bool f32 = kind[n] == 1;
  const long long dy = shift[2 * n], dxe = (long long)shift[2 * n + 1] * C;   // the column shift in ELEMENTS of a row
  const unsigned long long frame = (unsigned long long)addr[n] + (unsigned long long)k * fe * (f32 ? 4u : 1u);
  float* o = out + ((long long)n * K + k) * fe + i4;
  const bool on = colour != nullptr;
  float g0 = 1.f, g1 = 1.f, g2 = 1.f, b0 = 0.f, b1 = 0.f, b2 = 0.f;
  if (on) {
    const float* col = colour + (long long)n * 2 * C;       // gain[C], bias[C]
    g0 = col[0], b0 = col[C];
    if (C == 3) g1 = col[1], g2 = col[2], b1 = col[4], b2 = col[5];
  }
  auto tint = [=](float v, unsigned c) { return aug_tint(v, c, on, g0, g1, g2, b0, b1, b2); };
  if (RW % 4u != 0) {       // one element at a time
    for (unsigned j = 0; j < 4 && i4 + j < fe; ++j) {
      const unsigned y = (i4 + j) / RW, r = (i4 + j) - y * RW;
      const long long sy = (long long)y - dy, sr = (long long)r - dxe;
      const bool inside = sy >= 0 && sy < H && sr >= 0 && sr < (long long)RW;
      o[j] = inside ? tint(aug_load(frame, f32, sy * RW + sr), C == 3 ? r % 3u : 0u) : 0.f;
    }
    return;
  }
  const unsigned y = i4 / RW, r = i4 - y * RW;      // r % 4 == 0 and r + 3 < RW: the group lies in row y
  const long long sy = (long long)y - dy, sr = (long long)r - dxe;
  const unsigned c0 = C == 3 ? r % 3u : 0u;
  float e[4] = {0.f, 0.f, 0.f, 0.f};
  if (sy >= 0 && sy < H && sr + 3 >= 0 && sr < (long long)RW) {      // at least one source inside the frame
    const long long s0 = sy * RW + sr;
    if (sr >= 0 && sr + 3 < (long long)RW) {                         // all four
      if (f32) {
        const unsigned long long a = frame + (unsigned long long)s0 * 4;
        if ((a & 15u) == 0) {
          const f32x4 x = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a));
          e[0] = x.x, e[1] = x.y, e[2] = x.z, e[3] = x.w;
        } else {
          const float* s = reinterpret_cast<const float*>(a);
#pragma unroll
          for (int j = 0; j < 4; ++j) e[j] = s[j];
        }
      } else {
        const unsigned long long a = frame + (unsigned long long)s0, wa = a & ~3ull;
        if (wa == a || (wa >= frame && wa + 8 <= frame + fe)) {
          unsigned x = __builtin_nontemporal_load(reinterpret_cast<const unsigned*>(wa));
          if (wa != a) x = __builtin_amdgcn_alignbyte(__builtin_nontemporal_load(reinterpret_cast<const unsigned*>(wa + 4)), x, (unsigned)(a & 3u));
          u8x4_unit_div(x, e);
        } else {
          const unsigned char* s = reinterpret_cast<const unsigned char*>(a);
#pragma unroll
          for (int j = 0; j < 4; ++j) e[j] = u8_unit_div(s[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) e[j] = tint(e[j], C == 3 ? (c0 + j) % 3u : 0u);
    } else {                                                         // the group crosses the left or right edge of the image
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (sr + j >= 0 && sr + j < (long long)RW) e[j] = tint(aug_load(frame, f32, s0 + j), C == 3 ? (c0 + j) % 3u : 0u);
    }
  }
  *reinterpret_cast<f32x4*>(o) = f32x4{e[0], e[1], e[2], e[3]};
}

// ---- the host side: one record of the arguments, one check, one instance choice ------------------------------------------------
struct WindowGatherArgs {
  const int64_t* addr;      // [N] windows, or [N][K] frames
  const int32_t *kind, *shift;
  const float* colour;
  const int32_t* occ_rect;
  const float* occ_colour;
  const uint32_t* noise_key;
  float sigma;
  int tag, N, K, H, W, C;
  float* out;
  void* stream;
};

// The ONE argument check of the three entry points; ``who`` leads every message.  What differs between them: whether ``shift``
// must be set, and whether one-channel frames are taken at all (then with the shift and the tint only).
static int check_window_gather(const char* who, bool shift_required, bool one_channel, const WindowGatherArgs& a) {
  auto misaligned = [](const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; };
  GEECO_CHECK_ARG(a.addr && a.kind && (a.shift || !shift_required) && a.out, "%s: null pointer", who);
  GEECO_CHECK_ARG(a.N >= 1 && a.N <= 65535 && a.K >= 1 && a.K <= 65535, "%s: N=%d, K=%d outside 1..65535", who, a.N, a.K);
  GEECO_CHECK_ARG(a.H >= 1 && a.W >= 1, "%s: H=%d, W=%d must be >= 1", who, a.H, a.W);
  if (one_channel)
    GEECO_CHECK_ARG(a.C == 1 || a.C == 3, "%s: C=%d must be 1 or 3", who, a.C);
  else
    GEECO_CHECK_ARG(a.C == 3, "%s: C=%d must be 3 (occluders and noise are built for RGB streams)", who, a.C);
  const long long frame_elems = (long long)a.H * a.W * a.C;
  GEECO_CHECK_ARG(frame_elems <= 0x7fffffffLL, "%s: a frame of %lld elements is too large", who, frame_elems);
  GEECO_CHECK_ARG(a.sigma >= 0.f && a.sigma < 1.f, "%s: sigma=%g outside [0, 1)", who, (double)a.sigma);
  GEECO_CHECK_ARG(a.tag == 0 || a.tag == 1, "%s: tag=%d must be 0 (rgb) or 1 (target_rgb)", who, a.tag);
  GEECO_CHECK_ARG((a.occ_rect == nullptr) == (a.occ_colour == nullptr), "%s: occ_rect and occ_colour must be null together", who);
  GEECO_CHECK_ARG(a.noise_key || a.sigma == 0.f, "%s: sigma=%g needs a noise key", who, (double)a.sigma);
  GEECO_CHECK_ARG(a.C == 3 || (!a.occ_rect && a.sigma == 0.f),
                  "%s: C=%d takes the shift only (occluders and noise are built for RGB streams)", who, a.C);
  GEECO_CHECK_ARG(!misaligned(a.out, 15), "%s: out must be 16-byte aligned", who);
  GEECO_CHECK_ARG(!misaligned(a.addr, 7) && !misaligned(a.kind, 3) && !misaligned(a.shift, 3) && !misaligned(a.colour, 3) &&
                      !misaligned(a.occ_rect, 3) && !misaligned(a.occ_colour, 3) && !misaligned(a.noise_key, 3),
                  "%s: the tables must be aligned for their element types", who);
  return 0;
}

// The ONE instance choice, from (C, any extras); the grid is blockIdx = (unit of 1024 elements, k, n) for every kernel.  One-channel
// frames of consecutive windows (the check has refused their extras) go to the run-time-C kernel, see there.
template <typename Frames>
static void launch_window_gather(const WindowGatherArgs& a) {
  const dim3 grid((unsigned)cdiv64((int64_t)a.H * a.W * a.C, 1024), (unsigned)a.K, (unsigned)a.N);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, (hipStream_t)a.stream, (const long long*)a.addr, a.kind, a.shift, a.colour,
                       a.occ_rect, a.occ_colour, a.noise_key, a.sigma, (unsigned)a.tag, a.K, a.H, a.W, a.out);
  };
  if (a.C == 3 && (a.occ_rect || a.sigma != 0.f))
    launch(window_gather_kernel<3, Frames, true>);
  else if (a.C == 3)
    launch(window_gather_kernel<3, Frames, false>);
  else if constexpr (Frames::kTable)
    launch(window_gather_kernel<1, Frames, false>);
  else
    hipLaunchKernelGGL(gather_windows_augmented_kernel, grid, dim3(256), 0, (hipStream_t)a.stream, (const long long*)a.addr, a.kind,
                       a.shift, a.colour, a.K, a.H, a.W, a.C, a.out);
}

extern "C" int geeco_gather_windows_augmented(const int64_t* addr, const int32_t* kind, const int32_t* shift, const float* colour,
                                              int N, int K, int H, int W, int C, float* out, void* stream) {
  const WindowGatherArgs a{addr, kind, shift, colour, nullptr, nullptr, nullptr, 0.f, 0, N, K, H, W, C, out, stream};
  if (const int rc = check_window_gather("gather_windows_augmented", true, true, a)) return rc;
  launch_window_gather<WindowFrames>(a);
  GEECO_LAUNCH_CHECK();
  return 0;
}

extern "C" int geeco_gather_windows_scene(const int64_t* addr, const int32_t* kind, const int32_t* shift, const float* colour,
                                          const int32_t* occ_rect, const float* occ_colour, const uint32_t* noise_key, float sigma,
                                          int tag, int N, int K, int H, int W, int C, float* out, void* stream) {
  const WindowGatherArgs a{addr, kind, shift, colour, occ_rect, occ_colour, noise_key, sigma, tag, N, K, H, W, C, out, stream};
  if (const int rc = check_window_gather("gather_windows_scene", true, false, a)) return rc;
  launch_window_gather<WindowFrames>(a);
  GEECO_LAUNCH_CHECK();
  return 0;
}

// ---- frame-table entry: ONE ADDRESS PER FRAME (camera frame drops and latency) -------------------------------------
// out[n][k] is built from the frame at frame_addr[n][k]: a window whose slot k shows an earlier frame (a dropped frame delivered
// again, a camera that lags the encoders) is the same gather with another address source (TableFrames above); the body, and with
// it every value, is the other entries'.  The table is read when the kernel runs.  Alignment is a property of the FRAME here: a
// uint8 frame of H * W * 3 bytes that is no multiple of 4 puts consecutive frames at different residues, and a lagged or dropped
// slot points where its neighbours do not, so nothing about slot 0 may decide for slot k -- the body takes each load width from
// the element's own address and blockIdx = (unit, k, n) keeps that choice uniform per block wherever the frame base alone decides
// it.  The noise counter is (e / 4, k, n, tag) with k the OUTPUT slot: a frame shown twice gets fresh sensor noise each time.
extern "C" int geeco_gather_windows_frames(const int64_t* frame_addr, const int32_t* kind, const int32_t* shift, const float* colour,
                                           const int32_t* occ_rect, const float* occ_colour, const uint32_t* noise_key, float sigma,
                                           int tag, int N, int K, int H, int W, int C, float* out, void* stream) {
  const WindowGatherArgs a{frame_addr, kind, shift, colour, occ_rect, occ_colour, noise_key, sigma, tag, N, K, H, W, C, out, stream};
  if (const int rc = check_window_gather("gather_windows_frames", false, true, a)) return rc;
  launch_window_gather<TableFrames>(a);
  GEECO_LAUNCH_CHECK();
  return 0;
}

