// Episode replay for the dynamic-image controllers (geeco_amd/replay_dynimg.py): geeco-f (proc_obs 'dynimg') and
// 'sequence' x 'dyndiff'.  With the goal fixed for the episode every conv1 input of these models is a function of the frame
// number alone, so the episode's inputs are built in chunks of many frames, straight from the resident frames:
//      replay_images: for the windows t0 .. t1 - 1 the current frame (R, G, B, 0), the normalised pair image of (frame t, goal)
//                     and the normalised buffer image of the frames max(0, t - K + 1 + k), k = 0 .. K - 1 (the predictor's window
//                     after a reset at frame 0 and t pushes, predictor.py:192-200; replay.window_frames);
// and nothing else: the window states of the 'sequence' x 'dyndiff' model (geeco_replay_states_pair) come from the one state
// kernel in replay.hip, and the window checks, thread and block constants every replay entry point uses from replay_internal.h.
//
// The image stage is TWO launches and no block waits for another block: launch 1 forms both raw images in registers and leaves
// each block's min / max of them in ws; launch 2 folds a window's partials, forms the images AGAIN and stores them normalised,
// once.  The alternative -- store the raw images in launch 1, normalise in place in launch 2 -- was decided against by counted
// bytes per window pixel (uint8 frames, K = 16, both images):
//   recompute:  frames read 2 x (K + 2) x 3 B = 108 B, all but the first touch of a frame from cache (one episode is 19.7 MB);
//               written to memory 48 B (three images, once);
//   in place:   frames read 54 B from cache; written 48 B, then 32 B read back and 32 B written again: 112 B of image traffic
//               on buffers of T x HW x 32 B (210 MB at T = 100, 256 x 256: past every cache).
// So recomputing trades 54 B of cached reads for 64 B of memory traffic (float32 frames: 216 B for 64 B, nearer to even; one
// form serves both).  The one-pass stage's arrival counters (dynimg_goal.hip) rely on workgroups starting in index order,
// documented there as not guaranteed; this grid is windows x blocks of a launch nobody has characterised, so that wait is not
// copied: ws needs no zero-fill and there is no timeout word.
//
// Arithmetic: the sums of dynimg_wsum3_kernel (0 + alpha_0 X_0, + alpha_1 X_1, .. in frame order, compiled with the same
// contraction) and the normalisation of dynimg_norm_kernel ((D - min) / (max - min + 1e-6f), IEEE division); the uint8
// conversion is u8x4_unit of frame_ingest.h.  Both launches run ONE inlined body (ri_images), so launch 2 normalises exactly
// the values launch 1 took the extrema of.  Min / max are folded in a fixed order without atomics: two runs are bitwise equal.
//
// From replay_internal.h: RP_THREADS, RP_MAX_BLOCKS, check_replay_windows, DYN_MAXK; from frame_ingest.h: u8x4_unit, ld_vec.
#include "replay_internal.h"
#include "frame_ingest.h"

struct ReplayImgParams {
  const unsigned long long* addr;      // [T] device addresses of the episode's frames ([HW][3], uint8 or float32)
  const void* goal;                    // one frame of the same kind
  int t0, n, K, bpw;                   // first window, windows, window length, blocks per window
  long long HW;
  float* cur_out;                      // [n][HW][4]
  float* buf_out;                      // [n][HW][4] or null
  float* diff_out;                     // [n][HW][4]
  float* part;                         // [n][bpw][4]: min, max of the buffer image, min, max of the pair image, per block
  float alpha[DYN_MAXK];
  float alpha2[2];
};

// 4 pixels = three float4 of a frame: 12 bytes of a uint8 frame or 48 of a float32 one (plain loads: a frame is read by up to K
// windows and by both launches)
template <bool U8>
__device__ __forceinline__ void ri_load(const void* frame, long long u, f32x4& v0, f32x4& v1, f32x4& v2) {
  if (U8) {
    const unsigned int* s = reinterpret_cast<const unsigned int*>(frame) + u * 3;
    const unsigned int b0 = s[0], b1 = s[1], b2 = s[2];
    v0 = u8x4_unit(b0);
    v1 = u8x4_unit(b1);
    v2 = u8x4_unit(b2);
  } else {
    const f32x4* s = reinterpret_cast<const f32x4*>(frame) + u * 3;
    v0 = s[0];
    v1 = s[1];
    v2 = s[2];
  }
}

// Unit u (4 pixels) of window t: the current frame c, the raw buffer image A (BUF) and the raw pair image D, summed as
// dynimg_wsum3_kernel sums them
template <bool U8, bool BUF>
__device__ __forceinline__ void ri_images(const ReplayImgParams& p, int t, long long u, f32x4 (&c)[3], f32x4 (&A)[3], f32x4 (&D)[3]) {
  A[0] = A[1] = A[2] = f32x4{0, 0, 0, 0};
  D[0] = D[1] = D[2] = f32x4{0, 0, 0, 0};
  if (BUF) {
#pragma unroll 4
    for (int k = 0; k < p.K - 1; ++k) {
      int f = t - p.K + 1 + k;      // the frame slot k of window t shows
      if (f < 0) f = 0;             // first-frame padding after the reset at frame 0
      const float w = p.alpha[k];
      f32x4 v0, v1, v2;
      ri_load<U8>(reinterpret_cast<const void*>(p.addr[f]), u, v0, v1, v2);
      A[0] += w * v0;
      A[1] += w * v1;
      A[2] += w * v2;
    }
  }
  ri_load<U8>(reinterpret_cast<const void*>(p.addr[t]), u, c[0], c[1], c[2]);
  f32x4 g0, g1, g2;
  ri_load<U8>(p.goal, u, g0, g1, g2);
  if (BUF) {
    const float w = p.alpha[p.K - 1];
    A[0] += w * c[0];
    A[1] += w * c[1];
    A[2] += w * c[2];
  }
  const float w0 = p.alpha2[0], w1 = p.alpha2[1];
  D[0] += w0 * c[0];
  D[1] += w0 * c[1];
  D[2] += w0 * c[2];
  D[0] += w1 * g0;
  D[1] += w1 * g1;
  D[2] += w1 * g2;
}

__device__ __forceinline__ void ri_minmax(const f32x4 (&X)[3], float& mn, float& mx) {
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    mn = fminf(fminf(mn, fminf(X[q].x, X[q].y)), fminf(X[q].z, X[q].w));
    mx = fmaxf(fmaxf(mx, fmaxf(X[q].x, X[q].y)), fmaxf(X[q].z, X[q].w));
  }
}

// the four extrema of a block: lanes by wave_reduce, the four waves ascending; every thread returns them (one barrier inside)
__device__ __forceinline__ f32x4 ri_block_fold(float (&red)[4][4], float mn1, float mx1, float mn2, float mx2) {
  mn1 = wave_reduce_min(mn1);
  mx1 = wave_reduce_max(mx1);
  mn2 = wave_reduce_min(mn2);
  mx2 = wave_reduce_max(mx2);
  const int wid = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[wid][0] = mn1;
    red[wid][1] = mx1;
    red[wid][2] = mn2;
    red[wid][3] = mx2;
  }
  __syncthreads();
  f32x4 r = {red[0][0], red[0][1], red[0][2], red[0][3]};
#pragma unroll
  for (int i = 1; i < 4; ++i) {
    r.x = fminf(r.x, red[i][0]);
    r.y = fmaxf(r.y, red[i][1]);
    r.z = fminf(r.z, red[i][2]);
    r.w = fmaxf(r.w, red[i][3]);
  }
  return r;
}

// 4 pixels of an [n][HW][4] image: three RGB float4 -> four (R, G, B, 0)
__device__ __forceinline__ void ri_store(float* img, long long row, long long HW, long long u, const f32x4 (&X)[3]) {
  f32x4* dst = reinterpret_cast<f32x4*>(img + (row * HW + u * 4) * 4);
  dst[0] = f32x4{X[0].x, X[0].y, X[0].z, 0.f};
  dst[1] = f32x4{X[0].w, X[1].x, X[1].y, 0.f};
  dst[2] = f32x4{X[1].z, X[1].w, X[2].x, 0.f};
  dst[3] = f32x4{X[2].y, X[2].z, X[2].w, 0.f};
}

__device__ __forceinline__ void ri_normalise(f32x4 (&X)[3], float m, float r) {
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    X[q].x = (X[q].x - m) / r;
    X[q].y = (X[q].y - m) / r;
    X[q].z = (X[q].z - m) / r;
    X[q].w = (X[q].w - m) / r;
  }
}

// A work item = (window, block of 256 units); a block takes the items blockIdx.x, + gridDim.x, ..
// Launch 1: the item's min / max of both raw images -> part[item]
template <bool U8, bool BUF>
__global__ __launch_bounds__(RP_THREADS) void replay_images_minmax_kernel(const ReplayImgParams p) {
  __shared__ float red[4][4];
  const long long U = p.HW >> 2;
  const long long items = (long long)p.n * p.bpw;
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const int w = (int)(it / p.bpw), b = (int)(it - (long long)w * p.bpw);
    const long long u = (long long)b * RP_THREADS + threadIdx.x;
    float mn1 = INFINITY, mx1 = -INFINITY, mn2 = INFINITY, mx2 = -INFINITY;
    if (u < U) {
      f32x4 c[3], A[3], D[3];
      ri_images<U8, BUF>(p, p.t0 + w, u, c, A, D);
      if (BUF) ri_minmax(A, mn1, mx1);
      ri_minmax(D, mn2, mx2);
    }
    const f32x4 r = ri_block_fold(red, mn1, mx1, mn2, mx2);
    if (threadIdx.x == 0) *reinterpret_cast<f32x4*>(p.part + it * 4) = r;
    __syncthreads();      // red is written again in the next item
  }
}

// Launch 2: the window's partials folded (a thread over the blocks i, i + 256, .. ascending, then as a block's), both images formed
// again, normalised and stored with the current frame's padded copy
template <bool U8, bool BUF>
__global__ __launch_bounds__(RP_THREADS) void replay_images_emit_kernel(const ReplayImgParams p) {
  __shared__ float red[4][4];
  const long long U = p.HW >> 2;
  const long long items = (long long)p.n * p.bpw;
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const int w = (int)(it / p.bpw), b = (int)(it - (long long)w * p.bpw);
    const long long u = (long long)b * RP_THREADS + threadIdx.x;
    float mn1 = INFINITY, mx1 = -INFINITY, mn2 = INFINITY, mx2 = -INFINITY;
    for (int i = threadIdx.x; i < p.bpw; i += RP_THREADS) {
      const f32x4 q = *reinterpret_cast<const f32x4*>(p.part + ((long long)w * p.bpw + i) * 4);
      mn1 = fminf(mn1, q.x);
      mx1 = fmaxf(mx1, q.y);
      mn2 = fminf(mn2, q.z);
      mx2 = fmaxf(mx2, q.w);
    }
    const f32x4 r = ri_block_fold(red, mn1, mx1, mn2, mx2);
    if (u < U) {
      f32x4 c[3], A[3], D[3];
      ri_images<U8, BUF>(p, p.t0 + w, u, c, A, D);
      ri_store(p.cur_out, w, p.HW, u, c);
      if (BUF) {
        ri_normalise(A, r.x, r.y - r.x + 1e-6f);      // graph.py:49
        ri_store(p.buf_out, w, p.HW, u, A);
      }
      ri_normalise(D, r.z, r.w - r.z + 1e-6f);
      ri_store(p.diff_out, w, p.HW, u, D);
    }
    __syncthreads();      // red is written again in the next item
  }
}

extern "C" int64_t geeco_replay_images_ws_bytes(int windows, int64_t HW) {
  if (windows <= 0 || HW <= 0) return 0;
  return (int64_t)windows * cdiv64(HW >> 2, RP_THREADS) * 16;
}

extern "C" int geeco_replay_images(const void* const* frame_addr, const void* goal, int frames_u8, const float* alpha_host,
                                   const float* alpha2_host, int T, int t0, int t1, int K, int64_t HW, float* cur_out,
                                   float* buf_out, float* diff_out, void* ws, void* stream) {
  GEECO_CHECK_ARG(frame_addr && goal && alpha_host && alpha2_host && cur_out && diff_out && ws, "replay_images: null pointer");
  GEECO_CHECK_ARG(HW >= 4 && (HW & 3) == 0 && HW < (1ll << 40), "replay_images: HW=%lld must be a multiple of 4", (long long)HW);
  if (int rc = check_replay_windows("replay_images", T, t0, t1, t1 - t0, K)) return rc;      // (one output row per window)
  const uintptr_t outs = reinterpret_cast<uintptr_t>(cur_out) | reinterpret_cast<uintptr_t>(buf_out) |
                         reinterpret_cast<uintptr_t>(diff_out) | reinterpret_cast<uintptr_t>(ws);
  GEECO_CHECK_ARG((outs & 15) == 0, "replay_images: outputs and ws must be 16-byte aligned");
  GEECO_CHECK_ARG((reinterpret_cast<uintptr_t>(goal) & (frames_u8 ? 3 : 15)) == 0 && (reinterpret_cast<uintptr_t>(frame_addr) & 7) == 0,
                  "replay_images: misaligned goal frame or address table");
  ReplayImgParams p = {};
  p.addr = reinterpret_cast<const unsigned long long*>(frame_addr);
  p.goal = goal;
  p.t0 = t0; p.n = t1 - t0; p.K = K; p.HW = HW;
  p.bpw = (int)cdiv64(HW >> 2, RP_THREADS);
  p.cur_out = cur_out; p.buf_out = buf_out; p.diff_out = diff_out; p.part = (float*)ws;
  for (int k = 0; k < K; ++k) p.alpha[k] = alpha_host[k];
  p.alpha2[0] = alpha2_host[0]; p.alpha2[1] = alpha2_host[1];
  const unsigned grid = (unsigned)std::min<long long>((long long)p.n * p.bpw, RP_MAX_BLOCKS);
  hipStream_t s = (hipStream_t)stream;
#define RI_LAUNCH(U8, BUF)                                                                                                      \
  do {                                                                                                                          \
    geeco_note_kernel("replay_images_minmax_kernel<%s, %s>", U8 ? "true" : "false", BUF ? "true" : "false");                    \
    hipLaunchKernelGGL((replay_images_minmax_kernel<U8, BUF>), dim3(grid), dim3(RP_THREADS), 0, s, p);                          \
    GEECO_LAUNCH_CHECK();                                                                                                       \
    geeco_note_kernel("replay_images_emit_kernel<%s, %s>", U8 ? "true" : "false", BUF ? "true" : "false");                     \
    hipLaunchKernelGGL((replay_images_emit_kernel<U8, BUF>), dim3(grid), dim3(RP_THREADS), 0, s, p);                           \
  } while (0)
  if (frames_u8) {
    if (buf_out) RI_LAUNCH(true, true);
    else RI_LAUNCH(true, false);
  } else {
    if (buf_out) RI_LAUNCH(false, true);
    else RI_LAUNCH(false, false);
  }
#undef RI_LAUNCH
  GEECO_LAUNCH_CHECK();
  return 0;
}
