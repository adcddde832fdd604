// Input and output stages of the batched predictor (geeco_amd/batched_predictor.py): B control loops stepped by one call.
//
// Per env the semantics are the batch-1 predictor's (reference src/models/e2evmc/predictor.py:127-209): a window of the last
// K frames, padded with the first frame after a reset; frames range-checked on channels 0..2; the gripper logits re-mapped
// to argmax - 1.  One call = one H2D of a staging block, one replayed graph (range check -> window push -> forward -> output
// pack), one D2H.  All four stages are HBM streaming (or tiny): 16-byte loads and stores, one thread per fixed set of pixels.
//
// The control words `ctl` [B + 1] int32: ctl[b] = 1 when env b's frame failed the range check, ctl[B] = 1 when any did.  The
// range check only ever sets them; the output pack copies them out and zeroes them again, so every call starts from zeros.
//
// From frame_ingest.h: u8_unit_div, load_rgb4 (the uint8 / float32 frame loads of load_new) and ld_vec; from state_layout.h: the
// state columns and check_state_layout of the feature push.
#include "dynimg_internal.h"      // DYN_MAXK
#include "frame_ingest.h"
#include "state_layout.h"

#define PIO_MAXK DYN_MAXK       // the window lengths the input kernels of the models take
#define GEECO_PREDICT_FEAT_THREADS 1024      // one block per env in the feature push + gather

// ---- 1. frame range check ---------------------------------------------------------------------------------------------
// channels 0..2 of every env's new float frame inside [lo, hi]; a NaN fails (NaN compares false, as np.amin turns NaN)
template <int C>
__global__ __launch_bounds__(256) void range_check_kernel(const float* __restrict__ frames, long long HW, float lo, float hi,
                                                          int* __restrict__ ctl, int B) {
  const int b = blockIdx.y;
  const float* f = frames + (long long)b * HW * C;
  const long long n4 = HW * C / 4;           // float4 units of the env's frame (HW * C % 4 == 0 on this path)
  int bad = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(f) + i);
    if (C == 4) {            // one float4 = one pixel: r, g, b, depth (depth is not checked, predictor.py:135)
      bad |= !(v.x >= lo && v.x <= hi) | !(v.y >= lo && v.y <= hi) | !(v.z >= lo && v.z <= hi);
    } else {
      bad |= !(v.x >= lo && v.x <= hi) | !(v.y >= lo && v.y <= hi) | !(v.z >= lo && v.z <= hi) | !(v.w >= lo && v.w <= hi);
    }
  }
  if (__syncthreads_or(bad) && threadIdx.x == 0) {
    ctl[b] = 1;                // plain stores of the same value from every block that saw a bad pixel
    ctl[B] = 1;
  }
}

// any shape (HW * C % 4 != 0): one element per step
template <int C>
__global__ __launch_bounds__(256) void range_check_scalar_kernel(const float* __restrict__ frames, long long HW, float lo,
                                                                 float hi, int* __restrict__ ctl, int B) {
  const int b = blockIdx.y;
  const float* f = frames + (long long)b * HW * C;
  int bad = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < HW * C; i += (long long)gridDim.x * 256) {
    const float v = f[i];
    if (i % C < 3) bad |= !(v >= lo && v <= hi);
  }
  if (__syncthreads_or(bad) && threadIdx.x == 0) {
    ctl[b] = 1;
    ctl[B] = 1;
  }
}

extern "C" int geeco_predict_range_check(const float* frames, int B, int64_t HW, int C, float lo, float hi, int* ctl,
                                         void* stream) {
  GEECO_CHECK_ARG(frames && ctl, "predict_range_check: null pointer");
  GEECO_CHECK_ARG(B >= 1, "predict_range_check: B=%d must be >= 1", B);
  GEECO_CHECK_ARG(C == 3 || C == 4, "predict_range_check: C=%d must be 3 or 4", C);
  GEECO_CHECK_ARG(HW >= 1, "predict_range_check: HW=%lld", (long long)HW);
  const bool vec = (HW * C) % 4 == 0 && (reinterpret_cast<uintptr_t>(frames) & 15) == 0;
  const long long work = vec ? HW * C / 4 : HW * C;
  const int nblk = (int)std::min<long long>(cdiv64(work, 256 * 4), 64);
  dim3 grid((unsigned)nblk, (unsigned)B);
  hipStream_t s = (hipStream_t)stream;
  if (vec && C == 3) {
    geeco_note_kernel("range_check_kernel<3>");
    hipLaunchKernelGGL(range_check_kernel<3>, grid, dim3(256), 0, s, frames, (long long)HW, lo, hi, ctl, B);
  } else if (vec) {
    geeco_note_kernel("range_check_kernel<4>");
    hipLaunchKernelGGL(range_check_kernel<4>, grid, dim3(256), 0, s, frames, (long long)HW, lo, hi, ctl, B);
  } else if (C == 3) {
    geeco_note_kernel("range_check_scalar_kernel<3>");
    hipLaunchKernelGGL(range_check_scalar_kernel<3>, grid, dim3(256), 0, s, frames, (long long)HW, lo, hi, ctl, B);
  } else {
    geeco_note_kernel("range_check_scalar_kernel<4>");
    hipLaunchKernelGGL(range_check_scalar_kernel<4>, grid, dim3(256), 0, s, frames, (long long)HW, lo, hi, ctl, B);
  }
  GEECO_LAUNCH_CHECK();
  return 0;
}

// ---- joint-state window (both push forms): the last block of each env shifts its [K][J] window -------------------------
__device__ __forceinline__ void push_jnt(const float* __restrict__ jnt, int reset, int b, int K, int J, float* __restrict__ jw) {
  for (int j = threadIdx.x; j < J; j += blockDim.x) {
    const float v = jnt[(long long)b * J + j];
    float* w = jw + (long long)b * K * J + j;
    if (reset) {
      for (int t = 0; t < K; ++t) w[(long long)t * J] = v;
    } else {
      for (int t = 0; t + 1 < K; ++t) w[(long long)t * J] = w[(long long)(t + 1) * J];
      w[(long long)(K - 1) * J] = v;
    }
  }
}

// ---- 2. window push, dense form -------------------------------------------------------------------------------------
// rgb [B][K][HW][3], depth [B][K][HW] (C == 4: split out of the [HW][4] frame in registers), jnt_state [B][K][J].
// A thread owns PIX pixels of one env and walks t = 0..K-1 in order: it reads slot t + 1 before it writes slot t, and no
// other thread touches those pixels, so the shift is in place and race-free.
template <int PIX, int C, bool U8>
__device__ __forceinline__ void load_new(const void* frames, int b, long long HW, long long u, float (&px)[PIX * 3],
                                         float (&dp)[PIX]) {
  if (U8) {        // C == 3
    const unsigned char* f = reinterpret_cast<const unsigned char*>(frames) + (long long)b * HW * 3 + u * PIX * 3;
    if constexpr (PIX == 4) {
      load_rgb4(reinterpret_cast<const unsigned*>(f), px);
    } else {
#pragma unroll
      for (int k = 0; k < PIX * 3; ++k) px[k] = u8_unit_div(f[k]);
    }
    return;
  }
  const float* f = reinterpret_cast<const float*>(frames) + (long long)b * HW * C + u * PIX * C;
  if constexpr (PIX == 4 && C == 3) {
    load_rgb4(reinterpret_cast<const f32x4*>(f), px);
    return;
  }
  float v[PIX * C];
  if (PIX == 4) {
#pragma unroll
    for (int q = 0; q < C; ++q) {
      const f32x4 x = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(f) + q);
      v[q * 4 + 0] = x.x;
      v[q * 4 + 1] = x.y;
      v[q * 4 + 2] = x.z;
      v[q * 4 + 3] = x.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < PIX * C; ++k) v[k] = f[k];
  }
#pragma unroll
  for (int p = 0; p < PIX; ++p) {
#pragma unroll
    for (int c = 0; c < 3; ++c) px[p * 3 + c] = v[p * C + c];
    if (C == 4) dp[p] = v[p * C + 3];
  }
}

template <int PIX, int C>
__device__ __forceinline__ void slot_load(const float* rgb, const float* dep, float (&px)[PIX * 3], float (&dp)[PIX]) {
  if (PIX == 4) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const f32x4 x = reinterpret_cast<const f32x4*>(rgb)[q];
      px[q * 4 + 0] = x.x;
      px[q * 4 + 1] = x.y;
      px[q * 4 + 2] = x.z;
      px[q * 4 + 3] = x.w;
    }
    if (C == 4) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(dep);
      dp[0] = x.x;
      dp[1] = x.y;
      dp[2] = x.z;
      dp[3] = x.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < PIX * 3; ++k) px[k] = rgb[k];
    if (C == 4) {
#pragma unroll
      for (int k = 0; k < PIX; ++k) dp[k] = dep[k];
    }
  }
}

template <int PIX, int C>
__device__ __forceinline__ void slot_store(float* rgb, float* dep, const float (&px)[PIX * 3], const float (&dp)[PIX]) {
  if (PIX == 4) {
#pragma unroll
    for (int q = 0; q < 3; ++q)
      reinterpret_cast<f32x4*>(rgb)[q] = f32x4{px[q * 4 + 0], px[q * 4 + 1], px[q * 4 + 2], px[q * 4 + 3]};
    if (C == 4) *reinterpret_cast<f32x4*>(dep) = f32x4{dp[0], dp[1], dp[2], dp[3]};
  } else {
#pragma unroll
    for (int k = 0; k < PIX * 3; ++k) rgb[k] = px[k];
    if (C == 4) {
#pragma unroll
      for (int k = 0; k < PIX; ++k) dep[k] = dp[k];
    }
  }
}

template <int PIX, int C, bool U8>
__global__ __launch_bounds__(256) void push_dense_kernel(const void* __restrict__ frames, const float* __restrict__ jnt,
                                                         const int* __restrict__ reset, const int* __restrict__ any_bad, int K,
                                                         long long HW, int J, float* __restrict__ rgb, float* __restrict__ depth,
                                                         float* __restrict__ jnt_state) {
  if (*any_bad) return;      // a frame failed the range check: no env's window moves
  const int b = blockIdx.y;
  const int rs = reset[b];
  if (blockIdx.x == gridDim.x - 1) {
    push_jnt(jnt, rs, b, K, J, jnt_state);
    return;
  }
  const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
  if (u >= HW / PIX) return;
  float nv[PIX * 3], nd[PIX];
  load_new<PIX, C, U8>(frames, b, HW, u, nv, nd);
  float* r = rgb + (long long)b * K * HW * 3 + u * PIX * 3;
  float* d = C == 4 ? depth + (long long)b * K * HW + u * PIX : nullptr;
  if (!rs) {
    for (int t = 0; t + 1 < K; ++t) {
      float px[PIX * 3], dp[PIX];
      slot_load<PIX, C>(r + (long long)(t + 1) * HW * 3, C == 4 ? d + (long long)(t + 1) * HW : nullptr, px, dp);
      slot_store<PIX, C>(r + (long long)t * HW * 3, C == 4 ? d + (long long)t * HW : nullptr, px, dp);
    }
    slot_store<PIX, C>(r + (long long)(K - 1) * HW * 3, C == 4 ? d + (long long)(K - 1) * HW : nullptr, nv, nd);
  } else {                   // the first frame after a reset pads the whole window (predictor.py:197-198)
    for (int t = 0; t < K; ++t)
      slot_store<PIX, C>(r + (long long)t * HW * 3, C == 4 ? d + (long long)t * HW : nullptr, nv, nd);
  }
}

template <int PIX>
static void launch_push_dense(dim3 grid, hipStream_t s, const void* frames, int u8, int C, const float* jnt, const int* reset,
                              const int* any_bad, int K, long long HW, int J, float* rgb, float* depth, float* jnt_state) {
  if (u8) {
    geeco_note_kernel("push_dense_kernel<%d, 3, true>", PIX);
    hipLaunchKernelGGL((push_dense_kernel<PIX, 3, true>), grid, dim3(256), 0, s, frames, jnt, reset, any_bad, K, HW, J, rgb,
                       depth, jnt_state);
  } else if (C == 3) {
    geeco_note_kernel("push_dense_kernel<%d, 3, false>", PIX);
    hipLaunchKernelGGL((push_dense_kernel<PIX, 3, false>), grid, dim3(256), 0, s, frames, jnt, reset, any_bad, K, HW, J, rgb,
                       depth, jnt_state);
  } else {
    geeco_note_kernel("push_dense_kernel<%d, 4, false>", PIX);
    hipLaunchKernelGGL((push_dense_kernel<PIX, 4, false>), grid, dim3(256), 0, s, frames, jnt, reset, any_bad, K, HW, J, rgb,
                       depth, jnt_state);
  }
}

extern "C" int geeco_predict_push_dense(const void* frames, int frames_u8, const float* jnt, const int* reset, const int* any_bad,
                                        int B, int K, int64_t HW, int C, int J, float* rgb, float* depth, float* jnt_state,
                                        void* stream) {
  GEECO_CHECK_ARG(frames && jnt && reset && any_bad && rgb && jnt_state && (C != 4 || depth),
                  "predict_push_dense: null pointer");
  GEECO_CHECK_ARG(B >= 1, "predict_push_dense: B=%d must be >= 1", B);
  GEECO_CHECK_ARG(K >= 1 && K <= PIO_MAXK, "predict_push_dense: K=%d outside 1..%d", K, PIO_MAXK);
  GEECO_CHECK_ARG(C == 3 || C == 4, "predict_push_dense: C=%d must be 3 or 4", C);
  GEECO_CHECK_ARG(!frames_u8 || C == 3, "predict_push_dense: uint8 frames are RGB (C=3), got C=%d", C);
  GEECO_CHECK_ARG(HW >= 1 && J >= 1, "predict_push_dense: HW=%lld J=%d", (long long)HW, J);
  const uintptr_t al = reinterpret_cast<uintptr_t>(frames) | reinterpret_cast<uintptr_t>(rgb) |
                       reinterpret_cast<uintptr_t>(depth);
  const bool vec = HW % 4 == 0 && (al & 15) == 0;
  const int pix = vec ? 4 : 1;
  dim3 grid((unsigned)(cdiv64(HW / pix, 256) + 1), (unsigned)B);
  hipStream_t s = (hipStream_t)stream;
  if (vec) launch_push_dense<4>(grid, s, frames, frames_u8, C, jnt, reset, any_bad, K, HW, J, rgb, depth, jnt_state);
  else launch_push_dense<1>(grid, s, frames, frames_u8, C, jnt, reset, any_bad, K, HW, J, rgb, depth, jnt_state);
  GEECO_LAUNCH_CHECK();
  return 0;
}

// ---- 3. window push, ring form --------------------------------------------------------------------------------------
// ring [B][2K][FB] uint8 (FB = HW * 3 bytes per frame), mirrored: logical position q lives in slots q and q + K.  heads[b] =
// the position the next frame goes to.  A frame written at p (slots p and p + K) makes slots p + 1 .. p + K the env's window
// oldest first, always contiguous; the advance kernel writes that start into win_table[b] and moves the head.  No frame is
// ever moved: per env and call FB bytes are read and 2 FB written (2K FB after a reset: every slot gets the frame).
template <typename V>
__global__ __launch_bounds__(256) void push_ring_kernel(const unsigned char* __restrict__ frames, const float* __restrict__ jnt,
                                                        const int* __restrict__ reset, const int* __restrict__ any_bad,
                                                        const int* __restrict__ heads, int K, long long FB, int J,
                                                        unsigned char* __restrict__ ring, float* __restrict__ jnt_state) {
  if (*any_bad) return;
  const int b = blockIdx.y;
  const int rs = reset[b];
  if (blockIdx.x == gridDim.x - 1) {
    push_jnt(jnt, rs, b, K, J, jnt_state);
    return;
  }
  const long long sv = FB / (long long)sizeof(V);      // units of V per frame = the slot stride
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= sv) return;
  const V v = __builtin_nontemporal_load(reinterpret_cast<const V*>(frames + (long long)b * FB) + i);
  V* r = reinterpret_cast<V*>(ring + (long long)b * 2 * K * FB) + i;
  if (rs) {
    for (int t = 0; t < 2 * K; ++t) r[t * sv] = v;
  } else {
    const int p = heads[b];
    r[p * sv] = v;
    r[(p + K) * sv] = v;
  }
}

__global__ void ring_advance_kernel(const int* __restrict__ any_bad, int B, int K, long long FB, const unsigned char* ring,
                                    int* __restrict__ heads, long long* __restrict__ win_table) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B || *any_bad) return;
  const int p = heads[b];
  win_table[b] = (long long)(uintptr_t)(ring + ((long long)b * 2 * K + p + 1) * FB);
  heads[b] = p + 1 == K ? 0 : p + 1;
}

extern "C" int geeco_predict_push_ring(const unsigned char* frames, const float* jnt, const int* reset, const int* any_bad,
                                       int B, int K, int64_t HW, int J, unsigned char* ring, int* heads, int64_t* win_table,
                                       float* jnt_state, void* stream) {
  GEECO_CHECK_ARG(frames && jnt && reset && any_bad && ring && heads && win_table && jnt_state,
                  "predict_push_ring: null pointer");
  GEECO_CHECK_ARG(B >= 1, "predict_push_ring: B=%d must be >= 1", B);
  GEECO_CHECK_ARG(K >= 1 && K <= PIO_MAXK, "predict_push_ring: K=%d outside 1..%d", K, PIO_MAXK);
  GEECO_CHECK_ARG(HW >= 4 && HW % 4 == 0, "predict_push_ring: HW=%lld must be a multiple of 4 (4-byte aligned ring frames)",
                  (long long)HW);
  GEECO_CHECK_ARG(J >= 1, "predict_push_ring: J=%d", J);
  GEECO_CHECK_ARG(((reinterpret_cast<uintptr_t>(frames) | reinterpret_cast<uintptr_t>(ring)) & 3) == 0,
                  "predict_push_ring: frames and ring must be 4-byte aligned");
  const long long FB = HW * 3;
  const bool v16 = FB % 16 == 0 && ((reinterpret_cast<uintptr_t>(frames) | reinterpret_cast<uintptr_t>(ring)) & 15) == 0;
  hipStream_t s = (hipStream_t)stream;
  if (v16) {
    typedef unsigned __attribute__((ext_vector_type(4))) u32x4;
    dim3 grid((unsigned)(cdiv64(FB / 16, 256) + 1), (unsigned)B);
    geeco_note_kernel("push_ring_kernel<u32x4>");
    hipLaunchKernelGGL(push_ring_kernel<u32x4>, grid, dim3(256), 0, s, frames, jnt, reset, any_bad, heads, K, FB, J, ring,
                       jnt_state);
  } else {
    dim3 grid((unsigned)(cdiv64(FB / 4, 256) + 1), (unsigned)B);
    geeco_note_kernel("push_ring_kernel<unsigned>");
    hipLaunchKernelGGL(push_ring_kernel<unsigned>, grid, dim3(256), 0, s, frames, jnt, reset, any_bad, heads, K, FB, J, ring,
                       jnt_state);
  }
  GEECO_LAUNCH_CHECK();
  geeco_note_kernel("ring_advance_kernel");
  hipLaunchKernelGGL(ring_advance_kernel, dim3((unsigned)cdiv(B, 64)), dim3(64), 0, s, any_bad, B, K, FB,
                     (const unsigned char*)ring, heads, (long long*)win_table);
  GEECO_LAUNCH_CHECK();
  return 0;
}

// ---- 3b. incremental mode: newest-frame input pack -------------------------------------------------------------------
// The incremental predictor (batched_predictor.py, incremental=True) keeps no frame window: a call encodes only the B new
// frames.  frames [B][HW][C] (float32, or uint8 with C == 3) -> the encoder input x_in [B][HW][4]: RGB gets a zero fourth
// channel, RGB-D keeps depth there (the values geeco_pack_pixels gives for the dense windows' newest slot).
template <int PIX, int C, bool U8>
__global__ __launch_bounds__(256) void pack_newest_kernel(const void* __restrict__ frames, long long HW, float* __restrict__ x_in) {
  const int b = blockIdx.y;
  const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
  if (u >= HW / PIX) return;
  float px[PIX * 3], dp[PIX];
  load_new<PIX, C, U8>(frames, b, HW, u, px, dp);
  f32x4* o = reinterpret_cast<f32x4*>(x_in + ((long long)b * HW + u * PIX) * 4);
#pragma unroll
  for (int p = 0; p < PIX; ++p) o[p] = f32x4{px[p * 3 + 0], px[p * 3 + 1], px[p * 3 + 2], C == 4 ? dp[p] : 0.f};
}

template <int PIX>
static void launch_pack_newest(dim3 grid, hipStream_t s, const void* frames, int u8, int C, long long HW, float* x_in) {
  if (u8) {
    geeco_note_kernel("pack_newest_kernel<%d, 3, true>", PIX);
    hipLaunchKernelGGL((pack_newest_kernel<PIX, 3, true>), grid, dim3(256), 0, s, frames, HW, x_in);
  } else if (C == 3) {
    geeco_note_kernel("pack_newest_kernel<%d, 3, false>", PIX);
    hipLaunchKernelGGL((pack_newest_kernel<PIX, 3, false>), grid, dim3(256), 0, s, frames, HW, x_in);
  } else {
    geeco_note_kernel("pack_newest_kernel<%d, 4, false>", PIX);
    hipLaunchKernelGGL((pack_newest_kernel<PIX, 4, false>), grid, dim3(256), 0, s, frames, HW, x_in);
  }
}

extern "C" int geeco_predict_pack_newest(const void* frames, int frames_u8, int B, int64_t HW, int C, float* x_in, void* stream) {
  GEECO_CHECK_ARG(frames && x_in, "predict_pack_newest: null pointer");
  GEECO_CHECK_ARG(B >= 1, "predict_pack_newest: B=%d must be >= 1", B);
  GEECO_CHECK_ARG(C == 3 || C == 4, "predict_pack_newest: C=%d must be 3 or 4", C);
  GEECO_CHECK_ARG(!frames_u8 || C == 3, "predict_pack_newest: uint8 frames are RGB (C=3), got C=%d", C);
  GEECO_CHECK_ARG(HW >= 1, "predict_pack_newest: HW=%lld", (long long)HW);
  GEECO_CHECK_ARG((reinterpret_cast<uintptr_t>(x_in) & 15) == 0, "predict_pack_newest: x_in must be 16-byte aligned");
  const bool vec = HW % 4 == 0 && (reinterpret_cast<uintptr_t>(frames) & 15) == 0;
  const int pix = vec ? 4 : 1;
  dim3 grid((unsigned)cdiv64(HW / pix, 256), (unsigned)B);
  hipStream_t s = (hipStream_t)stream;
  if (vec) launch_pack_newest<4>(grid, s, frames, frames_u8, C, (long long)HW, x_in);
  else launch_pack_newest<1>(grid, s, frames, frames_u8, C, (long long)HW, x_in);
  GEECO_LAUNCH_CHECK();
  return 0;
}

// ---- 3c. incremental mode: feature push + state gather ------------------------------------------------------------------
// Per env a ring of the last K encoder feature vectors, feat_ring [B][K][cells][ch], and joint states, jnt_ring [B][K][J];
// heads[b] = the slot the next frame's features go to.  One block per env: it writes the new feature / joint state into slot
// p = heads[b] (into every slot where reset[b]: first-frame padding), writes the decoder's states[t][b] for t = 0..K-1 from
// slots p + 1, .., p + K - 1, p (mod K; oldest first) and moves the head on.  The new values are taken from the inputs, the
// K - 1 older ones from slots this launch does not write, so no thread reads what another one writes; the head is read by
// every thread before the block's barrier and written by one thread after it.  Column layout of a cell: state_layout.h.
// V = floats per load of the feature sources (4: ch % 4 == 0 and 16-byte aligned bases).  The state rows are stored one float
// per lane: with J = 7 a cell's columns start at odd offsets, a 16-byte store has nowhere aligned to go.
template <int V>
__global__ __launch_bounds__(GEECO_PREDICT_FEAT_THREADS) void push_features_kernel(
    const float* __restrict__ feat, const float* __restrict__ jnt, const int* __restrict__ reset, const int* __restrict__ any_bad,
    const float* __restrict__ tgt, int mode, int B, int K, int cells, int ch, int J, float* __restrict__ feat_ring,
    float* __restrict__ jnt_ring, int* __restrict__ heads, float* __restrict__ states, long long state_stride) {
  if (*any_bad) return;      // a frame failed the range check: no ring, no head moves
  const int b = blockIdx.x;
  const int rs = reset[b];
  int p = heads[b];
  if ((unsigned)p >= (unsigned)K) p = 0;     // heads come zero-filled and only this kernel moves them; never index past a ring
  const int FE = cells * ch;                 // floats of one feature vector
  const StateLayout<int> L = state_layout(mode, ch, J);
  const float* fnew = feat + (long long)b * FE;
  const float* tg = mode == GEECO_PREDICT_FEAT_PLAIN ? nullptr : tgt + (long long)b * FE;
  float* fr = feat_ring + (long long)b * K * FE;
  float* jr = jnt_ring + (long long)b * K * J;
  const int nq = FE / V;                     // feature units of V floats (ch % V == 0: a unit stays inside one cell)
  // 1. ring write: slot p, or all K slots after a reset
  const int s0 = rs ? 0 : p, ns = rs ? K : 1;
  for (int i = threadIdx.x; i < ns * nq; i += blockDim.x) {
    const int s = i / nq, q = i - s * nq;
    float v[V];
    ld_vec<V>(fnew + q * V, v);
    float* o = fr + (long long)(s0 + s) * FE + q * V;
    if (V == 4) *reinterpret_cast<f32x4*>(o) = f32x4{v[0], v[1], v[2], v[3]};
    else o[0] = v[0];
  }
  for (int i = threadIdx.x; i < ns * J; i += blockDim.x) {
    const int s = i / J, j = i - s * J;
    jr[(s0 + s) * J + j] = jnt[(long long)b * J + j];
  }
  // 2. gather, oldest first; slot p (and every slot after a reset) comes from the inputs
  for (int i = threadIdx.x; i < K * nq; i += blockDim.x) {
    const int t = i / nq, q = i - t * nq;
    int slot = p + 1 + t;
    if (slot >= K) slot -= K;
    const bool fresh = rs || slot == p;
    float v[V];
    ld_vec<V>(fresh ? fnew + q * V : fr + (long long)slot * FE + q * V, v);
    const int cell = (q * V) / ch, c = q * V - cell * ch;
    float* o = states + ((long long)t * B + b) * state_stride + cell * L.Ctot + c;
    if (mode == GEECO_PREDICT_FEAT_PLAIN) {
#pragma unroll
      for (int k = 0; k < V; ++k) o[k] = v[k];
    } else {
      float g[V];
      ld_vec<V>(tg + q * V, g);
      if (mode == GEECO_PREDICT_FEAT_CONSTANT) {
#pragma unroll
        for (int k = 0; k < V; ++k) {
          o[k] = v[k];
          o[L.jnt_off + J + k] = g[k];      // (= L.tgt_off, without its select)
        }
      } else {
#pragma unroll
        for (int k = 0; k < V; ++k) o[k] = g[k] - v[k];
      }
    }
  }
  const int CJ = cells * J;
  for (int i = threadIdx.x; i < K * CJ; i += blockDim.x) {
    const int t = i / CJ, r = i - t * CJ;
    const int cell = r / J, j = r - cell * J;
    int slot = p + 1 + t;
    if (slot >= K) slot -= K;
    const bool fresh = rs || slot == p;
    states[((long long)t * B + b) * state_stride + cell * L.Ctot + L.jnt_off + j] = fresh ? jnt[(long long)b * J + j] : jr[slot * J + j];
  }
  // 3. the head moves on: every thread of the block has read it before this barrier
  __syncthreads();
  if (threadIdx.x == 0) heads[b] = p + 1 == K ? 0 : p + 1;
}

extern "C" int geeco_predict_push_features(const float* feat, const float* jnt, const int* reset, const int* any_bad,
                                           const float* tgt_feat, int mode, int B, int K, int cells, int ch, int J,
                                           float* feat_ring, float* jnt_ring, int* heads, float* states, int64_t state_stride,
                                           void* stream) {
  GEECO_CHECK_ARG(feat && jnt && reset && any_bad && feat_ring && jnt_ring && heads && states,
                  "predict_push_features: null pointer");
  if (int rc = check_state_layout("predict_push_features", mode, cells, ch, J, state_stride)) return rc;
  GEECO_CHECK_ARG(mode == GEECO_PREDICT_FEAT_PLAIN || tgt_feat, "predict_push_features: null pointer (tgt_feat, mode %d)", mode);
  GEECO_CHECK_ARG(B >= 1, "predict_push_features: B=%d must be >= 1", B);
  GEECO_CHECK_ARG(K >= 1 && K <= PIO_MAXK, "predict_push_features: K=%d outside 1..%d", K, PIO_MAXK);
  const uintptr_t al = reinterpret_cast<uintptr_t>(feat) | reinterpret_cast<uintptr_t>(tgt_feat) |
                       reinterpret_cast<uintptr_t>(feat_ring);
  const bool vec = ch % 4 == 0 && (al & 15) == 0;
  hipStream_t s = (hipStream_t)stream;
  if (vec) {
    geeco_note_kernel("push_features_kernel<4>");
    hipLaunchKernelGGL(push_features_kernel<4>, dim3((unsigned)B), dim3(GEECO_PREDICT_FEAT_THREADS), 0, s, feat, jnt, reset,
                       any_bad, tgt_feat, mode, B, K, cells, ch, J, feat_ring, jnt_ring, heads, states, (long long)state_stride);
  } else {
    geeco_note_kernel("push_features_kernel<1>");
    hipLaunchKernelGGL(push_features_kernel<1>, dim3((unsigned)B), dim3(GEECO_PREDICT_FEAT_THREADS), 0, s, feat, jnt, reset,
                       any_bad, tgt_feat, mode, B, K, cells, ch, J, feat_ring, jnt_ring, heads, states, (long long)state_stride);
  }
  GEECO_LAUNCH_CHECK();
  return 0;
}

// ---- 4. output pack ---------------------------------------------------------------------------------------------------
// preds [B][P] (the decoder's heads side by side) -> out [B][F] in the order the API returns: each segment is a copy of
// `len` columns from `src`, or (argmax) ONE column = argmax over `len` logits - 1 (np.argmax: the first maximum; a NaN wins as
// the first maximum does there).  The control words go to ctl_out and are zeroed for the next call.  img0 / img1 (optional):
// [B][HW][4] channel-padded images -> img_out [nimg][B][HW][C].
struct PackSegs {
  int src[GEECO_PREDICT_PACK_MAXSEG], len[GEECO_PREDICT_PACK_MAXSEG], argmax[GEECO_PREDICT_PACK_MAXSEG];
  int n;
};

__global__ __launch_bounds__(256) void pack_preds_kernel(const float* __restrict__ preds, int P, int B, PackSegs sg, int F,
                                                         float* __restrict__ out, int* __restrict__ ctl, int* __restrict__ ctl_out) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b <= B) {
    ctl_out[b] = ctl[b];
    ctl[b] = 0;
  }
  if (b >= B) return;
  const float* p = preds + (long long)b * P;
  float* o = out + (long long)b * F;
  int col = 0;
  for (int s = 0; s < sg.n; ++s) {
    const float* q = p + sg.src[s];
    if (sg.argmax[s]) {
      int best = 0;
      float bv = q[0];
      for (int i = 1; i < sg.len[s] && bv == bv; ++i) {
        const float v = q[i];
        if (v > bv || v != v) {
          bv = v;
          best = i;
        }
      }
      o[col++] = (float)(best - 1);
    } else {
      for (int i = 0; i < sg.len[s]; ++i) o[col++] = q[i];
    }
  }
}

__global__ __launch_bounds__(256) void pack_image_kernel(const float* __restrict__ img, long long HW, int C, float* __restrict__ out) {
  const int b = blockIdx.y;
  const long long px = (long long)blockIdx.x * 256 + threadIdx.x;
  if (px >= HW) return;
  const f32x4 v = reinterpret_cast<const f32x4*>(img + (long long)b * HW * 4)[px];
  float* o = out + ((long long)b * HW + px) * C;
  if (C == 4) {
    *reinterpret_cast<f32x4*>(o) = v;
  } else {
    o[0] = v.x;
    o[1] = v.y;
    o[2] = v.z;
  }
}

extern "C" int geeco_predict_pack(const float* preds, int P, int B, int nseg, const int* seg_src, const int* seg_len,
                                  const int* seg_argmax, float* out, int F, int* ctl, int* ctl_out, const float* img0,
                                  const float* img1, int64_t HW, int C, float* img_out, void* stream) {
  GEECO_CHECK_ARG(preds && out && ctl && ctl_out && seg_src && seg_len && seg_argmax, "predict_pack: null pointer");
  GEECO_CHECK_ARG(B >= 1, "predict_pack: B=%d must be >= 1", B);
  GEECO_CHECK_ARG(nseg >= 1 && nseg <= GEECO_PREDICT_PACK_MAXSEG, "predict_pack: nseg=%d outside 1..%d", nseg,
                  GEECO_PREDICT_PACK_MAXSEG);
  PackSegs sg;
  sg.n = nseg;
  int f = 0;
  for (int s = 0; s < nseg; ++s) {
    GEECO_CHECK_ARG(seg_len[s] >= 1 && seg_src[s] >= 0 && seg_src[s] + seg_len[s] <= P,
                    "predict_pack: segment %d [%d, +%d) outside the %d prediction columns", s, seg_src[s], seg_len[s], P);
    sg.src[s] = seg_src[s];
    sg.len[s] = seg_len[s];
    sg.argmax[s] = seg_argmax[s] != 0;
    f += sg.argmax[s] ? 1 : seg_len[s];
  }
  GEECO_CHECK_ARG(f == F, "predict_pack: the segments give %d output columns, F=%d", f, F);
  if (img0 || img1) {
    GEECO_CHECK_ARG(img_out, "predict_pack: null pointer (img_out)");
    GEECO_CHECK_ARG(C == 3 || C == 4, "predict_pack: C=%d must be 3 or 4", C);
    GEECO_CHECK_ARG(HW >= 1, "predict_pack: HW=%lld", (long long)HW);
    GEECO_CHECK_ARG(((reinterpret_cast<uintptr_t>(img0) | reinterpret_cast<uintptr_t>(img1) |
                      reinterpret_cast<uintptr_t>(img_out)) & 15) == 0, "predict_pack: images must be 16-byte aligned");
  }
  hipStream_t s = (hipStream_t)stream;
  geeco_note_kernel("pack_preds_kernel");
  hipLaunchKernelGGL(pack_preds_kernel, dim3((unsigned)cdiv(B + 1, 256)), dim3(256), 0, s, preds, P, B, sg, F, out, ctl,
                     ctl_out);
  GEECO_LAUNCH_CHECK();
  const float* src[2] = {img0, img1};
  int k = 0;
  for (int i = 0; i < 2; ++i) {
    if (!src[i]) continue;
    geeco_note_kernel("pack_image_kernel");
    hipLaunchKernelGGL(pack_image_kernel, dim3((unsigned)cdiv64(HW, 256), (unsigned)B), dim3(256), 0, s, src[i],
                       (long long)HW, C, img_out + (long long)k * B * HW * C);
    GEECO_LAUNCH_CHECK();
    ++k;
  }
  return 0;
}
