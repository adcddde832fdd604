// What csrc/clip.hip and csrc/guard.hip share, one copy of each: the norm from the partial sums of squares, and
// the Adam update on the scaled total gradient (geeco_adam_tf_segments_clip / geeco_adam_tf_segments_guard) -- its element functions,
// the kernel and its launch.  GUARD = false is the kernel of 5.16 as it was; GUARD = true puts one uniform test in front of it.
#pragma once
#include "geeco_common.h"

// ---- the norm: sqrt of the sum of the partials, one fixed order --------------------------------------
// For a 256-thread block: thread t adds the partials t, t + 256, ... in ascending order, then the wave butterfly (6 levels) and the four
// wave sums left to right.  ``sw``: 4 floats of LDS.  The value is returned to thread 0 alone.
__device__ __forceinline__ float clip_norm_of_partials(const float* __restrict__ partials, long long nchunks, float* sw) {
  float acc = 0.f;
  for (long long i = threadIdx.x; i < nchunks; i += 256) acc += partials[i];
  acc = wave_reduce_sum(acc);
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = acc;
  __syncthreads();
  return threadIdx.x == 0 ? sqrtf(((sw[0] + sw[1]) + sw[2]) + sw[3]) : 0.f;
}

// ---- Adam on the clipped gradient ------------------------------------------------------------------
// adam_element / ema_decay_now / ema_element of csrc/misc.hip restated (that file's kernels are not touched), with the one change:
// the total gradient is multiplied by s = clip_dev[0] once it has been formed.  The multiplication feeds only other multiplications,
// so the contraction of the lines around it is the one adam_element gets, and s == 1.0f leaves bitwise the unclipped kernels' p, m, v
// and shadow arena (tests/test_clip_gpu.py pins it).
__device__ __forceinline__ void adam_clip_element(float& p, float g, float& m, float& v, float lr_t, float s, float b1, float b2, float eps,
                                                  float gscale, float l2) {
  float gg = g * gscale + l2 * p;
  gg = gg * s;
  m = b1 * m + (1.f - b1) * gg;
  v = b2 * v + (1.f - b2) * gg * gg;
  p = p - lr_t * m / (sqrtf(v) + eps);
}

// The scalar tail of a piece (count & 3 elements).  The tails of adam_kernel and adam_ema_kernel come out of the compiler with the total
// gradient fused as above but m and v as separately rounded products and sums (the two updates are packed into one two-wide
// multiply and one two-wide add, which leaves nothing to contract), so their last n & 3 elements are rounded unlike the rest.  To be
// bit for bit geeco_adam_tf on an arena of any length this tail says the same with contraction switched off.  (The arenas of a model
// are whole float4s: no model ever runs a tail.)
__device__ __forceinline__ void adam_clip_tail_element(float& p, float g, float& m, float& v, float lr_t, float s, float b1, float b2, float eps,
                                                       float gscale, float l2) {
#pragma clang fp contract(off)
  float gg = fmaf(g, gscale, l2 * p);
  gg = gg * s;
  m = b1 * m + (1.f - b1) * gg;
  v = b2 * v + (1.f - b2) * gg * gg;
  p = p - lr_t * m / (sqrtf(v) + eps);
}

struct AdamClipSegs {
  const float* g[GEECO_ADAM_SEGMENTS_MAX];
  long long p0[GEECO_ADAM_SEGMENTS_MAX];        // first element of the piece in the arena (a multiple of 4)
  long long cnt[GEECO_ADAM_SEGMENTS_MAX];       // its element count: cnt >> 2 float4s and a tail of cnt & 3
  int n;
};

// GUARD: guard[0] == 0 (the verdict of geeco_guard_decide: the norm of this step's gradient is not finite) makes the step one with no
// update: the grid writes g_out, where there is one, and neither reads nor writes p, m, v or the shadow arena.  The test is uniform
// over the grid (one scalar load per wave), and guard[0] != 0 runs the very code below it.
template <bool EMA, bool GUARD>
__global__ __launch_bounds__(256) void adam_segments_clip_kernel(float* __restrict__ p, float* __restrict__ g_out, float* __restrict__ m,
                                                                 float* __restrict__ v, float* __restrict__ ema, const AdamClipSegs s,
                                                                 const float* __restrict__ scal, const long long* __restrict__ step, float decay,
                                                                 const float* __restrict__ clip_dev, const long long* __restrict__ guard, float b1,
                                                                 float b2, float eps, float gscale, float l2) {
  // every block walks piece after piece with the whole grid's stride, as adam_segments_kernel does
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (GUARD && guard[0] == 0) {
    if (!g_out) return;
#pragma unroll
    for (int k = 0; k < GEECO_ADAM_SEGMENTS_MAX; ++k) {
      if (k >= s.n) break;
      const long long e0 = s.p0[k] >> 2, cnt = s.cnt[k], cnt4 = cnt >> 2;
      const float* __restrict__ gs = s.g[k];
      for (long long i = i0; i < cnt4; i += stride) reinterpret_cast<f32x4*>(g_out)[e0 + i] = reinterpret_cast<const f32x4*>(gs)[i];
      if (blockIdx.x == 0 && threadIdx.x < (cnt & 3)) {
        const long long r = (cnt4 << 2) + threadIdx.x;
        g_out[s.p0[k] + r] = gs[r];
      }
    }
    return;
  }
  const float lr_t = scal[0];
  const float sc = clip_dev[0];
  float d = 0.f;
  if (EMA) {      // d_t = min(decay, (1 + t) / (10 + t)), t = the counter the prepare work has already advanced
    const float t = (float)*step;
    d = fminf(decay, (1.f + t) / (10.f + t));
  }
#pragma unroll
  for (int k = 0; k < GEECO_ADAM_SEGMENTS_MAX; ++k) {
    if (k >= s.n) break;
    const long long e0 = s.p0[k] >> 2, cnt = s.cnt[k], cnt4 = cnt >> 2;
    const float* __restrict__ gs = s.g[k];
    for (long long i = i0; i < cnt4; i += stride) {
      const long long e = e0 + i;
      f32x4 pv = reinterpret_cast<f32x4*>(p)[e];
      f32x4 gv = reinterpret_cast<const f32x4*>(gs)[i];
      f32x4 mv = reinterpret_cast<f32x4*>(m)[e];
      f32x4 vv = reinterpret_cast<f32x4*>(v)[e];
      f32x4 sv = {0.f, 0.f, 0.f, 0.f};
      if (EMA) sv = reinterpret_cast<f32x4*>(ema)[e];
      if (g_out) reinterpret_cast<f32x4*>(g_out)[e] = gv;
      float pe[4] = {pv.x, pv.y, pv.z, pv.w}, ge[4] = {gv.x, gv.y, gv.z, gv.w};
      float me[4] = {mv.x, mv.y, mv.z, mv.w}, ve[4] = {vv.x, vv.y, vv.z, vv.w};
      float se[4] = {sv.x, sv.y, sv.z, sv.w};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        adam_clip_element(pe[c], ge[c], me[c], ve[c], lr_t, sc, b1, b2, eps, gscale, l2);
        if (EMA) se[c] = fmaf(se[c] - pe[c], d, pe[c]);
      }
      reinterpret_cast<f32x4*>(p)[e] = f32x4{pe[0], pe[1], pe[2], pe[3]};
      reinterpret_cast<f32x4*>(m)[e] = f32x4{me[0], me[1], me[2], me[3]};
      reinterpret_cast<f32x4*>(v)[e] = f32x4{ve[0], ve[1], ve[2], ve[3]};
      if (EMA) reinterpret_cast<f32x4*>(ema)[e] = f32x4{se[0], se[1], se[2], se[3]};
    }
    if (blockIdx.x == 0 && threadIdx.x < (cnt & 3)) {      // the piece's tail, as adam_kernel's
      const long long r = (cnt4 << 2) + threadIdx.x, i = s.p0[k] + r;
      const float g = gs[r];
      float pp = p[i], mm = m[i], vv = v[i];
      adam_clip_tail_element(pp, g, mm, vv, lr_t, sc, b1, b2, eps, gscale, l2);
      if (g_out) g_out[i] = g;
      m[i] = mm;
      v[i] = vv;
      p[i] = pp;
      if (EMA) ema[i] = fmaf(ema[i] - pp, d, pp);
    }
  }
}

// The argument checks, the table of pieces, the grid rule and the launch of both entry points; ``who`` names the caller in messages.
template <bool GUARD>
static int adam_segments_clip_launch(const char* who, float* p, float* g_out, float* m, float* v, float* ema_or_null, const geeco_adam_segment* segs,
                                     int nseg, const float* lr_t_dev, const int64_t* global_step_dev, float decay, const float* clip_dev,
                                     const int64_t* guard_dev, float beta1, float beta2, float eps, float grad_scale, float l2, void* stream) {
  GEECO_CHECK_ARG(p && m && v && lr_t_dev && clip_dev && segs && nseg >= 1 && nseg <= GEECO_ADAM_SEGMENTS_MAX && (!GUARD || guard_dev),
                  "%s: bad arguments (1..%d pieces)", who, GEECO_ADAM_SEGMENTS_MAX);
  GEECO_CHECK_ARG((((uintptr_t)p | (uintptr_t)g_out | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema_or_null) & 15) == 0,
                  "%s: arenas must be 16-byte aligned", who);
  if (ema_or_null) {
    GEECO_CHECK_ARG(global_step_dev, "%s: a shadow arena needs the step counter, got a null pointer", who);
    GEECO_CHECK_ARG(decay > 0.f && decay < 1.f, "%s: decay %g is outside (0, 1)", who, (double)decay);
  }
  AdamClipSegs s = {};
  s.n = nseg;
  long long longest4 = 1;
  for (int k = 0; k < nseg; ++k) {
    GEECO_CHECK_ARG(segs[k].g && ((uintptr_t)segs[k].g & 15) == 0 && segs[k].p_off >= 0 && segs[k].p_off % 4 == 0 && segs[k].count >= 1,
                    "%s: piece %d: the offset must be a multiple of 4 floats, the gradient source 16-byte aligned", who, k);
    s.g[k] = segs[k].g;
    s.p0[k] = segs[k].p_off;
    s.cnt[k] = segs[k].count;
    longest4 = (segs[k].count >> 2) > longest4 ? (segs[k].count >> 2) : longest4;
  }
  long long blocks = cdiv64(longest4, 256);      // the grid rule of the Adam launches of csrc/misc.hip (adam_grid)
  if (blocks > 2048) blocks = 2048;
  if (ema_or_null)
    hipLaunchKernelGGL((adam_segments_clip_kernel<true, GUARD>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g_out, m, v,
                       ema_or_null, s, lr_t_dev, (const long long*)global_step_dev, decay, clip_dev, (const long long*)guard_dev, beta1, beta2, eps,
                       grad_scale, l2);
  else
    hipLaunchKernelGGL((adam_segments_clip_kernel<false, GUARD>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g_out, m, v,
                       ema_or_null, s, lr_t_dev, (const long long*)global_step_dev, decay, clip_dev, (const long long*)guard_dev, beta1, beta2, eps,
                       grad_scale, l2);
  GEECO_LAUNCH_CHECK();
  return 0;
}
