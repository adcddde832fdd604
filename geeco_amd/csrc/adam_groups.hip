// Opt-in fine-tuning: the Adam update over pieces of the arena, each piece with its own learning-rate multiplier.  A
// frozen variable is not a multiplier of 0 but a piece the caller leaves out: what no piece covers is neither read nor written.
#include "clip_internal.h"      // adam_clip_element / adam_clip_tail_element: the one copy of the update's arithmetic on a scaled gradient

struct AdamScaledSegs {
  const float* g[GEECO_ADAM_SEGMENTS_MAX];
  long long p0[GEECO_ADAM_SEGMENTS_MAX];        // first element of the piece in the arena (a multiple of 4)
  long long cnt[GEECO_ADAM_SEGMENTS_MAX];       // its element count: cnt >> 2 float4s and a tail of cnt & 3
  float mul[GEECO_ADAM_SEGMENTS_MAX];           // its learning-rate multiplier (finite, > 0)
  int n;
};

// adam_segments_clip_kernel (csrc/clip_internal.h) with two differences.  Piece k runs lr_t * mul[k], one float32 product per piece
// formed from scal[0] as the prepare work left it (a schedule or a replayed graph is followed).  clip_dev and guard may be null: a null
// clip_dev is s = 1.0f, a run-time value, so the multiplication stays and the element rounds as under the clipped kernel with
// clip_dev[0] == 1.0f, which is bitwise the unclipped kernels' element; a null guard is a step that is always applied.  With every
// multiplier 1.0f (lr_t * 1.0f is lr_t) the results are bit for bit those of geeco_adam_tf_segments[_ema|_clip|_guard].
// HBM-streaming: 16-byte loads and stores, no LDS; the walk (every block walks piece after piece with the grid's stride) and the grid
// rule are the other Adam launches'.
template <bool EMA>
__global__ __launch_bounds__(256) void adam_segments_scaled_kernel(float* __restrict__ p, float* __restrict__ g_out, float* __restrict__ m,
                                                                   float* __restrict__ v, float* __restrict__ ema, const AdamScaledSegs s,
                                                                   const float* __restrict__ scal, const long long* __restrict__ step, float decay,
                                                                   const float* __restrict__ clip_dev, const long long* __restrict__ guard, float b1,
                                                                   float b2, float eps, float gscale, float l2) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (guard && guard[0] == 0) {      // a skipped step (geeco_guard_decide): g_out alone is written
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
  const float sc = clip_dev ? clip_dev[0] : 1.0f;
  float d = 0.f;
  if (EMA) {      // d_t = min(decay, (1 + t) / (10 + t)), t = the counter the prepare work has already advanced
    const float t = (float)*step;
    d = fminf(decay, (1.f + t) / (10.f + t));
  }
  // the piece loop is unrolled: static indices into the by-value argument (a dynamic index would copy it to scratch)
#pragma unroll
  for (int k = 0; k < GEECO_ADAM_SEGMENTS_MAX; ++k) {
    if (k >= s.n) break;
    const long long e0 = s.p0[k] >> 2, cnt = s.cnt[k], cnt4 = cnt >> 2;
    const float* __restrict__ gs = s.g[k];
    const float lr_k = lr_t * s.mul[k];
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
        adam_clip_element(pe[c], ge[c], me[c], ve[c], lr_k, sc, b1, b2, eps, gscale, l2);
        if (EMA) se[c] = fmaf(se[c] - pe[c], d, pe[c]);
      }
      reinterpret_cast<f32x4*>(p)[e] = f32x4{pe[0], pe[1], pe[2], pe[3]};
      reinterpret_cast<f32x4*>(m)[e] = f32x4{me[0], me[1], me[2], me[3]};
      reinterpret_cast<f32x4*>(v)[e] = f32x4{ve[0], ve[1], ve[2], ve[3]};
      if (EMA) reinterpret_cast<f32x4*>(ema)[e] = f32x4{se[0], se[1], se[2], se[3]};
    }
    if (blockIdx.x == 0 && threadIdx.x < (cnt & 3)) {      // the piece's tail: the contraction-off form of csrc/clip_internal.h
      const long long r = (cnt4 << 2) + threadIdx.x, i = s.p0[k] + r;
      const float g = gs[r];
      float pp = p[i], mm = m[i], vv = v[i];
      adam_clip_tail_element(pp, g, mm, vv, lr_k, sc, b1, b2, eps, gscale, l2);
      if (g_out) g_out[i] = g;
      m[i] = mm;
      v[i] = vv;
      p[i] = pp;
      if (EMA) ema[i] = fmaf(ema[i] - pp, d, pp);
    }
  }
}

extern "C" int geeco_adam_tf_segments_scaled(float* p, float* g_out, float* m, float* v, float* ema_or_null, const geeco_adam_segment* segs,
                                             const float* lr_mul, int nseg, const float* lr_t_dev, const int64_t* global_step_dev, float decay,
                                             const float* clip_dev_or_null, const int64_t* guard_dev_or_null, float beta1, float beta2, float eps,
                                             float grad_scale, float l2, void* stream) {
  const char* who = "adam_tf_segments_scaled";
  GEECO_CHECK_ARG(p && m && v && lr_t_dev && segs && lr_mul && nseg >= 1 && nseg <= GEECO_ADAM_SEGMENTS_MAX, "%s: bad arguments (1..%d pieces)", who,
                  GEECO_ADAM_SEGMENTS_MAX);
  GEECO_CHECK_ARG((((uintptr_t)p | (uintptr_t)g_out | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema_or_null) & 15) == 0,
                  "%s: arenas must be 16-byte aligned", who);
  if (ema_or_null) {
    GEECO_CHECK_ARG(global_step_dev, "%s: a shadow arena needs the step counter, got a null pointer", who);
    GEECO_CHECK_ARG(decay > 0.f && decay < 1.f, "%s: decay %g is outside (0, 1)", who, (double)decay);
  }
  AdamScaledSegs s = {};
  s.n = nseg;
  long long longest4 = 1;
  for (int k = 0; k < nseg; ++k) {
    GEECO_CHECK_ARG(segs[k].g && ((uintptr_t)segs[k].g & 15) == 0 && segs[k].p_off >= 0 && segs[k].p_off % 4 == 0 && segs[k].count >= 1,
                    "%s: piece %d: the offset must be a multiple of 4 floats, the gradient source 16-byte aligned", who, k);
    // (a NaN fails the first comparison, an infinity the second)
    GEECO_CHECK_ARG(lr_mul[k] > 0.f && lr_mul[k] <= 3.402823466e38f,
                    "%s: piece %d: the learning-rate multiplier %g is not a finite number > 0 (a frozen piece is one that is left out)", who, k,
                    (double)lr_mul[k]);
    s.g[k] = segs[k].g;
    s.p0[k] = segs[k].p_off;
    s.cnt[k] = segs[k].count;
    s.mul[k] = lr_mul[k];
    longest4 = (segs[k].count >> 2) > longest4 ? (segs[k].count >> 2) : longest4;
  }
  long long blocks = cdiv64(longest4, 256);      // the grid rule of the Adam launches of csrc/misc.hip (adam_grid)
  if (blocks > 2048) blocks = 2048;
  if (ema_or_null)
    hipLaunchKernelGGL((adam_segments_scaled_kernel<true>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g_out, m, v, ema_or_null,
                       s, lr_t_dev, (const long long*)global_step_dev, decay, clip_dev_or_null, (const long long*)guard_dev_or_null, beta1, beta2,
                       eps, grad_scale, l2);
  else
    hipLaunchKernelGGL((adam_segments_scaled_kernel<false>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g_out, m, v, ema_or_null,
                       s, lr_t_dev, (const long long*)global_step_dev, decay, clip_dev_or_null, (const long long*)guard_dev_or_null, beta1, beta2,
                       eps, grad_scale, l2);
  GEECO_LAUNCH_CHECK();
  return 0;
}
