// The Adam update (tf.train.AdamOptimizer semantics): ONE kernel template and one launcher behind the
// five entry points that take pieces of the arena, and the two whole-arena kernels.  The step counter and lr_t = scal[0] are the prepare work's (csrc/misc.hip: geeco_adam_prepare, or the last
// slab-sum launch of the backward).
#include "geeco_common.h"
#include "adam_grid.h"

// ---- one element -----------------------------------------------------------------------------------
// The total gradient G = g * gscale + l2 * p, under CLIP times s = clip_dev[0] once it has been formed.  The multiplication feeds only
// other multiplications, so the contraction of the lines around it is the one they get without it, and s == 1.0f leaves bitwise the
// unclipped p, m, v (tests/test_clip_gpu.py pins it).  Without CLIP the line is absent, not a multiplication by 1.
template <bool CLIP>
__device__ __forceinline__ void adam_element(float& p, float g, float& m, float& v, float lr_t, float s, float b1, float b2, float eps,
                                             float gscale, float l2) {
  float gg = g * gscale + l2 * p;
  if (CLIP) gg = gg * s;
  m = b1 * m + (1.f - b1) * gg;
  v = b2 * v + (1.f - b2) * gg * gg;
  p = p - lr_t * m / (sqrtf(v) + eps);
}

// The scalar tail of a piece (count & 3 elements).  Left to the compiler, a tail of the lines above comes out with the total gradient
// fused as in the float4 loop but m and v as separately rounded products and sums (the two updates are packed into one two-wide
// multiply and one two-wide add, which leaves nothing to contract), so the last n & 3 elements would be rounded unlike the rest and
// unlike from one instantiation to the next.  The tail says what that form computes with contraction switched off: every instantiation
// rounds its tail alike, and as the whole-arena kernels below do.  (The arenas of a model are whole float4s: no model ever runs a tail.)
template <bool CLIP>
__device__ __forceinline__ void adam_tail_element(float& p, float g, float& m, float& v, float lr_t, float s, float b1, float b2, float eps,
                                                  float gscale, float l2) {
#pragma clang fp contract(off)
  float gg = fmaf(g, gscale, l2 * p);
  if (CLIP) gg = gg * s;
  m = b1 * m + (1.f - b1) * gg;
  v = b2 * v + (1.f - b2) * gg * gg;
  p = p - lr_t * m / (sqrtf(v) + eps);
}

// Exponential moving average of the parameters (tf.train.ExponentialMovingAverage, zero_debias=False, num_updates=global_step),
// kept by the same pass: d_t = min(decay, (1 + t) / (10 + t)), t = the step counter the prepare work has already advanced (stream
// order).  Uniform over the launch and a handful of instructions, so every thread computes it.
__device__ __forceinline__ float ema_decay_now(const long long* __restrict__ step, float decay) {
  const float t = (float)*step;
  return fminf(decay, (1.f + t) / (10.f + t));
}

// s' = s - (s - p') (1 - d_t), p' = the parameter this step has just computed (still in registers), evaluated as p' + (s - p') d_t
// in one subtraction and one FMA: the same value with two roundings instead of four (1 - d_t is not formed, so not rounded), at
// most 0.5 ulp(s - p') d_t + 0.5 ulp(s') < 1.5 ulp of max(|s|, |p'|) from the exact result whatever the signs of s and p'.
__device__ __forceinline__ float ema_element(float s, float p, float d) { return fmaf(s - p, d, p); }

// ---- the pieces ------------------------------------------------------------------------------------
// Up to GEECO_ADAM_SEGMENTS_MAX pieces of the arena, each with its own gradient source (data parallel: the 99 % of the variables whose
// gradients arrived with the early bucket are updated while the late bucket is still on the wire; conv1 / conv2 of the encoders follow,
// their gradients read straight from the late bucket's staging buffer).  Element by element the arithmetic is the same whatever the
// pieces: any partition of the arena gives bitwise the one-pass result, which is itself the one-piece call.
struct AdamPieces {
  const float* g[GEECO_ADAM_SEGMENTS_MAX];
  long long p0[GEECO_ADAM_SEGMENTS_MAX];        // first element of the piece in the arena (a multiple of 4)
  long long cnt[GEECO_ADAM_SEGMENTS_MAX];       // its element count: cnt >> 2 float4s and a tail of cnt & 3
  float mul[GEECO_ADAM_SEGMENTS_MAX];           // its learning-rate multiplier (finite, > 0; read under MUL alone)
  int n;
};

// A skipped step: the pieces' gradients are copied to g_out and nothing else is read or written.
__device__ __forceinline__ void adam_copy_gradients(float* __restrict__ g_out, const AdamPieces& s, long long i0, long long stride) {
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
}

// ---- the kernel ------------------------------------------------------------------------------------
// HBM-streaming: 16-byte loads and stores of p, g, m, v (and the shadow arena), four element updates, no LDS.  What a flag does not
// ask for is absent from the instantiation:
//   EMA    the shadow arena ``ema`` (indexed like p) follows the new parameters while they are in registers;
//   CLIP   the total gradient is multiplied by clip_dev[0] (geeco_clip_scale / geeco_guard_decide);
//   GUARD  guard[0] == 0 (the verdict of geeco_guard_decide: the norm of this step's gradient is not finite) makes the step one with no
//          update: the grid writes g_out, where there is one, and neither reads nor writes p, m, v or the shadow arena.  The test is
//          uniform over the grid (one scalar load per wave), and guard[0] != 0 runs the very code below it;
//   MUL    piece k runs lr_t * mul[k], one float32 product per piece formed from scal[0] as the prepare work left it (a schedule or a
//          replayed graph is followed; lr_t * 1.0f is lr_t).  Its one caller passes CLIP and GUARD too and may leave clip_dev and guard
//          null: a null clip_dev is s = 1.0f, a run-time value, so the multiplication stays and rounds as clip_dev[0] == 1.0f does,
//          which is bitwise no multiplication; a null guard is a step that is always applied.
template <bool EMA, bool CLIP, bool GUARD, bool MUL>
__global__ __launch_bounds__(256) void adam_update_kernel(float* __restrict__ p, float* __restrict__ g_out, float* __restrict__ m,
                                                          float* __restrict__ v, float* __restrict__ ema, const AdamPieces s,
                                                          const float* __restrict__ scal, const long long* __restrict__ step, float decay,
                                                          const float* __restrict__ clip_dev, const long long* __restrict__ guard, float b1,
                                                          float b2, float eps, float gscale, float l2) {
  // Every block walks piece after piece with the whole grid's stride (pieces dealt to block groups side by side measured the same:
  // 36.4-36.8 us for the early pieces of the bench model against 33.8 for the undivided pass in the same place of the step).
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (GUARD && (!MUL || guard) && guard[0] == 0) {
    if (g_out) adam_copy_gradients(g_out, s, i0, stride);
    return;
  }
  const float lr_t = scal[0];
  const float sc = CLIP && (!MUL || clip_dev) ? clip_dev[0] : 1.0f;
  const float d = EMA ? ema_decay_now(step, decay) : 0.f;
  // the piece loop is unrolled: static indices into the by-value argument (a dynamic index would copy it to scratch)
#pragma unroll
  for (int k = 0; k < GEECO_ADAM_SEGMENTS_MAX; ++k) {
    if (k >= s.n) break;
    const long long e0 = s.p0[k] >> 2, cnt = s.cnt[k], cnt4 = cnt >> 2;
    const float* __restrict__ gs = s.g[k];
    const float lr_k = MUL ? lr_t * s.mul[k] : lr_t;
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
        adam_element<CLIP>(pe[c], ge[c], me[c], ve[c], lr_k, sc, b1, b2, eps, gscale, l2);
        if (EMA) se[c] = ema_element(se[c], pe[c], d);
      }
      reinterpret_cast<f32x4*>(p)[e] = f32x4{pe[0], pe[1], pe[2], pe[3]};
      reinterpret_cast<f32x4*>(m)[e] = f32x4{me[0], me[1], me[2], me[3]};
      reinterpret_cast<f32x4*>(v)[e] = f32x4{ve[0], ve[1], ve[2], ve[3]};
      if (EMA) reinterpret_cast<f32x4*>(ema)[e] = f32x4{se[0], se[1], se[2], se[3]};
    }
    if (blockIdx.x == 0 && threadIdx.x < (cnt & 3)) {      // the piece's tail
      const long long r = (cnt4 << 2) + threadIdx.x, i = s.p0[k] + r;
      const float g = gs[r];
      float pp = p[i], mm = m[i], vv = v[i];
      adam_tail_element<CLIP>(pp, g, mm, vv, lr_k, sc, b1, b2, eps, gscale, l2);
      if (g_out) g_out[i] = g;
      m[i] = mm;
      v[i] = vv;
      p[i] = pp;
      if (EMA) ema[i] = ema_element(ema[i], pp, d);
    }
  }
}

// ---- the launcher ----------------------------------------------------------------------------------
// (the grid: adam_grid of csrc/adam_grid.h, shared with the accumulate launch of csrc/grad_accum.hip)
// What every entry point checks (``who`` names it in messages), the table of pieces, the grid and the launch.  ``count_multiple``: 4 for
// the entry points that take whole float4s alone, 1 for those whose pieces may end in a tail.  ``lr_mul``: one multiplier per piece
// under MUL, else null.  The template arguments are the entry point's; EMA follows from ``ema_or_null``.
template <bool CLIP, bool GUARD, bool MUL>
static int adam_launch(const char* who, int count_multiple, float* p, float* g_out, float* m, float* v, float* ema_or_null,
                       const geeco_adam_segment* segs, const float* lr_mul, int nseg, const float* lr_t_dev, const int64_t* global_step_dev,
                       float decay, const float* clip_dev, const int64_t* guard_dev, float beta1, float beta2, float eps, float grad_scale,
                       float l2, void* stream) {
  const bool options_given = MUL ? lr_mul != nullptr : (!CLIP || clip_dev) && (!GUARD || guard_dev);      // (MUL: clip_dev, guard_dev may be null)
  GEECO_CHECK_ARG(p && m && v && lr_t_dev && segs && nseg >= 1 && nseg <= GEECO_ADAM_SEGMENTS_MAX && options_given,
                  "%s: bad arguments (1..%d pieces)", who, GEECO_ADAM_SEGMENTS_MAX);
  GEECO_CHECK_ARG((((uintptr_t)p | (uintptr_t)g_out | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema_or_null) & 15) == 0,
                  "%s: arenas must be 16-byte aligned", who);
  if (ema_or_null) {
    GEECO_CHECK_ARG(global_step_dev, "%s: a shadow arena needs the step counter, got a null pointer", who);
    GEECO_CHECK_ARG(decay > 0.f && decay < 1.f, "%s: decay %g is outside (0, 1)", who, (double)decay);
  }
  AdamPieces s = {};
  s.n = nseg;
  long long longest4 = 1;
  for (int k = 0; k < nseg; ++k) {
    GEECO_CHECK_ARG(segs[k].g && ((uintptr_t)segs[k].g & 15) == 0 && segs[k].p_off >= 0 && segs[k].p_off % 4 == 0 && segs[k].count >= count_multiple &&
                        segs[k].count % count_multiple == 0,
                    "%s: piece %d: the offset must be a multiple of 4 floats, the count a multiple of %d, the gradient source 16-byte aligned", who, k,
                    count_multiple);
    s.g[k] = segs[k].g;
    s.p0[k] = segs[k].p_off;
    s.cnt[k] = segs[k].count;
    if (MUL) {      // (a NaN fails the first comparison, an infinity the second)
      GEECO_CHECK_ARG(lr_mul[k] > 0.f && lr_mul[k] <= 3.402823466e38f,
                      "%s: piece %d: the learning-rate multiplier %g is not a finite number > 0 (a frozen piece is one that is left out)", who, k,
                      (double)lr_mul[k]);
      s.mul[k] = lr_mul[k];
    }
    longest4 = (segs[k].count >> 2) > longest4 ? (segs[k].count >> 2) : longest4;
  }
  auto kernel = ema_or_null ? adam_update_kernel<true, CLIP, GUARD, MUL> : adam_update_kernel<false, CLIP, GUARD, MUL>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)adam_grid(longest4)), dim3(256), 0, (hipStream_t)stream, p, g_out, m, v, ema_or_null, s, lr_t_dev,
                     (const long long*)global_step_dev, decay, clip_dev, (const long long*)guard_dev, beta1, beta2, eps, grad_scale, l2);
  GEECO_LAUNCH_CHECK();
  return 0;
}

// ---- the whole arena ---------------------------------------------------------------------------------
// geeco_adam_tf / geeco_adam_tf_ema keep kernels of their own: as the one-piece call of the template they measured 0.5-1.3 us slower
// on the bench model's arena (33.0-33.2 us against 33.6-34.4, profiles/adam_one_kernel/timing_whole_arena_unified.json).  The same
// element function and grid rule; the results are bitwise the one-piece call's (tests/test_clip_gpu.py), the tails included: these
// tails are the ones adam_tail_element is written to reproduce.
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, long long n,
                                                   const float* __restrict__ scal, float b1, float b2, float eps,
                                                   float gscale, float l2) {
  const float lr_t = scal[0];
  const long long n4 = n >> 2;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    f32x4 pv = reinterpret_cast<f32x4*>(p)[i];
    f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
    f32x4 mv = reinterpret_cast<f32x4*>(m)[i];
    f32x4 vv = reinterpret_cast<f32x4*>(v)[i];
    float pe[4] = {pv.x, pv.y, pv.z, pv.w}, ge[4] = {gv.x, gv.y, gv.z, gv.w};
    float me[4] = {mv.x, mv.y, mv.z, mv.w}, ve[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) adam_element<false>(pe[k], ge[k], me[k], ve[k], lr_t, 1.f, b1, b2, eps, gscale, l2);
    reinterpret_cast<f32x4*>(p)[i] = f32x4{pe[0], pe[1], pe[2], pe[3]};
    reinterpret_cast<f32x4*>(m)[i] = f32x4{me[0], me[1], me[2], me[3]};
    reinterpret_cast<f32x4*>(v)[i] = f32x4{ve[0], ve[1], ve[2], ve[3]};
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long long i = (n4 << 2) + threadIdx.x;
    float gg = g[i] * gscale + l2 * p[i];      // (adam_element's expressions, spelled out)
    float mm = b1 * m[i] + (1.f - b1) * gg;
    float vv = b2 * v[i] + (1.f - b2) * gg * gg;
    m[i] = mm;
    v[i] = vv;
    p[i] = p[i] - lr_t * mm / (sqrtf(vv) + eps);
  }
}

// adam_kernel with the shadow arena: the same walk (grid rule, 16-byte accesses, tail), one more arena read and written while the
// new parameters are in registers.  p, m, v come out bit for bit as adam_kernel leaves them.
__global__ __launch_bounds__(256) void adam_ema_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                       float* __restrict__ m, float* __restrict__ v, float* __restrict__ ema,
                                                       long long n, const float* __restrict__ scal,
                                                       const long long* __restrict__ step, float decay, float b1, float b2, float eps,
                                                       float gscale, float l2) {
  const float lr_t = scal[0];
  const float d = ema_decay_now(step, decay);
  const long long n4 = n >> 2;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    f32x4 pv = reinterpret_cast<f32x4*>(p)[i];
    f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
    f32x4 mv = reinterpret_cast<f32x4*>(m)[i];
    f32x4 vv = reinterpret_cast<f32x4*>(v)[i];
    f32x4 sv = reinterpret_cast<f32x4*>(ema)[i];
    float pe[4] = {pv.x, pv.y, pv.z, pv.w}, ge[4] = {gv.x, gv.y, gv.z, gv.w};
    float me[4] = {mv.x, mv.y, mv.z, mv.w}, ve[4] = {vv.x, vv.y, vv.z, vv.w};
    float se[4] = {sv.x, sv.y, sv.z, sv.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      adam_element<false>(pe[k], ge[k], me[k], ve[k], lr_t, 1.f, b1, b2, eps, gscale, l2);
      se[k] = ema_element(se[k], pe[k], d);
    }
    reinterpret_cast<f32x4*>(p)[i] = f32x4{pe[0], pe[1], pe[2], pe[3]};
    reinterpret_cast<f32x4*>(m)[i] = f32x4{me[0], me[1], me[2], me[3]};
    reinterpret_cast<f32x4*>(v)[i] = f32x4{ve[0], ve[1], ve[2], ve[3]};
    reinterpret_cast<f32x4*>(ema)[i] = f32x4{se[0], se[1], se[2], se[3]};
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long long i = (n4 << 2) + threadIdx.x;
    float pp = p[i], mm = m[i], vv = v[i];
    adam_element<false>(pp, g[i], mm, vv, lr_t, 1.f, b1, b2, eps, gscale, l2);
    m[i] = mm;
    v[i] = vv;
    p[i] = pp;
    ema[i] = ema_element(ema[i], pp, d);
  }
}

extern "C" int geeco_adam_tf(float* p, const float* g, float* m, float* v, int64_t n, const float* lr_t_dev,
                             float beta1, float beta2, float eps, float grad_scale, float l2, void* stream) {
  GEECO_CHECK_ARG(p && g && m && v && lr_t_dev && n >= 1, "adam_tf: bad arguments");
  GEECO_CHECK_ARG((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0,
                  "adam_tf: arenas must be 16-byte aligned");
  hipLaunchKernelGGL(adam_kernel, dim3((unsigned)adam_grid(n >> 2)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (long long)n,
                     lr_t_dev, beta1, beta2, eps, grad_scale, l2);
  GEECO_LAUNCH_CHECK();
  return 0;
}

extern "C" int geeco_adam_tf_ema(float* p, const float* g, float* m, float* v, float* ema, int64_t n, const float* lr_t_dev,
                                 const int64_t* global_step_dev, float decay, float beta1, float beta2, float eps, float grad_scale,
                                 float l2, void* stream) {
  GEECO_CHECK_ARG(p && g && m && v && lr_t_dev && n >= 1, "adam_tf_ema: bad arguments");
  GEECO_CHECK_ARG(ema && global_step_dev, "adam_tf_ema: null shadow arena or step counter");
  GEECO_CHECK_ARG(decay > 0.f && decay < 1.f, "adam_tf_ema: decay %g is outside (0, 1)", (double)decay);
  GEECO_CHECK_ARG((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 15) == 0,
                  "adam_tf_ema: arenas must be 16-byte aligned");
  hipLaunchKernelGGL(adam_ema_kernel, dim3((unsigned)adam_grid(n >> 2)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, ema,
                     (long long)n, lr_t_dev, (const long long*)global_step_dev, decay, beta1, beta2, eps, grad_scale, l2);
  GEECO_LAUNCH_CHECK();
  return 0;
}

// ---- the pieces' entry points: their own refusals, then the launcher ----------------------------------
// Offsets and counts are whole float4s.
extern "C" int geeco_adam_tf_segments(float* p, float* g_out, float* m, float* v, const geeco_adam_segment* segs, int nseg,
                                      const float* lr_t_dev, float beta1, float beta2, float eps, float grad_scale, float l2,
                                      void* stream) {
  return adam_launch<false, false, false>("adam_tf_segments", 4, p, g_out, m, v, nullptr, segs, nullptr, nseg, lr_t_dev, nullptr, 0.f, nullptr,
                                          nullptr, beta1, beta2, eps, grad_scale, l2, stream);
}

extern "C" int geeco_adam_tf_segments_ema(float* p, float* g_out, float* m, float* v, float* ema, const geeco_adam_segment* segs,
                                          int nseg, const float* lr_t_dev, const int64_t* global_step_dev, float decay, float beta1,
                                          float beta2, float eps, float grad_scale, float l2, void* stream) {
  GEECO_CHECK_ARG(ema && global_step_dev, "adam_tf_segments_ema: null shadow arena or step counter");
  return adam_launch<false, false, false>("adam_tf_segments_ema", 4, p, g_out, m, v, ema, segs, nullptr, nseg, lr_t_dev, global_step_dev, decay,
                                          nullptr, nullptr, beta1, beta2, eps, grad_scale, l2, stream);
}

// Offsets are multiples of 4 floats, counts any number >= 1, in this one and the two below.
extern "C" int geeco_adam_tf_segments_clip(float* p, float* g_out, float* m, float* v, float* ema_or_null, const geeco_adam_segment* segs, int nseg,
                                           const float* lr_t_dev, const int64_t* global_step_dev, float decay, const float* clip_dev, float beta1,
                                           float beta2, float eps, float grad_scale, float l2, void* stream) {
  return adam_launch<true, false, false>("adam_tf_segments_clip", 1, p, g_out, m, v, ema_or_null, segs, nullptr, nseg, lr_t_dev, global_step_dev,
                                         decay, clip_dev, nullptr, beta1, beta2, eps, grad_scale, l2, stream);
}

extern "C" int geeco_adam_tf_segments_guard(float* p, float* g_out, float* m, float* v, float* ema_or_null, const geeco_adam_segment* segs, int nseg,
                                            const float* lr_t_dev, const int64_t* global_step_dev, float decay, const float* clip_dev,
                                            const int64_t* guard_dev, float beta1, float beta2, float eps, float grad_scale, float l2, void* stream) {
  return adam_launch<true, true, false>("adam_tf_segments_guard", 1, p, g_out, m, v, ema_or_null, segs, nullptr, nseg, lr_t_dev, global_step_dev,
                                        decay, clip_dev, guard_dev, beta1, beta2, eps, grad_scale, l2, stream);
}

// Opt-in fine-tuning: each piece with its own learning-rate multiplier.  A frozen variable is not a multiplier of 0 but a piece the
// caller leaves out: what no piece covers is neither read nor written.  clip_dev and guard may be null (the kernel's MUL).
extern "C" int geeco_adam_tf_segments_scaled(float* p, float* g_out, float* m, float* v, float* ema_or_null, const geeco_adam_segment* segs,
                                             const float* lr_mul, int nseg, const float* lr_t_dev, const int64_t* global_step_dev, float decay,
                                             const float* clip_dev_or_null, const int64_t* guard_dev_or_null, float beta1, float beta2, float eps,
                                             float grad_scale, float l2, void* stream) {
  return adam_launch<true, true, true>("adam_tf_segments_scaled", 1, p, g_out, m, v, ema_or_null, segs, lr_mul, nseg, lr_t_dev, global_step_dev,
                                       decay, clip_dev_or_null, guard_dev_or_null, beta1, beta2, eps, grad_scale, l2, stream);
}
