// Opt-in global-norm gradient clipping (tf.clip_by_global_norm in front of Adam), kept on the device: the sum of squares
// of the total gradient in fixed chunks of the arena, the scale from it, and the Adam update that consumes the scaled gradient.
#include "geeco_common.h"

// The total gradient of element i is the one the Adam kernels form: G_i = g_i * grad_scale + l2 * p_i (csrc/misc.hip: adam_element).
// Here it is written with explicit operations, so that every path of the kernel below (16-byte or scalar load, any piece) rounds it
// alike: the product l2 * p rounded, then one FMA.
__device__ __forceinline__ float clip_total_grad(float g, float p, float gscale, float l2) { return fmaf(g, gscale, l2 * p); }

// ---- sum of squares of the total gradient, one partial per fixed chunk of the arena ----------------
// Chunk k is the arena offsets [k * CH, (k + 1) * CH), whatever the pieces are.  Thread t of the chunk's block owns the float4s
// t, t + 256, t + 512, t + 768 of the chunk and adds their 16 squares in ascending offset order (one FMA each); then the wave butterfly
// (6 levels) and the four wave sums left to right.  An element's gradient is looked up in the table of pieces; the VALUE does not
// depend on how it was loaded, so any partition of the same elements into pieces gives bitwise the same partials.
#define GEECO_CLIP_CHUNK 4096
static_assert(GEECO_CLIP_CHUNK % 1024 == 0, "a chunk is a whole number of float4s per thread of a 256-thread block");

struct ClipSegs {
  const float* g[GEECO_ADAM_SEGMENTS_MAX];
  long long off[GEECO_ADAM_SEGMENTS_MAX];       // first element of the piece in the arena (any offset)
  long long cnt[GEECO_ADAM_SEGMENTS_MAX];       // its element count (any count >= 1)
  int n;
};

template <bool L2>
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ p, const ClipSegs s, long long n, float gscale, float l2,
                                                         float* __restrict__ partials) {
  __shared__ float sw[4];
  const long long base = (long long)blockIdx.x * GEECO_CLIP_CHUNK;
  float acc = 0.f;
#pragma unroll 1      // (the piece lookup below is 8 unrolled cases: unrolled four times more it is 34 KB of code for no earlier load)
  for (int j = 0; j < GEECO_CLIP_CHUNK / 1024; ++j) {
    const long long e = base + 4ll * (threadIdx.x + 256 * j);
    if (e >= n) break;
    const int lanes = n - e >= 4 ? 4 : (int)(n - e);      // the arena's tail (n & 3): 1..3 elements
    float ge[4] = {0.f, 0.f, 0.f, 0.f};
    bool have[4] = {false, false, false, false};          // an element no piece covers adds 0
    // the piece loop is unrolled: static indices into the by-value argument (a dynamic index would copy it to scratch)
#pragma unroll
    for (int k = 0; k < GEECO_ADAM_SEGMENTS_MAX; ++k) {
      if (k >= s.n) break;
      const long long r = e - s.off[k], cnt = s.cnt[k];   // element e is element r of piece k
      if (r <= -4 || r >= cnt) continue;                  // the piece holds none of e .. e + 3
      const float* __restrict__ gs = s.g[k];
      if (lanes == 4 && r >= 0 && r + 4 <= cnt && (r & 3) == 0 && ((uintptr_t)gs & 15) == 0) {
        const f32x4 gv = reinterpret_cast<const f32x4*>(gs)[r >> 2];
        ge[0] = gv.x; ge[1] = gv.y; ge[2] = gv.z; ge[3] = gv.w;
        have[0] = have[1] = have[2] = have[3] = true;
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const long long rc = r + c;
          if (c < lanes && rc >= 0 && rc < cnt) {         // tested against the piece's count before the address is formed
            ge[c] = gs[rc];
            have[c] = true;
          }
        }
      }
    }
    float pe[4] = {0.f, 0.f, 0.f, 0.f};
    if (L2) {      // p is read only when l2 != 0
      if (lanes == 4) {
        const f32x4 pv = reinterpret_cast<const f32x4*>(p)[e >> 2];
        pe[0] = pv.x; pe[1] = pv.y; pe[2] = pv.z; pe[3] = pv.w;
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c < lanes) pe[c] = p[e + c];
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float G = have[c] ? (L2 ? clip_total_grad(ge[c], pe[c], gscale, l2) : ge[c] * gscale) : 0.f;
      acc = fmaf(G, G, acc);
    }
  }
  acc = wave_reduce_sum(acc);
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ((sw[0] + sw[1]) + sw[2]) + sw[3];
}

extern "C" int64_t geeco_clip_ws_floats(int64_t n) { return n >= 1 ? cdiv64(n, GEECO_CLIP_CHUNK) : 0; }

extern "C" int geeco_grad_sumsq_segments(const float* p, const geeco_adam_segment* segs, int nseg, int64_t n, float grad_scale, float l2,
                                         float* partials, void* stream) {
  GEECO_CHECK_ARG(partials && segs && n >= 1 && nseg >= 1 && nseg <= GEECO_ADAM_SEGMENTS_MAX, "grad_sumsq_segments: bad arguments (1..%d pieces)",
                  GEECO_ADAM_SEGMENTS_MAX);
  GEECO_CHECK_ARG(l2 == 0.f || (p && ((uintptr_t)p & 15) == 0), "grad_sumsq_segments: l2 != 0 needs the parameter arena, 16-byte aligned");
  ClipSegs s = {};
  s.n = nseg;
  for (int k = 0; k < nseg; ++k) {
    GEECO_CHECK_ARG(segs[k].g && ((uintptr_t)segs[k].g & 3) == 0 && segs[k].p_off >= 0 && segs[k].count >= 1 && segs[k].count <= n - segs[k].p_off,
                    "grad_sumsq_segments: piece %d: null or misaligned gradients, or [offset, offset + count) outside the arena of %lld floats", k,
                    (long long)n);
    for (int q = 0; q < k; ++q)
      GEECO_CHECK_ARG(segs[k].p_off >= segs[q].p_off + segs[q].count || segs[q].p_off >= segs[k].p_off + segs[k].count,
                      "grad_sumsq_segments: pieces %d and %d overlap", q, k);
    s.g[k] = segs[k].g;
    s.off[k] = segs[k].p_off;
    s.cnt[k] = segs[k].count;
  }
  const dim3 grid((unsigned)cdiv64(n, GEECO_CLIP_CHUNK));
  if (l2 != 0.f)
    hipLaunchKernelGGL(grad_sumsq_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, p, s, (long long)n, grad_scale, l2, partials);
  else
    hipLaunchKernelGGL(grad_sumsq_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, p, s, (long long)n, grad_scale, l2, partials);
  GEECO_LAUNCH_CHECK();
  return 0;
}

// ---- the scale: s = clip / max(norm, clip) ---------------------------------------------------------
// One block: thread t adds the partials t, t + 256, ... in ascending order, then the same tree as above.  s is exactly 1.0f whenever
// norm <= clip (clip / clip).  A non-finite norm is not guarded: norm - norm is then NaN and so is s, hence every update, as
// tf.clip_by_global_norm leaves it (for a finite norm the term is +0 and changes nothing).
__global__ __launch_bounds__(256) void clip_scale_kernel(const float* __restrict__ partials, long long nchunks, float clip, float* __restrict__ out2) {
  __shared__ float sw[4];
  float acc = 0.f;
  for (long long i = threadIdx.x; i < nchunks; i += 256) acc += partials[i];
  acc = wave_reduce_sum(acc);
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float norm = sqrtf(((sw[0] + sw[1]) + sw[2]) + sw[3]);
    out2[0] = clip / (norm <= clip ? clip : norm) + (norm - norm);
    out2[1] = norm;
  }
}

extern "C" int geeco_clip_scale(const float* partials, int64_t nchunks, float clip, float* out2, void* stream) {
  GEECO_CHECK_ARG(partials && out2 && nchunks >= 1, "clip_scale: bad arguments");
  GEECO_CHECK_ARG(clip > 0.f && clip <= 3.402823466e38f, "clip_scale: clip %g is not a finite number > 0", (double)clip);
  hipLaunchKernelGGL(clip_scale_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, (long long)nchunks, clip, out2);
  GEECO_LAUNCH_CHECK();
  return 0;
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

template <bool EMA>
__global__ __launch_bounds__(256) void adam_segments_clip_kernel(float* __restrict__ p, float* __restrict__ g_out, float* __restrict__ m,
                                                                 float* __restrict__ v, float* __restrict__ ema, const AdamClipSegs s,
                                                                 const float* __restrict__ scal, const long long* __restrict__ step, float decay,
                                                                 const float* __restrict__ clip_dev, float b1, float b2, float eps, float gscale,
                                                                 float l2) {
  const float lr_t = scal[0];
  const float sc = clip_dev[0];
  float d = 0.f;
  if (EMA) {      // d_t = min(decay, (1 + t) / (10 + t)), t = the counter the prepare work has already advanced
    const float t = (float)*step;
    d = fminf(decay, (1.f + t) / (10.f + t));
  }
  // every block walks piece after piece with the whole grid's stride, as adam_segments_kernel does
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
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

extern "C" int geeco_adam_tf_segments_clip(float* p, float* g_out, float* m, float* v, float* ema_or_null, const geeco_adam_segment* segs, int nseg,
                                           const float* lr_t_dev, const int64_t* global_step_dev, float decay, const float* clip_dev, float beta1,
                                           float beta2, float eps, float grad_scale, float l2, void* stream) {
  GEECO_CHECK_ARG(p && m && v && lr_t_dev && clip_dev && segs && nseg >= 1 && nseg <= GEECO_ADAM_SEGMENTS_MAX,
                  "adam_tf_segments_clip: bad arguments (1..%d pieces)", GEECO_ADAM_SEGMENTS_MAX);
  GEECO_CHECK_ARG((((uintptr_t)p | (uintptr_t)g_out | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema_or_null) & 15) == 0,
                  "adam_tf_segments_clip: arenas must be 16-byte aligned");
  if (ema_or_null) {
    GEECO_CHECK_ARG(global_step_dev, "adam_tf_segments_clip: a shadow arena needs the step counter, got a null pointer");
    GEECO_CHECK_ARG(decay > 0.f && decay < 1.f, "adam_tf_segments_clip: decay %g is outside (0, 1)", (double)decay);
  }
  AdamClipSegs s = {};
  s.n = nseg;
  long long longest4 = 1;
  for (int k = 0; k < nseg; ++k) {
    GEECO_CHECK_ARG(segs[k].g && ((uintptr_t)segs[k].g & 15) == 0 && segs[k].p_off >= 0 && segs[k].p_off % 4 == 0 && segs[k].count >= 1,
                    "adam_tf_segments_clip: piece %d: the offset must be a multiple of 4 floats, the gradient source 16-byte aligned", k);
    s.g[k] = segs[k].g;
    s.p0[k] = segs[k].p_off;
    s.cnt[k] = segs[k].count;
    longest4 = (segs[k].count >> 2) > longest4 ? (segs[k].count >> 2) : longest4;
  }
  long long blocks = cdiv64(longest4, 256);      // the grid rule of the Adam launches of csrc/misc.hip (adam_grid)
  if (blocks > 2048) blocks = 2048;
  if (ema_or_null)
    hipLaunchKernelGGL(adam_segments_clip_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g_out, m, v, ema_or_null, s,
                       lr_t_dev, (const long long*)global_step_dev, decay, clip_dev, beta1, beta2, eps, grad_scale, l2);
  else
    hipLaunchKernelGGL(adam_segments_clip_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g_out, m, v, ema_or_null, s,
                       lr_t_dev, (const long long*)global_step_dev, decay, clip_dev, beta1, beta2, eps, grad_scale, l2);
  GEECO_LAUNCH_CHECK();
  return 0;
}
