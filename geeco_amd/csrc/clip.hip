// Opt-in global-norm gradient clipping (tf.clip_by_global_norm in front of Adam), kept on the device: the sum of squares
// of the total gradient in fixed chunks of the arena and the scale from it.  The Adam update that consumes the scaled gradient:
// geeco_adam_tf_segments_clip, csrc/adam.hip.
#include "clip_internal.h"      // the norm from the partials, shared with csrc/guard.hip

// The total gradient of element i is the one the Adam kernel forms: G_i = g_i * grad_scale + l2 * p_i (csrc/adam.hip: adam_element).
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
// One block: the partials are added in the one order of clip_norm_of_partials (csrc/clip_internal.h).  s is exactly 1.0f whenever
// norm <= clip (clip / clip).  A non-finite norm is not guarded: norm - norm is then NaN and so is s, hence every update, as
// tf.clip_by_global_norm leaves it (for a finite norm the term is +0 and changes nothing).  The opt-in that does guard it:
// geeco_guard_decide, csrc/guard.hip.
__global__ __launch_bounds__(256) void clip_scale_kernel(const float* __restrict__ partials, long long nchunks, float clip, float* __restrict__ out2) {
  __shared__ float sw[4];
  const float norm = clip_norm_of_partials(partials, nchunks, sw);
  if (threadIdx.x == 0) {
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
