// Opt-in gradient accumulation over micro-batches: the pieces of a micro-batch's gradient are stored into (the first
// micro-batch of a group) or added to (every later one) the accumulator arena, which the optimiser step of the group's last
// micro-batch then reads in the gradient arena's place.  One streaming launch where Adam's pieces go in the step without the option.
#include "geeco_common.h"
#include "adam_grid.h"

// The table of pieces, as AdamPieces of csrc/adam.hip: by value, indexed statically.
struct AccumPieces {
  const float* g[GEECO_ADAM_SEGMENTS_MAX];
  long long p0[GEECO_ADAM_SEGMENTS_MAX];        // first element of the piece in the accumulator (a multiple of 4)
  long long cnt[GEECO_ADAM_SEGMENTS_MAX];       // its element count: cnt >> 2 float4s and a tail of cnt & 3
  int n;
};

// HBM-streaming: 16-byte loads of g (and of acc unless OVERWRITE), one float32 addition per element, 16-byte stores, no LDS.  The
// addition has no multiplication beside it to contract with, so float4 body and scalar tail round alike and any partition of a range
// gives bitwise the one-piece result, numpy's float32 acc + g.  OVERWRITE: acc is not read at all -- whatever it held (the NaNs of a
// group whose step was skipped) is gone, with no zeroing pass.
template <bool OVERWRITE>
__global__ __launch_bounds__(256) void grad_accumulate_kernel(float* __restrict__ acc, const AccumPieces s) {
  // every block walks piece after piece with the whole grid's stride (adam_update_kernel's walk)
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  // the piece loop is unrolled: static indices into the by-value argument (a dynamic index would copy it to scratch)
#pragma unroll
  for (int k = 0; k < GEECO_ADAM_SEGMENTS_MAX; ++k) {
    if (k >= s.n) break;
    const long long e0 = s.p0[k] >> 2, cnt = s.cnt[k], cnt4 = cnt >> 2;
    const float* __restrict__ gs = s.g[k];
    for (long long i = i0; i < cnt4; i += stride) {
      f32x4 gv = reinterpret_cast<const f32x4*>(gs)[i];
      if (!OVERWRITE) {
        const f32x4 av = reinterpret_cast<const f32x4*>(acc)[e0 + i];
        gv = f32x4{av.x + gv.x, av.y + gv.y, av.z + gv.z, av.w + gv.w};
      }
      reinterpret_cast<f32x4*>(acc)[e0 + i] = gv;
    }
    if (blockIdx.x == 0 && threadIdx.x < (cnt & 3)) {      // the piece's tail
      const long long r = (cnt4 << 2) + threadIdx.x, i = s.p0[k] + r;
      acc[i] = OVERWRITE ? gs[r] : acc[i] + gs[r];
    }
  }
}

extern "C" int geeco_grad_accumulate_segments(float* acc, const geeco_adam_segment* segs, int nseg, int64_t n, int overwrite, void* stream) {
  GEECO_CHECK_ARG(acc && segs && n >= 1 && nseg >= 1 && nseg <= GEECO_ADAM_SEGMENTS_MAX, "grad_accumulate_segments: bad arguments (1..%d pieces)",
                  GEECO_ADAM_SEGMENTS_MAX);
  GEECO_CHECK_ARG(((uintptr_t)acc & 15) == 0, "grad_accumulate_segments: the accumulator must be 16-byte aligned");
  AccumPieces s = {};
  s.n = nseg;
  long long longest4 = 1;
  for (int k = 0; k < nseg; ++k) {
    GEECO_CHECK_ARG(segs[k].g && ((uintptr_t)segs[k].g & 15) == 0 && segs[k].p_off >= 0 && segs[k].p_off % 4 == 0 && segs[k].count >= 1,
                    "grad_accumulate_segments: piece %d: the offset must be a multiple of 4 floats, the count >= 1, the gradient source 16-byte aligned", k);
    GEECO_CHECK_ARG(segs[k].p_off < n && segs[k].count <= n - segs[k].p_off,
                    "grad_accumulate_segments: piece %d: [offset, offset + count) lies outside the accumulator of %lld floats", k, (long long)n);
    s.g[k] = segs[k].g;
    s.p0[k] = segs[k].p_off;
    s.cnt[k] = segs[k].count;
    longest4 = (segs[k].count >> 2) > longest4 ? (segs[k].count >> 2) : longest4;
  }
  // no source may lie in a stretch of the accumulator this launch writes (its own piece's, or another's: the walk orders nothing)
  for (int k = 0; k < nseg; ++k) {
    const uintptr_t g_lo = (uintptr_t)segs[k].g, g_hi = g_lo + 4 * (uintptr_t)segs[k].count;
    for (int q = 0; q < nseg; ++q) {
      const uintptr_t a_lo = (uintptr_t)(acc + segs[q].p_off), a_hi = a_lo + 4 * (uintptr_t)segs[q].count;
      GEECO_CHECK_ARG(g_hi <= a_lo || a_hi <= g_lo, "grad_accumulate_segments: the source of piece %d overlaps the accumulator's range of piece %d", k, q);
    }
  }
  const dim3 grid((unsigned)adam_grid(longest4));
  if (overwrite)
    hipLaunchKernelGGL(grad_accumulate_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, acc, s);
  else
    hipLaunchKernelGGL(grad_accumulate_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, acc, s);
  GEECO_LAUNCH_CHECK();
  return 0;
}
