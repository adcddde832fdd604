// Opt-in skipping of optimiser steps whose gradient is not finite, kept on the device: the decision from the partial
// sums of squares that geeco_grad_sumsq_segments (csrc/clip.hip) leaves.  The Adam update that honours it: geeco_adam_tf_segments_guard,
// csrc/adam.hip.
#include "clip_internal.h"

// ---- the decision -----------------------------------------------------------------------------------
// One block; norm is clip_scale_kernel's, partial by partial (clip_norm_of_partials).  A NaN or an infinity anywhere in the total
// gradient reaches its chunk's partial and from there the norm; so does a finite gradient whose squares overflow float32.  The step
// is applied iff the norm is finite.  Then out2 is what geeco_clip_scale leaves (clip > 0; its NaN term is +0 for a finite norm) or
// [1, norm] (clip == 0: no clipping), else [0, norm].  guard = {this step's verdict, skipped steps in all, skipped steps in a row}.
__global__ __launch_bounds__(256) void guard_decide_kernel(const float* __restrict__ partials, long long nchunks, float clip, float* __restrict__ out2,
                                                           long long* __restrict__ guard) {
  __shared__ float sw[4];
  const float norm = clip_norm_of_partials(partials, nchunks, sw);
  if (threadIdx.x == 0) {
    const bool finite = norm - norm == 0.f;      // NaN and +-inf give NaN here
    float s = 0.f;
    if (finite) s = clip > 0.f ? clip / (norm <= clip ? clip : norm) : 1.f;
    out2[0] = s;
    out2[1] = norm;
    guard[0] = finite ? 1 : 0;
    if (!finite) guard[1] += 1;
    guard[2] = finite ? 0 : guard[2] + 1;
  }
}

extern "C" int geeco_guard_decide(const float* partials, int64_t nchunks, float clip, float* out2, int64_t* guard, void* stream) {
  GEECO_CHECK_ARG(partials && out2 && guard && nchunks >= 1, "guard_decide: bad arguments");
  GEECO_CHECK_ARG(clip >= 0.f && clip <= 3.402823466e38f, "guard_decide: clip %g is not a finite number >= 0 (0 = no clipping)", (double)clip);
  hipLaunchKernelGGL(guard_decide_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, (long long)nchunks, clip, out2, (long long*)guard);
  GEECO_LAUNCH_CHECK();
  return 0;
}
