// Integrated-gradients and SmoothGrad attributions (geeco_amd/attribution.py): many input gradients along a family
// of perturbed inputs, summed on the device.  What is here are the three streaming stages around the model's own forward,
// backward and input-gradient pass:
//   1. attr_path_point:  dst = b + alpha (x - b) + sigma z   the perturbed input, written into the model's input buffer;
//   2. attr_accumulate:  acc = (overwrite ? 0 : acc) + weight g   one step's gradient into the running sum;
//   3. attr_finish:      attr = (x - b) acc or acc, saliency = max_c |attr| per pixel, sample_sum = sum of attr per sample.
// All are HBM-streaming: 16-byte accesses where the pointers (and, for a broadcast baseline, its period) allow, one float per
// access otherwise, grid-stride, no LDS but the sample sum's fold, no atomics.  Every product, difference and sum is rounded to
// float32 on its own (no contraction into an FMA: attr_stream.h), so the 16-byte body, the scalar form and
// numpy's float32 arithmetic give the same bits (tests/_attribution_ref.py).  The loop over groups of four elements, the pointer
// checks and the step from runtime flags to template arguments are attr_stream.h's, shared with perturbation.hip;
// tests/test_attr_variants_gpu.py pins the name of every instantiation an entry point can launch.
#include "geeco_common.h"
#include "philox_normal.h"
#include "attr_stream.h"      // the uncontracted float32 operations, the four-element accesses and their loop, the baseline rule, the launch path

#define AT_SUM_THREADS 1024       // the sample sum: one block per sample

// ---- 1. the path point ---------------------------------------------------------------------------------------------------------
// A thread owns groups of four consecutive elements (the last group of n may hold fewer), on either access path, so ONE Philox
// call serves a group: z of element i is normal i % 4 of the counter (i / 4 low word, i / 4 high word, step, 0) under the key
// (key low word, key high word) -- it depends on (key, step, i) alone.  sigma == 0 draws nothing.  No clamp.
template <bool V, bool BV>
__global__ __launch_bounds__(AT_THREADS) void attr_path_point_kernel(float* __restrict__ dst, const float* __restrict__ x,
                                                                    const float* __restrict__ baseline, long long period,
                                                                    float alpha, float sigma, unsigned k0, unsigned k1,
                                                                    unsigned step, long long n) {
  const bool small = n <= 0xffffffffLL;
  attr_for_groups4(n, [&](long long e, int cnt) {
    const long long g = e >> 2;
    float xv[4], b[4], o[4];
    attr_load4<V>(x, e, cnt, xv);
    attr_baseline4<BV>(baseline, period, small, e, cnt, b);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = at_add(b[j], at_mul(alpha, at_sub(xv[j], b[j])));
    if (sigma != 0.f) {
      unsigned w[4];
      float z[4];
      philox4x32_10((unsigned)g, (unsigned)((unsigned long long)g >> 32), step, 0u, k0, k1, w);
      philox_normal_pair(w[0], w[1], z[0], z[1]);
      philox_normal_pair(w[2], w[3], z[2], z[3]);
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = at_add(o[j], at_mul(sigma, z[j]));
    }
    attr_store4<V>(dst, e, cnt, o);
  });
}

extern "C" int geeco_attr_path_point(float* dst, const float* x, const float* baseline, int64_t baseline_period, float alpha,
                                     float sigma, uint64_t key, uint32_t step, int64_t n, void* stream) {
  GEECO_CHECK_ARG(dst && x, "attr_path_point: null pointer");
  GEECO_CHECK_ARG(n >= 1, "attr_path_point: n=%lld must be >= 1", (long long)n);
  if (int rc = check_baseline("attr_path_point", baseline, baseline_period, n)) return rc;
  GEECO_CHECK_ARG(sigma >= 0.f && sigma == sigma && alpha == alpha, "attr_path_point: alpha=%g, sigma=%g (sigma >= 0, no NaN)",
                  (double)alpha, (double)sigma);
  GEECO_CHECK_ARG(attr_aligned<4>(dst, x), "attr_path_point: dst and x must be 4-byte aligned");
  GEECO_CHECK_ARG(attr_apart(dst, 4 * (uintptr_t)n, x, 4 * (uintptr_t)n), "attr_path_point: dst overlaps x (the clean input is read by every step)");
  const bool v = attr_aligned<16>(dst, x);
  const bool bv = baseline && baseline_period % 4 == 0 && attr_aligned<16>(baseline);
  const unsigned grid = attr_grid((n + 3) >> 2);
  const unsigned k0 = (unsigned)key, k1 = (unsigned)(key >> 32);
  attr_select([&](auto V, auto BV) {
    geeco_note_kernel("attr_path_point_kernel<%s, %s>", attr_tf(V()), attr_tf(BV()));
    hipLaunchKernelGGL((attr_path_point_kernel<V(), BV()>), dim3(grid), dim3(AT_THREADS), 0, (hipStream_t)stream, dst, x, baseline,
                       (long long)(baseline ? baseline_period : 1), alpha, sigma, k0, k1, (unsigned)step, (long long)n);
  }, v, bv);
  GEECO_LAUNCH_CHECK();
  return 0;
}

// ---- 2. the accumulator --------------------------------------------------------------------------------------------------------
// OVERWRITE: acc is not read (whatever it held is gone, with no zeroing pass); the sum with the constant 0 is still formed, so the
// value is numpy's float32(0) + weight * g to the bit (a product of -0 is stored as +0).
template <bool V, bool OVERWRITE>
__global__ __launch_bounds__(AT_THREADS) void attr_accumulate_kernel(float* __restrict__ acc, const float* __restrict__ g, float weight,
                                                                    long long n) {
  attr_for_groups4(n, [&](long long e, int cnt) {
    float gv[4], a[4] = {0.f, 0.f, 0.f, 0.f};
    attr_load4<V>(g, e, cnt, gv);
    if (!OVERWRITE) attr_load4<V>(acc, e, cnt, a);
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = at_add(a[j], at_mul(weight, gv[j]));
    attr_store4<V>(acc, e, cnt, a);
  });
}

extern "C" int geeco_attr_accumulate(float* acc, const float* g, float weight, int64_t n, int overwrite, void* stream) {
  GEECO_CHECK_ARG(acc && g, "attr_accumulate: null pointer");
  GEECO_CHECK_ARG(n >= 1, "attr_accumulate: n=%lld must be >= 1", (long long)n);
  GEECO_CHECK_ARG(attr_aligned<4>(acc, g), "attr_accumulate: acc and g must be 4-byte aligned");
  GEECO_CHECK_ARG(attr_apart(acc, 4 * (uintptr_t)n, g, 4 * (uintptr_t)n), "attr_accumulate: acc overlaps g");
  const unsigned grid = attr_grid((n + 3) >> 2);
  attr_select([&](auto V, auto O) {
    geeco_note_kernel("attr_accumulate_kernel<%s, %s>", attr_tf(V()), attr_tf(O()));
    hipLaunchKernelGGL((attr_accumulate_kernel<V(), O()>), dim3(grid), dim3(AT_THREADS), 0, (hipStream_t)stream, acc, g, weight, (long long)n);
  }, attr_aligned<16>(acc, g), overwrite != 0);
  GEECO_LAUNCH_CHECK();
  return 0;
}

// ---- 3. the finish -------------------------------------------------------------------------------------------------------------
// First launch, elementwise: a thread owns units of four consecutive pixels = C groups of four elements (the last unit may hold
// fewer pixels), so attr moves in 16-byte words and the four saliency values of a unit are one 16-byte store.  Pixels are
// numbered over the whole tensor [N][frames][HW]; the sample structure matters to the second launch alone.  attr may be acc
// (no __restrict__ on the two): a thread reads the elements it writes, and no other thread touches them.
template <int C, bool V, bool BV>
__global__ __launch_bounds__(AT_THREADS) void attr_finish_kernel(float* attr, float* __restrict__ saliency, const float* acc,
                                                                const float* __restrict__ x,
                                                                const float* __restrict__ baseline, long long period, int multiply,
                                                                long long pixels) {
  const long long units = (pixels + 3) >> 2, stride = (long long)gridDim.x * AT_THREADS, n = pixels * C;
  const bool small = n <= 0xffffffffLL;
  for (long long u = (long long)blockIdx.x * AT_THREADS + threadIdx.x; u < units; u += stride) {
    const long long p0 = u << 2, e0 = p0 * C;
    const int np = pixels - p0 >= 4 ? 4 : (int)(pixels - p0);
    float a[4 * C];
#pragma unroll
    for (int q = 0; q < C; ++q) {
      const long long e = e0 + 4 * q;
      const int cnt = np == 4 ? 4 : (np * C - 4 * q < 0 ? 0 : (np * C - 4 * q > 4 ? 4 : np * C - 4 * q));
      if (cnt == 0) {
        a[4 * q] = a[4 * q + 1] = a[4 * q + 2] = a[4 * q + 3] = 0.f;
        continue;
      }
      attr_load4<V>(acc, e, cnt, a + 4 * q);
      if (multiply) {
        float xv[4], b[4];
        attr_load4<V>(x, e, cnt, xv);
        attr_baseline4<BV>(baseline, period, small, e, cnt, b);
#pragma unroll
        for (int j = 0; j < 4; ++j) a[4 * q + j] = at_mul(at_sub(xv[j], b[j]), a[4 * q + j]);
      }
      attr_store4<V>(attr, e, cnt, a + 4 * q);
    }
    float s[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      float m = fabsf(a[p * C]);
#pragma unroll
      for (int c = 1; c < C; ++c) {
        const float t = fabsf(a[p * C + c]);
        m = (t > m || t != t) ? t : m;        // a NaN attribution makes the pixel's saliency NaN
      }
      s[p] = m;
    }
    attr_store4<V>(saliency, p0, np, s);
  }
}

// Second launch, the sample sums: ONE block of 1024 threads per sample.  The S elements of a sample in groups of four: group q
// belongs to thread q % 1024, which adds its groups in ascending order and the four elements of a group in ascending order
// (elements past S add nothing); the 1024 partial sums are folded by halves (512, 256, .., 1: slot j takes slot j + half).  The
// access path (16-byte words when the sample's first element is aligned and S % 4 == 0) does not change the order.
template <bool V>
__global__ __launch_bounds__(AT_SUM_THREADS) void attr_sample_sum_kernel(const float* __restrict__ attr, long long S,
                                                                        float* __restrict__ sample_sum) {
  __shared__ float sm[AT_SUM_THREADS];
  const float* a = attr + (long long)blockIdx.x * S;
  const long long groups = (S + 3) >> 2;
  float s = 0.f;
  for (long long q = threadIdx.x; q < groups; q += AT_SUM_THREADS) {      // (its own loop: a shared one cost the finish 1 %, profiles/attr_core)
    const long long e = q << 2;
    const int cnt = S - e >= 4 ? 4 : (int)(S - e);
    float v[4];
    attr_load4<V>(a, e, cnt, v);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < cnt) s = at_add(s, v[j]);
  }
  sm[threadIdx.x] = s;
  __syncthreads();
  for (int half = AT_SUM_THREADS / 2; half > 0; half >>= 1) {
    if ((int)threadIdx.x < half) sm[threadIdx.x] = at_add(sm[threadIdx.x], sm[threadIdx.x + half]);
    __syncthreads();
  }
  if (threadIdx.x == 0) sample_sum[blockIdx.x] = sm[0];
}

extern "C" int geeco_attr_finish(float* attr, float* saliency, float* sample_sum, const float* acc, const float* x,
                                 const float* baseline, int64_t baseline_period, int multiply_by_input, int N,
                                 int frames_per_sample, int64_t HW, int C, void* stream) {
  GEECO_CHECK_ARG(attr && saliency && sample_sum && acc && (x || !multiply_by_input), "attr_finish: null pointer");
  GEECO_CHECK_ARG(N >= 1 && frames_per_sample >= 1 && HW >= 1, "attr_finish: N=%d, frames_per_sample=%d, HW=%lld must be >= 1", N,
                  frames_per_sample, (long long)HW);
  GEECO_CHECK_ARG(C >= 1 && C <= 4, "attr_finish: C=%d outside 1..4", C);
  GEECO_CHECK_ARG(HW <= (int64_t)1 << 40 && (int64_t)N * frames_per_sample <= (int64_t)1 << 20, "attr_finish: the tensor is too large");
  const long long pixels = (long long)N * frames_per_sample * HW, n = pixels * C, S = (long long)frames_per_sample * HW * C;
  if (multiply_by_input)
    if (int rc = check_baseline("attr_finish", baseline, baseline_period, n)) return rc;
  GEECO_CHECK_ARG(attr_aligned<4>(attr, saliency, sample_sum, acc, x), "attr_finish: every pointer must be 4-byte aligned");
  const uintptr_t bytes = 4 * (uintptr_t)n;
  GEECO_CHECK_ARG(attr_apart(attr, bytes, saliency, 4 * (uintptr_t)pixels) && attr_apart(attr, bytes, sample_sum, 4 * (uintptr_t)N),
                  "attr_finish: attr overlaps another output");
  // in place (attr == acc: a thread reads exactly what it writes) or apart; a partial overlap would let one thread read what another wrote
  GEECO_CHECK_ARG(attr == acc || attr_apart(attr, bytes, acc, bytes), "attr_finish: attr overlaps acc in part (attr == acc or disjoint)");
  GEECO_CHECK_ARG(!multiply_by_input || attr_apart(attr, bytes, x, bytes), "attr_finish: attr overlaps x");
  const bool v = attr_aligned<16>(attr, saliency, acc) && (!multiply_by_input || attr_aligned<16>(x));
  const bool bv = multiply_by_input && baseline && baseline_period % 4 == 0 && attr_aligned<16>(baseline);
  const unsigned grid = attr_grid((pixels + 3) >> 2);
  const long long period = (multiply_by_input && baseline) ? baseline_period : 1;
  const float* bl = multiply_by_input ? baseline : nullptr;
  hipStream_t s = (hipStream_t)stream;
  attr_channels(C, [&](auto C_) {
    attr_select([&](auto V, auto BV) {
      geeco_note_kernel("attr_finish_kernel<%d, %s, %s>", C_(), attr_tf(V()), attr_tf(BV()));
      hipLaunchKernelGGL((attr_finish_kernel<C_(), V(), BV()>), dim3(grid), dim3(AT_THREADS), 0, s, attr, saliency, acc, x, bl, period,
                         multiply_by_input, pixels);
    }, v, bv);
  });
  GEECO_LAUNCH_CHECK();
  attr_select([&](auto V) {
    geeco_note_kernel("attr_sample_sum_kernel<%s>", attr_tf(V()));
    hipLaunchKernelGGL(attr_sample_sum_kernel<V()>, dim3((unsigned)N), dim3(AT_SUM_THREADS), 0, s, (const float*)attr, S, sample_sum);
  }, attr_aligned<16>(attr) && S % 4 == 0);
  GEECO_LAUNCH_CHECK();
  return 0;
}
