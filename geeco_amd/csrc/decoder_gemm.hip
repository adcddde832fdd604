// =====================================================================================================
// dense f32 GEMM on MFMA 16x16x4 with split-K slabs (LSTM gate matmul and its backward)
// =====================================================================================================
#include "decoder_internal.h"

__global__ __launch_bounds__(256) void gemm_f32_kernel(const GemmParams p) {
  __shared__ float sA[2][GEMM_BK * GEMM_LD];
  __shared__ float sB[2][GEMM_BK * GEMM_LD];
  gemm_block(p, blockIdx.x, blockIdx.y, blockIdx.z, sA, sB, NoStore());
}

__global__ __launch_bounds__(256) void gemm_reduce_kernel(const GemmParams p) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long MN = (long long)p.M * p.N;
  if (i >= MN) return;
  float s = 0.f;
  const float* src = p.part + i;
  int k = 0;
  for (; k + 8 <= p.S; k += 8) {      // 8 independent loads in flight; the sum keeps the slab order
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = src[(long long)(k + u) * MN];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  for (; k < p.S; ++k) s += src[(long long)k * MN];
  const int m = (int)(i / p.N), n = (int)(i - (long long)m * p.N);
  float* c = p.C + (long long)m * p.ldc + n;
  *c = p.accumulate ? *c + s : s;
}

void gemm_plan(int M, int N, int K, int* S, int* kps) {
  long long tiles = (long long)cdiv(M, 64) * cdiv(N, 64);
  long long s = 512 / tiles;
  if (s < 1) s = 1;
  long long maxs = K / 64;
  if (maxs < 1) maxs = 1;
  if (s > maxs) s = maxs;
  int k = cdiv(cdiv(K, (int)s), 16) * 16;
  *kps = k;
  *S = cdiv(K, k);
}

int launch_gemm_f32(const GemmParams& p, hipStream_t s) {
  hipLaunchKernelGGL(gemm_f32_kernel, dim3((unsigned)cdiv(p.N, 64), (unsigned)cdiv(p.M, 64), (unsigned)p.S), dim3(256), 0, s, p);
  GEECO_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t geeco_gemm_ws_bytes(int M, int N, int K) {
  int S, kps;
  gemm_plan(M, N, K, &S, &kps);
  return S > 1 ? (int64_t)S * M * N * 4 : 16;
}

extern "C" int geeco_gemm_f32(const float* A, int64_t lda, int ta, const float* B, int64_t ldb, int tb, float* C,
                              int64_t ldc, int M, int N, int K, int accumulate, void* ws, void* stream) {
  GEECO_CHECK_ARG(A && B && C, "gemm_f32: null pointer");
  GEECO_CHECK_ARG(M >= 1 && N >= 1 && K >= 1, "gemm_f32: bad dims");
  GemmParams p = {};
  p.A = A; p.B = B; p.C = C; p.part = (float*)ws; p.lda = lda; p.ldb = ldb; p.ldc = ldc;
  p.M = M; p.N = N; p.K = K; p.ta = ta; p.tb = tb; p.accumulate = accumulate;
  gemm_plan(M, N, K, &p.S, &p.k_per_split);
  GEECO_CHECK_ARG(p.S == 1 || ws, "gemm_f32: workspace required for split-K");
  hipStream_t s = (hipStream_t)stream;
  if (int rc = launch_gemm_f32(p, s)) return rc;
  if (p.S > 1) {
    hipLaunchKernelGGL(gemm_reduce_kernel, dim3((unsigned)cdiv64((long long)M * N, 256)), dim3(256), 0, s, p);
    GEECO_LAUNCH_CHECK();
  }
  return 0;
}
