// =====================================================================================================
// LSTM gate math (tf.nn.rnn_cell.LSTMCell, gate order i, j, f, o; forget_bias = 1)
// =====================================================================================================
#include "decoder_internal.h"

__global__ __launch_bounds__(256) void lstm_gates_fwd_kernel(const float* __restrict__ z, const float* __restrict__ bias,
                                                             const float* __restrict__ c_prev, float* __restrict__ c,
                                                             float* __restrict__ h, float* __restrict__ gates, int N,
                                                             int H) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N * H) return;
  const int n = i / H, u = i - n * H;
  const float* zr = z + (long long)n * 4 * H;
  const float zi = zr[u] + bias[u], zj = zr[H + u] + bias[H + u];
  const float zf = zr[2 * H + u] + bias[2 * H + u], zo = zr[3 * H + u] + bias[3 * H + u];
  const float si = sigmoidf_(zi), tj = tanhf(zj), sf = sigmoidf_(zf + 1.0f), so = sigmoidf_(zo);
  const float cp = c_prev ? c_prev[i] : 0.f;
  const float cn = sf * cp + si * tj;
  c[i] = cn;
  h[i] = so * tanhf(cn);
  float* gr = gates + (long long)n * 4 * H;
  gr[u] = si; gr[H + u] = tj; gr[2 * H + u] = sf; gr[3 * H + u] = so;
}

__global__ __launch_bounds__(256) void lstm_gates_bwd_kernel(const float* __restrict__ gates,
                                                             const float* __restrict__ c_prev, const float* __restrict__ c,
                                                             const float* __restrict__ dh, const float* __restrict__ dc,
                                                             float* __restrict__ dz, float* __restrict__ dc_prev, int N,
                                                             int H) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N * H) return;
  const int n = i / H, u = i - n * H;
  const float* gr = gates + (long long)n * 4 * H;
  const float si = gr[u], tj = gr[H + u], sf = gr[2 * H + u], so = gr[3 * H + u];
  const float tc = tanhf(c[i]);
  const float dhv = dh ? dh[i] : 0.f;
  const float dct = (dc ? dc[i] : 0.f) + dhv * so * (1.f - tc * tc);
  const float cp = c_prev ? c_prev[i] : 0.f;
  float* dr = dz + (long long)n * 4 * H;
  dr[u] = dct * tj * si * (1.f - si);
  dr[H + u] = dct * si * (1.f - tj * tj);
  dr[2 * H + u] = dct * cp * sf * (1.f - sf);
  dr[3 * H + u] = dhv * tc * so * (1.f - so);
  if (dc_prev) dc_prev[i] = dct * sf;
}

// The first LSTM step (zero state: z = X Wx alone) with the split-K slab sum of the input projection INSIDE the gate kernel: one
// dependent launch fewer (~5 us of a step whose decoder is pure launch latency).  Block = 64 (sample, unit) pairs x 4 gates:
// wave g sums gate g's slabs in the slab order of gemm_reduce_kernel (bitwise the same z), LDS hands the four sums to wave 0.
__global__ __launch_bounds__(256) void lstm_gates_fwd_slabs_kernel(const float* __restrict__ part, int S,
                                                                   const float* __restrict__ bias, float* __restrict__ z,
                                                                   float* __restrict__ c, float* __restrict__ h,
                                                                   float* __restrict__ gates, int N, int H) {
  __shared__ float sz[4][64];
  const int g = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i = blockIdx.x * 64 + lane;
  const bool live = i < N * H;
  const int n = live ? i / H : 0, u = live ? i - n * H : 0;
  const long long MN = (long long)N * 4 * H;
  const long long col = (long long)n * 4 * H + g * H + u;
  float s = 0.f;
  if (live) {
    const float* src = part + col;
    int k = 0;
    for (; k + 8 <= S; k += 8) {
      float v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = src[(long long)(k + q) * MN];
#pragma unroll
      for (int q = 0; q < 8; ++q) s += v[q];
    }
    for (; k < S; ++k) s += src[(long long)k * MN];
    z[col] = s;
  }
  sz[g][lane] = s + (live ? bias[g * H + u] : 0.f);
  __syncthreads();
  if (g != 0 || !live) return;
  const float zi = sz[0][lane], zj = sz[1][lane], zf = sz[2][lane], zo = sz[3][lane];
  const float si = sigmoidf_(zi), tj = tanhf(zj), sf = sigmoidf_(zf + 1.0f), so = sigmoidf_(zo);
  const float cn = sf * 0.f + si * tj;
  c[i] = cn;
  h[i] = so * tanhf(cn);
  float* gr = gates + (long long)n * 4 * H;
  gr[u] = si; gr[H + u] = tj; gr[2 * H + u] = sf; gr[3 * H + u] = so;
}

extern "C" int geeco_lstm_input_step_fwd(const float* x, int64_t ldx, const float* wx, int64_t ldw, const float* bias, float* z,
                                         float* c, float* h, float* gates, int N, int H, int D, void* ws, void* stream) {
  GEECO_CHECK_ARG(x && wx && bias && z && c && h && gates, "lstm_input_step_fwd: null pointer");
  GEECO_CHECK_ARG(N >= 1 && H >= 1 && D >= 1 && ldx >= D && ldw >= 4 * (int64_t)H, "lstm_input_step_fwd: bad dims");
  GemmParams p = {};
  p.A = x; p.B = wx; p.C = z; p.part = (float*)ws; p.lda = ldx; p.ldb = ldw; p.ldc = 4 * H;
  p.M = N; p.N = 4 * H; p.K = D;
  gemm_plan(p.M, p.N, p.K, &p.S, &p.k_per_split);
  GEECO_CHECK_ARG(p.S == 1 || ws, "lstm_input_step_fwd: workspace required for split-K (geeco_gemm_ws_bytes(N, 4H, D))");
  hipStream_t s = (hipStream_t)stream;
  if (int rc = launch_gemm_f32(p, s)) return rc;
  if (p.S > 1)
    hipLaunchKernelGGL(lstm_gates_fwd_slabs_kernel, dim3((unsigned)cdiv(N * H, 64)), dim3(256), 0, s, (const float*)p.part, p.S,
                       bias, z, c, h, gates, N, H);
  else
    hipLaunchKernelGGL(lstm_gates_fwd_kernel, dim3((unsigned)cdiv(N * H, 256)), dim3(256), 0, s, (const float*)z, bias,
                       (const float*)nullptr, c, h, gates, N, H);
  GEECO_LAUNCH_CHECK();
  return 0;
}

extern "C" int geeco_lstm_gates_fwd(const float* z, const float* bias, const float* c_prev, float* c, float* h,
                                    float* gates, int N, int H, void* stream) {
  GEECO_CHECK_ARG(z && bias && c && h && gates && N >= 1 && H >= 1, "lstm_gates_fwd: bad arguments");
  hipLaunchKernelGGL(lstm_gates_fwd_kernel, dim3((unsigned)cdiv(N * H, 256)), dim3(256), 0, (hipStream_t)stream, z,
                     bias, c_prev, c, h, gates, N, H);
  GEECO_LAUNCH_CHECK();
  return 0;
}

extern "C" int geeco_lstm_gates_bwd(const float* gates, const float* c_prev, const float* c, const float* dh,
                                    const float* dc, float* dz, float* dc_prev, int N, int H, void* stream) {
  GEECO_CHECK_ARG(gates && c && dz && N >= 1 && H >= 1, "lstm_gates_bwd: bad arguments");
  hipLaunchKernelGGL(lstm_gates_bwd_kernel, dim3((unsigned)cdiv(N * H, 256)), dim3(256), 0, (hipStream_t)stream,
                     gates, c_prev, c, dh, dc, dz, dc_prev, N, H);
  GEECO_LAUNCH_CHECK();
  return 0;
}
