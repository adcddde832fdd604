// =====================================================================================================
// inference decoder of the per-frame controllers (T = K steps from the zero state) after the hoisted input projection, ONE launch
// (graph.py:217-260).  The samples of a batch are independent and the state is zero at every call: one 512-thread workgroup owns
// one sample and walks t = 0..T-1 by itself -- nothing in it waits for another block, and a sample's result depends on its own zx
// rows and the weights alone (not on N, its index or its neighbours), bitwise.
//   * Wh [H][4H] (256 KB at H = 128: more than a CU's LDS, less than its register file) stays in REGISTERS across the T steps: thread
//     (u, q) = (tid / 4, tid % 4) keeps rows 32 q .. 32 q + 31 of the four gate columns of unit u (128 floats; two waves per SIMD
//     leave 256 registers per lane).  Per step it reads its 32 values of h from LDS (eight 16-byte reads, four addresses per wave),
//     runs 4 x 32 FMAs, and two quad shuffles sum the four row parts; every lane of a quad then holds all four pre-activations of
//     its unit and runs the gate math, lane 0 stores h to the other half of a double buffer: ONE barrier per step.
//   * zx: lane q carries gate q's zx + bias into its partial sum.  A thread fetches its own column of up to 16 steps at once into
//     LDS slots only it reads (one exposed load latency per 16 steps, no barrier).
//   * fc1/kernel rows and the heads' columns are fetched into registers BEFORE the recurrence (their latency hides behind it);
//     fc1 = 512 / Hfc row parts folded through LDS in ascending order, heads = 16 lanes per output and a shuffle sum.
// Step 0 has no h Wh term at all (a zero state times Wh is never formed), T = 1 does not read wh.
// =====================================================================================================
#include "decoder_internal.h"

constexpr int SQ_THREADS = 512, SQ_HMAX = 128, SQ_KQ = SQ_HMAX / 4, SQ_TCHUNK = 16, SQ_TMAX = 64;

struct SeqParams {
  const float* zx;
  const float* wh;
  const float* bias;
  const float* fc1_w;
  const float* fc1_b;
  const float* hw[GEECO_MAX_HEADS];
  const float* hb[GEECO_MAX_HEADS];
  int size[GEECO_MAX_HEADS], off[GEECO_MAX_HEADS];
  long long ldz, ldw;
  int nheads, OT, N, T, H;
  float* preds;
  float* h_last;
  float* c_last;
};

template <int F>
__global__ __launch_bounds__(SQ_THREADS) void lstm_seq_heads_kernel(const SeqParams p) {
  constexpr int P = SQ_THREADS / F, R = SQ_HMAX / P;      // fc1: P row parts of R rows each
  constexpr int FL = F / 16;                              // heads: 16 lanes per output, FL products each
  __shared__ __attribute__((aligned(16))) float sH[2][SQ_HMAX];
  __shared__ float sZx[SQ_TCHUNK][SQ_THREADS];
  __shared__ float sPart[P][F];
  __shared__ float sA1[F];
  const int tid = threadIdx.x, n = blockIdx.x, H = p.H, T = p.T;
  const int u = tid >> 2, q = tid & 3;
  const bool live = u < H;
  const int col = q * H + u;                              // the zx / bias column this lane carries: gate q of unit u
  // ---- everything the weights contribute, fetched once ---------------------------------------------------------------------
  float w[4][SQ_KQ];
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int k = 0; k < SQ_KQ; ++k) {
      const int row = q * SQ_KQ + k;
      w[g][k] = (T > 1 && live && row < H) ? p.wh[(long long)row * p.ldw + g * H + u] : 0.f;
    }
  const int f = tid % F, part = tid / F;
  float w1[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int row = part * R + r;
    w1[r] = row < H ? p.fc1_w[(long long)row * F + f] : 0.f;
  }
  const int o = tid >> 4, l = tid & 15;
  float wo[FL], hbv = 0.f;
  {
    const bool ov = o < p.OT;
    int hd = 0;
#pragma unroll
    for (int k = 1; k < GEECO_MAX_HEADS; ++k)
      if (k < p.nheads && o >= p.off[k]) hd = k;
    const int sz = sel5(p.size, hd), cc = o - sel5(p.off, hd);
    const float* hw = sel5(p.hw, hd);
#pragma unroll
    for (int j = 0; j < FL; ++j) wo[j] = ov ? hw[(long long)(l + 16 * j) * sz + cc] : 0.f;
    if (ov) hbv = sel5(p.hb, hd)[cc];
  }
  const float b1 = tid < F ? p.fc1_b[tid] : 0.f;
  const float b = live ? p.bias[col] : 0.f;
  if (tid < 2 * SQ_HMAX) (&sH[0][0])[tid] = 0.f;          // units >= H stay zero: their (zero) weight rows meet no garbage
  __syncthreads();
  // ---- the recurrence ------------------------------------------------------------------------------------------------------
  float c = 0.f, hv = 0.f;
  int cur = 0;
  for (int t = 0; t < T; ++t) {
    const int ti = t & (SQ_TCHUNK - 1);
    if (ti == 0) {
#pragma unroll
      for (int i = 0; i < SQ_TCHUNK; ++i)
        if (live && t + i < T) sZx[i][tid] = p.zx[((long long)(t + i) * p.N + n) * p.ldz + col] + b;
    }
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (t > 0) {
      const f32x4* hq = reinterpret_cast<const f32x4*>(&sH[cur][q * SQ_KQ]);
#pragma unroll
      for (int k4 = 0; k4 < SQ_KQ / 4; ++k4) {
        const f32x4 h4 = hq[k4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = 4 * k4 + j;
          a0 = fmaf(h4[j], w[0][k], a0);
          a1 = fmaf(h4[j], w[1][k], a1);
          a2 = fmaf(h4[j], w[2][k], a2);
          a3 = fmaf(h4[j], w[3][k], a3);
        }
      }
    }
    const float zq = live ? sZx[ti][tid] : 0.f;
    a0 += q == 0 ? zq : 0.f;
    a1 += q == 1 ? zq : 0.f;
    a2 += q == 2 ? zq : 0.f;
    a3 += q == 3 ? zq : 0.f;
#pragma unroll
    for (int m = 1; m < 4; m <<= 1) {
      a0 += __shfl_xor(a0, m, 64);
      a1 += __shfl_xor(a1, m, 64);
      a2 += __shfl_xor(a2, m, 64);
      a3 += __shfl_xor(a3, m, 64);
    }
    // tf.nn.rnn_cell.LSTMCell: gate order i, j, f, o; forget_bias 1 (lstm_gates_fwd_kernel's expressions)
    const float si = sigmoidf_(a0), tj = tanhf(a1), sf = sigmoidf_(a2 + 1.0f), so = sigmoidf_(a3);
    c = sf * c + si * tj;
    hv = so * tanhf(c);
    cur ^= 1;
    if (q == 0 && live) sH[cur][u] = hv;
    __syncthreads();
  }
  if (q == 0 && live) {
    if (p.h_last) p.h_last[(long long)n * H + u] = hv;
    if (p.c_last) p.c_last[(long long)n * H + u] = c;
  }
  // ---- a1 = relu(h W1 + b1), predictions = a1 Wheads + bheads                                        graph.py:229-259 ----------
  {
    const float* hh = &sH[cur][part * R];
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r) s = fmaf(hh[r], w1[r], s);
    sPart[part][f] = s;
  }
  __syncthreads();
  if (tid < F) {
    float v = b1;
#pragma unroll
    for (int pp = 0; pp < P; ++pp) v += sPart[pp][tid];
    sA1[tid] = fmaxf(v, 0.f);
  }
  __syncthreads();
  {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < FL; ++j) s = fmaf(sA1[l + 16 * j], wo[j], s);
#pragma unroll
    for (int m = 8; m > 0; m >>= 1) s += __shfl_xor(s, m, 64);
    if (l == 0 && o < p.OT) p.preds[(long long)n * p.OT + o] = s + hbv;
  }
}

extern "C" int geeco_lstm_seq_heads_fwd(const float* zx, int64_t ldz, const float* wh, int64_t ldw, const float* bias,
                                        const float* fc1_w, const float* fc1_b, int nheads, const float* const* heads_w,
                                        const float* const* heads_b, const int* head_size, int N, int T, int H, int Hfc,
                                        float* preds, float* h_last, float* c_last, void* stream) {
  GEECO_CHECK_ARG(zx && wh && bias && fc1_w && fc1_b && heads_w && heads_b && head_size && preds, "lstm_seq_heads: null pointer");
  GEECO_CHECK_ARG(N >= 1, "lstm_seq_heads: N=%d < 1", N);
  GEECO_CHECK_ARG(T >= 1 && T <= SQ_TMAX, "lstm_seq_heads: T=%d outside 1..%d", T, SQ_TMAX);
  GEECO_CHECK_ARG(nheads >= 1 && nheads <= GEECO_MAX_HEADS, "lstm_seq_heads: nheads=%d outside 1..%d", nheads, GEECO_MAX_HEADS);
  SeqParams p = {};
  int off = 0;
  for (int i = 0; i < nheads; ++i) {
    GEECO_CHECK_ARG(heads_w[i] && heads_b[i], "lstm_seq_heads: head %d null pointer", i);
    GEECO_CHECK_ARG(head_size[i] >= 1 && head_size[i] <= 32, "lstm_seq_heads: head %d size %d", i, head_size[i]);
    p.hw[i] = heads_w[i]; p.hb[i] = heads_b[i]; p.size[i] = head_size[i]; p.off[i] = off;
    off += head_size[i];
  }
  GEECO_CHECK_ARG(off <= 32, "lstm_seq_heads: %d outputs > 32", off);
  GEECO_CHECK_ARG(H >= 1 && Hfc >= 1 && ldz >= 4 * (int64_t)H && ldw >= 4 * (int64_t)H, "lstm_seq_heads: bad dims");
  if (H > SQ_HMAX || (Hfc != 64 && Hfc != 128)) return GEECO_ENOSUP;      // nothing launched: the caller runs the step chain
  p.zx = zx; p.wh = wh; p.bias = bias; p.fc1_w = fc1_w; p.fc1_b = fc1_b; p.ldz = ldz; p.ldw = ldw;
  p.nheads = nheads; p.OT = off; p.N = N; p.T = T; p.H = H; p.preds = preds; p.h_last = h_last; p.c_last = c_last;
  geeco_note_kernel("lstm_seq_heads_kernel");
  if (Hfc == 128)
    hipLaunchKernelGGL(lstm_seq_heads_kernel<128>, dim3((unsigned)N), dim3(SQ_THREADS), 0, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(lstm_seq_heads_kernel<64>, dim3((unsigned)N), dim3(SQ_THREADS), 0, (hipStream_t)stream, p);
  GEECO_LAUNCH_CHECK();
  return 0;
}
