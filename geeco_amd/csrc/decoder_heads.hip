// =====================================================================================================
// fc1 + heads + losses, forward and backward, one workgroup (everything is tiny: N x 128)
// =====================================================================================================
#include "decoder_internal.h"

// C[M][N] = A[M][K] B[K][N] inside ONE workgroup on MFMA 16x16x4: waves take 16x16 output tiles
// round-robin; operands are fetched straight from global memory (everything is L2-resident and
// tiny), 2 loads per MFMA per lane.  A(i, k) = a[i * a_rs + k * a_ks], B(k, j) = b[k * b_ks + j * b_cs]
// (pointer + strides, so the K loop is pure pointer bumps); st(i, j, v) stores.
template <class FS>
__device__ __forceinline__ void block_mfma_gemm(int M, int N, int K, const float* a, int a_rs, int a_ks,
                                                const float* b, int b_ks, int b_cs, FS st) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int tn = (N + 15) >> 4, nt = ((M + 15) >> 4) * tn;
  for (int t = wave; t < nt; t += nw) {
    const int ti = t / tn, tj = t - ti * tn;
    const int i = ti * 16 + r, j = tj * 16 + r;
    const bool iv = i < M, jv = j < N;
    const float* ap = a + (long long)(iv ? i : 0) * a_rs + q * a_ks;
    const float* bp = b + (long long)(jv ? j : 0) * b_cs + q * b_ks;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};

    for (int k0 = 0; k0 < K; k0 += 4) {
      const bool kv = k0 + q < K;
      const float av = (iv && kv) ? ap[(long long)k0 * a_ks] : 0.f;
      const float bv = (jv && kv) ? bp[(long long)k0 * b_ks] : 0.f;
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
    }
    const float e[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int io = ti * 16 + 4 * q + k;
      if (io < M && jv) st(io, j, e[k]);
    }
  }
}

// SHAPED: P3 and the loss means follow tf.losses' weights= / label_smoothing= / huber_loss (decoder_internal.h); the unshaped
// instantiation keeps the arithmetic it always had
template <bool SHAPED>
__global__ __launch_bounds__(1024) void heads_loss_kernel(const HeadsParams p) {
  constexpr int NT = 1024;
  const int tid = threadIdx.x;
  const int N = p.N, H = p.H, F = p.Hfc, OT = p.OT;
  __shared__ float s_red[16][GEECO_MAX_HEADS];
  __shared__ int s_cnt[SHAPED ? NT / 64 : 1][2];
  [[maybe_unused]] int cnt_reg = N, cnt_cls = N;
  if constexpr (SHAPED) shaped_counts<NT>(p, s_cnt, &cnt_reg, &cnt_cls);
  __shared__ float s_hb[32];
  __shared__ int s_hd[32], s_hc[32];
  float* whm = p.dpred + (long long)N * OT;     // ws: [OT][F] = the head kernels side by side, transposed
  // P0: per-output-column tables and the packed [OT][F] head matrix
  if (tid < OT) {
    int hd = 0;
#pragma unroll
    for (int k = 1; k < GEECO_MAX_HEADS; ++k)
      if (k < p.nheads && tid >= p.off[k]) hd = k;
    s_hd[tid] = hd;
    s_hc[tid] = tid - sel5(p.off, hd);
    s_hb[tid] = sel5(p.hb, hd)[tid - sel5(p.off, hd)];
  }
  __syncthreads();
  for (int e = tid; e < OT * F; e += NT) {
    const int o = e / F, f = e - o * F;
    const int hd = s_hd[o];
    whm[e] = sel5(p.hw, hd)[f * sel5(p.size, hd) + s_hc[o]];
  }
  // P1: a1 = relu(h W1 + b1)                                   graph.py:229-230
  block_mfma_gemm(N, F, H, p.h, H, 1, p.fc1_w, F, 1,
                  [&](int n, int j, float v) { p.a1[n * F + j] = fmaxf(v + p.fc1_b[j], 0.f); });
  __syncthreads();
  // P2: preds[n][sum of head sizes]                             graph.py:233-259
  block_mfma_gemm(N, OT, F, p.a1, F, 1, whm, 1, F, [&](int n, int o, float v) { p.preds[n * OT + o] = v + s_hb[o]; });
  __syncthreads();
  // P3: losses and d(loss)/d(pred)           graph.py:430-500, estimator.py:206-239
  //   kind 0: tf.losses.mean_squared_error (mean over N*size); kind 1: softmax cross-entropy against
  //   one_hot(rint(target) + 1) (mean over N)
  float lsum[GEECO_MAX_HEADS];
#pragma unroll
  for (int k = 0; k < GEECO_MAX_HEADS; ++k) lsum[k] = 0.f;
  const float invn = 1.f / N;
  for (int n = tid; n < N; n += NT) {
    const float* pr = p.preds + n * OT;
    float* dp = p.dpred + n * OT;
#pragma unroll
    for (int hd = 0; hd < GEECO_MAX_HEADS; ++hd) {
      if (hd >= p.nheads) break;
      const int sz = p.size[hd], of = p.off[hd];
      const float* tg = p.tgt[hd] + (long long)n * p.tstride[hd];
      const float wsc = p.weight[hd] * p.loss_scale;
      if constexpr (SHAPED) {
        const bool cls = p.class_w && hd == p.cls_head;
        const float sw = shaped_sample_w(p, n);
        lsum[hd] += shaped_head_terms(p, hd, pr + of, tg, dp + of, cls ? shaped_class_w(p, sw, tg[0]) : sw,
                                      cls ? cnt_cls : cnt_reg);
      } else if (p.kind[hd] == 0) {
        const float c2 = 2.f / (float)(N * sz) * wsc;
        for (int c = 0; c < sz; ++c) {
          const float d = pr[of + c] - tg[c];
          lsum[hd] += d * d;
          dp[of + c] = d * c2;
        }
      } else {
        const int label = (int)rintf(tg[0]) + 1;             // estimator.py:213-215
        float mx = pr[of];
        for (int c = 1; c < sz; ++c) mx = fmaxf(mx, pr[of + c]);
        float se = 0.f;
        for (int c = 0; c < sz; ++c) se += expf(pr[of + c] - mx);
        const bool lv = label >= 0 && label < sz;             // one_hot of an out-of-range label is all-zero
        if (lv) lsum[hd] += mx + logf(se) - pr[of + label];
        for (int c = 0; c < sz; ++c)
          dp[of + c] = lv ? (expf(pr[of + c] - mx) / se - (c == label ? 1.f : 0.f)) * invn * wsc : 0.f;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < GEECO_MAX_HEADS; ++k) {
    lsum[k] = wave_reduce_sum(lsum[k]);
    if ((tid & 63) == 0) s_red[tid >> 6][k] = lsum[k];
  }
  __syncthreads();
  if (tid == 0) {
    float total = 0.f;
    for (int hd = 0; hd < p.nheads; ++hd) {
      float a = 0.f;
      for (int w = 0; w < 16; ++w) a += s_red[w][hd];
      if constexpr (SHAPED) {
        const int cnt = (p.class_w && hd == p.cls_head) ? cnt_cls : cnt_reg;
        a *= cnt == 0 ? 0.f : (p.kind[hd] == 1 ? 1.f / cnt : 1.f / (float)(cnt * p.size[hd]));
      } else {
        a *= p.kind[hd] == 0 ? 1.f / (float)(N * p.size[hd]) : invn;
      }
      p.losses[1 + hd] = a;
      total += p.weight[hd] * a;
    }
    p.losses[0] = total;
  }
  if (!p.backward) return;
  __syncthreads();
  // P4: head gradients  d_hw[f][o] = sum_n a1[n][f] dpred[n][o];  da1 = (dpred Wh^T) * relu'
  block_mfma_gemm(F, OT, N, p.a1, 1, F, p.dpred, OT, 1, [&](int f, int o, float v) {
    const int hd = s_hd[o];
    sel5(p.dhw, hd)[f * sel5(p.size, hd) + s_hc[o]] = v;
  });
  for (int o = tid; o < OT; o += NT) {
    float sum = 0.f;
    for (int n = 0; n < N; ++n) sum += p.dpred[n * OT + o];
    sel5(p.dhb, s_hd[o])[s_hc[o]] = sum;
  }
  block_mfma_gemm(N, F, OT, p.dpred, OT, 1, whm, F, 1,
                  [&](int n, int f, float v) { p.da1[n * F + f] = p.a1[n * F + f] > 0.f ? v : 0.f; });
  __syncthreads();
  // P5: fc1 gradients and d(h)
  block_mfma_gemm(H, F, N, p.h, 1, H, p.da1, F, 1, [&](int k, int j, float v) { p.d_fc1_w[k * F + j] = v; });
  for (int j = tid; j < F; j += NT) {
    float sum = 0.f;
    for (int n = 0; n < N; ++n) sum += p.da1[n * F + j];
    p.d_fc1_b[j] = sum;
  }
  block_mfma_gemm(N, H, F, p.da1, F, 1, p.fc1_w, 1, F, [&](int n, int k, float v) { p.dh[n * H + k] = v; });
}

// =====================================================================================================
// fc1 + heads + losses per SAMPLE (round 5).  Everything from the LSTM output to d(loss)/d(h) is independent per sample
// (graph.py:229-259, 430-500): only the loss means and the weight / bias gradients sum over the batch.  Round 2-4 ran the
// whole tail in ONE workgroup (six dependent MFMA tile loops with a barrier between: 34 us of pure latency at N = 32, three
// MFLOP of work).  Here:
//   * heads_sample_kernel: one 1024-thread workgroup per sample, N workgroups side by side: fc1/kernel staged in LDS once
//     (read twice: forward and d(h)), every product a few hundred FMAs per thread on the vector ALU (a 1 x 128 row times a
//     128 x 128 matrix is no MFMA shape), partial sums folded through LDS / half-wave shuffles in a fixed order.  Writes the
//     predictions, the per-sample loss terms, a1, d(a1), d(pred) and d(h).
//     FUSE (one-step decoders, zero initial state: the goal model's dynimg branch): the same workgroup first sums the split-K
//     slabs of its sample's gate pre-activations and runs the gate math (lstm_gates_fwd_slabs_kernel's work, same slab
//     order), and at the end turns d(h) into the gate gradients dz (lstm_gates_bwd_kernel's work): two dependent launches
//     less around the heads.
//   * heads_finish_role: what sums over the batch -- d(fc1/kernel) = h^T d(a1) (row tiles), the head kernels' gradients,
//     the bias gradients and the loss means, each a sum over n in ascending order.  A handful of independent blocks that ride
//     at the end of another launch's grid (lstm_step_bwd_finish_kernel) or run as heads_finish_kernel.
// Shapes: H <= 128, Hfc in {64, 128} (the reference's defaults are 128 / 128, params.py:21-22); anything else takes the
// single-workgroup heads_loss_kernel above.
// =====================================================================================================
constexpr int HS_WP = HS_FMAX + 4;      // LDS row pitch of fc1/kernel: rows of two half-waves fall on different bank groups
constexpr size_t HS_LDS_BYTES = (size_t)(HS_HMAX * HS_WP + HS_THREADS * 4) * 4;

struct StepFuse {
  const float* part;        // split-K slabs of z = x Wx: [S][N][4H]
  int S;
  const float* bias;        // lstm_cell/bias [4H]
  float* z;                 // [N][4H] slab sums (kept: geeco_lstm_input_step_fwd writes them too)
  float* c; float* hout;    // [N][H]
  float* gates;             // [N][4H] activated gates i, j, f, o
  float* dz;                // backward: gate gradients [N][4H]
};

// SHAPED: P3 follows tf.losses' weights= / label_smoothing= / huber_loss (decoder_internal.h).  Every workgroup forms the batch's
// two counts of non-zero effective weights itself, from the N <= 4096 weights and gripper labels (four loads per thread, issued
// with the rest of P0): no atomics, no extra launch, no dependency on another block.
template <bool FUSE, int G, bool SHAPED>   // G = Hfc / 4: float4 column groups of fc1/kernel, 16 or 32
__global__ __launch_bounds__(HS_THREADS) void heads_sample_kernel(const HeadsParams p, const StepFuse sf) {
  const int tid = threadIdx.x, n = blockIdx.x;
  const int H = p.H, OT = p.OT, N = p.N;
  constexpr int F = 4 * G;
  constexpr int P = HS_THREADS / G;      // row parts (fc1 forward) / rows per pass (d(h))
  extern __shared__ __attribute__((aligned(16))) float hs_dyn[];           // HS_LDS_BYTES (more than the 64 KiB a static array may take)
  float* sW1 = hs_dyn;                                                        // [H][HS_WP] fc1/kernel
  float* sPart = hs_dyn + HS_HMAX * HS_WP;                                    // [P][F] partial sums of the fc1 forward
  __shared__ __attribute__((aligned(16))) float sH[HS_HMAX], sA1[HS_FMAX], sDA[HS_FMAX], sDH[HS_HMAX], sB1[HS_FMAX];
  __shared__ float sZ[FUSE ? 4 * HS_HMAX : 1];
  __shared__ float sPr[32], sDp[32], sHb[32], sTg[32];
  __shared__ int sHd[32], sHc[32];
  __shared__ float sWh[32 * HS_FMAX];     // the head kernels side by side, transposed: [o][f] (both uses walk f across lanes)
  __shared__ int sCnt[SHAPED ? HS_THREADS / 64 : 1][2];
  // ---- P0: fc1/kernel -> LDS (issued first: independent of everything), small tables, the sample's LSTM output -----------
  f32x4 wv[4];
  const int W4 = H * G;                  // float4 of fc1/kernel (<= 4096 = 4 per thread)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e4 = tid + HS_THREADS * i;
    wv[i] = e4 < W4 ? reinterpret_cast<const f32x4*>(p.fc1_w)[e4] : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  // every global input of the sample is fetched here, up front: after this phase only LDS is read
  if (tid < OT) {
    const int hd = heads_head_of(p, tid), cc = tid - sel5(p.off, hd);
    sHd[tid] = hd;
    sHc[tid] = cc;
    sHb[tid] = sel5(p.hb, hd)[cc];
    if (sel5(p.kind, hd) != 1 || cc == 0) sTg[tid] = sel5(p.tgt, hd)[(long long)n * sel5(p.tstride, hd) + cc];
  }
  if (tid < F) sB1[tid] = p.fc1_b[tid];
  [[maybe_unused]] float s_w = 1.f;
  [[maybe_unused]] int cnt_reg = N, cnt_cls = N;
  if constexpr (SHAPED) {
    s_w = shaped_sample_w(p, n);
    shaped_counts<HS_THREADS>(p, sCnt, &cnt_reg, &cnt_cls);
  }
  for (int e = tid; e < OT * F; e += HS_THREADS) {      // consecutive threads: consecutive o of one f (the variables are [f][size])
    const int f = e / OT, o = e - f * OT;
    const int hd = heads_head_of(p, o);
    sWh[o * HS_FMAX + f] = sel5(p.hw, hd)[(long long)f * sel5(p.size, hd) + (o - sel5(p.off, hd))];
  }
  [[maybe_unused]] float g_si = 0.f, g_tj = 0.f, g_sf = 0.f, g_so = 0.f, g_tc = 0.f;
  if (FUSE) {
    // gate pre-activations of this sample: column tid of [4H], slabs summed in slab order (as gemm_reduce_kernel)
    if (tid < 4 * H) {
      const long long MN = (long long)N * 4 * H;
      const float* src = sf.part + (long long)n * 4 * H + tid;
      float s = 0.f;
      int k = 0;
      for (; k + 16 <= sf.S; k += 16) {
        float v[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) v[q] = src[(long long)(k + q) * MN];
#pragma unroll
        for (int q = 0; q < 16; ++q) s += v[q];
      }
      if (k < sf.S) {      // the remaining slabs (< 16) in ONE round of predicated loads; a skipped slab adds nothing
        float v[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) v[q] = k + q < sf.S ? src[(long long)(k + q) * MN] : 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q)
          if (k + q < sf.S) s += v[q];
      }
      sf.z[(long long)n * 4 * H + tid] = s;
      sZ[tid] = s + sf.bias[tid];
    }
  } else {
    if (tid < H) sH[tid] = p.h[(long long)n * H + tid];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e4 = tid + HS_THREADS * i;
    if (e4 < W4) *reinterpret_cast<f32x4*>(sW1 + (e4 / G) * HS_WP + (e4 % G) * 4) = wv[i];
  }
  __syncthreads();
  if (FUSE) {
    if (tid < H) {      // tf.nn.rnn_cell.LSTMCell from a zero state (graph.py:217-225): gate order i, j, f, o; forget_bias 1
      const int u = tid;
      g_si = sigmoidf_(sZ[u]); g_tj = tanhf(sZ[H + u]); g_sf = sigmoidf_(sZ[2 * H + u] + 1.0f); g_so = sigmoidf_(sZ[3 * H + u]);
      const float cn = g_sf * 0.f + g_si * g_tj;
      g_tc = tanhf(cn);
      const float hv = g_so * g_tc;
      const long long i = (long long)n * H + u;
      sf.c[i] = cn;
      sf.hout[i] = hv;
      float* gr = sf.gates + (long long)n * 4 * H;
      gr[u] = g_si; gr[H + u] = g_tj; gr[2 * H + u] = g_sf; gr[3 * H + u] = g_so;
      sH[u] = hv;
    }
    __syncthreads();
  }
  // ---- P1: a1 = relu(h W1 + b1)                                                              graph.py:229-230 ----------
  {
    const int pp = tid / G, g = tid - pp * G;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int hh = pp; hh < H; hh += P) acc += sH[hh] * *reinterpret_cast<const f32x4*>(sW1 + hh * HS_WP + 4 * g);
    *reinterpret_cast<f32x4*>(sPart + pp * F + 4 * g) = acc;
  }
  __syncthreads();
  if (tid < F) {
    float v = sB1[tid];
#pragma unroll 16
    for (int pp = 0; pp < P; ++pp) v += sPart[pp * F + tid];
    v = fmaxf(v, 0.f);
    sA1[tid] = v;
    if (p.backward) p.a1[(long long)n * F + tid] = v;
  }
  __syncthreads();
  // ---- P2: predictions = a1 Wh + bh (all heads side by side)                                   graph.py:233-259 ----------
  if (tid < OT * 32) {
    const int o = tid >> 5, l = tid & 31;
    float s = 0.f;
#pragma unroll
    for (int f = l; f < F; f += 32) s += sA1[f] * sWh[o * HS_FMAX + f];
#pragma unroll
    for (int m = 16; m > 0; m >>= 1) s += __shfl_xor(s, m, 64);
    if (l == 0) {
      const float v = s + sHb[o];
      sPr[o] = v;
      p.preds[(long long)n * OT + o] = v;
    }
  }
  __syncthreads();
  // ---- P3: this sample's loss terms and d(loss)/d(pred)                 graph.py:430-500, estimator.py:206-239 ----------
  if (tid < p.nheads) {
    const int hd = tid;
    const int sz = sel5(p.size, hd), of = sel5(p.off, hd);
    const float* tg = sTg + of;
    const float wsc = sel5(p.weight, hd) * p.loss_scale;
    const float invn = 1.f / N;
    float l = 0.f;
    if constexpr (SHAPED) {
      const bool cls = p.class_w && hd == p.cls_head;
      l = shaped_head_terms(p, hd, sPr + of, tg, sDp + of, cls ? shaped_class_w(p, s_w, tg[0]) : s_w, cls ? cnt_cls : cnt_reg);
    } else if (sel5(p.kind, hd) == 0) {
      const float c2 = 2.f / (float)(N * sz) * wsc;
      for (int cc = 0; cc < sz; ++cc) {
        const float d = sPr[of + cc] - tg[cc];
        l += d * d;
        sDp[of + cc] = d * c2;
      }
    } else {
      const int label = (int)rintf(tg[0]) + 1;             // estimator.py:213-215
      float mx = sPr[of];
      for (int cc = 1; cc < sz; ++cc) mx = fmaxf(mx, sPr[of + cc]);
      float se = 0.f;
      for (int cc = 0; cc < sz; ++cc) se += expf(sPr[of + cc] - mx);
      const bool lv = label >= 0 && label < sz;             // one_hot of an out-of-range label is all-zero
      if (lv) l = mx + logf(se) - sPr[of + label];
      for (int cc = 0; cc < sz; ++cc)
        sDp[of + cc] = lv ? (expf(sPr[of + cc] - mx) / se - (cc == label ? 1.f : 0.f)) * invn * wsc : 0.f;
    }
    p.lterm[(long long)n * 8 + hd] = l;
  }
  if constexpr (SHAPED) {      // the counts travel to the finish role in the free slots of the lterm row (every block: the same values)
    if (tid == HS_CNT_REG) p.lterm[(long long)n * 8 + HS_CNT_REG] = (float)cnt_reg;
    if (tid == HS_CNT_CLS) p.lterm[(long long)n * 8 + HS_CNT_CLS] = (float)cnt_cls;
  }
  if (!p.backward) return;
  __syncthreads();
  // ---- P4: d(a1) = ReluGrad(dpred Wh^T) ----------------------------------------------------------------------------------
  if (tid < OT) p.dpred[(long long)n * OT + tid] = sDp[tid];
  if (tid < F) {
    float s = 0.f;
#pragma unroll 4
    for (int o = 0; o < OT; ++o) s += sDp[o] * sWh[o * HS_FMAX + tid];
    s = sA1[tid] > 0.f ? s : 0.f;
    sDA[tid] = s;
    p.da1[(long long)n * F + tid] = s;
  }
  __syncthreads();
  // ---- P5: d(h) = d(a1) W1^T: G lanes share a row of fc1/kernel, half-wave shuffle sum ----------------------------------------
  {
    const int r = tid / G, g = tid - r * G;
    const f32x4 d4 = *reinterpret_cast<const f32x4*>(sDA + 4 * g);
    for (int hh = r; hh < H; hh += P) {
      const f32x4 w4 = *reinterpret_cast<const f32x4*>(sW1 + hh * HS_WP + 4 * g);
      float s = d4.x * w4.x + d4.y * w4.y + d4.z * w4.z + d4.w * w4.w;
#pragma unroll
      for (int m = G >> 1; m > 0; m >>= 1) s += __shfl_xor(s, m, 64);
      if (g == 0) sDH[hh] = s;
    }
  }
  __syncthreads();
  if (tid < H) {
    const float dhv = sDH[tid];
    if (p.dh) p.dh[(long long)n * H + tid] = dhv;
    if (FUSE) {      // lstm_gates_bwd_kernel for the zero-state single step: dc = 0, c_prev = 0
      const int u = tid;
      const float dct = 0.f + dhv * g_so * (1.f - g_tc * g_tc);
      float* dr = sf.dz + (long long)n * 4 * H;
      dr[u] = dct * g_tj * g_si * (1.f - g_si);
      dr[H + u] = dct * g_si * (1.f - g_tj * g_tj);
      dr[2 * H + u] = dct * 0.f * g_sf * (1.f - g_sf);
      dr[3 * H + u] = dhv * g_tc * g_so * (1.f - g_so);
    }
  }
}

extern "C" int64_t geeco_heads_ws_bytes(int N, int H, int Hfc) {
  (void)H;
  return ((int64_t)2 * N * Hfc + (int64_t)N * 32 + (int64_t)32 * Hfc + (int64_t)N * 8) * 4;
}

// the per-sample kernel serves these shapes; the rest takes the single-workgroup kernel
static bool heads_sample_shapes(int H, int Hfc, int OT) {
  return H >= 1 && H <= HS_HMAX && (Hfc == 64 || Hfc == 128) && OT <= 32;
}

static int heads_fill(HeadsParams* pp, const float* h, const float* fc1_w, const float* fc1_b, int nheads,
                      const float* const* heads_w, const float* const* heads_b, const int* head_size, const int* head_kind,
                      const float* head_weight, const float* const* targets, const int64_t* target_stride, float loss_scale,
                      int N, int H, int Hfc, float* preds, float* losses, int backward, float* dh, float* d_fc1_w,
                      float* d_fc1_b, float* const* d_heads_w, float* const* d_heads_b, float* ws,
                      const geeco_loss_shaping* shaping = nullptr, int shaped = 0) {
  GEECO_CHECK_ARG(!shaped || shaping, "heads_loss: shaping is null");
  GEECO_CHECK_ARG(fc1_w && fc1_b && heads_w && heads_b && head_size && head_kind && head_weight && targets &&
                      target_stride && preds && losses && ws, "heads_loss: null pointer");
  GEECO_CHECK_ARG(nheads >= 1 && nheads <= GEECO_MAX_HEADS, "heads_loss: nheads=%d outside 1..%d", nheads, GEECO_MAX_HEADS);
  GEECO_CHECK_ARG(N >= 1 && N <= 4096 && H >= 1 && Hfc >= 1, "heads_loss: bad dims");
  GEECO_CHECK_ARG(!backward || (d_fc1_w && d_fc1_b && d_heads_w && d_heads_b), "heads_loss: null gradient pointer");
  HeadsParams& p = *pp;
  p = HeadsParams{};
  p.h = h; p.fc1_w = fc1_w; p.fc1_b = fc1_b; p.nheads = nheads; p.loss_scale = loss_scale;
  p.N = N; p.H = H; p.Hfc = Hfc; p.backward = backward; p.preds = preds; p.losses = losses;
  p.dh = dh; p.d_fc1_w = d_fc1_w; p.d_fc1_b = d_fc1_b;
  int off = 0;
  for (int i = 0; i < nheads; ++i) {
    GEECO_CHECK_ARG(head_size[i] >= 1 && head_size[i] <= 16, "heads_loss: head %d size %d", i, head_size[i]);
    GEECO_CHECK_ARG(head_kind[i] == 0 || head_kind[i] == 1 || (shaped && head_kind[i] == 2), "heads_loss: head %d kind %d", i,
                    head_kind[i]);
    GEECO_CHECK_ARG(heads_w[i] && heads_b[i] && targets[i], "heads_loss: head %d null pointer", i);
    p.hw[i] = heads_w[i]; p.hb[i] = heads_b[i]; p.tgt[i] = targets[i]; p.tstride[i] = target_stride[i];
    p.size[i] = head_size[i]; p.off[i] = off; p.kind[i] = head_kind[i]; p.weight[i] = head_weight[i];
    off += head_size[i];
    if (backward) {
      GEECO_CHECK_ARG(d_heads_w[i] && d_heads_b[i], "heads_loss: head %d null gradient pointer", i);
      p.dhw[i] = d_heads_w[i]; p.dhb[i] = d_heads_b[i];
    }
  }
  GEECO_CHECK_ARG(off <= 32, "heads_loss: %d outputs > 32", off);
  p.OT = off;
  p.a1 = ws; p.da1 = ws + (long long)N * Hfc; p.dpred = ws + 2ll * N * Hfc;
  p.lterm = ws + 2ll * N * Hfc + (long long)N * 32 + 32ll * Hfc;
  p.cls_head = -1;
  if (!shaped) return 0;
  p.shaped = 1;
  GEECO_CHECK_ARG(shaping->label_smoothing >= 0.f && shaping->label_smoothing < 1.f,
                  "heads_loss: shaping->label_smoothing=%g outside [0, 1)", (double)shaping->label_smoothing);
  GEECO_CHECK_ARG(!shaping->sample_weight || shaping->sample_weight_stride >= 1 || N == 1,
                  "heads_loss: shaping->sample_weight_stride=%lld", (long long)shaping->sample_weight_stride);
  int ncls = 0;
  for (int i = 0; i < nheads; ++i) {
    if (head_kind[i] == 1) {
      if (ncls++ == 0) p.cls_head = i;
    } else if (head_kind[i] == 2) {
      const float d = shaping->huber_delta[i];
      GEECO_CHECK_ARG(d > 0.f && d <= 3.402823466e38f, "heads_loss: shaping->huber_delta[%d]=%g must be finite and > 0", i, (double)d);
      p.huber[i] = d;
    }
  }
  GEECO_CHECK_ARG(!shaping->class_weight || ncls == 1, "heads_loss: shaping->class_weight needs exactly one kind-1 head (%d given)",
                  ncls);
  p.sample_w = shaping->sample_weight; p.sample_w_stride = shaping->sample_weight_stride;
  p.class_w = shaping->class_weight; p.smooth = shaping->label_smoothing;
  if (!p.class_w) p.cls_head = -1;
  return 0;
}

template <bool FUSE, int G, bool SHAPED>
static int launch_heads_sample_g(const HeadsParams& p, const StepFuse& sf, hipStream_t stream) {
  if (int rc = geeco_lds_opt_in<&heads_sample_kernel<FUSE, G, SHAPED>>(HS_LDS_BYTES)) return rc;
  geeco_note_kernel(SHAPED ? "heads_sample_kernel<%s, shaped>" : "heads_sample_kernel<%s>", FUSE ? "true" : "false");
  hipLaunchKernelGGL((heads_sample_kernel<FUSE, G, SHAPED>), dim3((unsigned)p.N), dim3(HS_THREADS), HS_LDS_BYTES, stream, p, sf);
  GEECO_LAUNCH_CHECK();
  return 0;
}

template <bool FUSE>
static int launch_heads_sample(const HeadsParams& p, const StepFuse& sf, hipStream_t stream) {
  if (p.shaped)
    return p.Hfc == 128 ? launch_heads_sample_g<FUSE, 32, true>(p, sf, stream) : launch_heads_sample_g<FUSE, 16, true>(p, sf, stream);
  return p.Hfc == 128 ? launch_heads_sample_g<FUSE, 32, false>(p, sf, stream) : launch_heads_sample_g<FUSE, 16, false>(p, sf, stream);
}

static int heads_loss_impl(const float* h, const float* fc1_w, const float* fc1_b, int nheads, const float* const* heads_w,
                           const float* const* heads_b, const int* head_size, const int* head_kind, const float* head_weight,
                           const float* const* targets, const int64_t* target_stride, float loss_scale, int N, int H, int Hfc,
                           float* preds, float* losses, int backward, float* dh, float* d_fc1_w, float* d_fc1_b,
                           float* const* d_heads_w, float* const* d_heads_b, float* ws, const geeco_loss_shaping* shaping,
                           int shaped, void* stream) {
  GEECO_CHECK_ARG(h && (!backward || dh), "heads_loss: null pointer");
  HeadsParams p;
  if (int rc = heads_fill(&p, h, fc1_w, fc1_b, nheads, heads_w, heads_b, head_size, head_kind, head_weight, targets, target_stride,
                          loss_scale, N, H, Hfc, preds, losses, backward, dh, d_fc1_w, d_fc1_b, d_heads_w, d_heads_b, ws, shaping,
                          shaped))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  if (heads_sample_shapes(H, Hfc, p.OT)) {
    if (int rc = launch_heads_sample<false>(p, StepFuse{}, s)) return rc;
    return launch_heads_finish(p, h, s);
  }
  geeco_note_kernel(shaped ? "heads_loss_kernel<shaped>" : "heads_loss_kernel");
  if (shaped)
    hipLaunchKernelGGL(heads_loss_kernel<true>, dim3(1), dim3(1024), 0, s, p);
  else
    hipLaunchKernelGGL(heads_loss_kernel<false>, dim3(1), dim3(1024), 0, s, p);
  GEECO_LAUNCH_CHECK();
  return 0;
}

extern "C" int geeco_heads_loss_fwd_bwd(const float* h, const float* fc1_w, const float* fc1_b, int nheads,
                                        const float* const* heads_w, const float* const* heads_b,
                                        const int* head_size, const int* head_kind, const float* head_weight,
                                        const float* const* targets, const int64_t* target_stride, float loss_scale,
                                        int N, int H, int Hfc, float* preds, float* losses, int backward, float* dh,
                                        float* d_fc1_w, float* d_fc1_b, float* const* d_heads_w,
                                        float* const* d_heads_b, float* ws, void* stream) {
  return heads_loss_impl(h, fc1_w, fc1_b, nheads, heads_w, heads_b, head_size, head_kind, head_weight, targets, target_stride,
                         loss_scale, N, H, Hfc, preds, losses, backward, dh, d_fc1_w, d_fc1_b, d_heads_w, d_heads_b, ws, nullptr, 0,
                         stream);
}

// geeco_heads_loss_fwd_bwd with tf.losses' optional arguments (head_kind 2 = tf.losses.huber_loss): the same launches, shaped kernels
extern "C" int geeco_heads_loss_shaped_fwd_bwd(const float* h, const float* fc1_w, const float* fc1_b, int nheads,
                                               const float* const* heads_w, const float* const* heads_b,
                                               const int* head_size, const int* head_kind, const float* head_weight,
                                               const float* const* targets, const int64_t* target_stride, float loss_scale,
                                               int N, int H, int Hfc, const geeco_loss_shaping* shaping, float* preds,
                                               float* losses, int backward, float* dh, float* d_fc1_w, float* d_fc1_b,
                                               float* const* d_heads_w, float* const* d_heads_b, float* ws, void* stream) {
  return heads_loss_impl(h, fc1_w, fc1_b, nheads, heads_w, heads_b, head_size, head_kind, head_weight, targets, target_stride,
                         loss_scale, N, H, Hfc, preds, losses, backward, dh, d_fc1_w, d_fc1_b, d_heads_w, d_heads_b, ws, shaping, 1,
                         stream);
}

extern "C" int64_t geeco_loss_shaping_sizeof(void) { return (int64_t)sizeof(geeco_loss_shaping); }

// One-step decoder (zero initial state): gate GEMM, then ONE per-sample launch for the gate math, fc1, the heads, the losses and --
// with `backward` -- everything back to the gate gradients dz.  `pending` non-null: the batch sums of the heads' backward (and
// the loss means) are left for geeco_lstm_step_bwd to run at the end of its second grid; null: heads_finish_kernel runs here.
static int lstm_step_heads_impl(const float* x, int64_t ldx, const float* wx, int64_t ldw, const float* bias, float* z, float* c,
                                float* h, float* gates, int N, int H, int D, void* gemm_ws, const float* fc1_w,
                                const float* fc1_b, int nheads, const float* const* heads_w, const float* const* heads_b,
                                const int* head_size, const int* head_kind, const float* head_weight,
                                const float* const* targets, const int64_t* target_stride, float loss_scale, int Hfc,
                                float* preds, float* losses, int backward, float* dz, float* d_fc1_w, float* d_fc1_b,
                                float* const* d_heads_w, float* const* d_heads_b, float* heads_ws, geeco_heads_finish* pending,
                                const geeco_loss_shaping* shaping, int shaped, void* stream) {
  GEECO_CHECK_ARG(x && wx && bias && z && c && h && gates && (!backward || dz), "lstm_step_heads: null pointer");
  GEECO_CHECK_ARG(N >= 1 && H >= 1 && D >= 1 && ldx >= D && ldw >= 4 * (int64_t)H, "lstm_step_heads: bad dims");
  if (pending) reinterpret_cast<HeadsPending*>(pending)->valid = 0;
  HeadsPending hp;
  if (int rc = heads_fill(&hp.p, h, fc1_w, fc1_b, nheads, heads_w, heads_b, head_size, head_kind, head_weight, targets,
                          target_stride, loss_scale, N, H, Hfc, preds, losses, backward, nullptr, d_fc1_w, d_fc1_b, d_heads_w,
                          d_heads_b, heads_ws, shaping, shaped))
    return rc;
  if (!heads_sample_shapes(H, Hfc, hp.p.OT)) return GEECO_ENOSUP;      // nothing launched: the caller runs the separate entry points
  GemmParams g = {};
  g.A = x; g.B = wx; g.C = z; g.part = (float*)gemm_ws; g.lda = ldx; g.ldb = ldw; g.ldc = 4 * H;
  g.M = N; g.N = 4 * H; g.K = D;
  gemm_plan(g.M, g.N, g.K, &g.S, &g.k_per_split);
  GEECO_CHECK_ARG(g.S == 1 || gemm_ws, "lstm_step_heads: workspace required for split-K (geeco_gemm_ws_bytes(N, 4H, D))");
  hipStream_t s = (hipStream_t)stream;
  geeco_note_kernel("gemm_f32_kernel");
  if (int rc = launch_gemm_f32(g, s)) return rc;
  StepFuse sf = {};
  sf.part = g.S > 1 ? (const float*)g.part : (const float*)z;      // unsplit: the GEMM wrote z itself (one "slab")
  sf.S = g.S; sf.bias = bias; sf.z = z; sf.c = c; sf.hout = h; sf.gates = gates; sf.dz = dz;
  if (int rc = launch_heads_sample<true>(hp.p, sf, s)) return rc;
  if (pending) {
    hp.h = h;
    hp.valid = 1;
    *reinterpret_cast<HeadsPending*>(pending) = hp;
  } else {
    return launch_heads_finish(hp.p, h, s);
  }
  return 0;
}

extern "C" int geeco_lstm_step_heads_fwd_bwd(const float* x, int64_t ldx, const float* wx, int64_t ldw, const float* bias,
                                             float* z, float* c, float* h, float* gates, int N, int H, int D, void* gemm_ws,
                                             const float* fc1_w, const float* fc1_b, int nheads, const float* const* heads_w,
                                             const float* const* heads_b, const int* head_size, const int* head_kind,
                                             const float* head_weight, const float* const* targets,
                                             const int64_t* target_stride, float loss_scale, int Hfc, float* preds,
                                             float* losses, int backward, float* dz, float* d_fc1_w, float* d_fc1_b,
                                             float* const* d_heads_w, float* const* d_heads_b, float* heads_ws,
                                             geeco_heads_finish* pending, void* stream) {
  return lstm_step_heads_impl(x, ldx, wx, ldw, bias, z, c, h, gates, N, H, D, gemm_ws, fc1_w, fc1_b, nheads, heads_w, heads_b,
                              head_size, head_kind, head_weight, targets, target_stride, loss_scale, Hfc, preds, losses, backward,
                              dz, d_fc1_w, d_fc1_b, d_heads_w, d_heads_b, heads_ws, pending, nullptr, 0, stream);
}

// geeco_lstm_step_heads_fwd_bwd with tf.losses' optional arguments: the same launches, the shaped per-sample kernel
extern "C" int geeco_lstm_step_heads_shaped_fwd_bwd(const float* x, int64_t ldx, const float* wx, int64_t ldw, const float* bias,
                                                    float* z, float* c, float* h, float* gates, int N, int H, int D,
                                                    void* gemm_ws, const float* fc1_w, const float* fc1_b, int nheads,
                                                    const float* const* heads_w, const float* const* heads_b,
                                                    const int* head_size, const int* head_kind, const float* head_weight,
                                                    const float* const* targets, const int64_t* target_stride,
                                                    float loss_scale, int Hfc, const geeco_loss_shaping* shaping, float* preds,
                                                    float* losses, int backward, float* dz, float* d_fc1_w, float* d_fc1_b,
                                                    float* const* d_heads_w, float* const* d_heads_b, float* heads_ws,
                                                    geeco_heads_finish* pending, void* stream) {
  return lstm_step_heads_impl(x, ldx, wx, ldw, bias, z, c, h, gates, N, H, D, gemm_ws, fc1_w, fc1_b, nheads, heads_w, heads_b,
                              head_size, head_kind, head_weight, targets, target_stride, loss_scale, Hfc, preds, losses, backward,
                              dz, d_fc1_w, d_fc1_b, d_heads_w, d_heads_b, heads_ws, pending, shaping, 1, stream);
}
