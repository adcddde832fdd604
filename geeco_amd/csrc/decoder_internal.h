// Policy head: state concat, LSTM cell (MFMA gate GEMM + fused gate math), fc1 + heads + losses (decoder_*.hip).
//
// Replaces reference src/models/e2evmc/graph.py:123-192 (concats), :198-260 (lstm_decoder),
// :452-500 (losses) and the loss composition of src/models/e2evmc/estimator.py:206-239.
//
// Internal (non-ABI): the structs and device helpers more than one of the decoder files uses, and the host functions they call
// across translation units.  The file that defines one and every file that calls it include this header, so a signature that
// drifts is a compile error instead of a link error; a kernel is launched only from the file that defines it.
#pragma once
#include "geeco_common.h"

// ---- state concat (decoder_concat.hip) -----------------------------------------------------------------------------------
struct ConcatParams {
  const float* feats[3];
  float* dfeats[3];
  int ch[3];
  int off[3];       // channel offset of feature i inside a cell
  int nfeat, jnt_off, J, Ctot;
  const float* jnt;
  long long jnt_stride;
  const float* sub_from;
  int N, cells;
  float* state;
  long long state_stride;
  int accumulate;
  float scale;
};

// the scatter of one element of d(state) into the encoders' feature gradients: concat_bwd_kernel's work as a gemm_block store
struct ConcatScatter {
  const ConcatParams& c;
  __device__ __forceinline__ void operator()(int n, int d, float v) const {
    const int cell = d / c.Ctot, ch = d - cell * c.Ctot;
    if (cell >= c.cells || (ch >= c.jnt_off && ch < c.jnt_off + c.J)) return;
    int f = 0;
#pragma unroll
    for (int k = 1; k < 3; ++k)
      if (k < c.nfeat && ch >= c.off[k]) f = k;
    if (!c.dfeats[f]) return;
    const long long i = ((long long)n * c.cells + cell) * c.ch[f] + (ch - c.off[f]);
    c.dfeats[f][i] = c.feats[f][i] > 0.f ? v * c.scale : 0.f;       // ReluGrad of the encoder's last layer
  }
};

// fills the channel layout of p (ch, off, jnt_off, J, nfeat, Ctot); returns Ctot
int fill_concat(ConcatParams* p, const int* feat_ch, int nfeat, int jnt_pos, int J);

// ---- dense f32 GEMM (decoder_gemm.hip) -----------------------------------------------------------------------------------
struct GemmParams {
  const float* A;
  const float* B;
  float* C;
  float* part;
  long long lda, ldb, ldc;
  int M, N, K, ta, tb, accumulate, S, k_per_split;
};

constexpr int GEMM_LD = 80, GEMM_BK = 16;   // LD = 16 (mod 32): conflict-free ds_read_b32

// One 64 x 64 tile (bx = N tile, by = M tile, bz = K split) of C = op(A) op(B).  `store(gm, gn, value)` is called for
// every element of an unsplit product (S == 1) after C has been written: the one-launch LSTM backward hangs the
// state-concat scatter on it.
template <class Store>
__device__ __forceinline__ void gemm_block(const GemmParams& p, int bx, int by, int bz, float (*sA)[GEMM_BK * GEMM_LD],
                                           float (*sB)[GEMM_BK * GEMM_LD], Store store) {
  constexpr int BMg = 64, BNg = 64, BKg = GEMM_BK, LD = GEMM_LD;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int m0 = by * BMg, n0 = bx * BNg;
  const int kbeg = bz * p.k_per_split;
  int kend = kbeg + p.k_per_split;
  if (kend > p.K) kend = p.K;
  const int r = lane & 15, q = lane >> 4;
  const int wm = (wid & 1) * 32, wn = (wid >> 1) * 32;

  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  float ra[4], rb[4];
  // element e = tid + 256*i of a 16 x 64 tile.  For row-major-in-k sources (A not transposed, B
  // transposed) consecutive threads walk k; otherwise they walk m/n, which keeps loads coalesced.
  auto load_tiles = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int e = tid + 256 * i;
      int kk, mm;
      if (!p.ta) { kk = e & 15; mm = e >> 4; } else { mm = e & 63; kk = e >> 6; }
      int gk = k0 + kk, gm = m0 + mm;
      bool v = gk < kend && gm < p.M;
      ra[i] = v ? (p.ta ? p.A[(long long)gk * p.lda + gm] : p.A[(long long)gm * p.lda + gk]) : 0.f;
      int kb, nn;
      if (p.tb) { kb = e & 15; nn = e >> 4; } else { nn = e & 63; kb = e >> 6; }
      int gkb = k0 + kb, gn = n0 + nn;
      bool vb = gkb < kend && gn < p.N;
      rb[i] = vb ? (p.tb ? p.B[(long long)gn * p.ldb + gkb] : p.B[(long long)gkb * p.ldb + gn]) : 0.f;
    }
  };
  auto store_tiles = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int e = tid + 256 * i;
      int kk, mm;
      if (!p.ta) { kk = e & 15; mm = e >> 4; } else { mm = e & 63; kk = e >> 6; }
      sA[buf][kk * LD + mm] = ra[i];
      int kb, nn;
      if (p.tb) { kb = e & 15; nn = e >> 4; } else { nn = e & 63; kb = e >> 6; }
      sB[buf][kb * LD + nn] = rb[i];
    }
  };

  const int nk = kend > kbeg ? (kend - kbeg + BKg - 1) / BKg : 0;
  if (nk > 0) {
    load_tiles(kbeg);
    store_tiles(0);
  }
  __syncthreads();
  for (int ks = 0; ks < nk; ++ks) {
    const int buf = ks & 1;
    const bool more = ks + 1 < nk;
    if (more) load_tiles(kbeg + (ks + 1) * BKg);
#pragma unroll
    for (int blk = 0; blk < 4; ++blk) {
      float av[2], bv[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) av[i] = sA[buf][(blk * 4 + q) * LD + wm + i * 16 + r];
#pragma unroll
      for (int j = 0; j < 2; ++j) bv[j] = sB[buf][(blk * 4 + q) * LD + wn + j * 16 + r];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
    }
    if (more) store_tiles(buf ^ 1);
    __syncthreads();
  }
  // D[i = m][j = n]: lane holds n = lane & 15, m = 4 (lane >> 4) + reg
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int gn = n0 + wn + j * 16 + r;
      if (gn >= p.N) continue;
      const float e[4] = {acc[i][j].x, acc[i][j].y, acc[i][j].z, acc[i][j].w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int gm = m0 + wm + i * 16 + 4 * q + k;
        if (gm >= p.M) continue;
        if (p.S == 1) {
          float* c = p.C + (long long)gm * p.ldc + gn;
          const float v = p.accumulate ? *c + e[k] : e[k];
          *c = v;
          store(gm, gn, v);
        } else {
          p.part[((long long)bz * p.M + gm) * p.N + gn] = e[k];
        }
      }
    }
}

struct NoStore {
  __device__ __forceinline__ void operator()(int, int, float) const {}
};

// split-K plan of an M x N x K product: S slabs of k_per_split
void gemm_plan(int M, int N, int K, int* S, int* kps);
// gemm_f32_kernel over the tiles and slabs of p; with p.S > 1 the slabs land in p.part and their sum is the caller's
int launch_gemm_f32(const GemmParams& p, hipStream_t s);

// ---- LSTM gate math (decoder_lstm.hip, decoder_heads.hip, decoder_seq.hip) ---------------------------------------------------
__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// ---- fc1 + heads + losses (decoder_heads.hip, decoder_step_bwd.hip, decoder_seq.hip) -----------------------------------------
#define GEECO_MAX_HEADS 5
struct HeadsParams {
  const float* h;
  const float* fc1_w;
  const float* fc1_b;
  const float* hw[GEECO_MAX_HEADS];
  const float* hb[GEECO_MAX_HEADS];
  const float* tgt[GEECO_MAX_HEADS];
  long long tstride[GEECO_MAX_HEADS];
  int size[GEECO_MAX_HEADS], off[GEECO_MAX_HEADS], kind[GEECO_MAX_HEADS];
  float weight[GEECO_MAX_HEADS];
  int nheads, OT;
  float loss_scale;
  int N, H, Hfc, backward;
  float* preds;
  float* losses;
  float* dh;
  float* d_fc1_w;
  float* d_fc1_b;
  float* dhw[GEECO_MAX_HEADS];
  float* dhb[GEECO_MAX_HEADS];
  float* a1;    // ws: [N][Hfc]
  float* da1;   // ws: [N][Hfc]
  float* dpred; // ws: [N][OT]  (the single-workgroup kernel keeps its packed head matrix behind it: [N * OT ...)
  float* lterm; // ws: [N][8] per-sample loss terms of every head (per-sample kernel -> finish role)
  // ---- loss shaping (tf.losses' weights= / label_smoothing= / huber_loss(delta=)); all optional, read only where shaped != 0 ----
  int shaped;              // the shaped entry points: kind 2 heads allowed, means over the non-zero weights
  int cls_head;            // the kind-1 head class_w belongs to (-1: none)
  const float* sample_w;   // [N] at sample_w[n * sample_w_stride], or null (every weight 1)
  long long sample_w_stride;
  const float* class_w;    // device table [size of head cls_head], or null
  float smooth;            // label_smoothing of the kind-1 heads
  float huber[GEECO_MAX_HEADS];      // delta of the kind-2 heads
};

// slots of a sample's lterm row behind the (<= 5) loss terms: the batch's counts of non-zero effective weights, as every
// workgroup of the shaped per-sample kernel forms them (identical in every row; the finish role reads row 0)
constexpr int HS_CNT_REG = 5, HS_CNT_CLS = 6;

template <class T>
__device__ __forceinline__ T sel5(T const (&a)[GEECO_MAX_HEADS], int i) {
  return i == 0 ? a[0] : (i == 1 ? a[1] : (i == 2 ? a[2] : (i == 3 ? a[3] : a[4])));
}

constexpr int HS_THREADS = 1024, HS_HMAX = 128, HS_FMAX = 128;

// ---- loss shaping: what the shaped P3 of both heads kernels shares ----------------------------------------------------------
// effective weight of sample n for the regression heads
__device__ __forceinline__ float shaped_sample_w(const HeadsParams& p, int n) {
  return p.sample_w ? p.sample_w[(long long)n * p.sample_w_stride] : 1.f;
}
// ... and for the kind-1 head that carries the class table: sample weight x class_weight[label] (an out-of-range label: 0)
__device__ __forceinline__ float shaped_class_w(const HeadsParams& p, float sw, float target) {
  const int label = (int)rintf(target) + 1;
  return sw * ((label >= 0 && label < sel5(p.size, p.cls_head)) ? p.class_w[label] : 0.f);
}

// The two integer counts of non-zero effective weights over the whole batch (x: regression heads and kind-1 heads without the
// class table, y: the head with the class table), formed by ONE workgroup of NT threads from the N <= 4096 weights and labels
// (L2-resident): integer adds through a wave reduction and `s_cnt` ([NT / 64][2] ints of LDS).  Every thread must call this; the
// result is valid in every thread.  Contains two barriers.
template <int NT>
__device__ __forceinline__ void shaped_counts(const HeadsParams& p, int (*s_cnt)[2], int* cnt_reg, int* cnt_cls) {
  if (!p.sample_w && !p.class_w) {      // uniform
    *cnt_reg = p.N;
    *cnt_cls = p.N;
    return;
  }
  const int tid = threadIdx.x;
  int c0 = 0, c1 = 0;
  for (int m = tid; m < p.N; m += NT) {
    const float sw = shaped_sample_w(p, m);
    c0 += sw != 0.f;
    if (p.class_w) c1 += shaped_class_w(p, sw, sel5(p.tgt, p.cls_head)[(long long)m * sel5(p.tstride, p.cls_head)]) != 0.f;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    c0 += __shfl_xor(c0, o, 64);
    c1 += __shfl_xor(c1, o, 64);
  }
  if ((tid & 63) == 0) {
    s_cnt[tid >> 6][0] = c0;
    s_cnt[tid >> 6][1] = c1;
  }
  __syncthreads();
  c0 = 0;
  c1 = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    c0 += s_cnt[w][0];
    c1 += s_cnt[w][1];
  }
  __syncthreads();
  *cnt_reg = c0;
  *cnt_cls = p.class_w ? c1 : c0;
}

// One head of one sample, shaped (TF 1.15 tf.losses with reduction SUM_BY_NONZERO_WEIGHTS): returns w * sum_c l_c and writes
// d(loss)/d(pred) of the head's `sz` outputs to dp.  pr / tg / dp: the head's predictions, targets and gradient slots; w: the
// sample's effective weight for this head; cnt: the batch's count of non-zero effective weights for this head.  With w == 1,
// cnt == N, smooth == 0 and kind != 2 every product below is by 1.0f or a sum with 0.0f: bitwise the unshaped arithmetic.
__device__ __forceinline__ float shaped_head_terms(const HeadsParams& p, int hd, const float* pr, const float* tg, float* dp,
                                                   float w, int cnt) {
  const int sz = sel5(p.size, hd), kind = sel5(p.kind, hd);
  const float wsc = sel5(p.weight, hd) * p.loss_scale;
  float l = 0.f;
  if (cnt == 0 || w == 0.f) {      // a zero weight contributes exact zeros (and no non-zero weight at all: tf.div_no_nan gives 0)
    for (int c = 0; c < sz; ++c) dp[c] = 0.f;
    return 0.f;
  }
  if (kind == 0) {
    const float c2 = 2.f / (float)(cnt * sz) * wsc;
    for (int c = 0; c < sz; ++c) {
      const float d = pr[c] - tg[c];
      l += d * d;
      dp[c] = d * c2 * w;
    }
  } else if (kind == 2) {          // tf.losses.huber_loss: 0.5 q^2 + delta (a - q), q = min(a, delta)
    const float dl = sel5(p.huber, hd);
    const float c1 = 1.f / (float)(cnt * sz) * wsc;
    for (int c = 0; c < sz; ++c) {
      const float d = pr[c] - tg[c];
      const float a = fabsf(d), q = fminf(a, dl);
      l += 0.5f * q * q + dl * (a - q);
      dp[c] = (a <= dl ? d : copysignf(dl, d)) * c1 * w;
    }
  } else {                         // softmax cross-entropy against one_hot * (1 - smooth) + smooth / C
    const int label = (int)rintf(tg[0]) + 1;             // estimator.py:213-215
    float mx = pr[0];
    for (int c = 1; c < sz; ++c) mx = fmaxf(mx, pr[c]);
    float se = 0.f;
    for (int c = 0; c < sz; ++c) se += expf(pr[c] - mx);
    const float lo = p.smooth / (float)sz, hi = 1.f * (1.f - p.smooth) + lo;      // one_hot of an out-of-range label is all-zero
    float ysum = 0.f;
    for (int c = 0; c < sz; ++c) {
      const float y = c == label ? hi : lo;
      ysum += y;
      if (y != 0.f) l += y * (mx + logf(se) - pr[c]);
    }
    const float invc = 1.f / cnt;
    for (int c = 0; c < sz; ++c) dp[c] = (expf(pr[c] - mx) / se * ysum - (c == label ? hi : lo)) * invc * wsc * w;
  }
  return l * w;
}

__device__ __forceinline__ int heads_head_of(const HeadsParams& p, int o) {
  int hd = 0;
#pragma unroll
  for (int k = 1; k < GEECO_MAX_HEADS; ++k)
    if (k < p.nheads && o >= p.off[k]) hd = k;
  return hd;
}

struct HeadsPending {       // what geeco_heads_finish (include/geeco_hip.h) holds
  HeadsParams p;
  const float* h;
  int valid;
};
static_assert(sizeof(HeadsPending) <= sizeof(geeco_heads_finish), "geeco_heads_finish is too small for HeadsPending");

// heads_finish_kernel: the batch sums behind heads_sample_kernel (decoder_step_bwd.hip)
int launch_heads_finish(const HeadsParams& p, const float* h, hipStream_t s);
