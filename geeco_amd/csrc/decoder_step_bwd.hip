// =====================================================================================================
// what sums over the batch behind heads_sample_kernel (decoder_heads.hip), and the one-step LSTM backward that carries it
// =====================================================================================================
#include "decoder_internal.h"

// ---- what sums over the batch: role blocks of 256 threads ---------------------------------------------------------------
// blocks [0, nW): rows of d(fc1/kernel) = h^T d(a1), 256 / G rows each; blocks [nW, nW + nWh): the head kernels' gradients, 256
// elements each; the last block: the bias gradients and the loss means.  Forward only: just the loss means (one block).
__host__ __device__ __forceinline__ int heads_finish_blocks(int H, int F, int OT, int backward) {
  return backward ? (H + 256 / (F >> 2) - 1) / (256 / (F >> 2)) + (F * OT + 255) / 256 + 1 : 1;
}

constexpr int HF_NC = 32;      // samples staged per chunk

// `lds`: HF_LDS_FLOATS floats of shared memory lent by the calling kernel (the GEMM tile buffers of lstm_step_bwd_heads_kernel: a
// block of that grid must not need more LDS than a tile block, or fewer of them fit on a CU)
constexpr int HF_LDS_FLOATS = HF_NC * HS_FMAX + HF_NC * 32;

__device__ __forceinline__ void heads_finish_role(const HeadsParams& p, const float* h, int role, float* lds) {
  const int tid = threadIdx.x;
  const int N = p.N, H = p.H, F = p.Hfc, OT = p.OT;
  const int G = F >> 2, R = 256 / G;
  const int nW = (H + R - 1) / R;
  // Operands come through LDS in chunks of HF_NC samples, fetched with independent coalesced loads (all in flight at once): a
  // thread that walks n with dependent global loads pays a memory latency per sample (the first form of these roles: 36 us).
  float* sA = lds;                             // a chunk of d(a1) or a1: [n][F]
  float* sB = lds + HF_NC * HS_FMAX;           // a chunk of h rows [n][R] or of dpred [n][OT]
  // (rows past the chunk's end are zero-filled and every loop below runs all HF_NC rows: constant trip counts, so the LDS reads of
  // consecutive samples are issued together instead of one latency per sample)
  auto stage = [&](const float* src, int n0, int nc) {                    // [nc][F] floats (F % 4 == 0, rows contiguous)
    const f32x4* s4 = reinterpret_cast<const f32x4*>(src + (long long)n0 * F);
    for (int e = tid; e < HF_NC * G; e += 256) reinterpret_cast<f32x4*>(sA)[e] = e < nc * G ? s4[e] : f32x4{0.f, 0.f, 0.f, 0.f};
  };
  if (p.backward && role < nW) {            // d(fc1/kernel)[hh][4g..] = sum_n h[n][hh] d(a1)[n][4g..]
    const int r = tid / G, g = tid - r * G, hh = role * R + r;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int n0 = 0; n0 < N; n0 += HF_NC) {
      const int nc = N - n0 < HF_NC ? N - n0 : HF_NC;
      if (n0) __syncthreads();
      stage(p.da1, n0, nc);
      for (int e = tid; e < HF_NC * R; e += 256) {
        const int nn = e / R, rr = e - nn * R;
        sB[e] = (nn < nc && role * R + rr < H) ? h[(long long)(n0 + nn) * H + role * R + rr] : 0.f;
      }
      __syncthreads();
#pragma unroll 8
      for (int nn = 0; nn < HF_NC; ++nn) acc += sB[nn * R + r] * reinterpret_cast<const f32x4*>(sA + nn * F)[g];
    }
    if (hh < H) reinterpret_cast<f32x4*>(p.d_fc1_w + (long long)hh * F)[g] = acc;
    return;
  }
  const int nWh = (F * OT + 255) / 256;
  if (p.backward && role < nW + nWh) {      // head kernel gradients [f][c] = sum_n a1[n][f] dpred[n][o], one element per thread
    const int e = (role - nW) * 256 + tid;
    const bool live = e < F * OT;
    const int f = live ? e / OT : 0, o = live ? e - f * OT : 0;
    float acc = 0.f;
    for (int n0 = 0; n0 < N; n0 += HF_NC) {
      const int nc = N - n0 < HF_NC ? N - n0 : HF_NC;
      if (n0) __syncthreads();
      stage(p.a1, n0, nc);
      for (int i = tid; i < HF_NC * OT; i += 256) sB[i] = i < nc * OT ? p.dpred[(long long)n0 * OT + i] : 0.f;
      __syncthreads();
#pragma unroll 8
      for (int nn = 0; nn < HF_NC; ++nn) acc += sA[nn * F + f] * sB[nn * OT + o];
    }
    if (live) {
      const int hd = heads_head_of(p, o);
      sel5(p.dhw, hd)[(long long)f * sel5(p.size, hd) + (o - sel5(p.off, hd))] = acc;
    }
    return;
  }
  // bias gradients and loss means
  float accb = 0.f, acco = 0.f, accl = 0.f;      // thread f < F: d(fc1/bias)[f]; thread o < OT: d(head bias)[o]; thread hd: loss sum
  for (int n0 = 0; n0 < N; n0 += HF_NC) {
    const int nc = N - n0 < HF_NC ? N - n0 : HF_NC;
    if (n0) __syncthreads();
    if (p.backward) {
      stage(p.da1, n0, nc);
      for (int e = tid; e < HF_NC * OT; e += 256) sB[e] = e < nc * OT ? p.dpred[(long long)n0 * OT + e] : 0.f;
    }
    __shared__ float sL[HF_NC * 8];
    for (int e = tid; e < HF_NC * 8; e += 256) sL[e] = (e < nc * 8 && (e & 7) < p.nheads) ? p.lterm[(long long)n0 * 8 + e] : 0.f;
    __syncthreads();
    if (p.backward) {
      if (tid < F) {
#pragma unroll 8
        for (int nn = 0; nn < HF_NC; ++nn) accb += sA[nn * F + tid];
      }
      if (tid < OT) {
#pragma unroll 8
        for (int nn = 0; nn < HF_NC; ++nn) acco += sB[nn * OT + tid];
      }
    }
    if (tid < p.nheads) {
#pragma unroll 8
      for (int nn = 0; nn < HF_NC; ++nn) accl += sL[nn * 8 + tid];
    }
  }
  if (p.backward) {
    if (tid < F) p.d_fc1_b[tid] = accb;
    if (tid < OT) {
      const int hd = heads_head_of(p, tid);
      sel5(p.dhb, hd)[tid - sel5(p.off, hd)] = acco;
    }
  }
  __shared__ float s_l[GEECO_MAX_HEADS];
  if (tid < p.nheads) {
    float mean = sel5(p.kind, tid) == 0 ? 1.f / (float)(N * sel5(p.size, tid)) : 1.f / N;
    if (p.shaped) {      // means over the non-zero effective weights: the counts heads_sample_kernel<.., SHAPED> left in row 0 of lterm
      const int cnt = (int)p.lterm[(p.class_w && tid == p.cls_head) ? HS_CNT_CLS : HS_CNT_REG];
      mean = cnt == 0 ? 0.f : (sel5(p.kind, tid) == 1 ? 1.f / cnt : 1.f / (float)(cnt * sel5(p.size, tid)));
    }
    const float sum = accl * mean;
    p.losses[1 + tid] = sum;
    s_l[tid] = sum;
  }
  __syncthreads();
  if (tid == 0) {
    float total = 0.f;
    for (int hd = 0; hd < p.nheads; ++hd) total += sel5(p.weight, hd) * s_l[hd];
    p.losses[0] = total;
  }
}

__global__ __launch_bounds__(256) void heads_finish_kernel(const HeadsParams p, const float* h) {
  __shared__ __attribute__((aligned(16))) float lds[HF_LDS_FLOATS];
  heads_finish_role(p, h, (int)blockIdx.x, lds);      // (forward only: one block, which falls through to the loss means)
}

int launch_heads_finish(const HeadsParams& p, const float* h, hipStream_t s) {
  geeco_note_kernel("heads_finish_kernel");
  hipLaunchKernelGGL(heads_finish_kernel, dim3((unsigned)heads_finish_blocks(p.H, p.Hfc, p.OT, p.backward)), dim3(256), 0, s, p, h);
  GEECO_LAUNCH_CHECK();
  return 0;
}

// ---- one LSTM step's weight / input gradients in ONE launch --------------------------------------------------------
// With one LSTM step (the goal model's dynimg branch: graph.py:405-407) everything after the gate gradients dz depends
// on dz alone: dWx = X^T dz, db = column sums of dz, dX = dz Wx^T, and the scatter of dX into the encoders' feature
// gradients (state concat backward + ReluGrad of conv8).  As separate launches that is gemm, colsum, gemm + split-K
// reduce, concat_bwd = five dependent kernel boundaries of ~4.5 us each for ~0.2 GFLOP; here they are the blocks of one
// two grids: (1) [0, nA) tiles of dWx, [nA, nA + nB) split-K tiles of dX (slabs; a K loop of this latency-bound GEMM costs
// ~0.7 us per 16-deep step, so the 512-deep product keeps its 8-way split: unsplit it measured +22 us on the step), the
// rest the bias column sums; (2) the slab sum of dX with the feature-gradient scatter in its epilogue.
struct LstmBwdBatch {
  GemmParams a, b;          // a: dWx (S == 1), b: dX (split-K into b.part)
  int nA, nB, ax, bx, by;   // block counts and tile counts of the two products
  const float* dz; long long ldz; int Mz, Nz; float* db;       // column sums
  ConcatParams cc;          // scatter of dX (cc.dfeats[i] may be null); cc.nfeat == 0: no scatter
};

__device__ __forceinline__ void lstm_step_bwd_body(const LstmBwdBatch& q, int blk, float (*sA)[GEMM_BK * GEMM_LD],
                                                   float (*sB)[GEMM_BK * GEMM_LD]) {
  if (blk < q.nA) {
    gemm_block(q.a, blk % q.ax, blk / q.ax, 0, sA, sB, NoStore());
  } else if (blk < q.nA + q.nB) {
    const int l = blk - q.nA, t = l % (q.bx * q.by);
    if (q.b.S == 1 && q.cc.nfeat > 0)
      gemm_block(q.b, t % q.bx, t / q.bx, l / (q.bx * q.by), sA, sB, ConcatScatter{q.cc});
    else
      gemm_block(q.b, t % q.bx, t / q.bx, l / (q.bx * q.by), sA, sB, NoStore());
  } else {
    const int j = (blk - q.nA - q.nB) * 256 + threadIdx.x;
    if (j >= q.Nz) return;
    float s = 0.f;
    for (int i = 0; i < q.Mz; ++i) s += q.dz[(long long)i * q.ldz + j];     // row order, as geeco_colsum
    q.db[j] = s;
  }
}

__global__ __launch_bounds__(256) void lstm_step_bwd_kernel(const LstmBwdBatch q) {
  __shared__ float sA[2][GEMM_BK * GEMM_LD];
  __shared__ float sB[2][GEMM_BK * GEMM_LD];
  lstm_step_bwd_body(q, (int)blockIdx.x, sA, sB);
}

// slab sum of dX (fixed slab order, as gemm_reduce_kernel) + the state-concat scatter of the sums
__device__ __forceinline__ void lstm_step_bwd_finish_body(const LstmBwdBatch& q, int block) {
  const long long i = (long long)block * 256 + threadIdx.x;
  const long long MN = (long long)q.b.M * q.b.N;
  if (i >= MN) return;
  float s = 0.f;
  const float* src = q.b.part + i;
  int k = 0;
  for (; k + 8 <= q.b.S; k += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = src[(long long)(k + u) * MN];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  for (; k < q.b.S; ++k) s += src[(long long)k * MN];
  const int m = (int)(i / q.b.N), n = (int)(i - (long long)m * q.b.N);
  q.b.C[(long long)m * q.b.ldc + n] = s;
  if (q.cc.nfeat > 0) ConcatScatter{q.cc}(m, n, s);
}

__global__ __launch_bounds__(256) void lstm_step_bwd_finish_kernel(const LstmBwdBatch q) {
  lstm_step_bwd_finish_body(q, (int)blockIdx.x);
}

extern "C" int64_t geeco_lstm_step_bwd_ws_bytes(int N, int D, int H4) { return geeco_gemm_ws_bytes(N, D, H4); }

// Grid 1 of geeco_lstm_step_bwd with the heads' pending batch sums as its FIRST blocks: a handful of independent ~5 us blocks
// beside the tiles of dWx / dX (13 us), in a launch that exists anyway (at the end of the SECOND grid, whose blocks take ~1 us,
// they set that launch's length: measured 15.7 instead of 5.0 us).
__global__ __launch_bounds__(256) void lstm_step_bwd_heads_kernel(const LstmBwdBatch q, const HeadsParams hp, const float* h, int hb) {
  static_assert(4 * GEMM_BK * GEMM_LD >= HF_LDS_FLOATS, "the finish roles borrow the tile buffers");
  __shared__ __attribute__((aligned(16))) float tiles[4][GEMM_BK * GEMM_LD];      // sA[2], sB[2]
  if ((int)blockIdx.x < hb)
    heads_finish_role(hp, h, (int)blockIdx.x, &tiles[0][0]);
  else
    lstm_step_bwd_body(q, (int)blockIdx.x - hb, &tiles[0], &tiles[2]);
}

extern "C" int geeco_lstm_step_bwd(const float* x, int64_t ldx, const float* dz, int64_t ldz, const float* wx, int64_t ldw,
                                   float* dwx, int64_t lddw, float* db, float* dx, int64_t lddx, int N, int D, int H4,
                                   const float* const* feats_fwd, float* const* dfeats, const int* feat_ch, int nfeat,
                                   int jnt_pos, int J, int cells, void* ws, const geeco_heads_finish* pending, void* stream) {
  GEECO_CHECK_ARG(x && dz && wx && dwx && db && dx, "lstm_step_bwd: null pointer");
  GEECO_CHECK_ARG(N >= 1 && D >= 1 && H4 >= 1, "lstm_step_bwd: bad dims");
  GEECO_CHECK_ARG(nfeat >= 0 && nfeat <= 3 && (nfeat == 0 || (feats_fwd && dfeats && feat_ch && jnt_pos >= 0 && jnt_pos <= nfeat)),
                  "lstm_step_bwd: concat description");
  LstmBwdBatch q = {};
  // dWx [D][4H] = X^T dz: A = X [N][D] transposed, B = dz [N][4H]
  q.a.A = x; q.a.lda = ldx; q.a.ta = 1; q.a.B = dz; q.a.ldb = ldz; q.a.tb = 0; q.a.C = dwx; q.a.ldc = lddw;
  q.a.M = D; q.a.N = H4; q.a.K = N; q.a.S = 1; q.a.k_per_split = cdiv(N, 16) * 16;
  // dX [N][D] = dz Wx^T: A = dz [N][4H], B = Wx [D][4H] transposed
  q.b.A = dz; q.b.lda = ldz; q.b.ta = 0; q.b.B = wx; q.b.ldb = ldw; q.b.tb = 1; q.b.C = dx; q.b.ldc = lddx;
  q.b.M = N; q.b.N = D; q.b.K = H4; q.b.part = (float*)ws;
  gemm_plan(N, D, H4, &q.b.S, &q.b.k_per_split);
  GEECO_CHECK_ARG(q.b.S == 1 || ws, "lstm_step_bwd: workspace required (geeco_lstm_step_bwd_ws_bytes)");
  q.ax = cdiv(H4, 64); q.nA = q.ax * cdiv(D, 64);
  q.bx = cdiv(D, 64); q.by = cdiv(N, 64); q.nB = q.bx * q.by * q.b.S;
  q.dz = dz; q.ldz = ldz; q.Mz = N; q.Nz = H4; q.db = db;
  if (nfeat > 0) {
    const int ctot = fill_concat(&q.cc, feat_ch, nfeat, jnt_pos, J);
    GEECO_CHECK_ARG((int64_t)cells * ctot <= D, "lstm_step_bwd: %d cells x %d channels exceed the state width %d", cells, ctot, D);
    q.cc.N = N; q.cc.cells = cells; q.cc.scale = 1.f;
    for (int i = 0; i < nfeat; ++i) {
      GEECO_CHECK_ARG(!dfeats[i] || feats_fwd[i], "lstm_step_bwd: feats_fwd[%d] is null", i);
      q.cc.feats[i] = feats_fwd[i];
      q.cc.dfeats[i] = dfeats[i];
    }
  }
  const int blocks = q.nA + q.nB + cdiv(H4, 256);
  const HeadsPending* hp = reinterpret_cast<const HeadsPending*>(pending);
  if (hp && hp->valid) {
    const int hb = heads_finish_blocks(hp->p.H, hp->p.Hfc, hp->p.OT, hp->p.backward);
    geeco_note_kernel("lstm_step_bwd_heads_kernel");
    hipLaunchKernelGGL(lstm_step_bwd_heads_kernel, dim3((unsigned)(hb + blocks)), dim3(256), 0, (hipStream_t)stream, q, hp->p, hp->h, hb);
  } else {
    hipLaunchKernelGGL(lstm_step_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, q);
  }
  GEECO_LAUNCH_CHECK();
  if (q.b.S > 1) {
    hipLaunchKernelGGL(lstm_step_bwd_finish_kernel, dim3((unsigned)cdiv64((long long)N * D, 256)), dim3(256), 0,
                       (hipStream_t)stream, q);
    GEECO_LAUNCH_CHECK();
  }
  return 0;
}
