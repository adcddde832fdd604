// Shared-frame training of the per-frame controllers (graph.py: E2EVMC / GoalE2EVMC with shared_frames=F).
//
// A batch of N consecutive K-frame windows of one or two episodes holds far fewer distinct frames than the N * K the dense
// step encodes, and conv_encoder sees one frame at a time: a frame's features are the same in every window that holds it and its
// feature gradient is the sum over those windows.  The step then encodes a table of F frame SLOTS once:
//   1. pack_frames_by_address: the table's resident frames (uint8 or float32 RGB) -> the encoder input x_in [F][HW][4];
//   2. window_states_fwd:      feat [F][cells][ch] + idx [N][K] (+ tgt_idx [N]) -> the decoder's states [K][N][D], ONE launch
//                              (columns: state_layout.h);
//   3. window_states_bwd:      its adjoint, d(states) -> dfeat [F][cells][ch], one block per slot, a fixed summation order.
// All three are HBM streaming (or tiny): 16-byte accesses where the layout allows, one float otherwise.  No atomics.
//
// From frame_ingest.h: u8_unit_div, load_rgb4 (the 4-pixel path of the frame pack) and ld_vec; from state_layout.h: the state
// columns and check_state_layout.
#include "frame_ingest.h"
#include "state_layout.h"

#define SF_THREADS 256
#define SF_MAX_POSITIONS 1024      // N * K of one launch: the backward's per-slot position list lives in LDS

// ---- 1. frame pack by address ---------------------------------------------------------------------------------------------
// blockIdx.y = slot.  A block takes the 4-pixel path when HW % 4 == 0 and ITS frame's address is aligned for it (4 bytes for
// uint8 words, 16 for float4), else one pixel per thread and step; both walk the frame with the same grid.
template <bool U8>
__global__ __launch_bounds__(SF_THREADS) void pack_frames_kernel(const long long* __restrict__ table, long long HW,
                                                                 float* __restrict__ x_in) {
  const int f = blockIdx.y;
  const unsigned long long addr = (unsigned long long)table[f];
  f32x4* o = reinterpret_cast<f32x4*>(x_in + (long long)f * HW * 4);
  const long long step = (long long)gridDim.x * SF_THREADS;
  const long long first = (long long)blockIdx.x * SF_THREADS + threadIdx.x;
  if (addr == 0) {                                   // an unused slot encodes zeros
    for (long long px = first; px < HW; px += step) o[px] = f32x4{0.f, 0.f, 0.f, 0.f};
    return;
  }
  const bool vec = HW % 4 == 0 && (addr & (U8 ? 3u : 15u)) == 0;
  if (vec) {
    for (long long u = first; u < HW / 4; u += step) {
      float px[12];
      if (U8) load_rgb4(reinterpret_cast<const unsigned*>(addr) + u * 3, px);
      else load_rgb4(reinterpret_cast<const f32x4*>(addr) + u * 3, px);
#pragma unroll
      for (int p = 0; p < 4; ++p) o[u * 4 + p] = f32x4{px[p * 3 + 0], px[p * 3 + 1], px[p * 3 + 2], 0.f};
    }
    return;
  }
  for (long long px = first; px < HW; px += step) {
    float e[3];
    if (U8) {
      const unsigned char* s = reinterpret_cast<const unsigned char*>(addr) + px * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) e[c] = u8_unit_div(s[c]);
    } else {
      const float* s = reinterpret_cast<const float*>(addr) + px * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) e[c] = s[c];
    }
    o[px] = f32x4{e[0], e[1], e[2], 0.f};
  }
}

extern "C" int geeco_pack_frames_by_address(const int64_t* table, int F, int frames_u8, int64_t HW, float* x_in, void* stream) {
  GEECO_CHECK_ARG(table && x_in, "pack_frames_by_address: null pointer");
  GEECO_CHECK_ARG(F >= 1 && F <= 65535, "pack_frames_by_address: F=%d outside 1..65535", F);
  GEECO_CHECK_ARG(HW >= 1, "pack_frames_by_address: HW=%lld", (long long)HW);
  GEECO_CHECK_ARG((reinterpret_cast<uintptr_t>(x_in) & 15) == 0, "pack_frames_by_address: x_in must be 16-byte aligned");
  GEECO_CHECK_ARG((reinterpret_cast<uintptr_t>(table) & 7) == 0, "pack_frames_by_address: table must be 8-byte aligned");
  const long long units = HW % 4 == 0 ? HW / 4 : HW;
  dim3 grid((unsigned)cdiv64(units, SF_THREADS), (unsigned)F);
  hipStream_t s = (hipStream_t)stream;
  if (frames_u8) {
    geeco_note_kernel("pack_frames_kernel<true>");
    hipLaunchKernelGGL(pack_frames_kernel<true>, grid, dim3(SF_THREADS), 0, s, (const long long*)table, (long long)HW, x_in);
  } else {
    geeco_note_kernel("pack_frames_kernel<false>");
    hipLaunchKernelGGL(pack_frames_kernel<false>, grid, dim3(SF_THREADS), 0, s, (const long long*)table, (long long)HW, x_in);
  }
  GEECO_LAUNCH_CHECK();
  return 0;
}

// ---- 2. window states, forward -------------------------------------------------------------------------------------------------
// One block per window position (blockIdx.x = n, blockIdx.y = t): states[t][n] <- the features of slot idx[n][t], the joint state
// jnt[n][t] and (goal modes) the features of slot tgt_idx[n].  V = floats per load of the feature rows (4: ch % 4 == 0, 16-byte
// aligned base).  The state rows are stored one float per lane: with J = 7 a cell's columns start at odd offsets.  A slot index
// outside [0, F) (the host never builds one) reads nothing and gives zeros.
template <int V>
__global__ __launch_bounds__(SF_THREADS) void window_states_fwd_kernel(const float* __restrict__ feat, const int* __restrict__ idx,
                                                                       const float* __restrict__ jnt, const int* __restrict__ tgt_idx,
                                                                       int mode, int F, int N, int K, int cells, int ch, int J,
                                                                       float* __restrict__ states, long long state_stride) {
  const int n = blockIdx.x, t = blockIdx.y;
  const int FE = cells * ch;
  const int slot = idx[n * K + t];
  const StateLayout<int> L = state_layout(mode, ch, J);
  const int tslot = mode == GEECO_PREDICT_FEAT_PLAIN ? -1 : tgt_idx[n];
  const float* fs = (unsigned)slot < (unsigned)F ? feat + (long long)slot * FE : nullptr;
  const float* tg = (unsigned)tslot < (unsigned)F ? feat + (long long)tslot * FE : nullptr;
  float* row = states + ((long long)t * N + n) * state_stride;
  const int nq = FE / V;                     // feature units of V floats (ch % V == 0: a unit stays inside one cell)
  for (int q = threadIdx.x; q < nq; q += SF_THREADS) {
    float v[V], g[V];
#pragma unroll
    for (int k = 0; k < V; ++k) v[k] = g[k] = 0.f;
    if (fs) ld_vec<V>(fs + q * V, v);
    if (tg) ld_vec<V>(tg + q * V, g);
    const int cell = (q * V) / ch, c = q * V - cell * ch;
    float* o = row + cell * L.Ctot + c;
    if (mode == GEECO_PREDICT_FEAT_PLAIN) {
#pragma unroll
      for (int k = 0; k < V; ++k) o[k] = v[k];
    } else if (mode == GEECO_PREDICT_FEAT_CONSTANT) {
#pragma unroll
      for (int k = 0; k < V; ++k) {
        o[k] = v[k];
        o[L.jnt_off + J + k] = g[k];      // (= L.tgt_off, without its select)
      }
    } else {
#pragma unroll
      for (int k = 0; k < V; ++k) o[k] = g[k] - v[k];
    }
  }
  const float* jn = jnt + ((long long)n * K + t) * J;
  for (int i = threadIdx.x; i < cells * J; i += SF_THREADS) {
    const int cell = i / J, j = i - cell * J;
    row[cell * L.Ctot + L.jnt_off + j] = jn[j];
  }
}

static int sf_check_states(const char* what, int mode, int F, int N, int K, int cells, int ch, int J, int64_t state_stride) {
  if (int rc = check_state_layout(what, mode, cells, ch, J, state_stride)) return rc;
  GEECO_CHECK_ARG(F >= 1 && F <= 65535, "%s: F=%d outside 1..65535", what, F);
  GEECO_CHECK_ARG(N >= 1 && K >= 1 && K <= 65535 && (int64_t)N * K <= SF_MAX_POSITIONS, "%s: N=%d K=%d (N * K within 1..%d)", what, N, K,
                  SF_MAX_POSITIONS);
  return 0;
}

extern "C" int geeco_window_states_fwd(const float* feat, const int* idx, const float* jnt, const int* tgt_idx, int mode, int F,
                                       int N, int K, int cells, int ch, int J, float* states, int64_t state_stride, void* stream) {
  GEECO_CHECK_ARG(feat && idx && jnt && states, "window_states_fwd: null pointer");
  if (int rc = sf_check_states("window_states_fwd", mode, F, N, K, cells, ch, J, state_stride)) return rc;
  GEECO_CHECK_ARG(mode == GEECO_PREDICT_FEAT_PLAIN || tgt_idx, "window_states_fwd: null pointer (tgt_idx, mode %d)", mode);
  const bool vec = ch % 4 == 0 && (reinterpret_cast<uintptr_t>(feat) & 15) == 0;
  dim3 grid((unsigned)N, (unsigned)K);
  hipStream_t s = (hipStream_t)stream;
  if (vec) {
    geeco_note_kernel("window_states_fwd_kernel<4>");
    hipLaunchKernelGGL(window_states_fwd_kernel<4>, grid, dim3(SF_THREADS), 0, s, feat, idx, jnt, tgt_idx, mode, F, N, K, cells, ch, J,
                       states, (long long)state_stride);
  } else {
    geeco_note_kernel("window_states_fwd_kernel<1>");
    hipLaunchKernelGGL(window_states_fwd_kernel<1>, grid, dim3(SF_THREADS), 0, s, feat, idx, jnt, tgt_idx, mode, F, N, K, cells, ch, J,
                       states, (long long)state_stride);
  }
  GEECO_LAUNCH_CHECK();
  return 0;
}

// ---- 3. window states, backward -------------------------------------------------------------------------------------------------
// One block per slot f.  Its first wave lists the positions e = n * K + t with idx[e] == f, ascending (ballot + prefix count: the
// list order does not depend on timing), and the windows n with tgt_idx[n] == f; every thread then sums its feature unit over the
// list in that order -- window positions first (sign -1 in RESIDUAL: the state holds tgt - feat), then, per target window n, its K
// steps t ascending (columns [ch + J, ..) in CONSTANT, the feature columns in RESIDUAL).  feat: the forward's features; the sum
// is masked by feat > 0, the ReluGrad of the encoder's last layer (what geeco_state_concat_bwd does per term).  A slot nobody
// references gets exact zeros.  (An episode's goal slot sums N * K terms in one block where a frame slot sums at most K: not
// split, its share of the step has not been measured.)
template <int V>
__global__ __launch_bounds__(SF_THREADS) void window_states_bwd_kernel(const float* __restrict__ dstates, long long state_stride,
                                                                       const float* __restrict__ feat, const int* __restrict__ idx,
                                                                       const int* __restrict__ tgt_idx, int mode, int N, int K,
                                                                       int cells, int ch, int J, float* __restrict__ dfeat) {
  __shared__ int s_pos[SF_MAX_POSITIONS];
  __shared__ int s_tgt[SF_MAX_POSITIONS];
  __shared__ int s_cnt[2];
  const int f = blockIdx.x;
  const int NK = N * K;
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    int cnt = 0;
    for (int base = 0; base < NK; base += 64) {
      const int e = base + lane;
      const bool m = e < NK && idx[e] == f;
      const unsigned long long mask = __ballot(m);
      if (m) s_pos[cnt + __popcll(mask & below)] = e;
      cnt += __popcll(mask);
    }
    int tcnt = 0;
    if (mode != GEECO_PREDICT_FEAT_PLAIN) {
      for (int base = 0; base < N; base += 64) {
        const int e = base + lane;
        const bool m = e < N && tgt_idx[e] == f;
        const unsigned long long mask = __ballot(m);
        if (m) s_tgt[tcnt + __popcll(mask & below)] = e;
        tcnt += __popcll(mask);
      }
    }
    if (lane == 0) {
      s_cnt[0] = cnt;
      s_cnt[1] = tcnt;
    }
  }
  __syncthreads();
  const int cnt = s_cnt[0], tcnt = s_cnt[1];
  const int FE = cells * ch;
  const StateLayout<int> L = state_layout(mode, ch, J);
  const int nq = FE / V;
  for (int q = threadIdx.x; q < nq; q += SF_THREADS) {
    const int cell = (q * V) / ch, c = q * V - cell * ch;
    const long long col = (long long)cell * L.Ctot + c;
    float acc[V];
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = 0.f;
    for (int i = 0; i < cnt; ++i) {
      const int e = s_pos[i];
      const int n = e / K, t = e - n * K;
      const float* d = dstates + ((long long)t * N + n) * state_stride + col;
#pragma unroll
      for (int k = 0; k < V; ++k) acc[k] += d[k] * L.feat_sign;
    }
    for (int i = 0; i < tcnt; ++i) {
      const int n = s_tgt[i];
      for (int t = 0; t < K; ++t) {
        const float* d = dstates + ((long long)t * N + n) * state_stride + col + L.tgt_off;
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k] += d[k];
      }
    }
    const long long at = (long long)f * FE + q * V;
    float v[V];
    ld_vec<V>(feat + at, v);
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = v[k] > 0.f ? acc[k] : 0.f;
    if (V == 4) *reinterpret_cast<f32x4*>(dfeat + at) = f32x4{acc[0], acc[1], acc[2], acc[3]};
    else dfeat[at] = acc[0];
  }
}

extern "C" int geeco_window_states_bwd(const float* dstates, int64_t state_stride, const float* feat, const int* idx,
                                       const int* tgt_idx, int mode, int F, int N, int K, int cells, int ch, int J, float* dfeat,
                                       void* stream) {
  GEECO_CHECK_ARG(dstates && feat && idx && dfeat, "window_states_bwd: null pointer");
  if (int rc = sf_check_states("window_states_bwd", mode, F, N, K, cells, ch, J, state_stride)) return rc;
  GEECO_CHECK_ARG(mode == GEECO_PREDICT_FEAT_PLAIN || tgt_idx, "window_states_bwd: null pointer (tgt_idx, mode %d)", mode);
  const uintptr_t al = reinterpret_cast<uintptr_t>(feat) | reinterpret_cast<uintptr_t>(dfeat);
  const bool vec = ch % 4 == 0 && (al & 15) == 0;
  hipStream_t s = (hipStream_t)stream;
  if (vec) {
    geeco_note_kernel("window_states_bwd_kernel<4>");
    hipLaunchKernelGGL(window_states_bwd_kernel<4>, dim3((unsigned)F), dim3(SF_THREADS), 0, s, dstates, (long long)state_stride, feat,
                       idx, tgt_idx, mode, N, K, cells, ch, J, dfeat);
  } else {
    geeco_note_kernel("window_states_bwd_kernel<1>");
    hipLaunchKernelGGL(window_states_bwd_kernel<1>, dim3((unsigned)F), dim3(SF_THREADS), 0, s, dstates, (long long)state_stride, feat,
                       idx, tgt_idx, mode, N, K, cells, ch, J, dfeat);
  }
  GEECO_LAUNCH_CHECK();
  return 0;
}
