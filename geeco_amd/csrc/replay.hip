// Episode replay (geeco_amd/replay.py): what a per-frame controller would have commanded at every frame of a
// recorded episode, and how far that is from what was recorded.  The T frames are encoded once each (frame pack by address +
// the encoder stack, shared_frames.hip / encoder.py); what is here is
//   1. replay_states: feat [T][cells][ch] + jnt [T][J] (+ tgt_feat [cells][ch]) -> the decoder's states [K][N][D] of the windows
//                     t0 .. t1 - 1, slot k of window t showing frame max(0, t - K + 1 + k) (the predictor's window after a reset
//                     at frame 0 and t pushes, predictor.py:192-200); columns: state_layout.h;
//   2. replay_errors: preds [T][P] against the recorded values -> per frame and head the mean squared error (regression heads) or
//                     the hit of the gripper class (logit heads), and their means over the episode in one fixed order.
// The first is a pure HBM gather (every feature row is read up to K times, from L2 after the first), grid-stride with 16-byte
// accesses where the layout allows; the second is tiny.  No atomics.
//
// From frame_ingest.h: ld_vec; from state_layout.h: the state columns and check_state_layout.
#include "dynimg_internal.h"      // DYN_MAXK
#include "frame_ingest.h"
#include "state_layout.h"

#define RP_THREADS 256
#define RP_MAXK DYN_MAXK          // the window lengths the predictors take
#define RP_MAX_BLOCKS 2048        // 8 blocks of 256 threads per CU: the grid-stride loop takes the rest

// ---- 1. window states ----------------------------------------------------------------------------------------------------------
// A unit = V floats of one feature row (ch % V == 0: a unit stays inside one cell); units are numbered (k, window, q) with q
// fastest, so a wave reads and writes consecutive addresses.  V = 4: 16-byte loads; VS: 16-byte stores as well (J % 4 == 0 and
// state_stride % 4 == 0, so every cell's columns start at a multiple of 4 floats).  The joint-state columns follow in a second
// loop of the same grid, one float per lane.
template <int V, bool VS>
__global__ __launch_bounds__(RP_THREADS) void replay_states_kernel(const float* __restrict__ feat, const float* __restrict__ jnt,
                                                                  const float* __restrict__ tgt, int mode, int t0, int n, int N,
                                                                  int K, int cells, int ch, int J, float* __restrict__ states,
                                                                  long long state_stride) {
  const int FE = cells * ch;
  const StateLayout<int> L = state_layout(mode, ch, J);
  const int nq = FE / V;
  const long long step = (long long)gridDim.x * RP_THREADS;
  const long long first = (long long)blockIdx.x * RP_THREADS + threadIdx.x;
  const long long units = (long long)K * n * nq;
  for (long long u = first; u < units; u += step) {
    const int q = (int)(u % nq);
    const long long r = u / nq;                  // = k * n + w
    const int w = (int)(r % n), k = (int)(r / n);
    int f = t0 + w - K + 1 + k;                  // the frame slot k of window t0 + w shows
    if (f < 0) f = 0;                            // first-frame padding after the reset at frame 0
    float v[V];
    ld_vec<V>(feat + (long long)f * FE + q * V, v);
    const int cell = (q * V) / ch, c = q * V - cell * ch;
    float* o = states + ((long long)k * N + w) * state_stride + cell * L.Ctot + c;
    if (mode != GEECO_PREDICT_FEAT_PLAIN) {
      float g[V];
      ld_vec<V>(tgt + q * V, g);
      if (mode == GEECO_PREDICT_FEAT_CONSTANT) {
        float* og = o + L.jnt_off + J;           // (= L.tgt_off, without its select)
        if (VS) {
          *reinterpret_cast<f32x4*>(og) = f32x4{g[0], g[1], g[2], g[3]};
        } else {
#pragma unroll
          for (int i = 0; i < V; ++i) og[i] = g[i];
        }
      } else {
#pragma unroll
        for (int i = 0; i < V; ++i) v[i] = g[i] - v[i];
      }
    }
    if (VS) {
      *reinterpret_cast<f32x4*>(o) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
      for (int i = 0; i < V; ++i) o[i] = v[i];
    }
  }
  const int CJ = cells * J;
  const long long junits = (long long)K * n * CJ;
  for (long long u = first; u < junits; u += step) {
    const int i = (int)(u % CJ);
    const long long r = u / CJ;
    const int w = (int)(r % n), k = (int)(r / n);
    int f = t0 + w - K + 1 + k;
    if (f < 0) f = 0;
    const int cell = i / J, j = i - cell * J;
    states[((long long)k * N + w) * state_stride + cell * L.Ctot + L.jnt_off + j] = jnt[(long long)f * J + j];
  }
}

extern "C" int geeco_replay_states(const float* feat, const float* jnt, const float* tgt_feat, int mode, int T, int t0, int t1,
                                   int N, int K, int cells, int ch, int J, float* states, int64_t state_stride, void* stream) {
  GEECO_CHECK_ARG(feat && jnt && states, "replay_states: null pointer");
  if (int rc = check_state_layout("replay_states", mode, cells, ch, J, state_stride)) return rc;
  GEECO_CHECK_ARG(mode == GEECO_PREDICT_FEAT_PLAIN || tgt_feat, "replay_states: null pointer (tgt_feat, mode %d)", mode);
  GEECO_CHECK_ARG(K >= 1 && K <= RP_MAXK, "replay_states: K=%d outside 1..%d", K, RP_MAXK);
  GEECO_CHECK_ARG(T >= 1 && t0 >= 0 && t0 < t1 && t1 <= T, "replay_states: windows [%d, %d) outside the %d frames", t0, t1, T);
  GEECO_CHECK_ARG(N >= t1 - t0, "replay_states: N=%d rows per step for %d windows", N, t1 - t0);
  const int n = t1 - t0;
  const uintptr_t src = reinterpret_cast<uintptr_t>(feat) | reinterpret_cast<uintptr_t>(tgt_feat);
  const bool vec = ch % 4 == 0 && (src & 15) == 0;
  const bool vst = vec && J % 4 == 0 && state_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(states) & 15) == 0;
  const long long units = std::max<long long>((long long)K * n * (cells * ch / (vec ? 4 : 1)), (long long)K * n * cells * J);
  const unsigned grid = (unsigned)std::min<long long>(cdiv64(units, RP_THREADS), RP_MAX_BLOCKS);
  hipStream_t s = (hipStream_t)stream;
#define RP_LAUNCH(V, VS)                                                                                                        \
  do {                                                                                                                          \
    geeco_note_kernel("replay_states_kernel<%d, %s>", V, VS ? "true" : "false");                                              \
    hipLaunchKernelGGL((replay_states_kernel<V, VS>), dim3(grid), dim3(RP_THREADS), 0, s, feat, jnt, tgt_feat, mode, t0, n, N, K, \
                       cells, ch, J, states, (long long)state_stride);                                                          \
  } while (0)
  if (vst) RP_LAUNCH(4, true);
  else if (vec) RP_LAUNCH(4, false);
  else RP_LAUNCH(1, false);
#undef RP_LAUNCH
  GEECO_LAUNCH_CHECK();
  return 0;
}

// ---- 2. errors -------------------------------------------------------------------------------------------------------------------
struct ReplayHeads {
  int off[GEECO_REPLAY_MAXHEADS], size[GEECO_REPLAY_MAXHEADS], kind[GEECO_REPLAY_MAXHEADS];
  int n;
};

// one thread per (frame, head).  Regression head: sum_c (p - l)^2 with c ascending, the difference, the product and every sum
// rounded to float32 on their own (no fused multiply-add: the order in the header is the order here), then / size.  Logit head:
// the first maximum; a NaN logit makes the frame's value NaN.
__global__ __launch_bounds__(RP_THREADS) void replay_errors_frame_kernel(const float* __restrict__ preds, const float* __restrict__ labels,
                                                                        long long T, int P, ReplayHeads hd, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * RP_THREADS + threadIdx.x;
  if (i >= T * hd.n) return;
  const long long t = i / hd.n;
  const int h = (int)(i - t * hd.n);
  const float* p = preds + t * P + hd.off[h];
  const float* l = labels + t * P + hd.off[h];
  const int size = hd.size[h];
  float r;
  if (hd.kind[h] == 0) {
    float s = 0.f;
    for (int c = 0; c < size; ++c) {
      const float d = __fsub_rn(p[c], l[c]);
      s = __fadd_rn(s, __fmul_rn(d, d));
    }
    r = __fdiv_rn(s, (float)size);
  } else {
    int best = 0;
    float bv = p[0];
    bool nan = bv != bv;
    for (int c = 1; c < size; ++c) {
      const float v = p[c];
      nan = nan || v != v;
      if (v > bv) {
        bv = v;
        best = c;
      }
    }
    r = nan ? __builtin_nanf("") : ((float)best == l[0] ? 1.f : 0.f);
  }
  out[i] = r;
}

// ONE block: thread i adds the frames i, i + 256, .. ascending; the partial sums are folded by halves; / T
__global__ __launch_bounds__(RP_THREADS) void replay_errors_episode_kernel(const float* __restrict__ frame, long long T, int nheads,
                                                                          float* __restrict__ out) {
  __shared__ float sm[RP_THREADS];
  for (int h = 0; h < nheads; ++h) {
    float s = 0.f;
    for (long long t = threadIdx.x; t < T; t += RP_THREADS) s = __fadd_rn(s, frame[t * nheads + h]);
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int half = RP_THREADS / 2; half > 0; half >>= 1) {
      if ((int)threadIdx.x < half) sm[threadIdx.x] = __fadd_rn(sm[threadIdx.x], sm[threadIdx.x + half]);
      __syncthreads();
    }
    if (threadIdx.x == 0) out[h] = __fdiv_rn(sm[0], (float)T);
    __syncthreads();
  }
}

extern "C" int geeco_replay_errors(const float* preds, const float* labels, int T, int P, int nheads, const int* head_off,
                                   const int* head_size, const int* head_kind, float* out_frame, float* out_episode, void* stream) {
  GEECO_CHECK_ARG(preds && labels && head_off && head_size && head_kind && out_frame && out_episode, "replay_errors: null pointer");
  GEECO_CHECK_ARG(T >= 1 && P >= 1, "replay_errors: T=%d P=%d", T, P);
  GEECO_CHECK_ARG(nheads >= 1 && nheads <= GEECO_REPLAY_MAXHEADS, "replay_errors: nheads=%d outside 1..%d", nheads,
                  GEECO_REPLAY_MAXHEADS);
  ReplayHeads hd;
  hd.n = nheads;
  for (int h = 0; h < nheads; ++h) {
    GEECO_CHECK_ARG(head_size[h] >= 1 && head_size[h] <= 64 && head_off[h] >= 0 && head_off[h] + head_size[h] <= P,
                    "replay_errors: head %d [%d, +%d) outside the %d prediction columns (1..64 columns per head)", h, head_off[h],
                    head_size[h], P);
    GEECO_CHECK_ARG(head_kind[h] == 0 || head_kind[h] == 1, "replay_errors: head %d kind=%d must be 0 (squared error) or 1 (class hit)",
                    h, head_kind[h]);
    hd.off[h] = head_off[h];
    hd.size[h] = head_size[h];
    hd.kind[h] = head_kind[h];
  }
  hipStream_t s = (hipStream_t)stream;
  geeco_note_kernel("replay_errors_frame_kernel");
  hipLaunchKernelGGL(replay_errors_frame_kernel, dim3((unsigned)cdiv64((long long)T * nheads, RP_THREADS)), dim3(RP_THREADS), 0, s,
                     preds, labels, (long long)T, P, hd, out_frame);
  GEECO_LAUNCH_CHECK();
  geeco_note_kernel("replay_errors_episode_kernel");
  hipLaunchKernelGGL(replay_errors_episode_kernel, dim3(1), dim3(RP_THREADS), 0, s, (const float*)out_frame, (long long)T, nheads,
                     out_episode);
  GEECO_LAUNCH_CHECK();
  return 0;
}
