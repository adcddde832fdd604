// Episode replay (geeco_amd/replay.py, replay_dynimg.py): what a controller would have commanded at every
// frame of a recorded episode, and how far that is from what was recorded.  The T frames are encoded once each (the encoder
// stacks, fed by shared_frames.hip or by the image stage of replay_dynimg.hip); what is here is
//   1. the window states: per-frame tables [T][cells][cw] + jnt [T][J] -> the decoder's states [K][N][D] of the windows
//                     t0 .. t1 - 1, slot k of window t showing frame max(0, t - K + 1 + k) (the predictor's window after a reset
//                     at frame 0 and t pushes, predictor.py:192-200).  ONE kernel behind both entry points:
//                     replay_states       one table and a constant target row, the columns of state_layout.h;
//                     replay_states_pair  two tables, per cell [feat (ch) | jnt (J) | tgt (ch_t)]: what the dense 'sequence' x
//                                         'dyndiff' model's concat writes (state_concat_fwd with jnt_pos = 1; graph.py:146-167
//                                         of the reference: tf.concat([feat, jnt, tgt_feat]));
//   2. replay_errors: preds [T][P] against the recorded values -> per frame and head the mean squared error (regression heads) or
//                     the hit of the gripper class (logit heads), and their means over the episode in one fixed order.
// The first is a pure HBM gather (every feature row is read up to K times, from L2 after the first), grid-stride with 16-byte
// accesses where the layout allows; the second is tiny.  No atomics.
//
// From replay_internal.h: RP_THREADS, RP_MAX_BLOCKS, RP_MAXK and check_replay_windows (shared with replay_dynimg.hip); from
// frame_ingest.h: ld_vec; from state_layout.h: the state columns and check_state_layout.
#include "replay_internal.h"
#include "frame_ingest.h"
#include "state_layout.h"

// ---- 1. window states ----------------------------------------------------------------------------------------------------------
// What the kernel reads by value: where every column of a cell comes from.
enum { RP_TGT_NONE = 0, RP_TGT_APPEND = 1, RP_TGT_RESIDUAL = 2 };
struct ReplayTable {
  const float* src;      // [T][cells][cw], indexed by the frame a slot shows; null: no such table
  int cw, c0;            // its width and its first column within a cell
};
struct ReplayStatesDesc {
  ReplayTable tab[2];
  int jnt_off;           // first joint-state column of a cell
  int Ctot;              // columns of one cell
  const float* tgt;      // [cells][tab[0].cw], constant over the episode; goes with table 0
  int tgt_op;            // RP_TGT_NONE; _APPEND: copied to the columns from tgt_c0; _RESIDUAL: the table's columns hold tgt - feat
  int tgt_c0;
};

// A unit = V floats of one table row (cw % V == 0: a unit stays inside one cell); units are numbered (k, window, q) with q
// fastest, so a wave reads and writes consecutive addresses; the tables one after the other.  V = 4: 16-byte loads; VS: 16-byte
// stores as well (J % 4 == 0 and state_stride % 4 == 0, so every table's columns start at a multiple of 4 floats).  The
// joint-state columns follow in a second loop of the same grid, one float per lane.
template <int V, bool VS>
__global__ __launch_bounds__(RP_THREADS) void replay_states_kernel(const ReplayStatesDesc d, const float* __restrict__ jnt, int t0,
                                                                  int n, int N, int K, int cells, int J, float* __restrict__ states,
                                                                  long long state_stride) {
  const long long step = (long long)gridDim.x * RP_THREADS;
  const long long first = (long long)blockIdx.x * RP_THREADS + threadIdx.x;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const float* __restrict__ src = d.tab[s].src;
    if (!src) break;
    const int cw = d.tab[s].cw, c0 = d.tab[s].c0;
    const int op = s == 0 ? d.tgt_op : RP_TGT_NONE;
    const int FE = cells * cw, nq = FE / V;
    const long long units = (long long)K * n * nq;
    for (long long u = first; u < units; u += step) {
      const int q = (int)(u % nq);
      const long long r = u / nq;                  // = k * n + w
      const int w = (int)(r % n), k = (int)(r / n);
      int f = t0 + w - K + 1 + k;                  // the frame slot k of window t0 + w shows
      if (f < 0) f = 0;                            // first-frame padding after the reset at frame 0
      float v[V];
      ld_vec<V>(src + (long long)f * FE + q * V, v);
      const int cell = (q * V) / cw, c = q * V - cell * cw;
      float* o = states + ((long long)k * N + w) * state_stride + cell * d.Ctot + c0 + c;
      if (op != RP_TGT_NONE) {
        float g[V];
        ld_vec<V>(d.tgt + q * V, g);
        if (op == RP_TGT_APPEND) {
          float* og = o + (d.tgt_c0 - c0);
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
    states[((long long)k * N + w) * state_stride + cell * d.Ctot + d.jnt_off + j] = jnt[(long long)f * J + j];
  }
}

// The one launch behind both entry points (arguments checked by the caller).  16-byte loads when EVERY table's width is a
// multiple of 4 and every source is 16-byte aligned -- a mixed case takes the scalar form as a whole --, 16-byte stores when J,
// the row pitch and states allow them as well; the grid covers the longest of the kernel's loops.
static int launch_replay_states(const ReplayStatesDesc& d, const float* jnt, int t0, int n, int N, int K, int cells, int J,
                                float* states, int64_t state_stride, hipStream_t s) {
  uintptr_t src = reinterpret_cast<uintptr_t>(d.tgt);
  int widths = 0, widest = 0;
  for (const ReplayTable& t : d.tab) {
    if (!t.src) continue;
    src |= reinterpret_cast<uintptr_t>(t.src);
    widths |= t.cw;
    widest = std::max(widest, t.cw);
  }
  const bool vec = widths % 4 == 0 && (src & 15) == 0;
  const bool vst = vec && J % 4 == 0 && state_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(states) & 15) == 0;
  const long long per = std::max<long long>(cells * widest / (vec ? 4 : 1), (long long)cells * J);
  const unsigned grid = (unsigned)std::min<long long>(cdiv64((long long)K * n * per, RP_THREADS), RP_MAX_BLOCKS);
#define RP_LAUNCH(V, VS)                                                                                                        \
  do {                                                                                                                          \
    geeco_note_kernel("replay_states_kernel<%d, %s>", V, VS ? "true" : "false");                                              \
    hipLaunchKernelGGL((replay_states_kernel<V, VS>), dim3(grid), dim3(RP_THREADS), 0, s, d, jnt, t0, n, N, K, cells, J, states, \
                       (long long)state_stride);                                                                                \
  } while (0)
  if (vst) RP_LAUNCH(4, true);
  else if (vec) RP_LAUNCH(4, false);
  else RP_LAUNCH(1, false);
#undef RP_LAUNCH
  GEECO_LAUNCH_CHECK();
  return 0;
}

extern "C" int geeco_replay_states(const float* feat, const float* jnt, const float* tgt_feat, int mode, int T, int t0, int t1,
                                   int N, int K, int cells, int ch, int J, float* states, int64_t state_stride, void* stream) {
  GEECO_CHECK_ARG(feat && jnt && states, "replay_states: null pointer");
  if (int rc = check_state_layout("replay_states", mode, cells, ch, J, state_stride)) return rc;
  GEECO_CHECK_ARG(mode == GEECO_PREDICT_FEAT_PLAIN || tgt_feat, "replay_states: null pointer (tgt_feat, mode %d)", mode);
  if (int rc = check_replay_windows("replay_states", T, t0, t1, N, K)) return rc;
  const StateLayout<int> L = state_layout(mode, ch, J);
  ReplayStatesDesc d = {};
  d.tab[0] = {feat, ch, 0};
  d.jnt_off = L.jnt_off;
  d.Ctot = L.Ctot;
  if (mode != GEECO_PREDICT_FEAT_PLAIN) {
    d.tgt = tgt_feat;
    d.tgt_op = mode == GEECO_PREDICT_FEAT_CONSTANT ? RP_TGT_APPEND : RP_TGT_RESIDUAL;
    d.tgt_c0 = L.tgt_off;
  }
  return launch_replay_states(d, jnt, t0, t1 - t0, N, K, cells, J, states, state_stride, (hipStream_t)stream);
}

extern "C" int geeco_replay_states_pair(const float* feat, const float* tgt_feat, const float* jnt, int T, int t0, int t1, int N,
                                        int K, int cells, int ch, int ch_t, int J, float* states, int64_t state_stride,
                                        void* stream) {
  GEECO_CHECK_ARG(feat && tgt_feat && jnt && states, "replay_states_pair: null pointer");
  GEECO_CHECK_ARG(cells >= 1 && ch >= 1 && ch_t >= 1 && J >= 1 && (int64_t)cells * ch <= (1 << 24) && (int64_t)cells * ch_t <= (1 << 24) &&
                      J <= (1 << 24),
                  "replay_states_pair: cells=%d ch=%d ch_t=%d J=%d", cells, ch, ch_t, J);
  GEECO_CHECK_ARG(state_stride >= (int64_t)cells * ((int64_t)ch + J + ch_t), "replay_states_pair: state_stride=%lld below cells * %lld columns",
                  (long long)state_stride, (long long)ch + J + ch_t);
  if (int rc = check_replay_windows("replay_states_pair", T, t0, t1, N, K)) return rc;
  ReplayStatesDesc d = {};
  d.tab[0] = {feat, ch, 0};
  d.tab[1] = {tgt_feat, ch_t, ch + J};
  d.jnt_off = ch;
  d.Ctot = ch + J + ch_t;
  return launch_replay_states(d, jnt, t0, t1 - t0, N, K, cells, J, states, state_stride, (hipStream_t)stream);
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
