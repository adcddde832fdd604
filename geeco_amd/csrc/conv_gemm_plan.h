// Host-side description of a gather-GEMM launch (conv_gemm.hip) in plain C++: the problem the kernel receives, the tile and
// split-K plan, and the grid.  No device code and no HIP type: tests/native/conv_plan_table.cpp compiles this header as a host
// program and holds every launch parameter of a sweep of shapes against a recorded table.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include "geeco_intmath.h"

// One parity class of a launch (forward: a single class with all 9 taps; dgrad of a stride-s conv:
// s*s classes, each with its own subset of taps and its own sub-grid of destination pixels).
struct ConvClass {
  long long M;          // N*Hc*Wc rows
  int Hc, Wc;           // iteration grid: rows enumerate (n, Y', X')
  int oy0, ox0;         // destination pixel = (Y'*ds + oy0, X'*ds + ox0)
  int ntaps;
  int tile0;            // first M-tile (blockIdx.x) of this class
  int dy[9], dx[9], wslab[9];
};

struct ConvGemmParams {
  const float* x;
  const float* w;
  const float* bias;
  const float* mask;
  float* out;
  float* part;          // split-K slabs [ksplit][G][N*Hd*Wd][Nout] (ksplit > 1)
  unsigned long long* stamps;   // -DGEECO_STAMPS builds only: [block][64] s_memtime timeline of thread 0
  long long gs_x, gs_w, gs_b, gs_out;
  int N, Hs, Ws, C;     // source tensor [N][Hs][Ws][C]
  int Hd, Wd, Nout;     // destination tensor [N][Hd][Wd][Nout]
  int ss;               // source pixel = (Y'*ss + dy, X'*ss + dx)
  int ds;
  int relu;
  int ncls;
  int ksplit;           // K-steps are dealt to ksplit blocks (blockIdx.y = ntile * ksplit + split)
  int groups;
  int bt;               // B operand from the HWIO kernel itself ([tap][n][k]: k contiguous) instead of a per-tap transposed copy
  int rot;              // != 0: M tiles per class; the M tile index is rotated by it per 256 blocks (see the kernel)
  ConvClass cls[4];
};

// The top layer's epilogue with the state concat of the one-step decoder in it (graph.py:169-192): besides out[g][n][cell][c]
// the ReLU'd features go to state[n][cell * Ctot + off[g] + c], and the blocks behind the epilogue's copy the joint state into
// every cell's columns [jnt_off, jnt_off + J) -- geeco_state_concat_fwd's values, one dependent launch fewer.
struct StateScatter {
  float* state;
  const float* jnt;
  long long state_stride, jnt_stride;
  int off[4];
  int Ctot, jnt_off, J, cells, epi_blocks;
};

constexpr int GEMM_BK = 16;            // K-step of every tile shape
constexpr int GEMM_ZERO_PAGE = 4096;   // floats: a whole tap of the widest layer the uniform-tap path serves

static inline void fill_fwd(ConvGemmParams* p, int N, int H, int W, int Cin, int Cout, int stride) {
  int Ho, Wo, pt, pl;
  same_pad(H, 3, stride, &Ho, &pt);
  same_pad(W, 3, stride, &Wo, &pl);
  p->N = N; p->Hs = H; p->Ws = W; p->C = Cin;
  p->Hd = Ho; p->Wd = Wo; p->Nout = Cout;
  p->ss = stride; p->ds = 1; p->ncls = 1;
  ConvClass& c = p->cls[0];
  c.Hc = Ho; c.Wc = Wo; c.oy0 = 0; c.ox0 = 0; c.ntaps = 9;
  c.M = (long long)N * Ho * Wo;
  for (int ky = 0; ky < 3; ++ky)
    for (int kx = 0; kx < 3; ++kx) {
      c.dy[ky * 3 + kx] = ky - pt;
      c.dx[ky * 3 + kx] = kx - pl;
      c.wslab[ky * 3 + kx] = ky * 3 + kx;
    }
}

static inline void fill_dgrad(ConvGemmParams* p, int N, int H, int W, int Cin, int Cout, int stride) {
  int Ho, Wo, pt, pl;
  same_pad(H, 3, stride, &Ho, &pt);
  same_pad(W, 3, stride, &Wo, &pl);
  const int s = stride;
  p->N = N; p->Hs = Ho; p->Ws = Wo; p->C = Cout;
  p->Hd = H; p->Wd = W; p->Nout = Cin;
  p->ss = 1; p->ds = s; p->relu = 0;
  int nc = 0;
  for (int py = 0; py < s; ++py)
    for (int px = 0; px < s; ++px) {
      ConvClass c = {};
      c.Hc = (H - py + s - 1) / s;
      c.Wc = (W - px + s - 1) / s;
      c.oy0 = py; c.ox0 = px;
      int nt = 0;
      for (int ky = 0; ky < 3; ++ky) {
        int vy = py + pt - ky;
        if (((vy % s) + s) % s != 0) continue;
        for (int kx = 0; kx < 3; ++kx) {
          int vx = px + pl - kx;
          if (((vx % s) + s) % s != 0) continue;
          c.dy[nt] = (vy >= 0 ? vy : vy - (s - 1)) / s;   // exact (vy % s == 0)
          c.dx[nt] = (vx >= 0 ? vx : vx - (s - 1)) / s;
          c.wslab[nt] = ky * 3 + kx;
          ++nt;
        }
      }
      c.ntaps = nt;
      c.M = (long long)N * c.Hc * c.Wc;
      if (c.M <= 0) continue;
      p->cls[nc++] = c;
    }
  p->ncls = nc;
}

// A forward problem with its operands.
static inline void conv_fwd_problem(ConvGemmParams* p, const float* x, const float* w, const float* b, float* y, int64_t gs_x,
                                    int64_t gs_w, int64_t gs_b, int64_t gs_y, int N, int H, int W, int Cin, int Cout, int stride,
                                    int relu) {
  fill_fwd(p, N, H, W, Cin, Cout, stride);
  p->x = x; p->w = w; p->bias = b; p->mask = nullptr; p->out = y;
  p->gs_x = gs_x; p->gs_w = gs_w; p->gs_b = gs_b; p->gs_out = gs_y;
  p->relu = relu;
}

// The gather GEMM reads the HWIO kernel itself (transposing it on the way into LDS) where its K-steps stay inside one
// tap: Cout a multiple of 16 that fits the zero page.  Only the remaining shapes need the per-tap transposed copy.
static inline bool dgrad_reads_hwio(int Cout) {
  return Cout % 16 == 0 && Cout <= GEMM_ZERO_PAGE;
}

// An input-gradient problem with its operands: the HWIO kernel w (bt = 1) where the kernel can read it, else the per-tap
// transposed copy wt.  p->w is left NULL when the shape needs a copy that was not given.
static inline void conv_dgrad_problem(ConvGemmParams* p, const float* dz, const float* w, const float* wt, const float* ymask,
                                      float* dx, int64_t gs_dz, int64_t gs_w, int64_t gs_wt, int64_t gs_dx, int N, int H, int W,
                                      int Cin, int Cout, int stride) {
  fill_dgrad(p, N, H, W, Cin, Cout, stride);
  p->x = dz; p->w = wt; p->bias = nullptr; p->mask = ymask; p->out = dx;
  p->gs_x = gs_dz; p->gs_w = gs_wt; p->gs_b = 0; p->gs_out = gs_dx;
  if (w && dgrad_reads_hwio(Cout)) {
    p->w = w; p->gs_w = gs_w; p->bt = 1;
  }
}

// The kernel divides row indices in 32 bits: the row count of the first class that does not fit (0: all fit).
static inline long long conv_rows_beyond_32bit(const ConvGemmParams& p) {
  for (int c = 0; c < p.ncls; ++c)
    if (p.cls[c].M + 256 >= (1ll << 31)) return p.cls[c].M;
  return 0;
}

struct ConvPlan {
  int bm, bn, ksplit;
};

// Tile choice and split-K factor.  Split only when the launch cannot fill the chip (tiny-M layers
// conv6..8 and their dgrads): blocks < 256 CUs and enough K-steps to share.
static inline ConvPlan conv_plan(const ConvGemmParams& p, int groups) {
  ConvPlan pl;
  long long Mtot = 0;
  int maxtaps = 0;
  for (int c = 0; c < p.ncls; ++c) {
    Mtot += p.cls[c].M;
    if (p.cls[c].ntaps > maxtaps) maxtaps = p.cls[c].ntaps;
  }
  pl.bn = (p.Nout % 64 == 0) ? 64 : (p.Nout % 48 == 0) ? 48 : (p.Nout % 32 == 0) ? 32 : 16;
  pl.bm = 128;
  if (pl.bn == 64 && Mtot * groups < 128 * 256) pl.bm = 64;
  // 128-wide N tiles halve the gathered A bytes per MFMA; only when they still fill the chip
  // (round 1: neutral to slower; since the kernel's VALU diet of round 2 the gathered bytes weigh more: -11 us per step)
  if (p.Nout % 128 == 0 && pl.bm == 128 && (Mtot / 128) * (p.Nout / 128) * groups >= 512) pl.bn = 128;
  // 96-wide N tiles where they (and not the 64-wide ones) make the block count a whole multiple of the CUs
  // (conv5 forward: 768 blocks instead of 1152 = 4.5 per CU: -10 us)
  if (pl.bn == 64 && pl.bm == 64 && p.Nout % 96 == 0 && p.ncls == 1 &&
      (cdiv64(Mtot, 64) * (p.Nout / 96) * groups) % 256 == 0 && (cdiv64(Mtot, 64) * (p.Nout / 64) * groups) % 256 != 0)
    pl.bn = 96;
  long long blocks = 0;
  for (int c = 0; c < p.ncls; ++c) blocks += cdiv64(p.cls[c].M, pl.bm);
  blocks *= (long long)cdiv(p.Nout, pl.bn) * groups;
  const int nk = cdiv(maxtaps * p.C, GEMM_BK);
  pl.ksplit = 1;
  if (blocks < 640 && nk >= 16) {   // fewer than 2.5 blocks per CU: long serial K loops and a ragged tail
    long long want = cdiv64(1024, blocks);
    long long maxs = nk / 8;   // at least 8 K-steps per block
    if (want > maxs) want = maxs;
    // prefer the factor nearest to that which makes the block count a whole multiple of the 256 CUs: all blocks are
    // co-resident and dealt evenly (scripts/dev/ub/placement.hip), so a ragged count leaves some CUs with one block
    // more than the others for the whole launch (conv6 forward: 3 -> 2 splits, 768 blocks, -4 us)
    long long best = 0;
    for (long long k = 2; k <= maxs; ++k)
      if ((blocks * k) % 256 == 0 && blocks * k <= 2048 && (best == 0 || llabs(k - want) < llabs(best - want))) best = k;
    if (best) want = best;
    if (want > 1) pl.ksplit = (int)want;
  }
  return pl;
}

static inline int64_t conv_ws_bytes(const ConvGemmParams& p, int groups) {
  ConvPlan pl = conv_plan(p, groups);
  if (pl.ksplit <= 1) return 0;
  return (int64_t)pl.ksplit * groups * p.N * p.Hd * p.Wd * p.Nout * 4;
}

// UT ("uniform tap"): C % BK == 0, so every K-step lies inside ONE tap (see the kernel), and a tap fits the zero page.
struct ConvGemmGrid {
  int gx, gy, gz;       // M tiles of all classes, N tiles x K splits, encoders
  bool ut;
};

// The grid of a launch with BM x BN tiles (p.ksplit is set): assigns every class its first M tile and the class rotation.
static inline ConvGemmGrid conv_gemm_grid(ConvGemmParams& p, int BM, int BN, int groups) {
  int tiles = 0;
  for (int c = 0; c < p.ncls; ++c) {
    p.cls[c].tile0 = tiles;
    tiles += (int)cdiv64(p.cls[c].M, BM);
  }
  bool equal = p.ncls > 1;                    // rotation by whole classes needs equally many tiles per class
  for (int c = 1; c < p.ncls; ++c) equal = equal && cdiv64(p.cls[c].M, BM) == cdiv64(p.cls[0].M, BM);
  p.rot = equal ? tiles / p.ncls : 0;
  ConvGemmGrid g;
  g.gx = tiles; g.gy = cdiv(p.Nout, BN) * p.ksplit; g.gz = groups;
  g.ut = p.C % GEMM_BK == 0 && p.C <= GEMM_ZERO_PAGE;
  return g;
}
