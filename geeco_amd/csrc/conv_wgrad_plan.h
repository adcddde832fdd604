// Host-side description of a filter-gradient launch (geeco_conv3x3_wgrad: conv_wgrad.hip, conv_wgrad_halo.hip,
// conv_halo_s2_bwd.hip, conv_halo_conv1.hip) in plain C++: which kernel family serves a shape, that family's tile, slice and
// slab plan, and which slab-sum kernel follows.  No device code and no HIP type: tests/native/conv_wgrad_cover.cpp compiles this
// header as a host program and holds the plan of every case of tests/native/conv_wgrad_cases.txt against the text recorded there.
// The .hip files include it and keep no second copy of anything below.
#pragma once
#include <stdint.h>
#include "geeco_intmath.h"

// ---- the families, in the order geeco_conv3x3_wgrad asks them -----------------------------------------------------------
enum WgradFamily {
  WGRAD_FAMILY_HALO = 0,     // conv2 type (32 -> 48, stride 2, even sizes): conv_s2_halo_wgrad_kernel, persistent blocks
  WGRAD_FAMILY_CONV1 = 1,    // conv1 (4 -> 32, stride 1): conv1_halo_wgrad_kernel
  WGRAD_FAMILY_LDS = 2,      // the stride-2 middle layers: conv_s2_wgrad_lds_kernel, six instantiations
  WGRAD_FAMILY_GENERIC = 3,  // everything else: conv_wgrad_kernel, four tiles
};

// ---- generic kernel: BR x BC tile of dw per block, the pixels dealt to S slices of m_per_split ---------------------------
struct WgradTilePlan {
  int BR, BC, MK;
  int Ho, Wo, pt, pl;
  long long M;               // N * Ho * Wo
  int Krows;                 // 9 * Cin
  int row_tiles, col_tiles;
  int S;                     // S == 1: the kernel writes dw / db itself, no slab and no slab sum
  long long m_per_split;     // pixels per slice, a multiple of every MK (the last slice may be ragged)
};

static inline WgradTilePlan wgrad_tile_plan(int groups, int N, int H, int W, int Cin, int Cout, int stride) {
  WgradTilePlan t = {};
  same_pad(H, 3, stride, &t.Ho, &t.pt);
  same_pad(W, 3, stride, &t.Wo, &t.pl);
  t.M = (long long)N * t.Ho * t.Wo;
  t.Krows = 9 * Cin;
  // 64-row tiles and at most 64 columns: 128-row / 128-column tiles halve the dz traffic per MFMA but measured on MI355X
  // ~1.5 % of the step slower (occupancy beats traffic here)
  t.BR = 64;
  t.BC = (Cout % 64 == 0) ? 64 : (Cout % 48 == 0) ? 48 : (Cout % 32 == 0) ? 32 : 16;
  t.MK = t.BC >= 48 ? 32 : 64;
  t.row_tiles = cdiv(t.Krows, t.BR);
  t.col_tiles = cdiv(Cout, t.BC);
  long long tiles = (long long)groups * t.row_tiles * t.col_tiles;
  long long S = 1024 / tiles;
  if (S < 1) S = 1;
  long long maxS = t.M / 512;          // at least 512 pixels per slice
  if (maxS < 1) maxS = 1;
  if (S > maxS) S = maxS;
  long long mps = cdiv64(t.M, S);
  mps = cdiv64(mps, 64) * 64;   // multiple of every MK
  S = cdiv64(t.M, mps);
  t.S = (int)S;
  t.m_per_split = mps;
  return t;
}

// ---- LDS-staged kernel of the stride-2 middle layers (conv_wgrad_halo.hip) ----------------------------------------------
struct WgradHaloPlan {
  int variant;       // 0 = not handled; 1 = CIB 48 (conv3 type), TW 16; 4 = CIB 48, TW 8; 2 = CIB 64, TW 16; 3 = CIB 64, TW 8;
                     // 5 = CIB 32 x COB 128, TW 8; 6 = CIB 64 x COB 96, TW 8
  int TH, TW, n_cib, n_cob, S;
  long long tiles;   // TH x TW tiles per group
  int n_sigma;       // groups * n_cib * S slices, dealt round-robin to the XCDs
  int blocks;        // 8 * cdiv(n_sigma, 8) * n_cob: the blocks past n_sigma's slices leave at once
};

static inline WgradHaloPlan wgrad_halo_plan(int groups, int N, int H, int W, int Cin, int Cout, int stride) {
  WgradHaloPlan pl = {};
  if (stride != 2 || (H & 1) || (W & 1) || Cout % 64 != 0) return pl;
  const int Ho = H / 2, Wo = W / 2;
  if (Wo < 8 || Ho < 2) return pl;                        // the tiny top layers stay with the gather kernel
  // tile shape: 2 x 16 or 4 x 8 output pixels (same LDS); the squarer one has 7 % less halo ((9 x 17) / (8 x 16) = 1.20
  // input pixels fetched per input pixel used, against (5 x 33) / (4 x 32) = 1.29)
  // (measured, bench shapes: conv3 209.8 -> 203.5 us, conv4 142.3 -> 139.0, conv5 116.5 -> 113.9)
  const bool wide = Wo >= 16 && Ho < 4;
  if (Cin == 48 && Wo >= 16) {
    pl.variant = wide ? 1 : 4; pl.TH = wide ? 2 : 4; pl.TW = wide ? 16 : 8; pl.n_cib = 1;
  } else if (Cin % 64 == 0) {
    pl.variant = wide ? 2 : 3;
    pl.TH = wide ? 2 : 4; pl.TW = wide ? 16 : 8;
    pl.n_cib = Cin / 64;
  } else {
    return pl;
  }
  pl.n_cob = Cout / 64;
  const long long tiles = (long long)N * cdiv(Ho, pl.TH) * cdiv(Wo, pl.TW);
  if (tiles >= (1ll << 30) || (long long)H * W * Cin >= (1ll << 31) || (long long)Ho * Wo * Cout >= (1ll << 31)) {
    pl.variant = 0;                                       // 32-bit tile counters / in-frame offsets
    return pl;
  }
  // One block per CU (its LDS images take > 80 KB).  Blocks are dealt round-robin to the 8 XCDs and the n_cob co
  // blocks of a slice sit on one XCD: a launch must not put more than 32 blocks on any XCD, or that XCD runs two
  // rounds while the others idle (measured on conv5: 33 blocks on four XCDs took 200 us instead of 100).
  // 32 x 128 blocks of dw instead of 64 x 64 (same slab bytes): 35.6 KB of DMA per tile instead of 47 KB for the same
  // MFMA work - the 64 x 64 blocks sit at the CU's ingest limit (5.1 B/clk next to MFMA waves)
  if (pl.variant == 3 && Cout % 128 == 0) {
    pl.variant = 5;
    pl.n_cib = Cin / 32;
    pl.n_cob = Cout / 128;
  }
  // 64 x 96 blocks where 128 does not divide Cout (conv5: 192 = 2 x 96): 256 blocks instead of 240 and 27 MFMAs per 12
  // fragment reads instead of 18 per 11, against 1.5x the slab bytes: 114.4 -> 111.6 us, the step -2.5 us
  if (pl.variant == 3 && Cout % 96 == 0) {
    pl.variant = 6;
    pl.n_cob = Cout / 96;
  }
  int S = (8 * (32 / pl.n_cob)) / (groups * pl.n_cib);
  if (S < 1) S = 1;
  if (S > tiles) S = (int)tiles;
  pl.S = S;
  pl.tiles = tiles;
  pl.n_sigma = groups * pl.n_cib * pl.S;
  pl.blocks = 8 * cdiv(pl.n_sigma, 8) * pl.n_cob;
  return pl;
}

// ---- conv1's kernel (conv_halo_conv1.hip): 4 x 16 tiles, S slices per encoder ---------------------------------------------
constexpr int CONV1_WGRAD_TH = 4, CONV1_WGRAD_TW = 16;

static inline bool conv1_wgrad_handles(int Cin, int Cout, int stride) { return stride == 1 && Cin == 4 && Cout == 32; }

static inline int conv1_wgrad_S(int groups) {
  int S = 768 / groups;
  return S < 1 ? 1 : S;
}

// ---- persistent one-block-per-CU kernels of the encoder bottom (conv2's filter gradient, the fused conv2-dgrad + conv1-wgrad):
// slices per encoder on `cus` compute units ------------------------------------------------------------------------------
struct BottomSlices {
  int S0, per, S, blocks;
};
// S0 = CUs / groups regular blocks per encoder.  When that leaves CUs over (three encoders on 256 CUs: one) and the tiles
// the regular blocks leave over (T mod S0 per encoder) fit ONE more block of the same length, that block takes them:
// bench shape, fused bottom: 85 x 49 tiles with the last two blocks short or empty and the 256th CU idle becomes
// 85 x 48 + 1 x (3 x 16); conv2's filter gradient 97 -> 96 tiles per block.  Otherwise ceil(T / S0) tiles per block.
// for_ws: the upper bound over all T (the workspace is sized for every CU).
static inline BottomSlices bottom_slices_on(int cus, int groups, long long T, bool for_ws) {
  BottomSlices b;
  b.S0 = cus / groups < 1 ? 1 : cus / groups;
  const long long fl = T / b.S0, rem = T - fl * b.S0;
  if (for_ws) {                       // upper bound over all T
    b.per = 0; b.S = b.S0 + 1; b.blocks = b.S0 * groups + 1;
    return b;
  }
  if (rem > 0 && fl >= 1 && cus - b.S0 * groups >= 1 && rem * groups <= fl) {
    b.per = (int)fl; b.S = b.S0 + 1; b.blocks = b.S0 * groups + 1;
  } else {
    b.per = (int)((T + b.S0 - 1) / b.S0); b.S = b.S0; b.blocks = b.S0 * groups;
  }
  return b;
}

// conv2's filter gradient (conv_halo_s2_bwd.hip): 4 x 16 tiles walked by the persistent blocks above
constexpr int HALO_WGRAD_TH = 4, HALO_WGRAD_TW = 16;
constexpr int WGRAD_CUS = 256;

static inline bool halo_wgrad_handles(int H, int W, int Cin, int Cout, int stride) {
  return stride == 2 && Cin == 32 && Cout == 48 && H % 2 == 0 && W % 2 == 0;
}

// the fused conv2-dgrad + conv1-wgrad (conv_halo_bottom.hip): 8 x 64 input pixels per tile, walked by the same persistent blocks.
// tests/native/conv_bottom_cover.cpp holds the plan of every case of tests/native/conv_bottom_cases.txt against the text recorded there.
constexpr int FUSED_BOTTOM_TH = 8, FUSED_BOTTOM_TW = 64;

struct FusedBottomLaunchPlan {
  int tiles_x, tiles_y;      // per frame
  int tiles;                 // per encoder: N * tiles_x * tiles_y
  int S0, per, S, blocks;    // BottomSlices
  long long slice_px;        // per * 8 * 64: the most pixels one slab accumulates (a ragged tile holds fewer; the remainder block
                             // walks at most per / groups tiles per encoder)
  bool remainder;            // the remainder-block form (S == S0 + 1): block S0 * groups walks what every encoder leaves over
};

static inline FusedBottomLaunchPlan fused_bottom_launch_plan(int cus, int groups, int N, int H, int W) {
  FusedBottomLaunchPlan l = {};
  l.tiles_x = cdiv(W, FUSED_BOTTOM_TW);
  l.tiles_y = cdiv(H, FUSED_BOTTOM_TH);
  l.tiles = N * l.tiles_x * l.tiles_y;
  const BottomSlices bs = bottom_slices_on(cus, groups, l.tiles, false);
  l.S0 = bs.S0; l.per = bs.per; l.S = bs.S; l.blocks = bs.blocks;
  l.slice_px = (long long)bs.per * FUSED_BOTTOM_TH * FUSED_BOTTOM_TW;
  l.remainder = bs.S == bs.S0 + 1;
  return l;
}

// ---- the dispatch order of geeco_conv3x3_wgrad ----------------------------------------------------------------------------
static inline WgradFamily wgrad_family(int groups, int N, int H, int W, int Cin, int Cout, int stride) {
  if (halo_wgrad_handles(H, W, Cin, Cout, stride)) return WGRAD_FAMILY_HALO;
  if (conv1_wgrad_handles(Cin, Cout, stride)) return WGRAD_FAMILY_CONV1;
  if (wgrad_halo_plan(groups, N, H, W, Cin, Cout, stride).variant) return WGRAD_FAMILY_LDS;
  return WGRAD_FAMILY_GENERIC;
}

// ---- slab sum (wgrad_reduce_kernel<SPLIT>) ----------------------------------------------------------------------------------
// few float4 columns and many slabs: split the slabs over the waves to get enough parallelism
static inline bool reduce_splits_slabs(int S, long long KC, int Cout, int groups) {
  return S >= 16 && (KC + Cout) / 4 * groups < 64 * 1024;
}
// float4 columns one block of the slab sum covers
static inline int reduce_block_span(bool split) { return split ? 64 : 256; }

// ---- one launch as a family serves it: what the tests pin ----------------------------------------------------------------------
// slice_px: the largest number of output pixels any one slice (slab) accumulates -- the length of the longest float32 sum in
// front of the slab sum.  Generic: m_per_split.  LDS, conv1 and halo kernels: the largest tile count of a slice times TH * TW (a
// ragged tile holds fewer pixels; the count is an upper bound).
struct WgradLaunchPlan {
  WgradFamily family;
  int variant;               // LDS family: wgrad_halo_plan's variant; generic: BC; else 0
  int S;                     // slabs per group
  long long slice_px;
  bool reduce;               // a slab-sum launch follows (every family but the generic kernel at S == 1)
  bool reduce_split;
  bool remainder;            // halo family: the remainder-block form (BottomSlices with S == S0 + 1)
  int blocks;                // thread blocks of the main launch
  long long tiles;           // tiles per group (0: generic)
};

// `family`: which family's plan to evaluate (wgrad_family() for the dispatcher's own choice); `cus`: compute units the
// persistent halo kernel may occupy.  Returns false where that family does not serve the shape.
static inline bool wgrad_launch_plan(WgradFamily family, int cus, int groups, int N, int H, int W, int Cin, int Cout, int stride,
                                     WgradLaunchPlan* out) {
  WgradLaunchPlan l = {};
  l.family = family;
  l.reduce = true;
  switch (family) {
    case WGRAD_FAMILY_HALO: {
      if (!halo_wgrad_handles(H, W, Cin, Cout, stride)) return false;
      l.tiles = (long long)N * cdiv(W / 2, HALO_WGRAD_TW) * cdiv(H / 2, HALO_WGRAD_TH);
      const BottomSlices bs = bottom_slices_on(cus, groups, l.tiles, false);
      l.S = bs.S;
      l.remainder = bs.S == bs.S0 + 1;
      l.slice_px = (long long)bs.per * HALO_WGRAD_TH * HALO_WGRAD_TW;      // the remainder block walks rem <= per tiles per encoder
      l.blocks = bs.blocks;
      break;
    }
    case WGRAD_FAMILY_CONV1: {
      if (!conv1_wgrad_handles(Cin, Cout, stride)) return false;
      l.tiles = (long long)N * cdiv(W, CONV1_WGRAD_TW) * cdiv(H, CONV1_WGRAD_TH);
      l.S = conv1_wgrad_S(groups);
      l.slice_px = cdiv64(l.tiles, l.S) * CONV1_WGRAD_TH * CONV1_WGRAD_TW;
      l.blocks = l.S * groups;
      break;
    }
    case WGRAD_FAMILY_LDS: {
      const WgradHaloPlan pl = wgrad_halo_plan(groups, N, H, W, Cin, Cout, stride);
      if (!pl.variant) return false;
      l.variant = pl.variant;
      l.tiles = pl.tiles;
      l.S = pl.S;
      l.slice_px = cdiv64(pl.tiles, pl.S) * pl.TH * pl.TW;
      l.blocks = pl.blocks;
      break;
    }
    case WGRAD_FAMILY_GENERIC: {
      if (Cin % 4 != 0 || Cin < 4 || Cout % 16 != 0) return false;
      const WgradTilePlan t = wgrad_tile_plan(groups, N, H, W, Cin, Cout, stride);
      l.variant = t.BC;
      l.S = t.S;
      l.slice_px = t.m_per_split;
      l.reduce = t.S > 1;
      l.blocks = t.S * t.row_tiles * t.col_tiles * groups;
      break;
    }
  }
  l.reduce_split = l.reduce && reduce_splits_slabs(l.S, 9ll * Cin * Cout, Cout, groups);
  *out = l;
  return true;
}
