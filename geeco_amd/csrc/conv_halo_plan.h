// Host-side description of the forward and input-gradient launches of the LDS-halo and LDS-staged kernels (conv_halo_s2_fwd.hip,
// conv_halo_conv1.hip, conv_halo_s2_bwd.hip, conv_dgrad_lds.hip) in plain C++: which kernel family serves a shape, the family
// order of geeco_conv3x3_fwd / geeco_conv3x3_dgrad, every launch's tile grid, item count, block count and dynamic LDS size, and
// how the blocks walk their items.  No device code and no HIP type: tests/native/conv_halo_cover.cpp compiles this header as a
// host program and holds the plan of every case of tests/native/conv_halo_cases.txt against the text recorded there.  The .hip
// files include it and keep no second copy of anything below (conv_wgrad_plan.h and conv_gemm_plan.h do the same for the filter
// gradient and the gather GEMM).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "geeco_intmath.h"

// ---- which family serves a layer --------------------------------------------------------------------------------------
enum ConvFamily { CONV_HALO, CONV_CONV1, CONV_DGRAD_LDS, CONV_GATHER_GEMM };

// conv2 type (32 -> 48) and conv3 type (48 -> 64), stride 2, even sizes: conv_halo_s2_fwd.hip
static inline int geeco_halo_fwd_handles(int H, int W, int Cin, int Cout, int stride) {
  if (stride != 2 || (H % 2) || (W % 2)) return 0;
  return (Cin == 32 && Cout == 48) || (Cin == 48 && Cout == 64);
}

// conv1 (4 -> 32, stride 1): conv_halo_conv1.hip
static inline int geeco_conv1_fwd_handles(int Cin, int Cout, int stride) { return stride == 1 && Cin == 4 && Cout == 32; }

// the same two layer types backward (given the HWIO kernel): conv_halo_s2_bwd.hip
static inline int geeco_halo_dgrad_handles(int H, int W, int Cin, int Cout, int stride) {
  if (stride != 2 || (H % 2) || (W % 2)) return 0;
  return (Cin == 48 && Cout == 64) || (Cin == 32 && Cout == 48);
}

// LDS-staged input gradient (conv_dgrad_lds.hip): the shape condition, stated once.  -> 0 declined; 1: 8 groups of 1 x 16 class
// pixels, a 16 x 32 input-pixel tile; 2: 8 x 8 class pixels per frame, one-frame tiles of 4 groups
static inline int dgrad_lds_shape(int H, int W, int Cin, int Cout, int stride) {
  if (stride != 2 || (H & 1) || (W & 1) || Cin % 64 != 0 || Cout % 16 != 0 || Cout < 32) return 0;
  const int Ho = H / 2, Wo = W / 2;
  int shape = 0;
  if (Ho % 8 == 0 && Wo % 16 == 0) shape = 1;
  else if (Ho == 8 && Wo == 8) shape = 2;
  if (!shape) return 0;
  // 32-bit limits: pixel and dz offsets inside a frame; weight granules are addressed by 32-bit BYTE offsets
  if ((long long)H * W * Cin >= (1ll << 31) || (long long)Ho * Wo * Cout >= (1ll << 31) || 9ll * Cin * Cout >= (1ll << 30)) return 0;
  return shape;
}
static inline int geeco_dgrad_lds_handles(int H, int W, int Cin, int Cout, int stride) { return dgrad_lds_shape(H, W, Cin, Cout, stride) != 0; }

// Forward: LDS-halo, conv1's, else the gather GEMM (conv_gemm.hip).
static inline ConvFamily conv_fwd_family(int H, int W, int Cin, int Cout, int stride) {
  if (geeco_halo_fwd_handles(H, W, Cin, Cout, stride)) return CONV_HALO;
  if (geeco_conv1_fwd_handles(Cin, Cout, stride)) return CONV_CONV1;
  return CONV_GATHER_GEMM;
}

// Input gradient: LDS-halo, LDS-staged, else the gather GEMM.
static inline ConvFamily conv_dgrad_family(int H, int W, int Cin, int Cout, int stride) {
  if (geeco_halo_dgrad_handles(H, W, Cin, Cout, stride)) return CONV_HALO;
  if (geeco_dgrad_lds_handles(H, W, Cin, Cout, stride)) return CONV_DGRAD_LDS;
  return CONV_GATHER_GEMM;
}

// ---- LDS-staged input gradient: conv_s2_dgrad_lds_kernel<PR, PC, FR, NCIT, NW> -------------------------------------------
// dynamic LDS of an instantiation: two weight chunks [9][NCIT][64] and two dz halo chunks, in 16-byte granules
constexpr size_t dgrad_lds_lds_bytes(int PR, int PC, int FR, int NCIT, int NW) {
  return (size_t)(2 * 9 * NCIT * 64 + 2 * ((4 * ((FR * ((NW / FR) * PR + 1) * (PC + 1) + 15) / 16 * 16) + 63) / 64 * 64)) * 16;
}

enum DgradLdsVariant {
  DGRAD_LDS_NONE = 0,
  DGRAD_LDS_64 = 1,        // <1, 16, 1, 4, 8>: 64-channel items, at most 256 blocks (one per CU)
  DGRAD_LDS_32 = 2,        // <1, 16, 1, 2, 8>: 32-channel items, at most 512 blocks (two per CU)
  DGRAD_LDS_FRAME = 3,     // <2, 8, 1, 2, 4>: one 16 x 16 frame per tile, 32-channel items, at most 768 blocks (three per CU)
};

struct DgradLdsPlan {
  int variant;             // DgradLdsVariant; DGRAD_LDS_NONE: the shape (or its item count) is left to the gather GEMM
  int PR, PC, FR, NCIT, NW;
  int n_cib;               // Cin / (16 NCIT)
  int tiles_y, tiles_x;    // tiles per frame
  int tiles_per_group;     // tiles of one encoder
  int items;               // groups * n_cib * tiles_per_group; block b takes items b, b + blocks, ...
  int blocks;
  size_t lds;
};

static inline DgradLdsPlan dgrad_lds_plan(int groups, int N, int H, int W, int Cin, int Cout, int stride) {
  DgradLdsPlan pl = {};
  const int shape = dgrad_lds_shape(H, W, Cin, Cout, stride);
  if (!shape) return pl;
  const int Ho = H / 2, Wo = W / 2;
  auto inst = [&](int variant, int PR, int PC, int FR, int NCIT, int NW, int cap) {
    pl.variant = variant; pl.PR = PR; pl.PC = PC; pl.FR = FR; pl.NCIT = NCIT; pl.NW = NW;
    pl.blocks = pl.items < cap ? pl.items : cap;
    pl.lds = dgrad_lds_lds_bytes(PR, PC, FR, NCIT, NW);
  };
  if (shape == 2) {
    // 8 x 8 class pixels per frame: one-frame tiles of 4 groups, 32-channel items, 256-thread blocks, three per CU.  The
    // two-frame / 8-wave form has only groups * (Cin / 64) * N / 2 items (conv6 of the bench: 144 for 256 CUs).
    pl.tiles_y = 1; pl.tiles_x = 1;
    pl.tiles_per_group = N;
    pl.n_cib = Cin / 32;
    const long long items = (long long)groups * pl.n_cib * N;
    if (items >= (1ll << 30)) return pl;
    pl.items = (int)items;
    inst(DGRAD_LDS_FRAME, 2, 8, 1, 2, 4, 768);
    return pl;
  }
  pl.tiles_y = Ho / 8; pl.tiles_x = Wo / 16;
  const long long tiles = (long long)N * pl.tiles_y * pl.tiles_x;
  pl.tiles_per_group = (int)tiles;
  // 64-channel items (one block per CU) or 32-channel items (two blocks per CU): whichever spreads the launch more evenly
  // over the 256 CUs; cost of an item in CU-time: 1 resp. 1/2.  Ties go to the 64-channel form (more reuse per staged byte).
  const long long items64 = (long long)groups * (Cin / 64) * tiles;
  if (items64 * 2 >= (1ll << 30)) return pl;
  const double span64 = (double)((items64 + 255) / 256), span32 = 0.5 * (double)((2 * items64 + 255) / 256);
  if (span32 < span64) {
    pl.n_cib = Cin / 32;
    pl.items = (int)(2 * items64);
    inst(DGRAD_LDS_32, 1, 16, 1, 2, 8, 512);
  } else {
    pl.n_cib = Cin / 64;
    pl.items = (int)items64;
    inst(DGRAD_LDS_64, 1, 16, 1, 4, 8, 256);
  }
  return pl;
}

// ---- LDS-halo kernels: persistent blocks over a grid of tiles ------------------------------------------------------------
struct HaloTileGrid {
  int tiles_x, tiles_y;      // tiles per image
  int tiles_per_group;       // N * tiles_y * tiles_x
  long long ntiles;          // groups * tiles_per_group
  int blocks;                // grid x
  int grid_y;                // 1, or the encoders (conv1's forward: every encoder has its own blocks)
};

// Block b of `blocks` takes the tiles [b per, min((b + 1) per, ntiles)), per = ceil(ntiles / blocks), in the order encoder, frame,
// tile row, tile column: both stride-2 forwards and both input-gradient kernels compute this range from gridDim.x.
static inline long long halo_tiles_per_block(long long ntiles, int blocks) { return (ntiles + blocks - 1) / blocks; }

// one block per tile up to one per CU
static inline int halo_blocks(long long ntiles, long long cus) { return (int)(ntiles < cus ? ntiles : cus); }
#define HALO_FWD_CUS 256

// 4 x 16 output-pixel tiles of the stride-2 forwards, at most 256 blocks
static inline HaloTileGrid halo_fwd_grid(int groups, int N, int H, int W) {
  HaloTileGrid t = {};
  t.tiles_x = cdiv(W / 2, 16); t.tiles_y = cdiv(H / 2, 4);
  t.tiles_per_group = N * t.tiles_x * t.tiles_y;
  t.ntiles = (long long)groups * t.tiles_per_group;
  t.blocks = halo_blocks(t.ntiles, HALO_FWD_CUS);
  t.grid_y = 1;
  return t;
}

// 8 x 64 input-pixel tiles of both input-gradient kernels.  The chunked kernel runs on 256 - reserved_cus blocks (data parallel:
// CUs left to the collective that runs beside it); conv2's kernel always on 256.
static inline HaloTileGrid halo_dgrad_grid(int groups, int N, int H, int W, int reserved_cus) {
  HaloTileGrid t = {};
  t.tiles_x = cdiv(W, 64); t.tiles_y = cdiv(H, 8);
  t.tiles_per_group = N * t.tiles_x * t.tiles_y;
  t.ntiles = (long long)groups * t.tiles_per_group;
  t.blocks = halo_blocks(t.ntiles, 256 - reserved_cus);
  t.grid_y = 1;
  return t;
}

// conv1's forward: 8 x 32 tiles, 768 blocks per encoder (256..2048 within 5 %), the encoder in the grid's y dimension; block b takes
// the tiles b, b + blocks, ... of its encoder
#define CONV1_FWD_BLOCKS_PER_GROUP 768
static inline HaloTileGrid conv1_fwd_grid(int groups, int N, int H, int W) {
  HaloTileGrid t = {};
  t.tiles_x = cdiv(W, 32); t.tiles_y = cdiv(H, 8);
  t.tiles_per_group = N * t.tiles_x * t.tiles_y;
  t.ntiles = (long long)groups * t.tiles_per_group;
  t.blocks = t.tiles_per_group < CONV1_FWD_BLOCKS_PER_GROUP ? t.tiles_per_group : CONV1_FWD_BLOCKS_PER_GROUP;
  t.grid_y = groups;
  return t;
}

// ---- dynamic LDS of the LDS-halo launches (conv1's forward has static LDS only) ---------------------------------------------
// conv_s2_halo_fwd_ws_kernel<32, COUT, LW>: three halo buffers of 39 DMA pieces, two reduction buffers, the store staging
constexpr size_t halo_fwd_ws_lds_bytes(int COUT) {
  return (size_t)(3 * (((9 * 17 * 16 + 63) / 64) * 64) + 2 * 4 * (COUT / 16) * 64 + 4 * 16 * (COUT / 4 + 1)) * 16;
}
// conv_s2_halo_fwd_chunked_kernel<CIN, COUT>: the resident kernel and two chunk images
constexpr size_t halo_fwd_chunked_lds_bytes(int CIN, int COUT) {
  return (size_t)(9 * (CIN / 4) * COUT + 2 * (((9 * 17 * 8 + 63) / 64) * 64)) * 16;
}
// conv_s2_halo_dgrad_kernel<32, COUT>: kernel rows at a pitch of 15 granules, two halos of COUT / 4 planes of 5 x 33 pixels
constexpr size_t halo_dgrad_lds_bytes(int CIN, int COUT) { return (size_t)(9 * CIN * 15 + 2 * (COUT / 4) * 165) * 16; }
// conv_s2_halo_dgrad_chunked_kernel<CIN, COUT, FIELDS>: kernel rows at a pitch of COUT / 4 + 2 granules, two chunk images
constexpr size_t halo_dgrad_chunked_lds_bytes(int CIN, int COUT) {
  return (size_t)(9 * CIN * (COUT / 4 + 2) + 2 * (((5 * 33 * 4 + 63) / 64) * 64)) * 16;
}
