// Stride-2 LDS-halo forwards (family: conv_halo_common.h):
//   conv2 (32 -> 48): conv_s2_halo_fwd_ws_kernel, warp specialised, the whole 32-channel halo per tile;
//   conv3 (48 -> 64): conv_s2_halo_fwd_chunked_kernel, the halo in 16-channel chunks beside the resident kernel;
// their dispatcher geeco_try_halo_fwd and the entry points that also write the ReLU sign fields of the output
// (geeco_conv2_fwd_relu_fields, geeco_conv3_fwd_relu_fields).  Also the dev stamp buffer of the whole family.
#define GEECO_ZERO_PAGE g_zero_page_s2_fwd
#include "conv_halo_common.h"
#include "conv_internal.h"
#include <type_traits>
#include <stdlib.h>

// ------------------------------------------------------------------------------------------------
// conv2-type forward: stride 2, CIN == 32, COUT % 16 == 0, tile = 4 x 16 output pixels.
// LDS: halo (filled by LDS-DMA) as [row][pixel pair][16 float4 = 2 pixels x 8 channel quads, XOR-swizzled by the pair index]:
// a pixel's 128 bytes are fetched by 8 consecutive lanes and the b128 A-fragments of 16 consecutive
// output columns (input pixels 2 r + kx) fall on distinct 16-byte slots.
// ------------------------------------------------------------------------------------------------
struct HaloFwdParams {
  const float* x;
  const float* w;      // HWIO [G][9][CIN][COUT]
  const float* bias;
  float* y;
  long long gs_x, gs_w, gs_b, gs_y;
  int N, H, W, Ho, Wo;
  int tiles_x, tiles_y;      // tiles per image
  long long ntiles;          // G*N*tiles_y*tiles_x
  int tiles_per_group;       // N*tiles_y*tiles_x
  int relu;
  unsigned long long* stamps;   // -DGEECO_STAMPS builds only: [block][2 waves][64] s_memtime timeline
  // optional ReLU sign fields of y (geeco_conv2_fwd_relu_fields): [G][N][fHp][fWp][4] uint16, field q bit 4 i + j <-> channel 16 i + 4 q + j
  unsigned short* fields;
  long long gs_fields;
  int fHp, fWp;
  // chunked forward (conv3): byte fields [G][N][Ho][Wo][COUT / 8]: byte (T >> 1) * 4 + q, bit 4 (T & 1) + j <-> channel 16 T + 4 q + j
  unsigned char* fields8;
  long long gs_fields8;
};

#ifdef GEECO_STAMPS
// Dev instrumentation (HALO_STAMP, conv_halo_common.h): one stamp buffer for the family, zeroed before every stamped launch
static unsigned long long* g_hstamps = nullptr;
unsigned long long* geeco_arm_halo_stamps() {
  if (!g_hstamps) (void)hipMalloc(&g_hstamps, 256 * 2 * 64 * 8);
  (void)hipMemset(g_hstamps, 0, 256 * 2 * 64 * 8);
  return g_hstamps;
}
extern "C" int geeco_debug_dump_halo_stamps(const char* path) {
  if (!g_hstamps) return 1;
  (void)hipDeviceSynchronize();
  const size_t n = 256 * 2 * 64;
  unsigned long long* h = (unsigned long long*)malloc(n * 8);
  (void)hipMemcpy(h, g_hstamps, n * 8, hipMemcpyDeviceToHost);
  FILE* f = fopen(path, "wb");
  if (!f) return 2;
  fwrite(h, 8, n, f);
  fclose(f);
  free(h);
  return 0;
}
#endif
#define HSTAMP(i) HALO_STAMP(blockIdx.x, i)      // per-tile timeline of wave 0 (K half 0) and wave 4 (K half 1) of every block

// ------------------------------------------------------------------------------------------------
// Warp-specialised conv2 forward: 8 compute waves (4 output rows x 2 K halves, kernel fragments
// in registers, loaded straight from the HWIO kernel) + LW loader waves that do nothing but issue the LDS-DMA of
// the halos TWO tiles ahead into a ring of three buffers; the output strip is transposed through LDS so that
// every store instruction writes 1 KiB of consecutive bytes.
// Why (in-kernel timelines, scripts/dev/halo_stamps.py): in the earlier form without loader waves (deleted, DESIGN.md
// §5.8) an LDS-DMA instruction holds the issuing wave for ~300-600 cycles, ~3k cycles per tile on the compute waves
// that issue the 39 pieces; they reach
// the tile barrier late and their partners idle (tile period 9.6k cycles for 6.9k cycles of MFMA work per SIMD).
// With loaders the compute waves' MFMA phase is 3.7k cycles (3.5k ideal); what remains is the CU's vector
// memory pipe: 39 KB in + 12 KB out per tile pass through it at ~5.5 B/clk whoever issues them (the epilogue's
// three store instructions wait ~3-4k cycles behind the loaders' pieces).  Measured: +3.5 % on the launch.
// All waves meet at ONE barrier per tile: loaders arrive once the halo of the NEXT tile has landed (`vmcnt`
// leaves the tile after it in flight), compute waves after their last fragment read of the current one.
// ------------------------------------------------------------------------------------------------
template <int CIN, int COUT, int LW>
__global__ __launch_bounds__(512 + 64 * LW) void conv_s2_halo_fwd_ws_kernel(const HaloFwdParams p) {
  constexpr int TH = 4, TW = 16;
  constexpr int CQ = CIN / 4;
  static_assert(CQ == 8 && CIN == 32, "pair-swizzled halo image is laid out for 8 channel quads; 2 K halves of 16");
  constexpr int HY = 2 * TH + 1;
  constexpr int ROW = 17 * 16;
  constexpr int HALO_USED = HY * ROW;
  constexpr int NDMA = (HALO_USED + 63) / 64;         // 39 pieces of 1 KiB per tile
  constexpr int HALO_F4 = NDMA * 64;
  constexpr int NSLOT = (NDMA + LW - 1) / LW;         // pieces per loader wave
  constexpr int TI = COUT / 16;
  constexpr int RED_F4 = 4 * TI * 64;
  constexpr int NBUF = 3;                             // halo ring: the DMA runs two tiles ahead of the MFMAs
  extern __shared__ __attribute__((aligned(16))) float smem[];
  f32x4* sH = reinterpret_cast<f32x4*>(smem);         // NBUF halo buffers
  f32x4* sR = sH + NBUF * HALO_F4;                    // 2 reduction buffers
  constexpr int OP = COUT / 4 + 1;                    // float4 pitch of an output pixel in the store staging (odd)
  f32x4* sO = sR + 2 * RED_F4;                        // 4 strips x [16 pixels][OP]: output transposed for full-line stores

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool loader = wid >= 8;
  const int r = lane & 15, q = lane >> 4;
  const int strip = wid & 3, khalf = (wid >> 2) & 1;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  const long long per = (p.ntiles + gridDim.x - 1) / gridDim.x;
  long long tile = (long long)blockIdx.x * per;
  long long tend = tile + per < p.ntiles ? tile + per : p.ntiles;
  if (tile >= tend) return;
  int g, n, ty, tx;
  {
    g = (int)(tile / p.tiles_per_group);
    int rem = (int)(tile - (long long)g * p.tiles_per_group);
    int per_img = p.tiles_x * p.tiles_y;
    n = rem / per_img;
    rem -= n * per_img;
    ty = rem / p.tiles_x;
    tx = rem - ty * p.tiles_x;
  }
  auto advance = [&](int& g_, int& n_, int& ty_, int& tx_) {
    if (++tx_ == p.tiles_x) {
      tx_ = 0;
      if (++ty_ == p.tiles_y) {
        ty_ = 0;
        if (++n_ == p.N) {
          n_ = 0;
          ++g_;
        }
      }
    }
  };
  if (loader) {
    // ===== loader waves ===================================================================================
    const int lw = wid - 8;
    int d_src[NSLOT];
    short d_hy[NSLOT], d_hx[NSLOT];
#pragma unroll
    for (int i = 0; i < NSLOT; ++i) {
      const int sl = (lw + LW * i) * 64 + lane;
      const int row = sl / ROW, rem = sl - row * ROW;
      const int pair = rem >> 4, u = (rem & 15) ^ (pair & 15);
      const int hx = 2 * pair + (u >> 3), cq = u & 7;
      const bool ok = sl < HALO_USED && hx <= 2 * TW;
      d_hy[i] = (short)(ok ? row : 30000);              // out-of-range marker fails the per-tile bounds test
      d_hx[i] = (short)hx;
      d_src[i] = (row * p.W + hx) * CIN + cq * 4;
    }
    auto dma_halo = [&](int buf, int g_, int n_, int ty_, int tx_) {
      const int iy0 = ty_ * TH * 2, ix0 = tx_ * TW * 2;      // TF SAME, stride 2, even input: pad_before = 0
      const float* xg = p.x + (long long)g_ * p.gs_x + (((long long)n_ * p.H + iy0) * p.W + ix0) * CIN;
#pragma unroll
      for (int i = 0; i < NSLOT; ++i) {
        if (lw + LW * i < NDMA) {                         // wave-uniform
          const bool v = iy0 + d_hy[i] < p.H && ix0 + d_hx[i] < p.W;
          const float* src = v ? xg + d_src[i] : g_zero_page;
          __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(sH + (lw + LW * i) * 64 + buf * HALO_F4), 16, 0, 0);
        }
      }
    };
    {
      // LDS-DMA ring: tiles t+1, t+2 are in flight ahead of the compute waves
      const int npieces = (NDMA - lw + LW - 1) / LW;       // 10 or 9 (wave-uniform)
      int g1 = g, n1 = n, ty1 = ty, tx1 = tx;              // tile + 1
      dma_halo(0, g, n, ty, tx);
      const bool has1 = tile + 1 < tend;
      if (has1) {
        advance(g1, n1, ty1, tx1);
        dma_halo(1, g1, n1, ty1, tx1);
      }
      if (has1) {
        if (npieces == NSLOT) wait_vm_imm<NSLOT>(); else wait_vm_imm<NSLOT - 1>();
      } else {
        wait_vm_imm<0>();
      }
      asm volatile("s_barrier" ::: "memory");             // (A) halo 0 landed
      int g2 = g1, n2 = n1, ty2 = ty1, tx2 = tx1;          // tile + 2
      int slot = 2;                                        // ring slot of tile + 2
      for (;;) {
        const bool more1 = tile + 1 < tend, more2 = tile + 2 < tend;
        if (more2) {
          advance(g2, n2, ty2, tx2);
          dma_halo(slot, g2, n2, ty2, tx2);
          slot = slot + 1 == NBUF ? 0 : slot + 1;
        }
        // tile barrier: the halo of tile + 1 must have landed (tile + 2 may stay in flight)
        if (more2) {
          if (npieces == NSLOT) wait_vm_imm<NSLOT>(); else wait_vm_imm<NSLOT - 1>();
        } else {
          wait_vm_imm<0>();
        }
        asm volatile("s_barrier" ::: "memory");
        if (!more1) break;
        ++tile;
      }
    }
    return;
  }

  // ===== compute waves ======================================================================================
  int g_w = g;
  f32x4 bias_r[TI];
  const int cq_lane = khalf * 4 + q;       // this wave sums channels [16 khalf, 16 khalf + 16)
  f32x4 wreg[9][TI];
  // kernel fragments straight from the HWIO kernel (no LDS staging): lane (r, q) of co tile i holds
  // w[tap][4 cq_lane + s][16 i + r], s = 0..3; 16 lanes read 64 consecutive bytes
  auto load_wreg = [&](int g_) {
    const float* wg = p.w + (long long)g_ * p.gs_w + (4 * cq_lane) * COUT + r;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int i = 0; i < TI; ++i) {
        const float* w0 = wg + tap * CIN * COUT + 16 * i;
        wreg[tap][i] = f32x4{w0[0], w0[COUT], w0[2 * COUT], w0[3 * COUT]};
      }
#pragma unroll
    for (int i = 0; i < TI; ++i) bias_r[i] = *reinterpret_cast<const f32x4*>(p.bias + (long long)g_ * p.gs_b + i * 16 + 4 * q);
  };
  load_wreg(g);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  asm volatile("s_barrier" ::: "memory");               // (A)
  int buf = 0;
  [[maybe_unused]] int tcount = 0;        // tile ordinal, for the dev stamps only
  for (;;) {
    const bool more = tile + 1 < tend;
    int g2 = g, n2 = n, ty2 = ty, tx2 = tx;
    HSTAMP(tcount < 10 ? 6 * tcount + 0 : 64);
    if (more) advance(g2, n2, ty2, tx2);
    HSTAMP(tcount < 10 ? 6 * tcount + 1 : 64);
    f32x4 acc[TI];
#pragma unroll
    for (int i = 0; i < TI; ++i) acc[i] = zero4;
    const f32x4* hA = sH + buf * HALO_F4 + (2 * strip) * ROW;
    f32x4 a_cur, a_nxt;
    auto frag = [&](int tap, f32x4& a) {
      const int ky = tap / 3, kx = tap - ky * 3;
      const int pair = r + (kx >> 1);
      a = hA[ky * ROW + pair * 16 + ((((kx & 1) << 3) | cq_lane) ^ (pair & 15))];
    };
    frag(0, a_cur);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      if (tap + 1 < 9) frag(tap + 1, a_nxt);
      __builtin_amdgcn_sched_barrier(0);   // keep the prefetch read ABOVE this group's MFMAs
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int i = 0; i < TI; ++i)
          acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(wreg[tap][i][s], a_cur[s], acc[i], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      a_cur = a_nxt;
    }
    HSTAMP(tcount < 10 ? 6 * tcount + 2 : 64);
    f32x4* red = sR + (int)(tile & 1) * RED_F4;
    if (khalf == 1) {
#pragma unroll
      for (int i = 0; i < TI; ++i) red[(strip * TI + i) * 64 + lane] = acc[i];
    }
    HSTAMP(tcount < 10 ? 6 * tcount + 3 : 64);
    lds_barrier();
    HSTAMP(tcount < 10 ? 6 * tcount + 4 : 64);   // tile barrier: partial sums visible; everyone is done with buf; the loaders' next halo landed
    if (khalf == 0) {
      // epilogue: lane owns pixel (ty*4 + strip, tx*16 + r), channels 16 i + 4 q .. +3.  The strip's 16 x COUT
      // outputs are 3 KB of consecutive NHWC bytes: they are transposed through LDS so that every store instruction
      // writes 1 KiB of consecutive bytes instead of 16 separate 64-byte pieces (in-kernel timeline: the three
      // piecewise stores held the wave ~3.6k cycles per tile - the kernel's critical path).
      f32x4* so = sO + strip * 16 * OP;
      unsigned field = 0;        // sign bits of this lane's 4 TI outputs (after the ReLU: > 0 <=> non-zero bits)
#pragma unroll
      for (int i = 0; i < TI; ++i) {
        f32x4 v = acc[i] + red[(strip * TI + i) * 64 + lane] + bias_r[i];
        if (p.relu) {
          v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
        }
        so[r * OP + 4 * i + q] = v;
        if (p.fields) {
#pragma unroll
          for (int j = 0; j < 4; ++j) field |= min(__float_as_uint(v[j]), 1u) << (4 * i + j);
        }
      }
      if (p.fields) {
        // the consumer (conv3's input-gradient kernel) holds the same (pixel r, quad q) layout in its accumulators, so
        // every lane stores its own 16-bit field: no cross-lane assembly; 16 pixels x 4 fields = 128 consecutive bytes
        const int fy = ty * TH + strip, fx = tx * TW + r;
        if (fy < p.Ho && fx < p.Wo)
          p.fields[(long long)g * p.gs_fields + (((long long)n * p.fHp + fy) * p.fWp + fx) * 4 + q] = (unsigned short)field;
      }
      // same-wave LDS round trip: the compiler's lgkmcnt wait orders the reads behind the writes
      const int oy = ty * TH + strip;
      float* yo = p.y + (long long)g * p.gs_y + (((long long)n * p.Ho + oy) * p.Wo + tx * TW) * COUT;
      constexpr int C4 = COUT / 4;
#pragma unroll
      for (int jj = 0; jj < TI; ++jj) {          // 16 * C4 float4 = TI x 64 lanes
        const int m = lane + 64 * jj;
        const int px = m / C4, c4 = m - px * C4;
        const f32x4 v = so[px * OP + c4];
        if (oy < p.Ho && tx * TW + px < p.Wo) stream_store<1>(yo + m * 4, v);
      }
    }
    HSTAMP(tcount < 10 ? 6 * tcount + 5 : 64);
    ++tcount;
    if (!more) break;
    if (g2 != g_w) {             // the range crosses into the next encoder: new kernel fragments
      load_wreg(g2);
      g_w = g2;
    }
    g = g2; n = n2; ty = ty2; tx = tx2;
    buf = buf + 1 == NBUF ? 0 : buf + 1;
    ++tile;
  }
}

template <int CIN, int COUT, int LW>
static int launch_s2_halo_fwd_ws(HaloFwdParams& p, hipStream_t s) {
  const size_t lds = halo_fwd_ws_lds_bytes(COUT);
  if (int rc = geeco_lds_opt_in<&conv_s2_halo_fwd_ws_kernel<CIN, COUT, LW>>(lds)) return rc;
  p.stamps = geeco_arm_halo_stamps();
  const int blocks = halo_blocks(p.ntiles, HALO_FWD_CUS);
  geeco_note_kernel("conv_s2_halo_fwd_ws_kernel<%d, %d, %d>", CIN, COUT, LW);
  hipLaunchKernelGGL((conv_s2_halo_fwd_ws_kernel<CIN, COUT, LW>), dim3((unsigned)blocks), dim3(512 + 64 * LW), lds, s, p);
  GEECO_LAUNCH_CHECK();
  return 0;
}

template <int CIN, int COUT>
static int launch_s2_halo_fwd(HaloFwdParams& p, hipStream_t s) {
  // 4 loader waves measured +3.5 % on the launch against none, 2 are too few (-5 %)
  return launch_s2_halo_fwd_ws<CIN, COUT, 4>(p, s);      // 8 compute waves + 4 loader waves
}

// ------------------------------------------------------------------------------------------------
// conv3-type forward (stride 2, CIN % 16 == 0, COUT % 32 == 0, kernel resident in LDS): the input halo of
// a 4 x 16 output tile is staged in 16-channel chunks - with 48 input channels the whole halo (twice) does
// not fit beside the 110 KB kernel.  Step (tile, chunk): 9 taps read their A fragments from the chunk image
// [row 9][pixel pair 17][8 float4 = 2 pixels x 4 quads, XOR-swizzled by pair & 7] while the next step's
// image lands in the other buffer by LDS-DMA (4 lanes fetch a pixel's 64 contiguous bytes).  Wave = (output
// row of the tile, half of the output channels); accumulators live across the chunks of a tile.
// Why: the gather GEMM fetches every input pixel 2.25 times from beyond L2 (PMC 744 MB for a 302 MB input)
// and the kernel slab once per block (340 MB), at the per-CU miss rate of the vector memory path.
// ------------------------------------------------------------------------------------------------
template <int CIN, int COUT>
__global__ __launch_bounds__(512) void conv_s2_halo_fwd_chunked_kernel(const HaloFwdParams p) {
  constexpr int NT = 512;
  constexpr int TH = 4, TW = 16;
  constexpr int CQ = CIN / 4;
  constexpr int NCH = CIN / 16;                       // chunks (steps) per tile
  constexpr int HY = 2 * TH + 1;
  constexpr int ROW = 17 * 8;                         // float4 per image row
  constexpr int IMG_F4 = HY * ROW;                    // 1224
  constexpr int NPIECE = (IMG_F4 + 63) / 64;          // 20
  constexpr int BUF_F4 = NPIECE * 64;
  constexpr int NSLOT = (NPIECE + 7) / 8;
  constexpr int W_F4 = 9 * CQ * COUT;
  constexpr int TI = COUT / 32;                       // co tiles per wave (each wave: half of the channels)
  static_assert(CIN % 16 == 0 && COUT % 32 == 0, "shape");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  f32x4* sW = reinterpret_cast<f32x4*>(smem);
  f32x4* sH = sW + W_F4;                              // 2 chunk images

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int strip = wid & 3, cohalf = wid >> 2;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  const long long per = (p.ntiles + gridDim.x - 1) / gridDim.x;
  long long tile = (long long)blockIdx.x * per;
  long long tend = tile + per < p.ntiles ? tile + per : p.ntiles;
  if (tile >= tend) return;
  int g, n, ty, tx;
  {
    g = (int)(tile / p.tiles_per_group);
    int rem = (int)(tile - (long long)g * p.tiles_per_group);
    int per_img = p.tiles_x * p.tiles_y;
    n = rem / per_img;
    rem -= n * per_img;
    ty = rem / p.tiles_x;
    tx = rem - ty * p.tiles_x;
  }
  auto advance = [&](int& g_, int& n_, int& ty_, int& tx_) {
    if (++tx_ == p.tiles_x) {
      tx_ = 0;
      if (++ty_ == p.tiles_y) {
        ty_ = 0;
        if (++n_ == p.N) {
          n_ = 0;
          ++g_;
        }
      }
    }
  };

  __builtin_assume(wid >= 0 && wid < 8);
  int d_src[NSLOT];
  short d_hy[NSLOT], d_hx[NSLOT];
#pragma unroll
  for (int i = 0; i < NSLOT; ++i) {
    const int sl = (wid + 8 * i) * 64 + lane;
    const int rw = sl / ROW, rem = sl - rw * ROW;
    const int pair = rem >> 3, u = (rem & 7) ^ (pair & 7);
    const int hx = 2 * pair + (u >> 2), cq4 = u & 3;
    const bool ok = sl < IMG_F4 && hx <= 2 * TW;
    d_hy[i] = (short)(ok ? rw : 30000);               // out-of-range marker fails the per-tile bounds test
    d_hx[i] = (short)hx;
    d_src[i] = (rw * p.W + hx) * CIN + cq4 * 4;
  }
  const float* zero_page = g_zero_page;             // its address ONCE, in scalar registers: referenced inside the tile loop the
  asm volatile("" : "+s"(zero_page));              // compiler re-fetches it through the GOT (s_getpc + s_load + s_waitcnt lgkmcnt(0)) per DMA piece
  auto dma_chunk = [&](int buf, int g_, int n_, int ty_, int tx_, int chunk) {
    const int iy0 = ty_ * TH * 2, ix0 = tx_ * TW * 2;      // TF SAME, stride 2, even input: pad_before = 0
    const float* xg = p.x + (long long)g_ * p.gs_x + (((long long)n_ * p.H + iy0) * p.W + ix0) * CIN + chunk * 16;
    const long long zero_x = zero_page - xg;             // tile-only values in scalar registers (as conv_wgrad_halo.hip)
    const int hy = p.H - iy0, hx = p.W - ix0;
#pragma unroll
    for (int i = 0; i < NSLOT; ++i) {
      if (8 * (i + 1) <= NPIECE || wid + 8 * i < NPIECE) {      // compile-time true except in the last slot (wid < 8)
        const bool v = d_hy[i] < hy && d_hx[i] < hx;
        const long long off = v ? (long long)d_src[i] : zero_x;
        __builtin_amdgcn_global_load_lds((gptr_t)(xg + off), (lptr_t)(sH + buf * BUF_F4 + (wid + 8 * i) * 64), 16, 0, 0);
      }
    }
  };
  auto load_weights = [&](int g_) {
    const float* wg = p.w + (long long)g_ * p.gs_w;
    // HWIO [tap][c][co] -> LDS [tap][c/4][co][c%4]
    for (int e = tid; e < 9 * CIN * COUT; e += NT) {
      int co = e % COUT;
      int tc = e / COUT;               // tap*CIN + c
      int c = tc % CIN, tap = tc / CIN;
      smem[((tap * CQ + (c >> 2)) * COUT + co) * 4 + (c & 3)] = wg[e];
    }
  };

  dma_chunk(0, g, n, ty, tx, 0);
  load_weights(g);
  int g_w = g;
  f32x4 bias_r[TI];
#pragma unroll
  for (int i = 0; i < TI; ++i)
    bias_r[i] = *reinterpret_cast<const f32x4*>(p.bias + (long long)g * p.gs_b + cohalf * (COUT / 2) + i * 16 + 4 * q);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  const f32x4* hB = sW + q * COUT + cohalf * (COUT / 2) + r;     // + ((tap*CQ + 4 chunk) * COUT + 16 i)
  // One tile; b0 = LDS buffer of its first chunk.  The chunk loop is fully unrolled and the tile loop below alternates
  // b0 (NCH is odd for conv3: the parity flips per tile), so the buffer index is a compile-time constant everywhere:
  // the fragment addresses are loop-invariant registers + immediates instead of VALU adds per chunk.
  auto tile_body = [&](auto b0c) -> bool {
    constexpr int b0 = decltype(b0c)::value;
    const bool more = tile + 1 < tend;
    int g2 = g, n2 = n, ty2 = ty, tx2 = tx;
    if (more) advance(g2, n2, ty2, tx2);
    f32x4 acc[TI];
#pragma unroll
    for (int i = 0; i < TI; ++i) acc[i] = zero4;
#pragma unroll
    for (int chunk = 0; chunk < NCH; ++chunk) {
      const int buf = (b0 + chunk) & 1;
      if (chunk + 1 < NCH)
        dma_chunk(buf ^ 1, g, n, ty, tx, chunk + 1);
      else if (more)
        dma_chunk(buf ^ 1, g2, n2, ty2, tx2, 0);
      const f32x4* hA = sH + buf * BUF_F4 + (2 * strip) * ROW;
      const f32x4* hBc = hB + 4 * chunk * COUT;
      f32x4 a_cur, b_cur[TI], a_nxt, b_nxt[TI];
      auto frag = [&](int tap, f32x4& a, f32x4 (&b)[TI]) {
        const int ky = tap / 3, kx = tap - ky * 3;
        const int pair = r + (kx >> 1);
        a = hA[ky * ROW + pair * 8 + ((((kx & 1) << 2) | q) ^ (pair & 7))];
#pragma unroll
        for (int i = 0; i < TI; ++i) b[i] = hBc[tap * CQ * COUT + i * 16];
      };
      frag(0, a_cur, b_cur);
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        if (tap + 1 < 9) frag(tap + 1, a_nxt, b_nxt);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int i = 0; i < TI; ++i)
            acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(b_cur[i][s], a_cur[s], acc[i], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        a_cur = a_nxt;
#pragma unroll
        for (int i = 0; i < TI; ++i) b_cur[i] = b_nxt[i];
      }
      if (chunk + 1 < NCH || more) dma_barrier();   // next image landed; everyone is done with this one
    }
    {
      // epilogue: pixel (oy, ox) = (ty*4 + strip, tx*16 + r); channels cohalf*COUT/2 + 16 i + 4 q .. +3
      const int oy = ty * TH + strip, ox = tx * TW + r;
      const bool ok = oy < p.Ho && ox < p.Wo;
      float* yo = p.y + (long long)g * p.gs_y + (((long long)n * p.Ho + oy) * p.Wo + ox) * COUT + cohalf * (COUT / 2);
      unsigned sign = 0;     // sign bits of this lane's 4 TI outputs (after the ReLU: > 0 <=> non-zero bits): bit 4 i + j
#pragma unroll
      for (int i = 0; i < TI; ++i) {
        f32x4 v = acc[i] + bias_r[i];
        if (p.relu) {
          v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
        }
        if (ok) stream_store<2>(yo + i * 16 + 4 * q, v);
        if (p.fields8) {
#pragma unroll
          for (int j = 0; j < 4; ++j) sign |= min(__float_as_uint(v[j]), 1u) << (4 * i + j);
        }
      }
      // sign fields for the next layer's input-gradient kernel (same (pixel r, quad q) accumulator layout: the lane owns
      // whole bytes: its TI = 2 channel tiles are tile pair `cohalf`)
      if (p.fields8 && ok) {
        static_assert(TI == 2, "one byte per lane = one pair of 16-channel tiles");
        p.fields8[(long long)g * p.gs_fields8 + (((long long)n * p.Ho + oy) * p.Wo + ox) * (COUT / 8) + cohalf * 4 + q] = (unsigned char)sign;
      }
    }
    if (!more) return false;
    if (g2 != g_w) {             // the range crosses into the next encoder: refresh the resident kernel
      load_weights(g2);
      g_w = g2;
#pragma unroll
      for (int i = 0; i < TI; ++i)
        bias_r[i] = *reinterpret_cast<const f32x4*>(p.bias + (long long)g2 * p.gs_b + cohalf * (COUT / 2) + i * 16 + 4 * q);
      __syncthreads();
    }
    g = g2; n = n2; ty = ty2; tx = tx2;
    ++tile;
    return true;
  };
  for (;;) {
    if (!tile_body(std::integral_constant<int, 0>{})) break;
    if (!tile_body(std::integral_constant<int, NCH & 1>{})) break;
  }
}

template <int CIN, int COUT>
static int launch_s2_halo_fwd_chunked(HaloFwdParams& p, hipStream_t s) {
  const size_t lds = halo_fwd_chunked_lds_bytes(CIN, COUT);
  if (int rc = geeco_lds_opt_in<&conv_s2_halo_fwd_chunked_kernel<CIN, COUT>>(lds)) return rc;
  const int blocks = halo_blocks(p.ntiles, HALO_FWD_CUS);
  geeco_note_kernel("conv_s2_halo_fwd_chunked_kernel<%d, %d>", CIN, COUT);
  hipLaunchKernelGGL((conv_s2_halo_fwd_chunked_kernel<CIN, COUT>), dim3((unsigned)blocks), dim3(512), lds, s, p);
  GEECO_LAUNCH_CHECK();
  return 0;
}

// operands and the grid of 4 x 16 output-pixel tiles both kernels walk
static HaloFwdParams halo_fwd_params(const float* x, const float* w, const float* b, float* y, int groups, int64_t gs_x,
                                     int64_t gs_w, int64_t gs_b, int64_t gs_y, int N, int H, int W, int relu) {
  HaloFwdParams p = {};
  p.x = x; p.w = w; p.bias = b; p.y = y;
  p.gs_x = gs_x; p.gs_w = gs_w; p.gs_b = gs_b; p.gs_y = gs_y;
  p.N = N; p.H = H; p.W = W; p.Ho = H / 2; p.Wo = W / 2;
  const HaloTileGrid tg = halo_fwd_grid(groups, N, H, W);      // 4 x 16 output-pixel tiles, at most 256 blocks: conv_halo_plan.h
  p.tiles_x = tg.tiles_x; p.tiles_y = tg.tiles_y;
  p.tiles_per_group = tg.tiles_per_group;
  p.ntiles = tg.ntiles;
  p.relu = relu;
  return p;
}

// geeco_halo_fwd_handles (conv_halo_plan.h): does the dispatcher below take this shape?  (geeco_conv3x3_fwd_state asks: a layer
// these kernels serve must not go through the gather GEMM there while every other path runs it through them)
// Returns 1 if handled, 0 if the shape is not covered (caller falls back to the gather-GEMM),
// or an error code < 0 / hipError.
int geeco_try_halo_fwd(const float* x, const float* w, const float* b, float* y, int groups, int64_t gs_x,
                       int64_t gs_w, int64_t gs_b, int64_t gs_y, int N, int H, int W, int Cin, int Cout, int stride,
                       int relu, hipStream_t stream, int* handled) {
  *handled = 0;
  if (!b) return 0;
  const bool conv2 = Cin == 32 && Cout == 48;
  if (geeco_halo_fwd_handles(H, W, Cin, Cout, stride)) {
    HaloFwdParams p = halo_fwd_params(x, w, b, y, groups, gs_x, gs_w, gs_b, gs_y, N, H, W, relu);
    int rc = conv2 ? launch_s2_halo_fwd<32, 48>(p, stream) : launch_s2_halo_fwd_chunked<48, 64>(p, stream);
    if (rc) return rc;
    *handled = 1;
  }
  return 0;
}

// ---- ReLU sign fields of conv2's output for conv3's input gradient (see HaloFwdParams::fields) ---------------------
extern "C" int64_t geeco_relu_fields_elems(int N, int H, int W) {    // uint16 elements per encoder; H, W of the 48-channel tensor
  return (int64_t)N * ((H + 7) / 8 * 8) * ((W + 63) / 64 * 64) * 4;
}

extern "C" int geeco_conv2_fwd_relu_fields(const float* x, const float* w, const float* b, float* y, uint16_t* fields,
                                           int groups, int64_t gs_x, int64_t gs_w, int64_t gs_b, int64_t gs_y,
                                           int64_t gs_fields, int N, int H, int W, void* stream) {
  GEECO_CHECK_ARG(x && w && b && y && fields, "conv2_fwd_relu_fields: null pointer");
  GEECO_CHECK_ARG(groups >= 1 && N >= 1 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0,
                  "conv2_fwd_relu_fields: H = %d, W = %d must be even", H, W);
  HaloFwdParams p = halo_fwd_params(x, w, b, y, groups, gs_x, gs_w, gs_b, gs_y, N, H, W, 1);
  p.fields = fields; p.gs_fields = gs_fields; p.fHp = (p.Ho + 7) / 8 * 8; p.fWp = (p.Wo + 63) / 64 * 64;
  return launch_s2_halo_fwd_ws<32, 48, 4>(p, (hipStream_t)stream);
}

// ---- ... and of conv3's output for conv4's input gradient (byte fields, see HaloFwdParams::fields8) ------------------
extern "C" int geeco_conv3_fwd_relu_fields(const float* x, const float* w, const float* b, float* y, uint8_t* fields,
                                           int groups, int64_t gs_x, int64_t gs_w, int64_t gs_b, int64_t gs_y,
                                           int64_t gs_fields, int N, int H, int W, void* stream) {
  GEECO_CHECK_ARG(x && w && b && y && fields, "conv3_fwd_relu_fields: null pointer");
  GEECO_CHECK_ARG(groups >= 1 && N >= 1 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0,
                  "conv3_fwd_relu_fields: H = %d, W = %d must be even", H, W);
  HaloFwdParams p = halo_fwd_params(x, w, b, y, groups, gs_x, gs_w, gs_b, gs_y, N, H, W, 1);
  p.fields8 = fields; p.gs_fields8 = gs_fields;
  return launch_s2_halo_fwd_chunked<48, 64>(p, (hipStream_t)stream);
}
