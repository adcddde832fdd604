// Stride-2 LDS-halo backwards (family: conv_halo_common.h):
//   conv2 (32 -> 48) filter/bias gradient: conv_s2_halo_wgrad_kernel, dispatcher geeco_try_halo_wgrad;
//   conv2 input gradient on its own:       conv_s2_halo_dgrad_kernel (the step runs it fused: conv_halo_bottom.hip);
//   conv3 (48 -> 64) input gradient:       conv_s2_halo_dgrad_chunked_kernel, ReluGrad mask as y2 or as its sign fields;
// the input-gradient dispatcher geeco_try_halo_dgrad and the entry point geeco_conv3_dgrad_relu_fields.
#define GEECO_ZERO_PAGE g_zero_page_s2_bwd
#include "conv_halo_common.h"
#include "conv_internal.h"

// ------------------------------------------------------------------------------------------------
// conv2-type filter/bias gradient with an LDS halo (stride 2, CIN == 32, COUT % 16 == 0).
//   dw[tap][ci][co] = sum_pixels x[halo(pixel, tap)][ci] * dz[pixel][co]       db[co] = sum dz
// A block walks a contiguous range of 4x16-pixel tiles of ONE encoder and keeps its partial dw in
// registers (wave = (output row of the tile, 16-channel half of ci): 9 taps x COUT/16 MFMA tiles =
// 108 accumulator registers); per tile it stages the x halo (same LDS image as the forward kernel,
// read here with ds_read_b32: bank = 8 (cq % 4) + 4 (pixel % 8) + (ci % 4), conflict free) and the
// dz tile [64 pixels][COUT] (row pitch COUT = 16 mod 32).  MFMA k = 4 consecutive pixels.
// At the end the four row-waves of each ci half are summed through LDS and the block writes one
// slab; wgrad_reduce_kernel (conv_wgrad.hip) sums the slabs in a fixed order.
// ------------------------------------------------------------------------------------------------
struct HaloWgradParams {
  unsigned long long* stamps;   // -DGEECO_STAMPS builds only (scripts/dev/wgrad2_stamps.py)
  const float* x;
  const float* dz;
  float* part;               // [G][S][9*CIN*COUT + COUT]
  long long gs_x, gs_dz;
  int N, H, W, Ho, Wo;
  int tiles_x, tiles_y;
  int tiles_per_group;
  int S;                     // slabs per group (S0, + 1 with the remainder block)
  int S0, per, groups;       // block b < S0 * groups: group b / S0, tiles [per * (b % S0), + per); block S0 * groups (if
                             // launched): the remainder [S0 * per, tiles_per_group) of EVERY group, one after the other
};

#define WSTAMP(i) HALO_STAMP(g == 0 ? split : -1, i)      // encoder 0: per-tile timeline of waves 0 and 4 of every slice

// Measured on this kernel (in-kernel timeline, scripts/dev/wgrad2_stamps.py; tile = 9.8 k cycles, its 216 MFMAs per SIMD
// = 6.9 k): the seven DMA pieces per wave hold both waves of a SIMD in the vector-memory queue for 1.3 - 2 k cycles per
// tile; issued from inside the MFMA loop they lengthen the loop by the same amount; without any DMA the tile takes
// 8.1 k; with four extra loader waves doing all DMA the MFMA waves finish after 7.3 k and then wait at the tile barrier
// until 10.8 k for the 51 KB to land.  The CU ingests ~5 B/clk here (3.1 TB/s chip-wide for 1.2 GB, all of it
// compulsory): the kernel is bound by that, not by where the loads sit.
template <int CIN, int COUT>
__global__ __launch_bounds__(512) void conv_s2_halo_wgrad_kernel(const HaloWgradParams p) {
  constexpr int NT = 512;
  constexpr int TH = 4, TW = 16;
  constexpr int HY = 2 * TH + 1;
  // LDS images, both filled by LDS-DMA (no VGPR staging, no ds_write):
  //   x halo  [row 9][pixel pair 17][16 float4 = 2 pixels x 8 channel quads]; the quad slot is XOR-swizzled by
  //           (pair & 3) << 2 so that the ds_read_b32 of a k-group (4 consecutive pixel pairs x 16 channels of one
  //           16-channel half) covers all 64 banks: bank = 4 ((half << 3 | cq) ^ swz) + (c % 4);
  //   dz tile [64 pixels][COUT] row-major (pitch COUT = 16 mod 32: the 4 pixels of a k-group use different banks).
  constexpr int ROW = 17 * 16;
  constexpr int HALO_USED = HY * ROW;                   // 2448 float4
  constexpr int NHP = (HALO_USED + 63) / 64;            // 39 pieces of 1 KiB
  constexpr int HALO_F4 = NHP * 64;
  constexpr int C4 = COUT / 4;
  constexpr int DZ_F4 = TH * TW * C4;                   // 768 float4 = 12 pieces
  constexpr int NZP = DZ_F4 / 64;
  constexpr int NDZ = (DZ_F4 + NT - 1) / NT;
  constexpr int NSLOT = (NHP + NZP + 7) / 8;            // DMA pieces per wave (halo pieces first, then dz)
  constexpr int TI = COUT / 16;
  static_assert(CIN == 32, "two ci halves <-> two wave groups; 8 quads per pixel");
  static_assert(COUT % 32 == 16 && DZ_F4 % 64 == 0, "dz row pitch must be 16 (mod 32) floats");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  f32x4* sH = reinterpret_cast<f32x4*>(smem);            // 2 halo buffers
  f32x4* sZ = sH + 2 * HALO_F4;                           // 2 dz tiles

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int strip = wid & 3, cit = wid >> 2;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  // Regular blocks own `per` tiles of one encoder; the remainder block (at most one per launch) walks the tiles the
  // regular blocks of every encoder leave over - one segment, one slab per encoder (bottom_slices() below).
  // (The segment body stays inline in this loop, at the kernel's indentation: as a __forceinline__ function called from
  // the loop it measured +1 % here and in the fused bottom, called through a lambda or from two sites 1.5 - 2 x slower.)
  const int nreg = p.S0 * p.groups;
  const bool regular = (int)blockIdx.x < nreg;
  const int nseg = regular ? 1 : p.groups;
#pragma unroll 1
  for (int seg = 0; seg < nseg; ++seg) {
  const int g = regular ? (int)blockIdx.x / p.S0 : seg;
  const int split = regular ? (int)blockIdx.x - g * p.S0 : p.S0;
  int tile = regular ? split * p.per : p.S0 * p.per;
  const int tend = regular && tile + p.per < p.tiles_per_group ? tile + p.per : p.tiles_per_group;
  const long long slab = 9ll * CIN * COUT + COUT;
  float* part = p.part + ((long long)g * p.S + split) * slab;

  int n, ty, tx;
  {
    int per_img = p.tiles_x * p.tiles_y;
    n = tile / per_img;
    int rem = tile - n * per_img;
    ty = rem / p.tiles_x;
    tx = rem - ty * p.tiles_x;
  }
  auto advance = [&](int& n_, int& ty_, int& tx_) {
    if (++tx_ == p.tiles_x) {
      tx_ = 0;
      if (++ty_ == p.tiles_y) {
        ty_ = 0;
        ++n_;
      }
    }
  };

  // this wave's DMA pieces: halo pieces kh = wid + 8 i (slots [64 kh, +64) of the halo image) and dz pieces kz = wid + 8 j
  // (float4 [64 kz, +64) of the dz tile), numbered separately: one role per slot for every wave, a (wave-uniform) range test only
  // in the last slot of each kind (as conv_wgrad_halo.hip / conv_dgrad_lds.hip)
  constexpr int NSH = (NHP + 7) / 8, NSZ = (NZP + 7) / 8;
  __builtin_assume(wid >= 0 && wid < 8);
  int h_src[NSH], z_src[NSZ];
  short h_a[NSH], h_b[NSH], z_a[NSZ], z_b[NSZ];       // halo: (row, hx); dz: (tile row, tile column)
#pragma unroll
  for (int i = 0; i < NSH; ++i) {
    const int sl = (wid + 8 * i) * 64 + lane;
    const int rw = sl / ROW, rem = sl - rw * ROW;
    const int pair = rem >> 4, u = (rem & 15) ^ ((pair & 3) << 2);
    const int hx = 2 * pair + (u >> 3), cq = u & 7;
    const bool ok = sl < HALO_USED && hx <= 2 * TW;
    h_a[i] = (short)(ok ? rw : 30000);                 // out-of-range marker fails the per-tile bounds test
    h_b[i] = (short)hx;
    h_src[i] = (rw * p.W + hx) * CIN + cq * 4;
  }
#pragma unroll
  for (int j = 0; j < NSZ; ++j) {
    const int f = (wid + 8 * j) * 64 + lane;
    const int px = f / C4, c4 = f - px * C4;
    z_a[j] = (short)(px >> 4);
    z_b[j] = (short)(px & 15);
    z_src[j] = ((px >> 4) * p.Wo + (px & 15)) * COUT + c4 * 4;
  }
  const float* zero_page = g_zero_page;             // its address ONCE, in scalar registers: referenced inside the tile loop the
  asm volatile("" : "+s"(zero_page));              // compiler re-fetches it through the GOT (s_getpc + s_load + s_waitcnt lgkmcnt(0)) per DMA piece
  auto dma_tile = [&](int buf, int n_, int ty_, int tx_) {
    const int iy0 = ty_ * TH * 2, ix0 = tx_ * TW * 2;
    const float* xg = p.x + (long long)g * p.gs_x + (((long long)n_ * p.H + iy0) * p.W + ix0) * CIN;
    const float* zg = p.dz + (long long)g * p.gs_dz + (((long long)n_ * p.Ho + ty_ * TH) * p.Wo + tx_ * TW) * COUT;
    // everything that depends on the tile only in scalar registers, once per tile; a piece is then two compares, a select
    // between its own offset and the zero page's, and one 64-bit add (as conv_wgrad_halo.hip)
    const long long zero_x = zero_page - xg, zero_z = zero_page - zg;
    const int hy = p.H - iy0, hx = p.W - ix0, zy = p.Ho - ty_ * TH, zx = p.Wo - tx_ * TW;
#pragma unroll
    for (int i = 0; i < NSH; ++i)
      if (8 * (i + 1) <= NHP || wid + 8 * i < NHP) {       // compile-time true except in the last slot
        const bool v = h_a[i] < hy && h_b[i] < hx;
        const long long off = v ? (long long)h_src[i] : zero_x;
        __builtin_amdgcn_global_load_lds((gptr_t)(xg + off), (lptr_t)(sH + buf * HALO_F4 + (wid + 8 * i) * 64), 16, 0, 0);
      }
#pragma unroll
    for (int j = 0; j < NSZ; ++j)
      if (8 * (j + 1) <= NZP || wid + 8 * j < NZP) {
        const bool v = z_a[j] < zy && z_b[j] < zx;
        const long long off = v ? (long long)z_src[j] : zero_z;
        __builtin_amdgcn_global_load_lds((gptr_t)(zg + off), (lptr_t)(sZ + buf * DZ_F4 + (wid + 8 * j) * 64), 16, 0, 0);
      }
  };

  f32x4 dbsum[NDZ];
#pragma unroll
  for (int i = 0; i < NDZ; ++i) dbsum[i] = zero4;
  f32x4 acc[9][TI];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int i = 0; i < TI; ++i) acc[t][i] = zero4;

  if (tile < tend) dma_tile(0, n, ty, tx);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // B-operand (x) of lane: channel 16 cit + r, pixel pair 4 s + q (+1 for kx = 2); A-operand (dz): co = r
  const int cq_lane = cit * 4 + (r >> 2);
  int xe[3];                                              // float offset of (pair q + (kx >> 1), half kx & 1, cq, c % 4)
#pragma unroll
  for (int kx = 0; kx < 3; ++kx) {
    const int pr = q + (kx >> 1);
    xe[kx] = ((pr * 16 + ((((kx & 1) << 3) | cq_lane) ^ ((pr & 3) << 2))) << 2) + (r & 3);
  }
  const int za_lane = (16 * strip + q) * COUT + r;
  int buf = 0;
  [[maybe_unused]] int tcount = 0;
  for (; tile < tend; ++tile, ++tcount) {
    const bool more = tile + 1 < tend;
    int n2 = n, ty2 = ty, tx2 = tx;
    WSTAMP(tcount < 10 ? 6 * tcount + 0 : 64);
    if (more) {
      advance(n2, ty2, tx2);
      dma_tile(buf ^ 1, n2, ty2, tx2);                    // lands behind this tile's MFMAs
    }
    WSTAMP(tcount < 10 ? 6 * tcount + 1 : 64);
    // bias gradient: every thread adds its share of the dz tile (NDZ float4 reads per tile)
#pragma unroll
    for (int i = 0; i < NDZ; ++i)
      if (tid + NT * i < DZ_F4) dbsum[i] += sZ[buf * DZ_F4 + tid + NT * i];
    const float* hx = reinterpret_cast<const float*>(sH + buf * HALO_F4) + (2 * strip) * ROW * 4;
    const float* hz = reinterpret_cast<const float*>(sZ + buf * DZ_F4) + za_lane;
    // operands of k-group s + 1 are read while the 27 MFMAs of k-group s run (the reads of a group issued right in
    // front of its MFMAs left ~150 cycles of LDS latency exposed four times per tile)
    float a_cur[TI], b_cur[9], a_nxt[TI], b_nxt[9];
    auto frag = [&](int s, float (&a)[TI], float (&b)[9]) {
#pragma unroll
      for (int i = 0; i < TI; ++i) a[i] = hz[(4 * s) * COUT + 16 * i];
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int ky = t / 3, kx = t - ky * 3;
        b[t] = hx[(ky * ROW + 4 * s * 16) * 4 + xe[kx]];
      }
    };
    WSTAMP(tcount < 10 ? 6 * tcount + 2 : 64);
    frag(0, a_cur, b_cur);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (s + 1 < 4) frag(s + 1, a_nxt, b_nxt);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int i = 0; i < TI; ++i)
          acc[t][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[i], b_cur[t], acc[t][i], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < TI; ++i) a_cur[i] = a_nxt[i];
#pragma unroll
      for (int t = 0; t < 9; ++t) b_cur[t] = b_nxt[t];
    }
    WSTAMP(tcount < 10 ? 6 * tcount + 3 : 64);
    dma_barrier();
    WSTAMP(tcount < 10 ? 6 * tcount + 4 : 64);
    n = n2; ty = ty2; tx = tx2;
    buf ^= 1;
  }

  // ---- block reduction: sum the 4 row-waves of each ci half, 3 taps per round, through LDS -------
  f32x4* sR = sH;     // [wave 8][k 3*TI][lane 64]
  constexpr int RK = 3 * TI;
#pragma unroll
  for (int rd = 0; rd < 3; ++rd) {
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int i = 0; i < TI; ++i) sR[(wid * RK + t * TI + i) * 64 + lane] = acc[rd * 3 + t][i];
    __syncthreads();
    for (int e = tid; e < 2 * RK * 64; e += NT) {
      const int ln = e & 63, k = (e >> 6) % RK, c = e / (64 * RK);
      f32x4 s4 = sR[((c * 4 + 0) * RK + k) * 64 + ln];
      s4 += sR[((c * 4 + 1) * RK + k) * 64 + ln];
      s4 += sR[((c * 4 + 2) * RK + k) * 64 + ln];
      s4 += sR[((c * 4 + 3) * RK + k) * 64 + ln];
      const int tap = rd * 3 + k / TI, ti = k % TI;
      const int ci = 16 * c + (ln & 15), co = 16 * ti + 4 * (ln >> 4);
      *reinterpret_cast<f32x4*>(part + ((long long)tap * CIN + ci) * COUT + co) = s4;
    }
  }
  // ---- bias gradient: per-thread dz sums -> LDS [pixel slot][COUT] -> fixed-order column sums ------
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NDZ; ++i)
    if (tid + NT * i < DZ_F4) sZ[tid + NT * i] = dbsum[i];
  __syncthreads();
  if (tid < COUT) {
    const float* zf = reinterpret_cast<const float*>(sZ);
    float s1 = 0.f;
    for (int px = 0; px < TH * TW; ++px) s1 += zf[px * COUT + tid];
    part[9ll * CIN * COUT + tid] = s1;
  }
  __syncthreads();     // the next segment stages into the images this one's sums were just read from
  }
}

int64_t geeco_halo_wgrad_ws_bytes(int groups, int N, int H, int W, int Cin, int Cout, int stride) {
  if (halo_wgrad_handles(H, W, Cin, Cout, stride))
    return (int64_t)groups * bottom_slices(groups, 0, true).S * (9ll * Cin * Cout + Cout) * 4;
  return 0;
}

int geeco_try_halo_wgrad(const float* x, const float* dz, float* dw, float* db, int groups, int64_t gs_x,
                         int64_t gs_dz, int64_t gs_dw, int64_t gs_db, int N, int H, int W, int Cin, int Cout,
                         int stride, void* ws, hipStream_t stream, int* handled) {
  *handled = 0;
  if (halo_wgrad_handles(H, W, Cin, Cout, stride)) {
    HaloWgradParams p = {};
    p.x = x; p.dz = dz; p.part = (float*)ws; p.gs_x = gs_x; p.gs_dz = gs_dz;
    const BottomSlices bs = fill_bottom_geometry(p, groups, N, H, W, cdiv(W / 2, HALO_WGRAD_TW), cdiv(H / 2, HALO_WGRAD_TH));
    p.stamps = geeco_arm_halo_stamps();
    constexpr int HALO_F4 = ((9 * 17 * 16 + 63) / 64) * 64;
    const size_t lds = (size_t)(2 * HALO_F4 + 2 * 4 * 16 * 12) * 16;
    if (int rc = geeco_lds_opt_in<&conv_s2_halo_wgrad_kernel<32, 48>>(lds)) return rc;
    geeco_note_kernel("conv_s2_halo_wgrad_kernel<32, 48>");
    hipLaunchKernelGGL((conv_s2_halo_wgrad_kernel<32, 48>), dim3((unsigned)bs.blocks), dim3(512), lds, stream, p);
    GEECO_LAUNCH_CHECK();
    geeco_launch_wgrad_reduce((const float*)ws, dw, db, gs_dw, gs_db, p.S, 9ll * Cin * Cout, Cout, groups, stream);
    GEECO_LAUNCH_CHECK();
    *handled = 1;
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------
// conv2-type input gradient with an LDS halo (stride 2, CIN == 32, COUT % 16 == 0, even H/W), fused
// with the ReluGrad of the layer below:   dx[y][x][ci] = (ymask > 0) * sum_{taps} dz[oy][ox][:] . w[tap][ci][:]
// For TF SAME / stride 2 / even sizes (pad_before = 0) input row y = 2 Y' + py receives
//   py = 0: (ky = 0, oy = Y'), (ky = 2, oy = Y' - 1);   py = 1: (ky = 1, oy = Y')          (same in x),
// i.e. four parity classes with 4 / 2 / 2 / 1 taps.  A block owns 8 x 64 input pixels (4 x 32 per
// class), stages the 5 x 33 dz halo as [co/4][row][col] float4 planes and keeps the HWIO kernel
// resident as [tap][ci][15 float4] rows (b128 B-fragments straight from the TF layout; in this unfused kernel pitch 15 =
// -1 mod 16 => at most one 2-way conflict per read).  Wave = (column half, Y' row): 4 classes x 2
// ci tiles = 8 accumulator tiles, 27 (tap, 16-co block) steps of 8 MFMAs per tile.
// ------------------------------------------------------------------------------------------------
struct HaloDgradParams {
  const float* dz;
  const float* w;      // HWIO [G][9][CIN][COUT]
  const float* mask;   // [G][N][H][W][CIN] or null
  const unsigned short* fields;   // FIELDS kernels: sign fields of the mask tensor (see HaloFwdParams) instead of mask
  long long gs_fields;
  int fHp, fWp;
  float* dx;
  long long gs_dz, gs_w, gs_dx;
  int N, H, W, Ho, Wo;
  int tiles_x, tiles_y;
  long long ntiles;
  int tiles_per_group;
};

template <int CIN, int COUT>
__global__ __launch_bounds__(512, 2) void conv_s2_halo_dgrad_kernel(const HaloDgradParams p) {
  constexpr int NT = 512;
  constexpr int COQ = COUT / 4;
  constexpr int KB = COUT / 16;
  constexpr int HR = 5, HC = 33;                       // dz halo rows / cols
  constexpr int PLANE = HR * HC;                       // 165 float4
  constexpr int SKEW = 0;                              // (the fused-bottom kernel below skews its planes; this one is off the step's path)
  constexpr int HALO_F4 = COQ * PLANE;
  constexpr int NLOAD = (HALO_F4 + NT - 1) / NT;
  constexpr int WP = 15;                               // float4 pitch of a (tap, ci) kernel row
  constexpr int W_F4 = 9 * CIN * WP;
  static_assert(CIN == 32 && COQ <= WP, "shape");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  f32x4* sW = reinterpret_cast<f32x4*>(smem);
  f32x4* sH = sW + W_F4;                               // 2 halo buffers

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int row = wid & 3, half = wid >> 2;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  const long long per = (p.ntiles + gridDim.x - 1) / gridDim.x;
  long long tile = (long long)blockIdx.x * per;
  const long long tend = tile + per < p.ntiles ? tile + per : p.ntiles;
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

  int l_off[NLOAD], l_src[NLOAD];
  short l_hy[NLOAD], l_hx[NLOAD];
#pragma unroll
  for (int i = 0; i < NLOAD; ++i) {
    int idx = tid + NT * i;
    int pix = idx / COQ, cq = idx - pix * COQ;
    int hy = pix / HC, hx = pix - hy * HC;
    l_hy[i] = (short)hy; l_hx[i] = (short)hx;
    l_off[i] = (idx < HALO_F4) ? cq * PLANE + hy * HC + hx : -1;
    l_src[i] = (hy * p.Wo + hx) * COUT + cq * 4;
  }
  f32x4 stage[NLOAD];
  auto load_halo = [&](int g_, int n_, int ty_, int tx_) {
    const int oy0 = ty_ * 4 - 1, ox0 = tx_ * 32 - 1;
    const float* zg = p.dz + (long long)g_ * p.gs_dz + (((long long)n_ * p.Ho + oy0) * p.Wo + ox0) * COUT;
#pragma unroll
    for (int i = 0; i < NLOAD; ++i) {
      int oy = oy0 + l_hy[i], ox = ox0 + l_hx[i];
      bool v = l_off[i] >= 0 && (unsigned)oy < (unsigned)p.Ho && (unsigned)ox < (unsigned)p.Wo;
      stage[i] = v ? *reinterpret_cast<const f32x4*>(zg + l_src[i]) : zero4;
    }
  };
  auto load_weights = [&](int g_) {
    const f32x4* wg = reinterpret_cast<const f32x4*>(p.w + (long long)g_ * p.gs_w);
    for (int e = tid; e < 9 * CIN * COQ; e += NT) {
      int rowi = e / COQ, c4 = e - rowi * COQ;
      sW[rowi * WP + c4] = wg[e];
    }
  };

  load_halo(g, n, ty, tx);
  load_weights(g);
  int g_w = g;
#pragma unroll
  for (int i = 0; i < NLOAD; ++i)
    if (l_off[i] >= 0) sH[l_off[i]] = stage[i];
  __syncthreads();

  // lane r = X' column inside the wave's 16-column strip; q selects the co quad of a 16-co block
  const int a_lane = q * PLANE + SKEW * (q >> 1) + (row + 1) * HC + 16 * half + r + 1;    // + kb*4*PLANE + dy*HC + dx
  const int b_lane = r * WP + q;                                          // + (tap*CIN + 16 cit)*WP + 4 kb
  int buf = 0;
  for (;;) {
    const bool more = tile + 1 < tend;
    int g2 = g, n2 = n, ty2 = ty, tx2 = tx;
    if (more) {
      advance(g2, n2, ty2, tx2);
      load_halo(g2, n2, ty2, tx2);
    }
    // ReluGrad mask of this wave's 4 x 2 output float4s: issued now, consumed in the epilogue
    const int yb = 2 * (ty * 4 + row), xb = 2 * (tx * 32 + 16 * half + r);
    f32x4 mk[4][2];
    bool okc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int y = yb + (c >> 1), x = xb + (c & 1);
      okc[c] = y < p.H && x < p.W;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        mk[c][t] = f32x4{1.f, 1.f, 1.f, 1.f};
        if (p.mask && okc[c])
          mk[c][t] = *reinterpret_cast<const f32x4*>(p.mask + (long long)g * p.gs_dx +
                                                     (((long long)n * p.H + y) * p.W + x) * CIN + 16 * t + 4 * q);
      }
    }
    f32x4 acc[4][2];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int t = 0; t < 2; ++t) acc[c][t] = zero4;
    const f32x4* hA = sH + buf * HALO_F4 + a_lane;
    const f32x4* hB = sW + b_lane;
    f32x4* hN = sH + (buf ^ 1) * HALO_F4;

    // static schedule: 9 taps x KB blocks; tap (ky, kx) feeds class (py, px) = (ky & 1, kx & 1) with
    // source offset dy = -(ky >> 1), dx = -(kx >> 1)
    f32x4 a_cur, b_cur[2], a_nxt, b_nxt[2];
    auto frag = [&](int it, f32x4& a, f32x4 (&b)[2]) {
      const int tap = it / KB, kb = it - tap * KB;
      const int ky = tap / 3, kx = tap - ky * 3;
      a = hA[kb * (4 * PLANE + 2 * SKEW) - (ky >> 1) * HC - (kx >> 1)];
      b[0] = hB[(tap * CIN) * WP + 4 * kb];
      b[1] = hB[(tap * CIN + 16) * WP + 4 * kb];
    };
    constexpr int NIT = 9 * KB;
    frag(0, a_cur, b_cur);
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      if (it + 1 < NIT) frag(it + 1, a_nxt, b_nxt);
      if (more && it >= NIT - NLOAD - 4 && it < NIT - 4) {
        const int j = it - (NIT - NLOAD - 4);
        if (l_off[j] >= 0) hN[l_off[j]] = stage[j];
      }
      __builtin_amdgcn_sched_barrier(0);
      {
        const int tap = it / KB;
        const int ky = tap / 3, kx = tap - ky * 3;
        const int c = (ky & 1) * 2 + (kx & 1);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int t = 0; t < 2; ++t)
            acc[c][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(b_cur[t][s], a_cur[s], acc[c][t], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
      a_cur = a_nxt;
      b_cur[0] = b_nxt[0];
      b_cur[1] = b_nxt[1];
    }
    // epilogue: class c -> pixel (yb + py, xb + px); lane owns ci = 16 t + 4 q .. +3
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (!okc[c]) continue;
      const int y = yb + (c >> 1), x = xb + (c & 1);
      float* o = p.dx + (long long)g * p.gs_dx + (((long long)n * p.H + y) * p.W + x) * CIN + 4 * q;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        f32x4 v = acc[c][t];
        const f32x4 m = mk[c][t];
        v.x = m.x > 0.f ? v.x : 0.f; v.y = m.y > 0.f ? v.y : 0.f;
        v.z = m.z > 0.f ? v.z : 0.f; v.w = m.w > 0.f ? v.w : 0.f;
        *reinterpret_cast<f32x4*>(o + 16 * t) = v;
      }
    }
    if (!more) break;
    lds_barrier();      // next halo complete; everyone is done with this buffer (and sW)
    if (g2 != g_w) {
      load_weights(g2);
      g_w = g2;
      __syncthreads();
    }
    g = g2; n = n2; ty = ty2; tx = tx2;
    buf ^= 1;
    ++tile;
  }
}

// ------------------------------------------------------------------------------------------------
// The same input gradient with the dz halo cut into 16-channel chunks (conv3: 48 <- 64 channels; any
// CIN % 16 == 0, COUT % 16 == 0 whose kernel fits LDS).  With 64 output channels the whole halo
// (5 x 33 pixels x 256 B, twice) no longer fits beside the resident kernel (9 x 48 rows x 256 B), so a
// tile is processed in COUT / 16 steps: step (tile, chunk) reads the chunk image [hy 5][hx 33][4 quads]
// (quads XOR-swizzled by (hx >> 1) & 3: the b128 reads of 16 consecutive columns are conflict free), while
// the next step's image lands in the other buffer by LDS-DMA (4 lanes fetch a pixel's 64 contiguous bytes;
// no VGPR staging).  Accumulators (4 parity classes x CIN / 16 tiles) live across the chunks of a tile.
// Why it pays: the gather GEMM re-fetches dz once per tap beyond L2 (PMC: 1.1 GB per conv3 launch for a
// 100 MB tensor) and runs at the per-CU miss rate of the vector memory path; here dz is read once.
// ------------------------------------------------------------------------------------------------
template <int CIN, int COUT, bool FIELDS>
__global__ __launch_bounds__(512) void conv_s2_halo_dgrad_chunked_kernel(const HaloDgradParams p) {
  constexpr int NT = 512;
  constexpr int NCH = COUT / 16;                       // chunks (steps) per tile
  constexpr int TCI = CIN / 16;                        // ci tiles per wave
  constexpr int HR = 5, HC = 33;                       // dz halo rows / cols
  // Chunk image of the dz halo, q-major: [co quad q of the chunk][pixel] with the pixel planes padded to a multiple of 16
  // granules, and kernel rows at a pitch of 2 (mod 16) granules: a ds_read_b128 is served in four groups of 16 lanes, each
  // holding every r = lane & 15 once from two neighbouring q; both pitches put the two q of a group on disjoint
  // 16-granule phases (conflict free).  The pixel-major image with an XOR swizzle and the odd row pitch of round 1 measured
  // 43 % LDS bank-conflict cycles.
  constexpr int NPIX = HR * HC;                        // 165
  constexpr int NPIXP = (NPIX + 15) / 16 * 16;         // 176
  constexpr int IMG_F4 = 4 * NPIXP;                    // 704 float4 per chunk image
  constexpr int NPIECE = (IMG_F4 + 63) / 64;           // 11 DMA pieces
  constexpr int BUF_F4 = NPIECE * 64;
  constexpr int NSLOT = (NPIECE + 7) / 8;              // pieces per wave
  constexpr int WP = COUT / 4 + 2;                     // float4 pitch of a (tap, ci) kernel row
  constexpr int W_F4 = 9 * CIN * WP;
  static_assert(CIN % 16 == 0 && COUT % 16 == 0, "shape");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  f32x4* sW = reinterpret_cast<f32x4*>(smem);
  f32x4* sH = sW + W_F4;                               // 2 chunk images

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int row = wid & 3, half = wid >> 2;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  const long long per = (p.ntiles + gridDim.x - 1) / gridDim.x;
  long long tile = (long long)blockIdx.x * per;
  const long long tend = tile + per < p.ntiles ? tile + per : p.ntiles;
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

  // this wave's DMA pieces: piece k = wid + 8 i covers image slots [64 k, 64 k + 64); lane -> (hy, hx, quad)
  __builtin_assume(wid >= 0 && wid < 8);
  int d_src[NSLOT];
  short d_hy[NSLOT], d_hx[NSLOT];
#pragma unroll
  for (int i = 0; i < NSLOT; ++i) {
    const int sl = (wid + 8 * i) * 64 + lane;
    const int quad = sl / NPIXP, pix = sl - quad * NPIXP;
    const int hy = pix / HC, hx = pix - hy * HC;
    d_hy[i] = (short)((sl < IMG_F4 && pix < NPIX) ? hy : 30000);   // out-of-range marker fails the per-tile bounds test
    d_hx[i] = (short)hx;
    d_src[i] = (hy * p.Wo + hx) * COUT + quad * 4;
  }
  auto dma_chunk = [&](int buf, int g_, int n_, int ty_, int tx_, int chunk) {
    const int oy0 = ty_ * 4 - 1, ox0 = tx_ * 32 - 1;
    const float* zg = p.dz + (long long)g_ * p.gs_dz + (((long long)n_ * p.Ho + oy0) * p.Wo + ox0) * COUT + chunk * 16;
#pragma unroll
    for (int i = 0; i < NSLOT; ++i) {
      if (8 * (i + 1) <= NPIECE || wid + 8 * i < NPIECE) {      // compile-time true except in the last slot (wid < 8)
        const int oy = oy0 + d_hy[i], ox = ox0 + d_hx[i];
        const bool v = (unsigned)oy < (unsigned)p.Ho && (unsigned)ox < (unsigned)p.Wo;
        const float* src = v ? zg + d_src[i] : g_zero_page;
        __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(sH + buf * BUF_F4 + (wid + 8 * i) * 64), 16, 0, 0);
      }
    }
  };
  auto load_weights = [&](int g_) {
    const f32x4* wg = reinterpret_cast<const f32x4*>(p.w + (long long)g_ * p.gs_w);
    constexpr int COQ = COUT / 4;
    for (int e = tid; e < 9 * CIN * COQ; e += NT) {
      int rowi = e / COQ, c4 = e - rowi * COQ;
      sW[rowi * WP + c4] = wg[e];
    }
  };

  dma_chunk(0, g, n, ty, tx, 0);
  load_weights(g);
  int g_w = g;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // lane r = X' column inside the wave's 16-column strip; q selects the co quad of the chunk
  const int hx_lane = 16 * half + r + 1;                                  // - dx
  const int b_lane = r * WP + q;                                          // + (tap*CIN + 16 t)*WP + 4 chunk
  static_assert(NCH % 2 == 0, "the chunk loop is unrolled with the LDS buffer index = chunk & 1: a tile must take an even number of chunks");
  // Deferred output stores: the (masked) results of tile t are kept in registers and leave one float4 at a time from inside the
  // tap loops of tile t + 1 (class c in chunk c * NCH / 4, after taps 1, 4, 7, ...).  In a block all eight waves reach the
  // end of a tile together, so an epilogue of 4 x TCI stores per lane is time in which no MFMA issues: measured with the
  // stores removed, 204-212 -> 179-180 us at the bench shape.
  f32x4 pend[4][TCI];
  float* pend_o[4];
  bool pend_ok[4] = {false, false, false, false};
#pragma unroll
  for (int c = 0; c < 4; ++c) pend_o[c] = p.dx;
  for (;;) {
    const bool more = tile + 1 < tend;
    int g2 = g, n2 = n, ty2 = ty, tx2 = tx;
    if (more) advance(g2, n2, ty2, tx2);
    // ReluGrad mask of this wave's 4 x TCI output float4s: issued now, consumed in the epilogue
    const int yb = 2 * (ty * 4 + row), xb = 2 * (tx * 32 + 16 * half + r);
    // FIELDS: one 16-bit sign field per class pixel (this lane's quad q: bit 4 t + j <-> channel 16 t + 4 q + j) instead
    // of TCI float4 of the activation itself: 4 two-byte loads per tile and lane instead of 12 sixteen-byte ones (the
    // field array is padded to whole tiles, so no bounds logic on the load)
    f32x4 mk[FIELDS ? 1 : 4][TCI];
    unsigned short mf[4];
    bool okc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int y = yb + (c >> 1), x = xb + (c & 1);
      okc[c] = y < p.H && x < p.W;
      if constexpr (FIELDS) {
        mf[c] = p.fields[(long long)g * p.gs_fields + (((long long)n * p.fHp + y) * p.fWp + x) * 4 + q];
      } else {
#pragma unroll
        for (int t = 0; t < TCI; ++t) {
          mk[c][t] = f32x4{1.f, 1.f, 1.f, 1.f};
          if (p.mask && okc[c])
            mk[c][t] = *reinterpret_cast<const f32x4*>(p.mask + (long long)g * p.gs_dx +
                                                       (((long long)n * p.H + y) * p.W + x) * CIN + 16 * t + 4 * q);
        }
      }
    }
    f32x4 acc[4][TCI];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int t = 0; t < TCI; ++t) acc[c][t] = zero4;

    // fully unrolled: the buffer index is a compile-time constant, so the fragment addresses are loop-invariant
    // registers + immediates instead of a dozen VALU adds per chunk (VALU work is paid in MFMA time)
#pragma unroll
    for (int chunk = 0; chunk < NCH; ++chunk) {
      const int buf = chunk & 1;
      // the next step's image lands in the other buffer while this one is consumed
      if (chunk + 1 < NCH)
        dma_chunk(buf ^ 1, g, n, ty, tx, chunk + 1);
      else if (more)
        dma_chunk(buf ^ 1, g2, n2, ty2, tx2, 0);
      const f32x4* hA = sH + buf * BUF_F4;
      const f32x4* hB = sW + b_lane + 4 * chunk;
      // static schedule: tap (ky, kx) feeds class (py, px) = (ky & 1, kx & 1) from the dz pixel at
      // (row + 1 - (ky >> 1), column - (kx >> 1))
      f32x4 a_cur, b_cur[TCI], a_nxt, b_nxt[TCI];
      auto frag = [&](int tap, f32x4& a, f32x4 (&b)[TCI]) {
        const int ky = tap / 3, kx = tap - ky * 3;
        const int hy = row + 1 - (ky >> 1), hx = hx_lane - (kx >> 1);
        a = hA[q * NPIXP + hy * HC + hx];
#pragma unroll
        for (int t = 0; t < TCI; ++t) b[t] = hB[(tap * CIN + 16 * t) * WP];
      };
      frag(0, a_cur, b_cur);
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        if (tap + 1 < 9) frag(tap + 1, a_nxt, b_nxt);
        __builtin_amdgcn_sched_barrier(0);
        {
          const int ky = tap / 3, kx = tap - ky * 3;
          const int c = (ky & 1) * 2 + (kx & 1);
#pragma unroll
          for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int t = 0; t < TCI; ++t)
              acc[c][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(b_cur[t][s], a_cur[s], acc[c][t], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        {
          // pending results of the previous tile: class pc's float4 number pt leaves behind tap min(3 pt + 1, 8) of its chunk
#pragma unroll
          for (int pc = 0; pc < 4; ++pc)
#pragma unroll
            for (int pt = 0; pt < TCI; ++pt)
              if (pc * NCH / 4 == chunk) {
                // (both waves of a SIMD store behind the same taps: staggering them by a tap measured 198-201 us against 193-197;
                // all of a class's stores behind tap 0, or behind taps 0, 1, 2: 201 / 196-203)
                if ((3 * pt + 1 < 8 ? 3 * pt + 1 : 8) == tap && pend_ok[pc]) stream_store<3>(pend_o[pc] + 16 * pt, pend[pc][pt]);
              }
          __builtin_amdgcn_sched_barrier(0);
        }
        a_cur = a_nxt;
#pragma unroll
        for (int t = 0; t < TCI; ++t) b_cur[t] = b_nxt[t];
      }
      if (chunk + 1 < NCH || more) dma_barrier();   // next image landed; everyone is done with this one
    }
    // epilogue: class c -> pixel (yb + py, xb + px); lane owns ci = 16 t + 4 q .. +3
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (!okc[c]) continue;
      const int y = yb + (c >> 1), x = xb + (c & 1);
      float* o = p.dx + (long long)g * p.gs_dx + (((long long)n * p.H + y) * p.W + x) * CIN + 4 * q;
#pragma unroll
      for (int t = 0; t < TCI; ++t) {
        f32x4 v = acc[c][t];
        if constexpr (FIELDS) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            v[j] = __int_as_float(__float_as_int(v[j]) & __builtin_amdgcn_sbfe((int)mf[c], 4 * t + j, 1));
        } else {
          const f32x4 m = mk[c][t];
          v.x = m.x > 0.f ? v.x : 0.f; v.y = m.y > 0.f ? v.y : 0.f;
          v.z = m.z > 0.f ? v.z : 0.f; v.w = m.w > 0.f ? v.w : 0.f;
        }
        pend[c][t] = v;
      }
      pend_o[c] = o;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) pend_ok[c] = okc[c];
    if (!more) {        // the block's last tile: nothing left to hide behind
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (pend_ok[c]) {
#pragma unroll
          for (int t = 0; t < TCI; ++t) stream_store<3>(pend_o[c] + 16 * t, pend[c][t]);
        }
    }
    if (!more) break;
    if (g2 != g_w) {          // (the barrier above already separated everyone from the old kernel)
      load_weights(g2);
      g_w = g2;
      __syncthreads();
    }
    g = g2; n = n2; ty = ty2; tx = tx2;
    ++tile;
  }
}

template <int CIN, int COUT, bool FIELDS = false>
static int launch_dgrad_chunked(HaloDgradParams& p, hipStream_t stream) {
  const size_t lds = halo_dgrad_chunked_lds_bytes(CIN, COUT);
  if (int rc = geeco_lds_opt_in<&conv_s2_halo_dgrad_chunked_kernel<CIN, COUT, FIELDS>>(lds)) return rc;
  // data parallel: the reserved CUs are left to the collective that runs beside part 2
  const int blocks = halo_blocks(p.ntiles, 256 - geeco_call_reserved_cus());
  geeco_note_kernel("conv_s2_halo_dgrad_chunked_kernel<%d, %d, %s>", CIN, COUT, FIELDS ? "true" : "false");
  hipLaunchKernelGGL((conv_s2_halo_dgrad_chunked_kernel<CIN, COUT, FIELDS>), dim3((unsigned)blocks), dim3(512), lds, stream, p);
  return 0;
}

// operands and the grid of 8 x 64 input-pixel tiles both input-gradient kernels walk
static HaloDgradParams halo_dgrad_params(const float* dz, const float* w_hwio, const float* ymask, float* dx, int groups,
                                         int64_t gs_dz, int64_t gs_w, int64_t gs_dx, int N, int H, int W) {
  HaloDgradParams p = {};
  p.dz = dz; p.w = w_hwio; p.mask = ymask; p.dx = dx;
  p.gs_dz = gs_dz; p.gs_w = gs_w; p.gs_dx = gs_dx;
  p.N = N; p.H = H; p.W = W; p.Ho = H / 2; p.Wo = W / 2;
  const HaloTileGrid tg = halo_dgrad_grid(groups, N, H, W, 0);      // 8 x 64 input-pixel tiles: conv_halo_plan.h
  p.tiles_x = tg.tiles_x; p.tiles_y = tg.tiles_y;
  p.tiles_per_group = tg.tiles_per_group;
  p.ntiles = tg.ntiles;
  return p;
}

// geeco_halo_dgrad_handles (conv_halo_plan.h): does the dispatcher below take this shape (given the HWIO kernel)?  Such layers
// never read the transposed copy.
int geeco_try_halo_dgrad(const float* dz, const float* w_hwio, const float* ymask, float* dx, int groups,
                         int64_t gs_dz, int64_t gs_w, int64_t gs_dx, int N, int H, int W, int Cin, int Cout,
                         int stride, hipStream_t stream, int* handled) {
  *handled = 0;
  if (!w_hwio || !geeco_halo_dgrad_handles(H, W, Cin, Cout, stride)) return 0;
  HaloDgradParams p = halo_dgrad_params(dz, w_hwio, ymask, dx, groups, gs_dz, gs_w, gs_dx, N, H, W);
  if (Cin == 48) {        // conv3
    int rc = launch_dgrad_chunked<48, 64>(p, stream);
    if (rc) return rc;
  } else {                // conv2
    const size_t lds = halo_dgrad_lds_bytes(32, 48);
    if (int rc = geeco_lds_opt_in<&conv_s2_halo_dgrad_kernel<32, 48>>(lds)) return rc;
    const int blocks = halo_blocks(p.ntiles, 256);
    geeco_note_kernel("conv_s2_halo_dgrad_kernel<32, 48>");
    hipLaunchKernelGGL((conv_s2_halo_dgrad_kernel<32, 48>), dim3((unsigned)blocks), dim3(512), lds, stream, p);
  }
  GEECO_LAUNCH_CHECK();
  *handled = 1;
  return 0;
}

extern "C" int geeco_conv3_dgrad_relu_fields(const float* dz, const float* w, const uint16_t* y2_fields, float* dx,
                                             int groups, int64_t gs_dz, int64_t gs_w, int64_t gs_fields, int64_t gs_dx,
                                             int N, int H, int W, void* stream, int reserved_cus) {
  GEECO_CHECK_ARG(dz && w && y2_fields && dx, "conv3_dgrad_relu_fields: null pointer");
  GEECO_CHECK_ARG(groups >= 1 && N >= 1 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0,
                  "conv3_dgrad_relu_fields: H = %d, W = %d must be even", H, W);
  HaloDgradParams p = halo_dgrad_params(dz, w, nullptr, dx, groups, gs_dz, gs_w, gs_dx, N, H, W);
  p.fields = y2_fields; p.gs_fields = gs_fields; p.fHp = (H + 7) / 8 * 8; p.fWp = (W + 63) / 64 * 64;
  if (int e = geeco_enter_reserved_cus(reserved_cus)) return e;
  int rc = launch_dgrad_chunked<48, 64, true>(p, (hipStream_t)stream);
  geeco_leave_reserved_cus();
  if (rc) return rc;
  GEECO_LAUNCH_CHECK();
  return 0;
}
