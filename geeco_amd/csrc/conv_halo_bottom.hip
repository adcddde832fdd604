// The fused bottom of the encoder's backward (family: conv_halo_common.h): conv2's input gradient and conv1's filter/bias
// gradient in one kernel, conv2_dgrad_conv1_wgrad_kernel, and its entry points geeco_conv2_dgrad_conv1_wgrad*.
// Every instantiation and launch form against float64 at small shapes: tests/native/conv_bottom_cases.txt.
#define GEECO_ZERO_PAGE g_zero_page_bottom
#include "conv_halo_common.h"
#include "conv_internal.h"

// ------------------------------------------------------------------------------------------------
// conv2 input gradient FUSED with conv1's filter/bias gradient (encoder bottom: conv1 4->32 s1, conv2 32->48 s2).
//   dz1 = (y1 > 0) * conv2_dgrad(dz2)          dw1[(tap, c)][co] = sum_p x[p + tap][c] dz1[p][co]     db1 = sum_p dz1[p]
// conv1 has no input gradient (its input is data), so dz1 has exactly one consumer; produced and consumed inside one
// kernel it never goes to HBM: the unfused pair writes and re-reads 805 MB per step and needs a second launch.
// Built on conv_s2_halo_dgrad_kernel (same tiles, resident kernel, dz2 halo, MFMA schedule).  Per tile the block
// also stages the 10 x 66 halo of conv1's input x (RGB padded to 4 channels) by LDS-DMA, double buffered.
// The dgrad MFMAs take the dz2 halo as the A operand (rows = 16 pixels of one parity class) and the kernel as B
// (columns = 16 conv1 channels), so a lane (r, q) ends up with dz1[pixels 4 q + 0..3][channel r]: register s of that
// accumulator IS the B operand (k = pixel, j = channel) of the filter-gradient MFMA whose k-group s takes the pixels
// {4 q + s}: no transposition, no LDS staging between the two products.  The A operand of that MFMA (rows = the 27
// (tap, RGB) columns) is read from the x halo at the same permuted pixels.  4 accumulator tiles (2 column tiles x 2
// channel tiles) live for the block's whole tile range; at the end the 8 waves are summed through LDS into one slab
// per block (wgrad_reduce_kernel adds the slabs in a fixed order).
// ------------------------------------------------------------------------------------------------
struct FusedBottomParams {
  const float* dz;      // dz2 [G][N][Ho][Wo][48]
  const float* w;       // conv2 kernel HWIO [G][9][32][48]
  const float* mask;    // y1 [G][N][H][W][32]
  const unsigned* bits; // BITS kernels: y1's ReLU sign bits [G][N][Hp][Wp] (geeco_conv1_fwd_relu_bits) instead of y1
  long long gs_bits;
  int Wp, Hp;
  const float* x;       // conv1 input [G][N][H][W][4]
  float* part;          // [G][S][9*CREAL*32 + 32]
  float* dx;            // optional: also store dz1 (null in training)
  long long gs_dz, gs_w, gs_y, gs_x;
  int N, H, W, Ho, Wo;
  int tiles_x, tiles_y, tiles_per_group, S;
  int S0, per, groups;          // slicing as HaloWgradParams (bottom_slices())
  unsigned long long* stamps;   // -DGEECO_STAMPS builds only (scripts/dev/fused_stamps.py)
};

constexpr int FB_WP = 14, FB_PLANE = 176, FB_XW = 67, FB_XPIECES = (10 * FB_XW + 63) / 64;
constexpr size_t FB_LDS_BYTES = (size_t)(9 * 32 * FB_WP + 2 * 12 * FB_PLANE + 2 * FB_XPIECES * 64) * 16;

#define FSTAMP(i) HALO_STAMP(g == 0 ? split : -1, i)      // encoder 0: per-tile timeline of waves 0 and 4 of every slice

// CREAL = real input channels of conv1 (3: RGB padded to 4, the pad column is skipped; 4: RGB-D)
// BITS: the ReluGrad mask comes as one sign-bit word per pixel (2 KB per tile) instead of y1 itself (64 KB per tile,
// 805 MB per step: the kernel's largest read by far, and what its waves queue behind in the vector-memory pipe)
template <int CREAL, bool BITS>
__global__ __launch_bounds__(512) void conv2_dgrad_conv1_wgrad_kernel(const FusedBottomParams p) {
  constexpr int CIN = 32, COUT = 48;
  constexpr int NT = 512;
  constexpr int COQ = COUT / 4;
  constexpr int KB = COUT / 16;
  constexpr int HR = 5, HC = 33;                       // dz2 halo rows / cols
  // A ds_read_b128 is served in four groups of 16 lanes, each with every r = lane & 15 once from two neighbouring
  // q = lane >> 4 (MI355X_MICROARCH.md, LDS): the group is conflict free iff both q hit the same 16-granule phase, i.e.
  // the plane pitch of the dz2 halo ([co quad q][row][col]) is a multiple of 16 granules (165 -> 176; measured
  // SQ_LDS_BANK_CONFLICT 49 % of the LDS cycles with 165), and the kernel row pitch WP gives (WP r + q) mod 16 distinct
  // over a group: 14 does (even phases for one q, odd for the other), 15 left one 2-way conflict per read.
  constexpr int PLANE_USED = HR * HC;                  // 165
  constexpr int PLANE = FB_PLANE;                      // 176
  // The staging stores (ds_write_b128: 8 consecutive lanes per LDS cycle group, banks = dword address mod 32, i.e. granule
  // mod 8) put the 8 - 12 co quads of ONE halo pixel side by side: with every plane at the same phase all 8 lanes of a
  // group hit one granule slot mod 8 (8-way conflict: 64 instead of 8 LDS cycles per store, 32 such stores per tile from
  // the 8 waves inside four MFMA steps; round-2 PMC: 41.8 % of this kernel's LDS cycles were conflict cycles).  The read
  // side only needs the planes of a quad PAIR (4 kb + {0, 1}, 4 kb + {2, 3}) at one phase mod 16, so pair m is skewed by
  // SKEW * m granules inside its 176-granule slot: the stores are 2-way (16 LDS cycles, under their 13-cycle issue cost)
  // and the fragment reads stay conflict free.
  constexpr int SKEW = 2;
  static_assert(PLANE >= PLANE_USED + SKEW * (COQ / 2 - 1) && PLANE % 16 == 0, "plane pitch");
  constexpr int HALO_USED = COQ * PLANE_USED;          // 1980 granules are loaded
  constexpr int HALO_F4 = COQ * PLANE;                 // 2112 granules per buffer
  constexpr int NLOAD = (HALO_USED + NT - 1) / NT;
  constexpr int WP = FB_WP;
  constexpr int W_F4 = 9 * CIN * WP;                   // 4032
  // x halo of the 8 x 64 pixel tile (conv1: stride 1, pad 1): 10 rows x 66 pixels, one pixel = RGB0 = one granule.
  // Row pitch 67 pixels = 268 floats = 12 (mod 64): the 16 (tap, channel) offsets a ds_read_b32 spreads over its r
  // lanes then span < 32 banks in each column tile and the pixel stride between q neighbours is 32 floats.
  constexpr int XH = 10, XW = FB_XW, XUSED = 66;
  constexpr int X_F4 = XH * XW;                        // 670 granules
  constexpr int NXP = FB_XPIECES;                      // 11 DMA pieces
  constexpr int SX_F4 = NXP * 64;                      // 704 (padded)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  f32x4* sW = reinterpret_cast<f32x4*>(smem);
  f32x4* sH = sW + W_F4;                               // 2 dz2 halo buffers
  f32x4* sX = sH + 2 * HALO_F4;                        // 2 x halo buffers

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int row = wid & 3, half = wid >> 2;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  // regular blocks: `per` tiles of one encoder; the remainder block: what they leave over, encoder after encoder
  const int nreg = p.S0 * p.groups;
  const bool regular = (int)blockIdx.x < nreg;
  const int nseg = regular ? 1 : p.groups;
#pragma unroll 1
  for (int seg = 0; seg < nseg; ++seg) {
  const int g = regular ? (int)blockIdx.x / p.S0 : seg;
  const int split = regular ? (int)blockIdx.x - g * p.S0 : p.S0;
  int tile = regular ? split * p.per : p.S0 * p.per;
  const int tend = regular && tile + p.per < p.tiles_per_group ? tile + p.per : p.tiles_per_group;
  const long long slab = 9 * CREAL * 32 + 32;       // [tap][real channel][32] + bias
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

  // dz2 halo staging (register staged, as conv_s2_halo_dgrad_kernel)
  int l_off[NLOAD], l_src[NLOAD];
  short l_hy[NLOAD], l_hx[NLOAD];
#pragma unroll
  for (int i = 0; i < NLOAD; ++i) {
    int idx = tid + NT * i;
    int pix = idx / COQ, cq = idx - pix * COQ;
    int hy = pix / HC, hx = pix - hy * HC;
    // lanes beyond the halo: row marker that fails every bounds test (they fetch the zero page) and a pad granule of
    // plane 0 as their LDS slot, so that neither the load nor the store needs a predicate
    l_hy[i] = (short)(idx < HALO_USED ? hy : 30000); l_hx[i] = (short)hx;
    l_off[i] = (idx < HALO_USED) ? cq * PLANE + SKEW * (cq >> 1) + hy * HC + hx : PLANE_USED + (tid & 7);
    l_src[i] = (hy * p.Wo + hx) * COUT + cq * 4;
  }
  f32x4 stage[NLOAD];
  auto load_halo_i = [&](int i, int n_, int ty_, int tx_) {
    const int oy0 = ty_ * 4 - 1, ox0 = tx_ * 32 - 1;
    const float* zg = p.dz + (long long)g * p.gs_dz + (((long long)n_ * p.Ho + oy0) * p.Wo + ox0) * COUT;
    int oy = oy0 + l_hy[i], ox = ox0 + l_hx[i];
    bool v = (unsigned)oy < (unsigned)p.Ho && (unsigned)ox < (unsigned)p.Wo;
    stage[i] = *reinterpret_cast<const f32x4*>(v ? zg + l_src[i] : g_zero_page);     // TF SAME zero padding
  };
  auto load_halo = [&](int n_, int ty_, int tx_) {
#pragma unroll
    for (int i = 0; i < NLOAD; ++i) load_halo_i(i, n_, ty_, tx_);
  };
  // x halo: LDS-DMA, pieces wid and wid + 8 (11 pieces): lane -> halo pixel (hy, hx), row-major with pitch XW
  auto dma_x = [&](int n_, int ty_, int tx_, f32x4* dst) {
    const int y0 = ty_ * 8 - 1, x0 = tx_ * 64 - 1;
    const float* xg = p.x + (long long)g * p.gs_x + (long long)n_ * p.H * p.W * 4;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int k = wid + 8 * i;                       // wave-uniform
      if (k < NXP) {
        const int idx = k * 64 + lane;
        const int hy = idx / XW, hx = idx - hy * XW;
        const int iy = y0 + hy, ix = x0 + hx;
        const bool v = idx < X_F4 && hx < XUSED && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
        const float* src = v ? xg + ((long long)iy * p.W + ix) * 4 : g_zero_page;
        __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(dst + k * 64), 16, 0, 0);
      }
    }
  };
  {
    const f32x4* wg = reinterpret_cast<const f32x4*>(p.w + (long long)g * p.gs_w);
    for (int e = tid; e < 9 * CIN * COQ; e += NT) {
      int rowi = e / COQ, c4 = e - rowi * COQ;
      sW[rowi * WP + c4] = wg[e];
    }
  }
  if (tile < tend) {
    dma_x(n, ty, tx, sX);
    load_halo(n, ty, tx);
#pragma unroll
    for (int i = 0; i < NLOAD; ++i) sH[l_off[i]] = stage[i];
  }

  // conv1 wgrad: only the 9 * CREAL real (tap, channel) columns are computed (RGB: the 4th input channel is
  // padding): lane's columns jj = 16 tj + r = CREAL tap + c and their offsets inside the x halo
  constexpr int NCOL = 9 * CREAL;
  constexpr int NJ = (NCOL + 15) / 16;
  int xoff[NJ];
#pragma unroll
  for (int tj = 0; tj < NJ; ++tj) {
    const int jj = 16 * tj + r;
    const int tap = jj / CREAL, c = jj - tap * CREAL;
    const int ky = tap / 3, kx = tap - ky * 3;
    xoff[tj] = jj < NCOL ? ((ky * XW + kx) << 2) + c : 0;    // columns >= NCOL: any valid address, never stored
  }
  f32x4 accw[NJ][2];    // [column tile][channel tile]: lane (r, q) register k = dw1[column 16 j + 4 q + k][channel 16 t + r]
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int t = 0; t < 2; ++t) accw[j][t] = zero4;
  float dbl[2] = {0.f, 0.f};

  // BITS: sign words of the wave's outputs, 8 consecutive pixels x = xb .. xb + 7 of both rows (class pixel (px, k) <->
  // word px + 2 k); those of the NEXT tile are loaded during the current tile's MFMA loop (mbn)
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  u32x4 mb[2][2], mbn[2][2];
  // (rows and columns of the word array are padded to whole tiles and the padding is zero: no bounds logic here)
  auto bits_row = [&](int py, int n_, int ty_, int tx_) {
    const int y = 2 * (ty_ * 4 + row) + py;
    return p.bits + (long long)g * p.gs_bits + ((long long)n_ * p.Hp + y) * p.Wp + 2 * (tx_ * 32 + 16 * half + 4 * q);
  };
  if constexpr (BITS) {
    if (tile < tend) {
#pragma unroll
      for (int m = 0; m < 4; ++m)
        mb[m >> 1][m & 1] = *reinterpret_cast<const u32x4*>(bits_row(m >> 1, n, ty, tx) + 4 * (m & 1));
    }
  }
  dma_barrier();
  const int a_lane = q * PLANE + SKEW * (q >> 1) + (row + 1) * HC + 16 * half + r + 1;
  const int b_lane = r * WP + q;
  int buf = 0;
  int tcount = 0;
  for (; tile < tend; ++tile, ++tcount) {
    const bool more = tile + 1 < tend;
    int n2 = n, ty2 = ty, tx2 = tx;
    FSTAMP(tcount < 10 ? 6 * tcount + 0 : 64);
    if (more) advance(n2, ty2, tx2);
    // ReluGrad mask of this wave's outputs in the accumulator layout: class c = (py, px), pixel j = 4 q + k of the
    // wave's 16 class pixels (x = 2 (tx 32 + 16 half + j) + px), channel 16 t + r.  A wave that issues all its global
    // loads at the top of the tile sits in vector-memory back-pressure for ~4 k cycles (in-kernel timeline,
    // scripts/dev/fused_stamps.py) while its SIMD's MFMA pipe idles, so every global load of the tile - the next
    // dz2 halo, the next x halo, the 32 mask dwords - is issued from inside the MFMA loop, two per step.
    // Pixels outside the image contribute nothing to dw1: the load address is clamped, the value zeroed by okf.
    const int yb = 2 * (ty * 4 + row), xb = 2 * (tx * 32 + 16 * half + 4 * q);
    const float* mbase[2];
    float oky[2];
    int moff[2][4];
    float okx[2][4];
#pragma unroll
    for (int py = 0; py < 2; ++py) {
      const int y = yb + py, yc = y < p.H ? y : p.H - 1;
      mbase[py] = p.mask + (long long)g * p.gs_y + ((long long)n * p.H + yc) * p.W * CIN;
      oky[py] = y < p.H ? 1.f : 0.f;
    }
#pragma unroll
    for (int px = 0; px < 2; ++px)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int x = xb + px + 2 * k, xc = x < p.W ? x : p.W - 1;
        moff[px][k] = xc * CIN + r;
        okx[px][k] = x < p.W ? 1.f : 0.f;
      }
    f32x4 mk[BITS ? 1 : 4][2];
    float xv[4][4][NJ];       // x halo operands of the filter-gradient MFMAs, read one step before their class starts
    const float* xt = reinterpret_cast<const float*>(sX + buf * SX_F4);
    f32x4 acc[4][2];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int t = 0; t < 2; ++t) acc[c][t] = zero4;
    const f32x4* hA = sH + buf * HALO_F4 + a_lane;
    const f32x4* hB = sW + b_lane;
    f32x4* hN = sH + (buf ^ 1) * HALO_F4;
    f32x4 a_cur, b_cur[2], a_nxt, b_nxt[2];
    // Tap order: the parity classes of the input gradient complete one after the other - class 3 = (odd, odd) has the
    // centre tap only, class 2 taps 3 / 5, class 1 taps 1 / 7, class 0 the four corners - so that (BITS) the
    // filter-gradient work of a finished class (mask, 16 MFMAs, 4 per step) runs inside the loop next to the taps of
    // the following class instead of as a latency-bound tail after it.
    constexpr int ORDER[9] = {4, 3, 5, 1, 7, 0, 2, 6, 8};
    auto frag = [&](int it, f32x4& a, f32x4 (&b)[2]) {
      const int tap = ORDER[it / KB], kb = it % KB;
      const int ky = tap / 3, kx = tap - ky * 3;
      a = hA[kb * (4 * PLANE + 2 * SKEW) - (ky >> 1) * HC - (kx >> 1)];
      b[0] = hB[(tap * CIN) * WP + 4 * kb];
      b[1] = hB[(tap * CIN + 16) * WP + 4 * kb];
    };
    constexpr int NIT = 9 * KB;
    f32x4 vv[2];              // dz1 of the class in flight: lane (r, q) register k = pixel 4 q + k, channel 16 t + r
    auto class_x = [&](int c) {         // class c's x operands: k-group s <-> class pixel 4 q + s
      const int py = c >> 1, px = c & 1;
      const float* xs = xt + (((2 * row + py) * XW + 2 * (16 * half + 4 * q) + px) << 2);
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int j = 0; j < NJ; ++j) xv[c][s][j] = xs[((2 * s) << 2) + xoff[j]];
    };
    auto class_mask = [&](int c) {      // ReluGrad of class c's finished accumulators -> vv, bias gradient
      const int py = c >> 1, px = c & 1;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if constexpr (BITS) {
          // channel 16 t + r <-> bit (r & 3) * 8 + (r >> 2) + 4 t of the pixel's word; bfe_i32 gives 0 / all ones
          // (pixels outside the image have zero words: they contribute nothing to dw1)
          const int wi = px + 2 * k;
          const unsigned word = mb[py][wi >> 2][wi & 3];
          const int sh = (r & 3) * 8 + (r >> 2);
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            const int keep = __builtin_amdgcn_sbfe((int)word, sh + 4 * t, 1);
            vv[t][k] = __int_as_float(__float_as_int(acc[c][t][k]) & keep);
            dbl[t] += vv[t][k];
          }
        } else {
          const float okf = okx[px][k] * oky[py];
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            vv[t][k] = mk[c][t][k] * okf > 0.f ? acc[c][t][k] : 0.f;
            dbl[t] += vv[t][k];
          }
        }
      }
      if (p.dx) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int y = yb + py, x = xb + px + 2 * k;
          if (y < p.H && x < p.W) {
            float* o = p.dx + (long long)g * p.gs_y + (((long long)n * p.H + y) * p.W + x) * CIN + r;
            o[0] = vv[0][k];
            o[16] = vv[1][k];
          }
        }
      }
    };
    auto class_mfma = [&](int c, int s) {   // k-group s of class c: k index q <-> class pixel 4 q + s
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int t = 0; t < 2; ++t)
          accw[j][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[c][s][j], vv[t][s], accw[j][t], 0, 0, 0);
    };
    __builtin_amdgcn_sched_barrier(0);
    FSTAMP(tcount < 10 ? 6 * tcount + 1 : 64);
    frag(0, a_cur, b_cur);
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      if (it + 1 < NIT) frag(it + 1, a_nxt, b_nxt);
      if (more && it >= NIT - NLOAD - 4 && it < NIT - 4) {
        const int j = it - (NIT - NLOAD - 4);
        hN[l_off[j]] = stage[j];
      }
      if (more && it < NLOAD) load_halo_i(it, n2, ty2, tx2);
      if (more && it == NLOAD) dma_x(n2, ty2, tx2, sX + (buf ^ 1) * SX_F4);
      if constexpr (BITS) {
        if (more && it > NLOAD && it <= NLOAD + 4) {  // the NEXT tile's sign words: 4 x 16 B per lane
          const int m = it - NLOAD - 1;
          mbn[m >> 1][m & 1] = *reinterpret_cast<const u32x4*>(bits_row(m >> 1, n2, ty2, tx2) + 4 * (m & 1));
        }
        if (it >= NIT - 4) class_x(it - (NIT - 4));
      } else {
        if (it > NLOAD && it <= NLOAD + 16) {         // two mask dwords per step: (class, pixel k) of both channel tiles
          const int m = it - NLOAD - 1, c = m >> 2, k = m & 3;
          const float* mp = mbase[c >> 1] + moff[c & 1][k];
          mk[c][0][k] = mp[0];
          mk[c][1][k] = mp[16];
        }
        if (it >= NIT - 4) class_x(it - (NIT - 4));
      }
      __builtin_amdgcn_sched_barrier(0);
      {
        const int tap = ORDER[it / KB];
        const int ky = tap / 3, kx = tap - ky * 3;
        const int c = (ky & 1) * 2 + (kx & 1);
        // D[i = pixel][j = channel]: A = dz2 halo (i = pixel r, k = co quad q), B = kernel (k, j = channel r)
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int t = 0; t < 2; ++t)
            acc[c][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[s], b_cur[t][s], acc[c][t], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
      a_cur = a_nxt;
      b_cur[0] = b_nxt[0];
      b_cur[1] = b_nxt[1];
    }
    FSTAMP(tcount < 10 ? 6 * tcount + 2 : 64);
    // ---- the classes still open: ReluGrad, then conv1's filter gradient straight from the accumulators ----------
#pragma unroll
    for (int c = 3; c >= 0; --c) {     // class order 3, 2, 1, 0 (the filter-gradient work of a finished class INSIDE the MFMA loop measured 484 vs 466 us: profiles/NEGATIVE_RESULTS.md)
      class_mask(c);
#pragma unroll
      for (int s = 0; s < 4; ++s) class_mfma(c, s);
    }
    if constexpr (BITS) {
      if (more) {
#pragma unroll
        for (int m = 0; m < 4; ++m) mb[m >> 1][m & 1] = mbn[m >> 1][m & 1];
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    FSTAMP(tcount < 10 ? 6 * tcount + 3 : 64);
    dma_barrier();      // end of tile: next dz2 / x halos complete; everyone is done with this tile's buffers
    FSTAMP(tcount < 10 ? 6 * tcount + 4 : 64);
    n = n2; ty = ty2; tx = tx2;
    buf ^= 1;
  }

  // ---- block reduction of conv1's gradient: [wave 8][2 NJ tiles][64 lanes] float4 (<= 48 KB) in the dz2 halo area ----
  __syncthreads();
  f32x4* sR = sH;
  constexpr int NTL = 2 * NJ;
  float* sD = reinterpret_cast<float*>(sR + 8 * NTL * 64);    // [wave 8][32 channels]
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int t = 0; t < 2; ++t) sR[(wid * NTL + j * 2 + t) * 64 + lane] = accw[j][t];
  // bias gradient: lane (r, q) holds the sum over its pixels for channels r and 16 + r; fold the 4 q lanes
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    dbl[t] += __shfl_xor(dbl[t], 16);
    dbl[t] += __shfl_xor(dbl[t], 32);
  }
  if (q == 0) {
    sD[wid * 32 + r] = dbl[0];
    sD[wid * 32 + 16 + r] = dbl[1];
  }
  __syncthreads();
  for (int e = tid; e < NTL * 64; e += NT) {
    const int ln = e & 63, k = e >> 6;
    f32x4 s4 = sR[(0 * NTL + k) * 64 + ln];
#pragma unroll
    for (int w = 1; w < 8; ++w) s4 += sR[(w * NTL + k) * 64 + ln];
    const int j = k >> 1, t = k & 1;
    const int co = 16 * t + (ln & 15);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int jj = 16 * j + 4 * (ln >> 4) + kk;
      if (jj < NCOL) part[jj * 32 + co] = s4[kk];     // slab layout [tap][real channel][32]: row jj
    }
  }
  if (tid < 32) {
    float s1 = 0.f;
    for (int w = 0; w < 8; ++w) s1 += sD[w * 32 + tid];
    part[NCOL * 32 + tid] = s1;
  }
  __syncthreads();     // the next segment stages into the area this one's sums were just read from
  }
}

extern "C" int64_t geeco_conv2_dgrad_conv1_wgrad_ws_bytes(int groups) {
  return (int64_t)groups * bottom_slices(groups, 0, true).S * (9 * 4 * 32 + 32) * 4;
}

// y1 (ReluGrad mask = conv1's output) or y1_bits (its sign bits): exactly one is given
static int fused_bottom_impl(const float* dz2, const float* w2, const float* y1, const uint32_t* y1_bits,
                             const float* x, float* dw1, float* db1, float* dz1, int groups, int64_t gs_dz2,
                             int64_t gs_w2, int64_t gs_y1, int64_t gs_bits, int64_t gs_x, int64_t gs_dw1, int64_t gs_db1,
                             int N, int H, int W, int real_channels, void* ws, void* stream) {
  GEECO_CHECK_ARG(dz2 && w2 && (y1 || y1_bits) && x && dw1 && db1 && ws, "conv2_dgrad_conv1_wgrad: null pointer");
  GEECO_CHECK_ARG(real_channels == 3 || real_channels == 4, "conv2_dgrad_conv1_wgrad: real_channels = %d (3 or 4)",
                  real_channels);
  GEECO_CHECK_ARG(groups >= 1 && N >= 1 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0,
                  "conv2_dgrad_conv1_wgrad: H = %d, W = %d must be even", H, W);
  FusedBottomParams p = {};
  p.dz = dz2; p.w = w2; p.mask = y1; p.x = x; p.part = (float*)ws; p.dx = dz1;
  p.bits = y1_bits; p.gs_bits = gs_bits; p.Wp = (int)geeco_relu_bits_pitch(W); p.Hp = (int)geeco_relu_bits_rows(H);
  p.gs_dz = gs_dz2; p.gs_w = gs_w2; p.gs_y = gs_y1; p.gs_x = gs_x;
  // tile grid and slicing: conv_wgrad_plan.h (plain C++ the host tests evaluate), on the CUs this call may occupy
  const FusedBottomLaunchPlan lp = fused_bottom_launch_plan(WGRAD_CUS - geeco_call_reserved_cus(), groups, N, H, W);
  p.N = N; p.H = H; p.W = W; p.Ho = H / 2; p.Wo = W / 2;
  p.tiles_x = lp.tiles_x; p.tiles_y = lp.tiles_y; p.tiles_per_group = lp.tiles;
  p.S = lp.S; p.S0 = lp.S0; p.per = lp.per; p.groups = groups;
  const size_t lds = FB_LDS_BYTES;
  // all four instantiations on the first call, as ever: none is left to opt in on a later call (inside a graph capture, say)
  int rc = geeco_lds_opt_in<&conv2_dgrad_conv1_wgrad_kernel<3, false>>(lds);
  if (!rc) rc = geeco_lds_opt_in<&conv2_dgrad_conv1_wgrad_kernel<4, false>>(lds);
  if (!rc) rc = geeco_lds_opt_in<&conv2_dgrad_conv1_wgrad_kernel<3, true>>(lds);
  if (!rc) rc = geeco_lds_opt_in<&conv2_dgrad_conv1_wgrad_kernel<4, true>>(lds);
  if (rc) return rc;
  p.stamps = geeco_arm_halo_stamps();
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)lp.blocks);
  const bool bits = y1_bits != nullptr;
  geeco_note_kernel("conv2_dgrad_conv1_wgrad_kernel<%d, %s>", real_channels == 3 ? 3 : 4, bits ? "true" : "false");
  if (real_channels == 3 && bits)
    hipLaunchKernelGGL((conv2_dgrad_conv1_wgrad_kernel<3, true>), grid, dim3(512), lds, s, p);
  else if (real_channels == 3)
    hipLaunchKernelGGL((conv2_dgrad_conv1_wgrad_kernel<3, false>), grid, dim3(512), lds, s, p);
  else if (bits)
    hipLaunchKernelGGL((conv2_dgrad_conv1_wgrad_kernel<4, true>), grid, dim3(512), lds, s, p);
  else
    hipLaunchKernelGGL((conv2_dgrad_conv1_wgrad_kernel<4, false>), grid, dim3(512), lds, s, p);
  GEECO_LAUNCH_CHECK();
  geeco_launch_wgrad_reduce((const float*)ws, dw1, db1, gs_dw1, gs_db1, p.S, 9 * real_channels * 32, 32, groups, s);
  GEECO_LAUNCH_CHECK();
  return 0;
}

extern "C" int geeco_conv2_dgrad_conv1_wgrad(const float* dz2, const float* w2, const float* y1, const float* x,
                                             float* dw1, float* db1, float* dz1, int groups, int64_t gs_dz2,
                                             int64_t gs_w2, int64_t gs_y1, int64_t gs_x, int64_t gs_dw1,
                                             int64_t gs_db1, int N, int H, int W, int real_channels, void* ws,
                                             void* stream) {
  GEECO_CHECK_ARG(y1, "conv2_dgrad_conv1_wgrad: null y1");
  return fused_bottom_impl(dz2, w2, y1, nullptr, x, dw1, db1, dz1, groups, gs_dz2, gs_w2, gs_y1, 0, gs_x, gs_dw1, gs_db1,
                           N, H, W, real_channels, ws, stream);
}

extern "C" int geeco_conv2_dgrad_conv1_wgrad_partial(const float* dz2, const float* w2, const float* y1, const float* x,
                                                     float* dw1, float* db1, float* dz1, int groups, int64_t gs_dz2,
                                                     int64_t gs_w2, int64_t gs_y1, int64_t gs_x, int64_t gs_dw1,
                                                     int64_t gs_db1, int N, int H, int W, int real_channels, void* ws,
                                                     void* stream, geeco_slab_reduce* pending, int reserved_cus) {
  GEECO_CHECK_ARG(pending && y1, "conv2_dgrad_conv1_wgrad_partial: null pending / y1");
  if (int e = geeco_enter_reserved_cus(reserved_cus)) return e;
  geeco_slab_reduce none = {};
  *pending = none;
  geeco_set_pending_reduce(pending);
  const int rc = fused_bottom_impl(dz2, w2, y1, nullptr, x, dw1, db1, dz1, groups, gs_dz2, gs_w2, gs_y1, 0, gs_x, gs_dw1,
                                   gs_db1, N, H, W, real_channels, ws, stream);
  geeco_set_pending_reduce(nullptr);
  geeco_leave_reserved_cus();
  return rc;
}

extern "C" int geeco_conv2_dgrad_conv1_wgrad_bits(const float* dz2, const float* w2, const uint32_t* y1_bits,
                                                  const float* x, float* dw1, float* db1, int groups, int64_t gs_dz2,
                                                  int64_t gs_w2, int64_t gs_bits, int64_t gs_x, int64_t gs_dw1,
                                                  int64_t gs_db1, int N, int H, int W, int real_channels, void* ws,
                                                  void* stream, geeco_slab_reduce* pending, int reserved_cus) {
  GEECO_CHECK_ARG(y1_bits, "conv2_dgrad_conv1_wgrad_bits: null y1_bits");
  if (int e = geeco_enter_reserved_cus(reserved_cus)) return e;
  if (pending) {
    geeco_slab_reduce none = {};
    *pending = none;
    geeco_set_pending_reduce(pending);
  }
  const int rc = fused_bottom_impl(dz2, w2, nullptr, y1_bits, x, dw1, db1, nullptr, groups, gs_dz2, gs_w2, 0, gs_bits, gs_x,
                                   gs_dw1, gs_db1, N, H, W, real_channels, ws, stream);
  if (pending) geeco_set_pending_reduce(nullptr);
  geeco_leave_reserved_cus();
  return rc;
}
