// 3x3 convolution forward / input-gradient as an implicit GEMM on f32 MFMA (gfx950).
//
// Replaces tf.layers.conv2d(kernel_size=3, padding='SAME') + bias + ReLU
// (reference src/models/e2evmc/graph.py:76-115) and its Conv2DBackpropInput + ReluGrad.
//
// GEMM view:  out[m][n] = sum_k A[m][k] * B[k][n]
//   m = (image, Y', X') output position,  k = (tap, channel),  n = output channel.
//   A is never materialised: each K-step gathers, per row m, BK contiguous channels of the source
//   pixel addressed by the tap (zero outside the image => TF SAME padding).
//   B = kernel slabs [tap][C][Nout] row-major (HWIO for forward, HWOI for dgrad).
// Forward and dgrad differ only by the tap table and the source/destination strides (dgrad of a
// stride-s conv = s*s parity classes, each a dense gather-GEMM over its own subset of taps), so
// one kernel serves both.
//
// MFMA mapping (v_mfma_f32_16x16x4_f32): roles are swapped so that D = W^T . A^T, i.e. the MFMA
// "row" index is the output channel and the "column" (lane & 15) is the pixel: each lane then owns
// 4 consecutive output channels of one pixel => one 16-byte NHWC store per tile.
//
// LDS images (double buffered):
//   sA[plane = k/4][row m][4 floats], rows XOR-swizzled by (plane & 3): ds_read_b128 of a 16-row
//       fragment hits 16 distinct 16-byte slots (conflict free), ds_write_b128 is 2-way.
//   sB[k][BN + 4]: ds_read_b32, row pitch = 4 (mod 8) dwords => the two k-rows of a 32-lane half
//       land in different bank halves (conflict free).
#include "geeco_common.h"
#include "conv_gemm_plan.h"
#include "conv_wgrad_body.h"
#include "conv_internal.h"
#include <type_traits>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>

// UT ("uniform tap"): C % BK == 0, so every K-step lies inside ONE tap; the per-row validity and the
// source / kernel pointers are then recomputed only when the tap changes (every C/BK steps) and the
// K loop itself is pointer bumps + loads: removes most of the gather's address VALU work.
#ifdef GEECO_STAMPS
#define STAMP(i)                                                                                  \
  do {                                                                                            \
    if (threadIdx.x == 0 && p.stamps && (i) < 64) stamp_base[(i)] = __builtin_amdgcn_s_memtime(); \
  } while (0)
#else
#define STAMP(i)
#endif

static __device__ float g_gemm_zero_page[GEMM_ZERO_PAGE + 64];

// block coordinates of the 3-D launch grid (x = M tile, y = N tile x K split, z = encoder): the body takes them as arguments
// so that it can also run as part of a heterogeneous grid (conv_top_bwd_kernel below)
struct GemmBlock {
  int x, y, z, gx, gy;
};
template <int BM, int BN, int BK>
constexpr int conv_gemm_smem_floats() {
  return 2 * (BM * BK + BK * (BN + 4)) + 60;
}

template <int BM, int BN, int BK, int WM, int WN, bool UT>
__device__ __forceinline__ void conv_gemm_body(const ConvGemmParams& p, const GemmBlock blk, float* smem) {
#ifdef GEECO_STAMPS
  unsigned long long* stamp_base = p.stamps + ((long long)(blk.z * blk.gy + blk.y) * blk.gx + blk.x) * 64;
  STAMP(0);
  if (threadIdx.x == 0 && p.stamps) stamp_base[63] = (unsigned)__builtin_amdgcn_s_getreg(4 | (31 << 11));
#endif
  constexpr int SPR = BK / 4;     // float4 slots per row per K-step
  constexpr int RPP = 256 / SPR;  // rows staged per pass
  constexpr int PA = BM / RPP;    // A staging passes
  constexpr int LDB = BN + 4;
  constexpr int BN4 = BN / 4;
  constexpr int NB4 = BK * BN4;   // float4s in the B tile
  constexpr int PB = (NB4 + 255) / 256;
  constexpr int WPIX = BM / WM;   // pixels per wave
  constexpr int WCO = BN / WN;    // output channels per wave
  constexpr int TJ = WPIX / 16;
  constexpr int TI = WCO / 16;
  constexpr int KB = BK / 16;
  static_assert(PA >= 1 && TJ >= 1 && TI >= 1 && WM * WN == 4, "bad tile");

  float* sA = smem;
  float* sB = smem + 2 * BM * BK;
  int* sTap = reinterpret_cast<int*>(smem + 2 * (BM * BK + BK * LDB));

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int g = blk.z;
  // Input gradients (ncls == 4 parity classes with 1 / 2 / 2 / 4 taps, i.e. K loops of unequal length): all blocks of a
  // launch are co-resident and dealt to the CUs in dispatch order, so blocks L, L + 256, L + 512 share a CU - and with
  // the M tile as the fastest grid index they would be tiles of the SAME class (conv7: three 4-tap blocks on one CU,
  // three 1-tap blocks on another).  p.rot rotates the M tile index by one class per 256 blocks.
  int bx = blk.x;
  if (p.rot) {
    const int row = blk.y + blk.gy * blk.z;
    bx = (bx + (int)(((long long)row * blk.gx) >> 8) * p.rot) % blk.gx;
  }
  const float* __restrict__ xg = p.x + (long long)g * p.gs_x;
  const float* __restrict__ wg = p.w + (long long)g * p.gs_w;
  int ci = 0;
#pragma unroll
  for (int c = 1; c < 4; ++c)
    if (c < p.ncls && bx >= p.cls[c].tile0) ci = c;
  const ConvClass& cl = p.cls[ci];
  const long long clsM = cl.M;
  const int clsHc = cl.Hc, clsWc = cl.Wc, ntaps = cl.ntaps;
  const long long m0 = (long long)(bx - cl.tile0) * BM;
  const int ntile = blk.y / p.ksplit;
  const int split = blk.y - ntile * p.ksplit;
  const int n0 = ntile * BN;
  const int C = p.C, C4 = p.C >> 2;

  if (tid < 9) {
    int t = tid;
    bool ok = t < ntaps;
    sTap[t] = ok ? cl.dy[t] : 0;
    sTap[12 + t] = ok ? cl.dx[t] : 0;
    sTap[24 + t] = ok ? (cl.dy[t] * p.Ws + cl.dx[t]) * C : 0;
    sTap[36 + t] = ok ? cl.wslab[t] * C : 0;
    sTap[48 + t] = ok ? cl.wslab[t] : 0;
  }
  __syncthreads();
  STAMP(1);

  // ---- per-thread staging state -----------------------------------------------------------
  const int kq = tid % SPR;
  long long rb[PA];
  int iy0[PA], ix0[PA];
  {
    const long long HcWc = (long long)clsHc * clsWc;
#pragma unroll
    for (int j = 0; j < PA; ++j) {
      long long m = m0 + tid / SPR + j * RPP;
      if (m < clsM) {
        // 32-bit division (conv_rows_beyond_32bit: every launch checks M < 2^31): the 64-bit form is a ~150-instruction routine
        long long n = (unsigned)m / (unsigned)HcWc;
        int rem = (int)(m - n * HcWc);
        int yp = rem / clsWc;
        int xp = rem - yp * clsWc;
        iy0[j] = yp * p.ss;
        ix0[j] = xp * p.ss;
        rb[j] = ((n * p.Hs + iy0[j]) * p.Ws + ix0[j]) * (long long)C;
      } else {
        iy0[j] = -(1 << 28);
        ix0[j] = -(1 << 28);
        rb[j] = 0;
      }
    }
  }
  STAMP(2);
  const int nk_all = (ntaps * C + BK - 1) / BK;
  const int per = (nk_all + p.ksplit - 1) / p.ksplit;
  const int ks_beg = split * per;
  const int nk = ks_beg >= nk_all ? 0 : (nk_all - ks_beg < per ? nk_all - ks_beg : per);
  const int slot0 = ks_beg * SPR + kq;
  int a_tap = slot0 / C4;
  int a_cq = slot0 - a_tap * C4;

  int b_row[PB], b_c4[PB], b_tap[PB], b_c[PB];
#pragma unroll
  for (int i = 0; i < PB; ++i) {
    int idx = tid + i * 256;
    b_row[i] = idx / BN4;
    b_c4[i] = idx - b_row[i] * BN4;
    const int k0 = ks_beg * BK + b_row[i];
    b_tap[i] = k0 / C;
    b_c[i] = k0 - b_tap[i] * C;
  }

  int bt_n[PB], bt_k4[PB];      // bt: column and K quad of this thread's float4 (BK / 4 quads per column)
#pragma unroll
  for (int i = 0; i < PB; ++i) {
    const int idx = tid + i * 256;
    bt_n[i] = idx / (BK / 4);
    bt_k4[i] = idx - bt_n[i] * (BK / 4);
  }
  f32x4 ra[PA], rbv[PB];
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  // ---- UT state: current tap, channel offset inside it, per-row / per-slot pointers ----------------
  int u_tap = 0, u_cc = 0;
  const float* u_ap[PA];
  bool u_av[PA];
  const float* u_bp[PB];
  long long u_bstep[PB];
  bool u_bv[PB];
  auto ut_setup = [&]() {     // (re)derive pointers for tap u_tap at channel offset u_cc
    const int t = u_tap < 9 ? u_tap : 8;
    const bool tv = u_tap < ntaps;
    const int dy = sTap[t], dx = sTap[12 + t], toff = sTap[24 + t];
#pragma unroll
    for (int j = 0; j < PA; ++j) {
      int iy = iy0[j] + dy, ix = ix0[j] + dx;
      u_av[j] = tv && (unsigned)iy < (unsigned)p.Hs && (unsigned)ix < (unsigned)p.Ws;
      // rows outside the image (TF SAME padding, M tail) walk a zero page instead of being predicated per K-step: a
      // select per load and K-step is VALU work next to the MFMAs (the page covers a whole tap: C <= ZERO_PAGE floats)
      u_ap[j] = u_av[j] ? xg + rb[j] + toff + u_cc + kq * 4 : g_gemm_zero_page + u_cc + kq * 4;
    }
#pragma unroll
    for (int i = 0; i < PB; ++i) {
      if (p.bt) {
        // HWIO kernel w[tap][n][k]: this thread's float4 = 4 consecutive k of ONE column n (bt_n, bt_k4 below); the
        // K-step advances along the contiguous axis
        u_bv[i] = (tid + i * 256 < NB4) && tv && (n0 + bt_n[i] < p.Nout);
        u_bp[i] = u_bv[i] ? wg + ((long long)sTap[48 + t] * p.Nout + n0 + bt_n[i]) * C + u_cc + bt_k4[i] * 4 : g_gemm_zero_page;
        u_bstep[i] = u_bv[i] ? BK : 0;
      } else {
        u_bv[i] = (tid + i * 256 < NB4) && tv && (n0 + b_c4[i] * 4 < p.Nout);
        u_bp[i] = u_bv[i] ? wg + (long long)(sTap[36 + t] + u_cc + b_row[i]) * p.Nout + n0 + b_c4[i] * 4 : g_gemm_zero_page;
        u_bstep[i] = u_bv[i] ? (long long)BK * p.Nout : 0;
      }
    }
  };
  if constexpr (UT) {
    const int k0 = ks_beg * BK;
    u_tap = k0 / C;
    u_cc = k0 - u_tap * C;
    ut_setup();
  }

  auto load_tiles = [&]() {
    if constexpr (UT) {
#pragma unroll
      for (int j = 0; j < PA; ++j) ra[j] = *reinterpret_cast<const f32x4*>(u_ap[j]);
#pragma unroll
      for (int i = 0; i < PB; ++i) rbv[i] = *reinterpret_cast<const f32x4*>(u_bp[i]);
      return;
    }
    {
      const int t = a_tap < 9 ? a_tap : 8;
      const bool tv = a_tap < ntaps;
      const int dy = sTap[t], dx = sTap[12 + t], toff = sTap[24 + t] + a_cq * 4;
#pragma unroll
      for (int j = 0; j < PA; ++j) {
        int iy = iy0[j] + dy, ix = ix0[j] + dx;
        bool v = tv && (unsigned)iy < (unsigned)p.Hs && (unsigned)ix < (unsigned)p.Ws;
        ra[j] = v ? *reinterpret_cast<const f32x4*>(xg + rb[j] + toff) : zero4;
      }
    }
#pragma unroll
    for (int i = 0; i < PB; ++i) {
      bool v = (tid + i * 256 < NB4) && (b_tap[i] < ntaps) && (n0 + b_c4[i] * 4 < p.Nout);
      const int t = b_tap[i] < 9 ? b_tap[i] : 8;
      rbv[i] = v ? *reinterpret_cast<const f32x4*>(wg + (long long)(sTap[36 + t] + b_c[i]) * p.Nout + n0 +
                                                   b_c4[i] * 4)
                 : zero4;
    }
  };
  auto advance = [&]() {
    if constexpr (UT) {
      u_cc += BK;
      if (u_cc >= C) {          // wave-uniform: next tap
        u_cc = 0;
        ++u_tap;
        ut_setup();
      } else {
#pragma unroll
        for (int j = 0; j < PA; ++j) u_ap[j] += BK;
#pragma unroll
        for (int i = 0; i < PB; ++i) u_bp[i] += u_bstep[i];
      }
      return;
    }
    a_cq += SPR;
    while (a_cq >= C4) {
      a_cq -= C4;
      ++a_tap;
    }
#pragma unroll
    for (int i = 0; i < PB; ++i) {
      b_c[i] += BK;
      while (b_c[i] >= C) {
        b_c[i] -= C;
        ++b_tap[i];
      }
    }
  };
  auto store_tiles = [&](int buf) {
    float* a = sA + buf * (BM * BK);
#pragma unroll
    for (int j = 0; j < PA; ++j) {
      int row = tid / SPR + j * RPP;
      *reinterpret_cast<f32x4*>(a + (kq * BM + (row ^ (kq & 3))) * 4) = ra[j];
    }
    float* b = sB + buf * (BK * LDB);
#pragma unroll
    for (int i = 0; i < PB; ++i) {
      if (tid + i * 256 < NB4) {
        if (UT && p.bt) {        // transposing store: 4 consecutive k of column bt_n
          float* d = b + bt_k4[i] * 4 * LDB + bt_n[i];
          d[0] = rbv[i].x; d[LDB] = rbv[i].y; d[2 * LDB] = rbv[i].z; d[3 * LDB] = rbv[i].w;
        } else {
          *reinterpret_cast<f32x4*>(b + b_row[i] * LDB + b_c4[i] * 4) = rbv[i];
        }
      }
    }
  };

  // ---- main loop ---------------------------------------------------------------------------
  const int r = lane & 15, q = lane >> 4;
  const int wm = wid % WM, wn = wid / WM;
  const int pixbase = wm * WPIX;
  const int cobase = wn * WCO;

  f32x4 acc[TI][TJ];
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < TJ; ++j) acc[i][j] = zero4;

  STAMP(3);
  if (nk > 0) {
    load_tiles();
    advance();
    STAMP(4);
    store_tiles(0);
  }
  __syncthreads();
  STAMP(5);

  // The K loop is unrolled by two by hand so that the LDS buffer index is a compile-time constant: the fragment
  // addresses then are loop-invariant registers + immediates (they cost 16 VALU instructions per K-step, and every
  // VALU instruction next to f32 MFMAs costs ~4 cycles of MFMA time).
  auto kstep = [&](auto bufc, int ks) {
    constexpr int buf = decltype(bufc)::value;
    const bool more = ks + 1 < nk;
    STAMP(ks < 18 ? 6 + 3 * ks : 64);
    if (more) {
      load_tiles();
      advance();
    }
    STAMP(ks < 18 ? 7 + 3 * ks : 64);
    const float* a = sA + buf * (BM * BK);
    const float* b = sB + buf * (BK * LDB);
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      f32x4 xf[TJ];
      float wf[TI][4];
#pragma unroll
      for (int j = 0; j < TJ; ++j)
        xf[j] = *reinterpret_cast<const f32x4*>(a + ((kb * 4 + q) * BM + ((pixbase + j * 16 + r) ^ q)) * 4);
#pragma unroll
      for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int s = 0; s < 4; ++s) wf[i][s] = b[(kb * 16 + 4 * q + s) * LDB + cobase + i * 16 + r];
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
          for (int j = 0; j < TJ; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[i][s], xf[j][s], acc[i][j], 0, 0, 0);
    }
    STAMP(ks < 18 ? 8 + 3 * ks : 64);
    if (more) store_tiles(buf ^ 1);
    __syncthreads();
  };
  for (int ks = 0; ks < nk; ks += 2) {
    kstep(std::integral_constant<int, 0>{}, ks);
    if (ks + 1 < nk) kstep(std::integral_constant<int, 1>{}, ks + 1);
  }
  STAMP(60);

  // ---- epilogue: lane owns pixel (lane & 15) of tile j, channels 4*(lane>>4)..+3 of tile i ----
  float* __restrict__ og = p.out + (long long)g * p.gs_out;
  const float* __restrict__ mg = p.mask ? p.mask + (long long)g * p.gs_out : nullptr;
  const float* __restrict__ bg = p.bias ? p.bias + (long long)g * p.gs_b : nullptr;
  const long long HcWc = (long long)clsHc * clsWc;
  const int oy0 = cl.oy0, ox0 = cl.ox0;
#pragma unroll
  for (int j = 0; j < TJ; ++j) {
    long long m = m0 + pixbase + j * 16 + r;
    if (m >= clsM) continue;
    long long n = (unsigned)m / (unsigned)HcWc;
    int rem = (int)(m - n * HcWc);
    int yp = rem / clsWc;
    int xp = rem - yp * clsWc;
    long long opix = (n * p.Hd + (yp * p.ds + oy0)) * p.Wd + (xp * p.ds + ox0);
#pragma unroll
    for (int i = 0; i < TI; ++i) {
      int co = n0 + cobase + i * 16 + 4 * q;
      if (co >= p.Nout) continue;
      f32x4 v = acc[i][j];
      if (p.ksplit > 1) {   // raw partial sums; conv_splitk_epilogue applies bias / ReLU / mask
        const long long npix = (long long)p.N * p.Hd * p.Wd;
        *reinterpret_cast<f32x4*>(p.part + (((long long)split * p.groups + g) * npix + opix) * p.Nout + co) = v;
        continue;
      }
      if (bg) v += *reinterpret_cast<const f32x4*>(bg + co);
      if (p.relu) {
        v.x = fmaxf(v.x, 0.f);
        v.y = fmaxf(v.y, 0.f);
        v.z = fmaxf(v.z, 0.f);
        v.w = fmaxf(v.w, 0.f);
      }
      if (mg) {
        f32x4 mk = *reinterpret_cast<const f32x4*>(mg + opix * p.Nout + co);
        v.x = mk.x > 0.f ? v.x : 0.f;
        v.y = mk.y > 0.f ? v.y : 0.f;
        v.z = mk.z > 0.f ? v.z : 0.f;
        v.w = mk.w > 0.f ? v.w : 0.f;
      }
      *reinterpret_cast<f32x4*>(og + opix * p.Nout + co) = v;
    }
  }
#ifdef GEECO_STAMPS
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  STAMP(61);
#endif
}

template <int BM, int BN, int BK, int WM, int WN, bool UT>
__global__ __launch_bounds__(256) void conv_gemm_kernel(const ConvGemmParams p) {
  __shared__ __attribute__((aligned(16))) float smem[conv_gemm_smem_floats<BM, BN, BK>()];
  conv_gemm_body<BM, BN, BK, WM, WN, UT>(p, GemmBlock{(int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z, (int)gridDim.x, (int)gridDim.y}, smem);
}

// Heterogeneous top of the backward (round 4): conv7's input gradient (this file's gather GEMM, 64 x 64 x 16 tiles, split K) and
// conv7's + conv8's filter gradients (conv_wgrad_body.h) all need only dz7 and each fills the 256 CUs badly on its own (768 / 432
// / 432 short blocks, 26 / 30 / 12 us): ONE grid runs them side by side -- independent work, no graph branch.  The filter-gradient
// blocks (the longest) come first; the rest decode to the input gradient's (M tile, N tile x split, encoder) grid.
struct TopBwdParams {
  ConvGemmParams d;
  WgradPairParams w;
  int wblocks, gx, gy;
};
template <bool UT>
__global__ __launch_bounds__(256) void conv_top_bwd_kernel(const TopBwdParams pp) {
  constexpr int SW = conv_wgrad_smem_floats<64, 64, 32>(), SG = conv_gemm_smem_floats<64, 64, 16>();
  __shared__ __attribute__((aligned(16))) float smem[SW > SG ? SW : SG];
  const int b = (int)blockIdx.x;
  if (b < pp.wblocks) {
    conv_wgrad_pair_body<64, 64, 32>(pp.w, b, smem);
  } else {
    const int l = b - pp.wblocks;
    const int x = l % pp.gx, r = l / pp.gx;
    conv_gemm_body<64, 64, 16, 2, 2, UT>(pp.d, GemmBlock{x, r % pp.gy, r / pp.gy, pp.gx, pp.gy}, smem);
  }
}

// Sums the split-K slabs and applies the epilogue (bias, ReLU, mask).  One thread = 4 channels.
__global__ __launch_bounds__(256) void conv_splitk_epilogue_kernel(const ConvGemmParams p) {
  const int g = blockIdx.y;
  const long long npix = (long long)p.N * p.Hd * p.Wd;
  const long long total4 = npix * p.Nout / 4;
  const long long i4 = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i4 >= total4) return;
  const long long e = i4 * 4;
  const int co = (int)(e % p.Nout);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  const float* src = p.part + (long long)g * npix * p.Nout + e;
  const long long slab = (long long)p.groups * npix * p.Nout;
  int s = 0;
  for (; s + 4 <= p.ksplit; s += 4) {     // 4 independent 16-byte loads in flight; the sum keeps the slab order
    f32x4 t[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) t[u] = *reinterpret_cast<const f32x4*>(src + (s + u) * slab);
#pragma unroll
    for (int u = 0; u < 4; ++u) v += t[u];
  }
  for (; s < p.ksplit; ++s) v += *reinterpret_cast<const f32x4*>(src + s * slab);
  if (p.bias) v += *reinterpret_cast<const f32x4*>(p.bias + (long long)g * p.gs_b + co);
  if (p.relu) {
    v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
  }
  if (p.mask) {
    f32x4 mk = *reinterpret_cast<const f32x4*>(p.mask + (long long)g * p.gs_out + e);
    v.x = mk.x > 0.f ? v.x : 0.f; v.y = mk.y > 0.f ? v.y : 0.f;
    v.z = mk.z > 0.f ? v.z : 0.f; v.w = mk.w > 0.f ? v.w : 0.f;
  }
  *reinterpret_cast<f32x4*>(p.out + (long long)g * p.gs_out + e) = v;
}

// The same with the state concat of the one-step decoder in it (StateScatter, conv_gemm_plan.h).  The slab sum is a second copy
// on purpose: as one __device__ function it reorders the instructions of both kernels (profiles/conv_gemm_split/README.md).
__global__ __launch_bounds__(256) void conv_splitk_epilogue_state_kernel(const ConvGemmParams p, const StateScatter sc) {
  const int g = blockIdx.y;
  if ((int)blockIdx.x >= sc.epi_blocks) {
    if (g != 0) return;
    const long long i = (long long)((int)blockIdx.x - sc.epi_blocks) * 256 + threadIdx.x;
    const long long per = (long long)sc.cells * sc.J;
    if (i >= per * p.N) return;
    const int n = (int)(i / per);
    const int rem = (int)(i - (long long)n * per);
    const int cell = rem / sc.J, j = rem - cell * sc.J;
    sc.state[(long long)n * sc.state_stride + cell * sc.Ctot + sc.jnt_off + j] = sc.jnt[(long long)n * sc.jnt_stride + j];
    return;
  }
  const long long npix = (long long)p.N * p.Hd * p.Wd;
  const long long total4 = npix * p.Nout / 4;
  const long long i4 = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i4 >= total4) return;
  const long long e = i4 * 4;
  const int co = (int)(e % p.Nout);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  const float* src = p.part + (long long)g * npix * p.Nout + e;
  const long long slab = (long long)p.groups * npix * p.Nout;
  int s = 0;
  for (; s + 4 <= p.ksplit; s += 4) {     // same slab order as conv_splitk_epilogue_kernel
    f32x4 t[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) t[u] = *reinterpret_cast<const f32x4*>(src + (s + u) * slab);
#pragma unroll
    for (int u = 0; u < 4; ++u) v += t[u];
  }
  for (; s < p.ksplit; ++s) v += *reinterpret_cast<const f32x4*>(src + s * slab);
  if (p.bias) v += *reinterpret_cast<const f32x4*>(p.bias + (long long)g * p.gs_b + co);
  if (p.relu) {
    v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
  }
  *reinterpret_cast<f32x4*>(p.out + (long long)g * p.gs_out + e) = v;
  const long long pix = e / p.Nout;
  const int n = (int)(pix / sc.cells), cell = (int)(pix - (long long)n * sc.cells);
  float* st = sc.state + (long long)n * sc.state_stride + cell * sc.Ctot + sc.off[g] + co;   // Ctot is odd in general: scalar stores
  st[0] = v.x; st[1] = v.y; st[2] = v.z; st[3] = v.w;
}

template <int BM, int BN, int BK, int WM, int WN>
static void launch_cfg(ConvGemmParams& p, int groups, hipStream_t s) {
  static_assert(BK == GEMM_BK, "conv_plan and conv_gemm_grid count K-steps of GEMM_BK");
  const ConvGemmGrid gr = conv_gemm_grid(p, BM, BN, groups);
  const dim3 grid((unsigned)gr.gx, (unsigned)gr.gy, (unsigned)gr.gz);
  geeco_note_kernel("conv_gemm_kernel<%d, %d, %d, %d, %d, %s>", BM, BN, BK, WM, WN, gr.ut ? "true" : "false");
  if (gr.ut)
    hipLaunchKernelGGL((conv_gemm_kernel<BM, BN, BK, WM, WN, true>), grid, dim3(256), 0, s, p);
  else
    hipLaunchKernelGGL((conv_gemm_kernel<BM, BN, BK, WM, WN, false>), grid, dim3(256), 0, s, p);
}

// The slab sum behind a split-K launch (p.ksplit > 1); with `scatter`, the form that carries the state concat.
static int launch_splitk_epilogue(const ConvGemmParams& p, int groups, hipStream_t s, const StateScatter* scatter) {
  const long long total4 = (long long)p.N * p.Hd * p.Wd * p.Nout / 4;
  dim3 grid((unsigned)cdiv64(total4, 256), (unsigned)groups);
  if (scatter) {
    StateScatter sc = *scatter;
    sc.epi_blocks = (int)grid.x;
    grid.x += (unsigned)cdiv64((long long)p.N * sc.cells * sc.J, 256);
    geeco_note_kernel("conv_splitk_epilogue_state_kernel");
    hipLaunchKernelGGL(conv_splitk_epilogue_state_kernel, grid, dim3(256), 0, s, p, sc);
  } else {
    geeco_note_kernel("conv_splitk_epilogue_kernel");
    hipLaunchKernelGGL(conv_splitk_epilogue_kernel, grid, dim3(256), 0, s, p);
  }
  GEECO_LAUNCH_CHECK();
  return 0;
}

#ifdef GEECO_STAMPS
// Dev instrumentation: one timeline per block of the LAST conv_gemm launch; geeco_debug_dump_stamps writes it out.
static unsigned long long* g_stamps = nullptr;
static const size_t kStampBlocks = 1 << 16;
static unsigned long long* geeco_stamp_buffer() {
  if (!g_stamps && hipMalloc(&g_stamps, kStampBlocks * 64 * 8) != hipSuccess) return nullptr;
  (void)hipMemset(g_stamps, 0, kStampBlocks * 64 * 8);
  return g_stamps;
}
extern "C" int geeco_debug_dump_stamps(const char* path) {
  if (!g_stamps) return 1;
  (void)hipDeviceSynchronize();
  unsigned long long* h = (unsigned long long*)malloc(kStampBlocks * 64 * 8);
  (void)hipMemcpy(h, g_stamps, kStampBlocks * 64 * 8, hipMemcpyDeviceToHost);
  FILE* f = fopen(path, "wb");
  if (!f) return 2;
  fwrite(h, 8, kStampBlocks * 64, f);
  fclose(f);
  free(h);
  return 0;
}
#endif

static int launch_conv_gemm(ConvGemmParams& p, int groups, void* ws, hipStream_t s, const StateScatter* scatter = nullptr) {
  if (const long long rows = conv_rows_beyond_32bit(p)) {
    geeco_set_error("conv3x3: %lld rows per launch exceed the 32-bit row index of the kernel", rows);
    return (int)hipErrorInvalidValue;
  }
#ifdef GEECO_STAMPS
  p.stamps = geeco_stamp_buffer();
#endif
  ConvPlan pl = conv_plan(p, groups);
  if (!ws) pl.ksplit = 1;
  if (scatter && pl.ksplit <= 1) return GEECO_ENOSUP;      // no epilogue launch to carry the concat: the caller launches it
  p.ksplit = pl.ksplit;
  p.groups = groups;
  p.part = (float*)ws;
  if (pl.bn == 128) {
    launch_cfg<128, 128, 16, 2, 2>(p, groups, s);
  } else if (pl.bn == 96) {
    launch_cfg<64, 96, 16, 2, 2>(p, groups, s);
  } else if (pl.bn == 64) {
    if (pl.bm == 64)
      launch_cfg<64, 64, 16, 2, 2>(p, groups, s);
    else
      launch_cfg<128, 64, 16, 2, 2>(p, groups, s);
  } else if (pl.bn == 48) {
    launch_cfg<128, 48, 16, 4, 1>(p, groups, s);
  } else if (pl.bn == 32) {
    launch_cfg<128, 32, 16, 4, 1>(p, groups, s);
  } else {
    launch_cfg<128, 16, 16, 4, 1>(p, groups, s);
  }
  GEECO_LAUNCH_CHECK();
  return p.ksplit > 1 ? launch_splitk_epilogue(p, groups, s, scatter) : 0;
}

// Which kernel family serves a layer, once per direction: every entry point below asks here, so a layer runs the same kernel
// on every path (the bitwise statements of the tests rest on it).  Forward: LDS-halo, conv1's, else this file's gather GEMM.
// Input gradient: LDS-halo, LDS-staged, else the gather GEMM.  conv_fwd_family and conv_dgrad_family: conv_halo_plan.h (through
// conv_internal.h), plain C++ that the host tests evaluate.

extern "C" int64_t geeco_conv3x3_fwd_ws_bytes(int groups, int N, int H, int W, int Cin, int Cout, int stride) {
  ConvGemmParams p = {};
  fill_fwd(&p, N, H, W, Cin, Cout, stride);
  return conv_ws_bytes(p, groups);
}

extern "C" int64_t geeco_conv3x3_dgrad_ws_bytes(int groups, int N, int H, int W, int Cin, int Cout, int stride) {
  if (stride > 2) return 0;
  ConvGemmParams p = {};
  fill_dgrad(&p, N, H, W, Cin, Cout, stride);
  return conv_ws_bytes(p, groups);
}

extern "C" int geeco_conv3x3_fwd(const float* x, const float* w, const float* b, float* y, int groups,
                                 int64_t gs_x, int64_t gs_w, int64_t gs_b, int64_t gs_y, int N, int H,
                                 int W, int Cin, int Cout, int stride, int relu, void* ws, void* stream) {
  GEECO_CHECK_ARG(x && w && y, "conv3x3_fwd: null pointer");
  GEECO_CHECK_ARG(groups >= 1 && N >= 1 && H >= 1 && W >= 1, "conv3x3_fwd: bad dims");
  GEECO_CHECK_ARG(Cin % 4 == 0 && Cin >= 4, "conv3x3_fwd: Cin=%d must be a multiple of 4", Cin);
  GEECO_CHECK_ARG(Cout % 16 == 0, "conv3x3_fwd: Cout=%d must be a multiple of 16", Cout);
  GEECO_CHECK_ARG(stride >= 1 && stride <= 4, "conv3x3_fwd: stride=%d", stride);
  {
    const ConvFamily fam = conv_fwd_family(H, W, Cin, Cout, stride);
    int handled = 0, rc = 0;
    if (fam == CONV_HALO)
      rc = geeco_try_halo_fwd(x, w, b, y, groups, gs_x, gs_w, gs_b, gs_y, N, H, W, Cin, Cout, stride, relu,
                              (hipStream_t)stream, &handled);
    else if (fam == CONV_CONV1)
      rc = geeco_try_conv1_fwd(x, w, b, y, groups, gs_x, gs_w, gs_b, gs_y, N, H, W, Cin, Cout, stride, relu,
                               (hipStream_t)stream, &handled);
    if (rc || handled) return rc;       // a family that declines (it needs the bias) leaves the layer to the gather GEMM
  }
  ConvGemmParams p = {};
  conv_fwd_problem(&p, x, w, b, y, gs_x, gs_w, gs_b, gs_y, N, H, W, Cin, Cout, stride, relu);
  return launch_conv_gemm(p, groups, ws, (hipStream_t)stream);
}

// conv8 + bias + ReLU of all encoders AND the one-step decoder's state concat (the epilogue of the split-K sum carries it).
// GEECO_ENOSUP (nothing launched) when this shape does not go through the split-K gather GEMM: the caller then runs
// geeco_conv3x3_fwd and geeco_state_concat_fwd.
extern "C" int geeco_conv3x3_fwd_state(const float* x, const float* w, const float* b, float* y, int groups, int64_t gs_x,
                                       int64_t gs_w, int64_t gs_b, int64_t gs_y, int N, int H, int W, int Cin, int Cout,
                                       int stride, void* ws, const int* feat_off, int Ctot, const float* jnt, int64_t jnt_stride,
                                       int jnt_off, int J, float* state, int64_t state_stride, void* stream) {
  GEECO_CHECK_ARG(x && w && y && feat_off && jnt && state, "conv3x3_fwd_state: null pointer");
  GEECO_CHECK_ARG(groups >= 1 && groups <= 4 && N >= 1 && H >= 1 && W >= 1, "conv3x3_fwd_state: bad dims");
  GEECO_CHECK_ARG(Cin % 4 == 0 && Cin >= 4 && Cout % 16 == 0 && stride >= 1 && stride <= 4, "conv3x3_fwd_state: Cin=%d Cout=%d stride=%d", Cin, Cout, stride);
  ConvGemmParams p = {};
  conv_fwd_problem(&p, x, w, b, y, gs_x, gs_w, gs_b, gs_y, N, H, W, Cin, Cout, stride, 1);
  const int cells = p.Hd * p.Wd;
  GEECO_CHECK_ARG(J >= 1 && jnt_off >= 0 && jnt_off + J <= Ctot && state_stride >= (int64_t)cells * Ctot, "conv3x3_fwd_state: joint columns / state_stride");
  for (int g = 0; g < groups; ++g) {
    GEECO_CHECK_ARG(feat_off[g] >= 0 && feat_off[g] + Cout <= Ctot && (feat_off[g] + Cout <= jnt_off || feat_off[g] >= jnt_off + J),
                    "conv3x3_fwd_state: feature columns of encoder %d", g);
  }
  if (!ws || conv_fwd_family(H, W, Cin, Cout, stride) != CONV_GATHER_GEMM) return GEECO_ENOSUP;
  StateScatter sc = {};
  sc.state = state; sc.jnt = jnt; sc.state_stride = state_stride; sc.jnt_stride = jnt_stride;
  for (int g = 0; g < groups; ++g) sc.off[g] = feat_off[g];
  sc.Ctot = Ctot; sc.jnt_off = jnt_off; sc.J = J; sc.cells = cells;
  return launch_conv_gemm(p, groups, ws, (hipStream_t)stream, &sc);
}

extern "C" int geeco_conv3x3_dgrad_needs_wt(int H, int W, int Cin, int Cout, int stride) {
  return conv_dgrad_family(H, W, Cin, Cout, stride) == CONV_GATHER_GEMM && !dgrad_reads_hwio(Cout);
}

extern "C" int geeco_conv3x3_dgrad(const float* dz, const float* w, const float* wt, const float* ymask, float* dx,
                                   int groups, int64_t gs_dz, int64_t gs_w, int64_t gs_wt, int64_t gs_dx, int N,
                                   int H, int W, int Cin, int Cout, int stride, void* ws, void* stream) {
  GEECO_CHECK_ARG(dz && dx && (wt || w), "conv3x3_dgrad: null pointer");
  GEECO_CHECK_ARG(groups >= 1 && N >= 1 && H >= 1 && W >= 1, "conv3x3_dgrad: bad dims");
  GEECO_CHECK_ARG(Cout % 4 == 0, "conv3x3_dgrad: Cout=%d must be a multiple of 4", Cout);
  GEECO_CHECK_ARG(Cin % 16 == 0, "conv3x3_dgrad: Cin=%d must be a multiple of 16", Cin);
  GEECO_CHECK_ARG(stride >= 1 && stride <= 2, "conv3x3_dgrad: stride=%d (1 or 2)", stride);
  {
    const ConvFamily fam = conv_dgrad_family(H, W, Cin, Cout, stride);
    int handled = 0, rc = 0;
    if (fam == CONV_HALO)
      rc = geeco_try_halo_dgrad(dz, w, ymask, dx, groups, gs_dz, gs_w, gs_dx, N, H, W, Cin, Cout, stride,
                                (hipStream_t)stream, &handled);
    else if (fam == CONV_DGRAD_LDS)
      rc = geeco_try_dgrad_lds(dz, w, ymask, dx, groups, gs_dz, gs_w, gs_dx, N, H, W, Cin, Cout, stride,
                               (hipStream_t)stream, &handled);
    if (rc || handled) return rc;       // a family that declines (it needs the HWIO kernel) leaves the layer to the gather GEMM
  }
  ConvGemmParams p = {};
  conv_dgrad_problem(&p, dz, w, wt, ymask, dx, gs_dz, gs_w, gs_wt, gs_dx, N, H, W, Cin, Cout, stride);
  GEECO_CHECK_ARG(p.w, "conv3x3_dgrad: this shape (Cout = %d) needs the per-tap transposed kernel wt", Cout);
  if (p.ncls == 0) return 0;
  return launch_conv_gemm(p, groups, ws, (hipStream_t)stream);
}

// conv7's input gradient + conv7's / conv8's filter gradients as ONE grid (conv_top_bwd_kernel).  The input gradient's arguments as
// geeco_conv3x3_dgrad (stride 2), the two filter-gradient problems as geeco_conv3x3_wgrad_pair.  GEECO_ENOSUP when any of the three
// is outside the kernels this launch combines (the caller then uses the separate entry points): nothing has been launched.
extern "C" int geeco_conv_top_bwd(const float* dz, const float* w, const float* wt, const float* ymask, float* dx, int64_t gs_dz,
                                  int64_t gs_w, int64_t gs_wt, int64_t gs_dx, int N, int H, int W, int Cin, int Cout, void* ws,
                                  const float* x0, const float* dz0, float* dw0, float* db0, int64_t gs_x0, int64_t gs_dz0,
                                  int64_t gs_dw0, int64_t gs_db0, int N0, int H0, int W0, int Cin0, int Cout0, void* ws0,
                                  const float* x1, const float* dz1, float* dw1, float* db1, int64_t gs_x1, int64_t gs_dz1,
                                  int64_t gs_dw1, int64_t gs_db1, int N1, int H1, int W1, int Cin1, int Cout1, void* ws1,
                                  int groups, int stride, void* stream, geeco_slab_reduce* pending2) {
  GEECO_CHECK_ARG(dz && dx && (wt || w) && ws, "conv_top_bwd: null pointer");
  GEECO_CHECK_ARG(groups >= 1 && N >= 1 && H >= 1 && W >= 1 && Cout % 4 == 0 && Cin % 16 == 0, "conv_top_bwd: bad dims");
  if (stride != 2 || conv_dgrad_family(H, W, Cin, Cout, stride) != CONV_GATHER_GEMM) {
    geeco_set_error("conv_top_bwd: the input gradient of this shape is not the gather GEMM's");
    return GEECO_ENOSUP;
  }
  TopBwdParams tp = {};
  ConvGemmParams& p = tp.d;
  conv_dgrad_problem(&p, dz, w, wt, ymask, dx, gs_dz, gs_w, gs_wt, gs_dx, N, H, W, Cin, Cout, stride);
  if (!p.w || p.ncls == 0) {
    geeco_set_error("conv_top_bwd: this input gradient needs the per-tap transposed kernel / is empty");
    return GEECO_ENOSUP;
  }
  if (const long long rows = conv_rows_beyond_32bit(p)) {
    geeco_set_error("conv_top_bwd: %lld rows per launch exceed the 32-bit row index of the kernel", rows);
    return GEECO_ENOSUP;
  }
  const ConvPlan pl = conv_plan(p, groups);
  if (pl.bm != 64 || pl.bn != 64) {
    geeco_set_error("conv_top_bwd: the input gradient's plan is not the 64 x 64 x 16 tile kernel");
    return GEECO_ENOSUP;
  }
  long long wblocks = 0;
  if (int rc = geeco_wgrad_pair_fill(&tp.w, x0, dz0, dw0, db0, gs_x0, gs_dz0, gs_dw0, gs_db0, N0, H0, W0, Cin0, Cout0, ws0, x1, dz1,
                                     dw1, db1, gs_x1, gs_dz1, gs_dw1, gs_db1, N1, H1, W1, Cin1, Cout1, ws1, groups, stride, &wblocks))
    return rc;
#ifdef GEECO_STAMPS
  p.stamps = nullptr;
#endif
  p.ksplit = pl.ksplit; p.groups = groups; p.part = (float*)ws;
  const ConvGemmGrid gr = conv_gemm_grid(p, 64, 64, groups);      // the grid of launch_cfg<64, 64, 16, 2, 2>, as a range of block indices
  tp.wblocks = (int)wblocks; tp.gx = gr.gx; tp.gy = gr.gy;
  const long long blocks = wblocks + (long long)gr.gx * gr.gy * gr.gz;
  hipStream_t s = (hipStream_t)stream;
  geeco_note_kernel("conv_top_bwd_kernel<%s>", gr.ut ? "true" : "false");
  if (gr.ut)
    hipLaunchKernelGGL(conv_top_bwd_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, tp);
  else
    hipLaunchKernelGGL(conv_top_bwd_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, tp);
  GEECO_LAUNCH_CHECK();
  if (p.ksplit > 1)
    if (int rc = launch_splitk_epilogue(p, groups, s, nullptr)) return rc;
  return geeco_wgrad_pair_finish(tp.w, groups, s, pending2);
}
