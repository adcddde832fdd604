// conv1 (3x3, stride 1, 4 -> 32 channels) of the LDS-halo family (conv_halo_common.h): forward conv1_halo_fwd_kernel with
// its dispatcher geeco_try_conv1_fwd and the entry points that also write the ReLU sign words (geeco_conv1_fwd_relu_bits*),
// filter/bias gradient conv1_halo_wgrad_kernel with its dispatcher geeco_try_conv1_wgrad.
#include "conv_halo_common.h"
#include "conv_internal.h"

// ------------------------------------------------------------------------------------------------
// conv1-type kernels: stride 1, CIN == 4 (RGB padded, or RGB-D), COUT == 32.
// K per tap is exactly one MFMA step (4 channels), so the 9 taps are 9 MFMA k-steps.
// Forward is bound by the 128 B/pixel output stream (805 MB per step at N = 32), wgrad by reading
// it back: both keep the tiny input halo in LDS and the kernel in registers.
// ------------------------------------------------------------------------------------------------
struct Conv1FwdParams {
  const float* x;       // [G][N][H][W][4]
  const float* w;       // [G][9][w_cin][32]: w_cin = 4 (padded copy) or 3 (the RGB variable itself, channel 3 taken as zero)
  const float* bias;
  float* y;             // [G][N][H][W][32]
  unsigned* bits;       // optional [G][N][Hp][Wp]: ReLU sign bits of y (geeco_conv1_fwd_relu_bits), else null
  long long gs_x, gs_w, gs_b, gs_y, gs_bits;
  int N, H, W, tiles_x, tiles_y, relu, Wp, Hp, w_cin;
};

// PACK3 (RGB, w_cin == 3): the 27 real (tap, channel) products are packed into 7 MFMA k-steps (k = 3 tap + c = 4 s + q)
// instead of 9 steps of (R, G, B, pad): 14 MFMAs and 7 fragment reads per 16-pixel strip instead of 18 / 9.  The dropped
// terms are exact zeros (pad channel x zero weight), added in the same order before: y is bitwise unchanged.  The kernel
// is issue bound, not only HBM bound (PMC: MFMA busy 51 %, 61 % of the wave time issuing), so the MFMAs saved show.
template <bool PACK3>
__global__ __launch_bounds__(256) void conv1_halo_fwd_kernel(const Conv1FwdParams p) {
  // Persistent blocks: a block keeps the kernel fragments and bias of its encoder in registers and walks the
  // tiles t = blockIdx.x, + gridDim.x, ...; the next tile's halo is fetched into registers before the current
  // tile is computed and lands in the other LDS buffer afterwards.  One block per tile (24 576 blocks of a few
  // microseconds each) was bound by workgroup dispatch and by the exposed latency of every block's own halo
  // and kernel loads: load, MFMA and store time simply added up (ablation: 267 = 90 + 52 + 85 + 56 us).
  constexpr int TH = 8, TW = 32, HW_ = TW + 2, HH = TH + 2;
  constexpr int NPX = HH * HW_;                    // 340 halo pixels
  constexpr int NLD = (NPX + 255) / 256;           // float4 per thread (2)
  __shared__ __attribute__((aligned(16))) float sX[2][NPX * 4];
  __shared__ __attribute__((aligned(16))) float sO[4][16 * 36];   // per wave: [pixel][32 + 4 pad]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int g = blockIdx.y;
  const int per_img = p.tiles_x * p.tiles_y, ntiles = p.N * per_img;
  int t = blockIdx.x;
  if (t >= ntiles) return;
  const float* xg0 = p.x + (long long)g * p.gs_x;
  // kernel fragments: lane (r = co, q = channel) of tap tp, co tile i
  const float* wg = p.w + (long long)g * p.gs_w;
  constexpr int NS = PACK3 ? 7 : 9;
  float wf[NS][2];
  int xo[NS];          // float offset of the lane's x operand of step s inside a strip's halo window (without the pixel r)
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    if (PACK3) {
      const int kk = 4 * s + q;                    // = 3 tap + c
      const bool v = kk < 27;
      const int tap = v ? kk / 3 : 0, c = v ? kk - tap * 3 : 0;
      const int ky = tap / 3, kx = tap - ky * 3;
      xo[s] = ((ky * HW_ + kx) << 2) + c;
#pragma unroll
      for (int i = 0; i < 2; ++i) wf[s][i] = v ? wg[kk * 32 + i * 16 + r] : 0.f;      // w [9][3][32]
    } else {
      const int ky = s / 3, kx = s - ky * 3;
      xo[s] = ((ky * HW_ + kx) << 2) + q;
#pragma unroll
      for (int i = 0; i < 2; ++i) wf[s][i] = q < p.w_cin ? wg[(s * p.w_cin + q) * 32 + i * 16 + r] : 0.f;
    }
  }
  f32x4 bias_r[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) bias_r[i] = *reinterpret_cast<const f32x4*>(p.bias + (long long)g * p.gs_b + i * 16 + 4 * q);

  f32x4 stage[NLD];
  auto load_halo = [&](int tt) {
    const int n = tt / per_img, rem = tt - n * per_img;
    const int ty = rem / p.tiles_x, tx = rem - ty * p.tiles_x;
    const int y0 = ty * TH, x0 = tx * TW;
    const float* xg = xg0 + (long long)n * p.H * p.W * 4;
#pragma unroll
    for (int k = 0; k < NLD; ++k) {
      const int i = tid + 256 * k;
      const int hy = i / HW_, hx = i - hy * HW_;
      const int iy = y0 + hy - 1, ix = x0 + hx - 1;        // TF SAME, stride 1: pad 1 on every side
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (i < NPX && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W)
        v = *reinterpret_cast<const f32x4*>(xg + ((long long)iy * p.W + ix) * 4);
      stage[k] = v;
    }
  };
  auto store_halo = [&](int buf) {
#pragma unroll
    for (int k = 0; k < NLD; ++k) {
      const int i = tid + 256 * k;
      if (i < NPX) *reinterpret_cast<f32x4*>(&sX[buf][i * 4]) = stage[k];
    }
  };
  load_halo(t);
  store_halo(0);
  __syncthreads();
  float* so = sO[wid];
  int buf = 0;
  for (;;) {
    const int t2 = t + gridDim.x;
    const bool more = t2 < ntiles;
    if (more) load_halo(t2);
    const int n = t / per_img, rem = t - n * per_img;
    const int ty = rem / p.tiles_x, tx = rem - ty * p.tiles_x;
    const int y0 = ty * TH, x0 = tx * TW;
    float* yg = p.y + (long long)g * p.gs_y + (long long)n * p.H * p.W * 32;
    // wave w: rows 2w, 2w+1; 2 column halves => 4 strips of 16 pixels.  The 16 x 32 output strip is 2 KB
    // contiguous in NHWC memory: it is transposed through LDS so that each store instruction writes 1 KB
    // of consecutive bytes (lane l -> pixel l / 8 (+8), channel quad l % 8) instead of 16 separate 64 B pieces.
    unsigned myword = 0;
    const float* xt[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) xt[s] = &sX[buf][((2 * wid * HW_ + r) << 2) + xo[s]];
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      const int oyl = 2 * wid + (st >> 1), oxl0 = 16 * (st & 1);
      f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
      // operand address = (per-lane part, formed once per tile) + (strip part: a compile-time immediate)
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const float xv = xt[s][(((st >> 1) * HW_ + 16 * (st & 1)) << 2)];
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s][i], xv, acc[i], 0, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        f32x4 v = acc[i] + bias_r[i];
        if (p.relu) {
          v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
        }
        *reinterpret_cast<f32x4*>(so + r * 36 + i * 16 + 4 * q) = v;      // lane owns pixel r, channels 16 i + 4 q
      }
      // same-wave LDS round trip: the compiler's lgkmcnt wait orders the reads behind the writes
      const int oy = y0 + oyl;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int px = 8 * h + (lane >> 3), c4 = lane & 7;
        const f32x4 v = *reinterpret_cast<const f32x4*>(so + px * 36 + c4 * 4);
        const int ox = x0 + oxl0 + px;
        if (oy < p.H && ox < p.W) stream_store<0>(yg + ((long long)oy * p.W + ox) * 32 + c4 * 4, v);
        if (p.bits) {
          // sign bits of the 8 pixels this instruction stores: a compare IS a ballot (lane = 8 pixel + channel quad),
          // so byte `pixel` of the four masks holds the bits of channels 4 c4 + {0, 1, 2, 3}; every lane assembles
          // the word of pixel lane & 7 (bit (c & 3) * 8 + (c >> 2) <-> channel c) and the lanes 8 (2 st + h) + j keep
          // it: after the four strips lane L holds the word of tile pixel (row 2 wid + (L >> 5), column L & 31)
          const unsigned long long bx = __ballot(v.x > 0.f), by = __ballot(v.y > 0.f), bz = __ballot(v.z > 0.f),
                                   bw = __ballot(v.w > 0.f);
          // byte lane & 7 of each 64-bit mask, placed in byte 0 / 1 / 2 / 3: one v_perm_b32 each (a 64-bit shift by a
          // per-lane amount is quarter rate and made this HBM-bound kernel 11 % slower)
          const unsigned j = lane & 7;
          const unsigned word = __builtin_amdgcn_perm((unsigned)(bx >> 32), (unsigned)bx, 0x0c0c0c00u | j) |
                                __builtin_amdgcn_perm((unsigned)(by >> 32), (unsigned)by, 0x0c0c000cu | (j << 8)) |
                                __builtin_amdgcn_perm((unsigned)(bz >> 32), (unsigned)bz, 0x0c000c0cu | (j << 16)) |
                                __builtin_amdgcn_perm((unsigned)(bw >> 32), (unsigned)bw, 0x000c0c0cu | (j << 24));
          if ((lane >> 3) == 2 * st + h) myword = word;
        }
      }
    }
    if (p.bits) {         // one coalesced store per wave: 2 rows x 32 words
      const int oy = y0 + 2 * wid + (lane >> 5), ox = x0 + (lane & 31);
      if (oy < p.H && ox < p.W) p.bits[(long long)g * p.gs_bits + ((long long)n * p.Hp + oy) * p.Wp + ox] = myword;
    }
    if (!more) break;
    store_halo(buf ^ 1);
    lds_barrier();      // the other buffer is complete; everyone is done with this one
    buf ^= 1;
    t = t2;
  }
}

static int launch_conv1_fwd(const float* x, const float* w, const float* b, float* y, unsigned* bits, int groups,
                            int64_t gs_x, int64_t gs_w, int64_t gs_b, int64_t gs_y, int64_t gs_bits, int N, int H, int W,
                            int relu, hipStream_t stream, int w_cin = 4) {
  Conv1FwdParams p = {};
  p.w_cin = w_cin;
  p.x = x; p.w = w; p.bias = b; p.y = y; p.gs_x = gs_x; p.gs_w = gs_w; p.gs_b = gs_b; p.gs_y = gs_y;
  p.bits = bits; p.gs_bits = gs_bits; p.Wp = (int)geeco_relu_bits_pitch(W); p.Hp = (int)geeco_relu_bits_rows(H);
  const HaloTileGrid tg = conv1_fwd_grid(groups, N, H, W);      // 8 x 32 tiles, 768 blocks per encoder: conv_halo_plan.h
  p.N = N; p.H = H; p.W = W; p.tiles_x = tg.tiles_x; p.tiles_y = tg.tiles_y; p.relu = relu;
  dim3 grid((unsigned)tg.blocks, (unsigned)tg.grid_y);
  geeco_note_kernel("conv1_halo_fwd_kernel<%s>", w_cin == 3 ? "true" : "false");
  if (w_cin == 3)
    hipLaunchKernelGGL(conv1_halo_fwd_kernel<true>, grid, dim3(256), 0, stream, p);
  else
    hipLaunchKernelGGL(conv1_halo_fwd_kernel<false>, grid, dim3(256), 0, stream, p);
  GEECO_LAUNCH_CHECK();
  return 0;
}

int geeco_try_conv1_fwd(const float* x, const float* w, const float* b, float* y, int groups, int64_t gs_x,
                        int64_t gs_w, int64_t gs_b, int64_t gs_y, int N, int H, int W, int Cin, int Cout, int stride,
                        int relu, hipStream_t stream, int* handled) {
  *handled = 0;
  if (!b || !geeco_conv1_fwd_handles(Cin, Cout, stride)) return 0;
  *handled = 1;
  return launch_conv1_fwd(x, w, b, y, nullptr, groups, gs_x, gs_w, gs_b, gs_y, 0, N, H, W, relu, stream);
}

extern "C" int64_t geeco_relu_bits_pitch(int W) { return (int64_t)(W + 63) / 64 * 64; }
extern "C" int64_t geeco_relu_bits_rows(int H) { return (int64_t)(H + 7) / 8 * 8; }

extern "C" int geeco_conv1_fwd_relu_bits(const float* x, const float* w, const float* b, float* y, uint32_t* bits,
                                         int groups, int64_t gs_x, int64_t gs_w, int64_t gs_b, int64_t gs_y,
                                         int64_t gs_bits, int N, int H, int W, void* stream) {
  GEECO_CHECK_ARG(x && w && b && y && bits, "conv1_fwd_relu_bits: null pointer");
  GEECO_CHECK_ARG(groups >= 1 && N >= 1 && H >= 1 && W >= 1, "conv1_fwd_relu_bits: bad dims");
  return launch_conv1_fwd(x, w, b, y, bits, groups, gs_x, gs_w, gs_b, gs_y, gs_bits, N, H, W, 1, (hipStream_t)stream);
}

// ... reading the RGB model's kernel variable [G][3][3][3][32] as it is stored (x stays channel-padded to 4; the pad
// channel's kernel rows are taken as zero): no padded copy to re-derive after every optimiser step
extern "C" int geeco_conv1_fwd_relu_bits_rgb(const float* x, const float* w3, const float* b, float* y, uint32_t* bits,
                                             int groups, int64_t gs_x, int64_t gs_w, int64_t gs_b, int64_t gs_y,
                                             int64_t gs_bits, int N, int H, int W, void* stream) {
  GEECO_CHECK_ARG(x && w3 && b && y && bits, "conv1_fwd_relu_bits_rgb: null pointer");
  GEECO_CHECK_ARG(groups >= 1 && N >= 1 && H >= 1 && W >= 1, "conv1_fwd_relu_bits_rgb: bad dims");
  return launch_conv1_fwd(x, w3, b, y, bits, groups, gs_x, gs_w, gs_b, gs_y, gs_bits, N, H, W, 1, (hipStream_t)stream, 3);
}

// ---- conv1 filter/bias gradient --------------------------------------------------------------------
// dw[(tap, c)][co] = sum_pixels x[halo(pixel, tap)][c] dz[pixel][co]: MFMA row i = co (2 tiles), column
// j = (tap, c) (36 of 48 = 3 tiles), k = 4 consecutive pixels.  Persistent blocks (wave = row of a
// 4 x 16 tile) keep the 6 accumulator tiles in registers over their whole tile range.
struct Conv1WgradParams {
  const float* x;
  const float* dz;
  float* part;             // [G][S][9*4*32 + 32]
  long long gs_x, gs_dz;
  int N, H, W, tiles_x, tiles_y, tiles_per_group, S;
};

__global__ __launch_bounds__(256) void conv1_halo_wgrad_kernel(const Conv1WgradParams p) {
  constexpr int TH = 4, TW = 16, HWD = TW + 2, HH = TH + 2;
  constexpr int ZP = 48;                                   // dz row pitch (floats): 16 mod 32
  constexpr int XF = HH * HWD * 4, ZF = TH * TW * ZP;
  __shared__ __attribute__((aligned(16))) float smem[2 * (XF + ZF)];
  float* sX = smem;                 // 2 x halo
  float* sZ = smem + 2 * XF;        // 2 x dz tile
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int g = blockIdx.y, split = blockIdx.x;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const int per = (p.tiles_per_group + p.S - 1) / p.S;
  int tile = split * per;
  const int tend = tile + per < p.tiles_per_group ? tile + per : p.tiles_per_group;
  const long long slab = 9 * 4 * 32 + 32;
  float* part = p.part + ((long long)g * p.S + split) * slab;
  int n, ty, tx;
  {
    int per_img = p.tiles_x * p.tiles_y;
    n = tile / per_img;
    int rem = tile - n * per_img;
    ty = rem / p.tiles_x;
    tx = rem - ty * p.tiles_x;
  }
  // staging slots: halo (108 pixels, one float4 each) and dz tile (64 pixels x 8 float4)
  const bool xs = tid < HH * HWD;
  const int x_hy = tid / HWD, x_hx = tid - x_hy * HWD;
  int z_px[2], z_c4[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int idx = tid + 256 * i;
    z_px[i] = idx >> 3;
    z_c4[i] = idx & 7;
  }
  f32x4 xst = zero4, zst[2], dbsum[2] = {zero4, zero4};
  auto load_tile = [&](int n_, int ty_, int tx_) {
    const float* xg = p.x + (long long)g * p.gs_x + (long long)n_ * p.H * p.W * 4;
    const int iy = ty_ * TH + x_hy - 1, ix = tx_ * TW + x_hx - 1;
    xst = (xs && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W)
              ? *reinterpret_cast<const f32x4*>(xg + ((long long)iy * p.W + ix) * 4) : zero4;
    const float* zg = p.dz + (long long)g * p.gs_dz + (long long)n_ * p.H * p.W * 32;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int oy = ty_ * TH + (z_px[i] >> 4), ox = tx_ * TW + (z_px[i] & 15);
      zst[i] = (oy < p.H && ox < p.W) ? *reinterpret_cast<const f32x4*>(zg + ((long long)oy * p.W + ox) * 32 + z_c4[i] * 4)
                                      : zero4;
    }
  };
  auto store_tile = [&](int buf) {
    if (xs) *reinterpret_cast<f32x4*>(sX + buf * XF + tid * 4) = xst;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      *reinterpret_cast<f32x4*>(sZ + buf * ZF + z_px[i] * ZP + z_c4[i] * 4) = zst[i];
      dbsum[i] += zst[i];
    }
  };
  // lane's three (tap, c) columns: jj = 16 tj + r
  int xoff[3];
  bool xval[3];
#pragma unroll
  for (int tj = 0; tj < 3; ++tj) {
    const int jj = 16 * tj + r;
    const int tap = jj >> 2, c = jj & 3;
    xval[tj] = jj < 36;
    const int ky = tap / 3, kx = tap - ky * 3;
    xoff[tj] = xval[tj] ? ((ky * HWD + kx) << 2) + c : 0;
  }
  f32x4 acc[2][3];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) acc[i][j] = zero4;

  if (tile < tend) {
    load_tile(n, ty, tx);
    store_tile(0);
  }
  __syncthreads();
  int buf = 0;
  for (; tile < tend; ++tile) {
    const bool more = tile + 1 < tend;
    int n2 = n, ty2 = ty, tx2 = tx;
    if (more) {
      if (++tx2 == p.tiles_x) {
        tx2 = 0;
        if (++ty2 == p.tiles_y) {
          ty2 = 0;
          ++n2;
        }
      }
      load_tile(n2, ty2, tx2);
    }
    const float* hx = sX + buf * XF + ((wid * HWD + q) << 2);           // wave = tile row; pixel 4 s + q
    const float* hz = sZ + buf * ZF + (16 * wid + q) * ZP + r;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      float a[2], b[3];
#pragma unroll
      for (int i = 0; i < 2; ++i) a[i] = hz[(4 * s) * ZP + 16 * i];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const float v = hx[((4 * s) << 2) + xoff[j]];
        b[j] = xval[j] ? v : 0.f;
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    if (more) store_tile(buf ^ 1);
    lds_barrier();
    n = n2; ty = ty2; tx = tx2;
    buf ^= 1;
  }
  // reduce the 4 waves through LDS: [wave][6 tiles][64 lanes] float4 = 24 KB (fits in the staging area)
  __syncthreads();
  f32x4* sR = reinterpret_cast<f32x4*>(smem);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) sR[(wid * 6 + i * 3 + j) * 64 + lane] = acc[i][j];
  __syncthreads();
  for (int e = tid; e < 6 * 64; e += 256) {
    const int ln = e & 63, k = e >> 6;
    f32x4 s4 = sR[(0 * 6 + k) * 64 + ln];
    s4 += sR[(1 * 6 + k) * 64 + ln];
    s4 += sR[(2 * 6 + k) * 64 + ln];
    s4 += sR[(3 * 6 + k) * 64 + ln];
    const int i = k / 3, j = k - i * 3;
    const int jj = 16 * j + (ln & 15), co = 16 * i + 4 * (ln >> 4);
    if (jj < 36) *reinterpret_cast<f32x4*>(part + jj * 32 + co) = s4;
  }
  __syncthreads();
  float* sD = smem;   // [64 pixel slots][32]
#pragma unroll
  for (int i = 0; i < 2; ++i) *reinterpret_cast<f32x4*>(sD + z_px[i] * 32 + z_c4[i] * 4) = dbsum[i];
  __syncthreads();
  if (tid < 32) {
    float s1 = 0.f;
    for (int px = 0; px < 64; ++px) s1 += sD[px * 32 + tid];
    part[9 * 4 * 32 + tid] = s1;
  }
}

int64_t geeco_conv1_wgrad_ws_bytes(int groups, int Cin, int Cout, int stride) {
  if (conv1_wgrad_handles(Cin, Cout, stride)) return (int64_t)groups * conv1_wgrad_S(groups) * (9 * 4 * 32 + 32) * 4;
  return 0;
}

int geeco_try_conv1_wgrad(const float* x, const float* dz, float* dw, float* db, int groups, int64_t gs_x,
                          int64_t gs_dz, int64_t gs_dw, int64_t gs_db, int N, int H, int W, int Cin, int Cout,
                          int stride, void* ws, hipStream_t stream, int* handled) {
  *handled = 0;
  if (!conv1_wgrad_handles(Cin, Cout, stride)) return 0;
  Conv1WgradParams p = {};
  p.x = x; p.dz = dz; p.part = (float*)ws; p.gs_x = gs_x; p.gs_dz = gs_dz;
  p.N = N; p.H = H; p.W = W; p.tiles_x = cdiv(W, CONV1_WGRAD_TW); p.tiles_y = cdiv(H, CONV1_WGRAD_TH);
  p.tiles_per_group = N * p.tiles_x * p.tiles_y;
  p.S = conv1_wgrad_S(groups);
  geeco_note_kernel("conv1_halo_wgrad_kernel");
  hipLaunchKernelGGL(conv1_halo_wgrad_kernel, dim3((unsigned)p.S, (unsigned)groups), dim3(256), 0, stream, p);
  GEECO_LAUNCH_CHECK();
  geeco_launch_wgrad_reduce((const float*)ws, dw, db, gs_dw, gs_db, p.S, 9 * 4 * 32, 32, groups, stream);
  GEECO_LAUNCH_CHECK();
  *handled = 1;
  return 0;
}
