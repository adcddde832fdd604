// Input gradients: d(loss)/d(frames) for saliency maps.  Three jobs, none of them part of the training step:
//   geeco_conv1_dgrad      conv1's input gradient (Conv2DBackpropInput of the 3x3 stride-1 SAME layer, 32 -> Cin channels);
//   geeco_pack_pixels_bwd  the adjoint of geeco_pack_pixels (channel padding / rgb || depth);
//   geeco_dynimg_bwd       the adjoint of geeco_dynimg_fwd, per-sample min / max normalisation included.
// The reference has no counterpart (tf.gradients(loss, frames) would give the same numbers: TF 1.15's Conv2DBackpropInput,
// and its reduce_min / reduce_max gradient that shares evenly among ties).
#include "dynimg_internal.h"

// ---- conv1 input gradient -----------------------------------------------------------------------------------------------
//   dx[f][y][x][ci] = sum_{ky,kx,co} dz1[f][y+1-ky][x+1-kx][co] * w1[ky][kx][ci][co]
// 4 outputs per pixel against 288 x 4 products: the layer is bound by reading dz1 (128 B per pixel), not by arithmetic, so
// it runs on plain VALU FMAs -- an MFMA tile would be bent around an N of 4.  One block = one 8 x 32 pixel tile of one frame:
// its 10 x 34 halo of dz1 goes through LDS (every dz1 value leaves HBM once per tile that needs it; the halo is read again
// from L2), one thread = one pixel, 16-byte LDS reads of the 32-channel rows.  The LDS pixel pitch is 36 floats: consecutive
// lanes read 16-byte slots 9 apart, a permutation of the 16 slots of a bank row, so the reads do not conflict.  The weights
// (4.6 KB) are indexed by compile-time constants off a block-uniform pointer: they arrive through the scalar cache into
// SGPRs and feed the FMAs as scalar operands.  Summation order per output: ky, kx ascending, co ascending, one fmaf chain.
#define C1D_TY 8
#define C1D_TX 32
#define C1D_PITCH 36
#define C1D_CO 32

template <int CIN>
__global__ __launch_bounds__(256, 3) void conv1_dgrad_kernel(const float* __restrict__ dz, const float* __restrict__ w,
                                                          float* __restrict__ dx, long long gs_dz, long long gs_w,
                                                          long long gs_dx, int H, int W, int tiles_x) {
  __shared__ __attribute__((aligned(16))) float tile[(C1D_TY + 2) * (C1D_TX + 2) * C1D_PITCH];
  const int g = blockIdx.z, f = blockIdx.y;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int y0 = ty * C1D_TY, x0 = tx * C1D_TX;
  const float* dzf = dz + g * gs_dz + (long long)f * H * W * C1D_CO;
  const float* wg = w + g * gs_w;
  // stage the halo: (TY + 2) x (TX + 2) pixels x 8 float4, zeros outside the image (SAME padding of the transposed conv)
  constexpr int HALO_PIX = (C1D_TY + 2) * (C1D_TX + 2);
  for (int i = threadIdx.x; i < HALO_PIX * 8; i += 256) {
    const int pix = i >> 3, q = i & 7;
    const int r = pix / (C1D_TX + 2), c = pix - r * (C1D_TX + 2);
    const int y = y0 - 1 + r, x = x0 - 1 + c;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (y >= 0 && y < H && x >= 0 && x < W)
      v = *reinterpret_cast<const f32x4*>(dzf + ((long long)y * W + x) * C1D_CO + q * 4);
    *reinterpret_cast<f32x4*>(&tile[pix * C1D_PITCH + q * 4]) = v;
  }
  __syncthreads();
  const int ly = threadIdx.x >> 5, lx = threadIdx.x & 31;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      // dz1 pixel (y + 1 - ky, x + 1 - kx) = halo row ly + 2 - ky, column lx + 2 - kx
      const float* src = &tile[((ly + 2 - ky) * (C1D_TX + 2) + (lx + 2 - kx)) * C1D_PITCH];
      const float* wt = wg + (ky * 3 + kx) * CIN * C1D_CO;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + q * 4);
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci) {
          const float* wr = wt + ci * C1D_CO + q * 4;
          acc[ci] = fmaf(v.x, wr[0], acc[ci]);
          acc[ci] = fmaf(v.y, wr[1], acc[ci]);
          acc[ci] = fmaf(v.z, wr[2], acc[ci]);
          acc[ci] = fmaf(v.w, wr[3], acc[ci]);
        }
      }
    }
  }
  const int y = y0 + ly, x = x0 + lx;
  if (y < H && x < W) {
    float* o = dx + g * gs_dx + (((long long)f * H + y) * W + x) * 4;
    *reinterpret_cast<f32x4*>(o) = f32x4{acc[0], acc[1], acc[2], CIN == 4 ? acc[3] : 0.f};
  }
}

extern "C" int geeco_conv1_dgrad(const float* dz1, const float* w1, float* dx, int groups, int64_t gs_dz, int64_t gs_w,
                                 int64_t gs_dx, int F, int H, int W, int Cin, int Cout, void* stream) {
  if ((Cin != 3 && Cin != 4) || Cout != C1D_CO) {
    geeco_set_error("conv1_dgrad: built for conv1 (Cin 3 or 4, 32 output channels), got Cin=%d Cout=%d", Cin, Cout);
    return GEECO_ENOSUP;
  }
  GEECO_CHECK_ARG(dz1 && w1 && dx, "conv1_dgrad: null pointer");
  GEECO_CHECK_ARG(groups >= 1 && groups <= 65535 && F >= 1 && F <= 65535 && H >= 1 && W >= 1, "conv1_dgrad: bad dims");
  GEECO_CHECK_ARG(((uintptr_t)dz1 & 15) == 0 && ((uintptr_t)dx & 15) == 0 && ((uintptr_t)w1 & 3) == 0 && gs_dz % 4 == 0 &&
                  gs_dx % 4 == 0, "conv1_dgrad: dz1 / dx must be 16-byte aligned (group strides included)");
  const int tiles_x = cdiv(W, C1D_TX), tiles_y = cdiv(H, C1D_TY);
  GEECO_CHECK_ARG((long long)tiles_x * tiles_y <= 0x7fffffffLL, "conv1_dgrad: image too large");
  dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)F, (unsigned)groups);
  geeco_note_kernel("conv1_dgrad_valu<cin%d>", Cin);
  if (Cin == 3)
    hipLaunchKernelGGL(conv1_dgrad_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, dz1, w1, dx, (long long)gs_dz,
                       (long long)gs_w, (long long)gs_dx, H, W, tiles_x);
  else
    hipLaunchKernelGGL(conv1_dgrad_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, dz1, w1, dx, (long long)gs_dz,
                       (long long)gs_w, (long long)gs_dx, H, W, tiles_x);
  GEECO_LAUNCH_CHECK();
  return 0;
}

// ---- adjoint of geeco_pack_pixels ---------------------------------------------------------------------------------------
// d_src[n][p][0..C1) (+)= d_dst[n][p][0..C1), d_src2[n][p][0..C2) (+)= d_dst[n][p][C1..C1+C2): one thread per pixel, one add
// per element at most (bitwise a copy / one IEEE add).
__global__ __launch_bounds__(256) void pack_pixels_bwd_kernel(const float* __restrict__ d_dst, float* d_src, long long s1,
                                                              int acc1, float* d_src2, long long s2, int acc2, long long HW,
                                                              int C1, int C2, int Cpad) {
  const int n = blockIdx.y;
  const long long px = (long long)blockIdx.x * 256 + threadIdx.x;
  if (px >= HW) return;
  const float* gsrc = d_dst + ((long long)n * HW + px) * Cpad;
  if (d_src) {
    float* a = d_src + (long long)n * s1 + px * C1;
    for (int c = 0; c < C1; ++c) a[c] = acc1 ? a[c] + gsrc[c] : gsrc[c];
  }
  if (d_src2) {
    float* b = d_src2 + (long long)n * s2 + px * C2;
    for (int c = 0; c < C2; ++c) b[c] = acc2 ? b[c] + gsrc[C1 + c] : gsrc[C1 + c];
  }
}

extern "C" int geeco_pack_pixels_bwd(const float* d_dst, float* d_src, int64_t src_sample_stride, int accumulate, float* d_src2,
                                     int64_t src2_sample_stride, int accumulate2, int N, int64_t HW, int C1, int C2, int Cpad,
                                     void* stream) {
  GEECO_CHECK_ARG(d_dst && (d_src || d_src2), "pack_pixels_bwd: null pointer");
  GEECO_CHECK_ARG(N >= 1 && N <= 65535 && HW >= 1 && C1 >= 1 && C2 >= 0 && C1 + (d_src2 ? C2 : 0) <= Cpad,
                  "pack_pixels_bwd: bad dims");
  dim3 grid((unsigned)cdiv64(HW, 256), (unsigned)N);
  hipLaunchKernelGGL(pack_pixels_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, d_dst, d_src, (long long)src_sample_stride,
                     accumulate, d_src2, (long long)src2_sample_stride, accumulate2, (long long)HW, C1, d_src2 ? C2 : 0, Cpad);
  GEECO_LAUNCH_CHECK();
  return 0;
}

// ---- adjoint of geeco_dynimg_fwd ----------------------------------------------------------------------------------------
// out = (D - mn) / r, D = sum_t alpha_t X_t, mn / mx over the sample's H W C elements, r = mx - mn + 1e-6:
//   dD_i = g_i / r + [D_i == mn] (sum_j g_j (out_j - 1) / r) / n_min - [D_i == mx] (sum_j g_j out_j / r) / n_max
// (n_min / n_max = how many elements equal the extremum: TF 1.15's reduce_min / reduce_max gradient shares evenly among
// ties).  Both launches recompute D with the forward's own chain (acc = 0; acc += alpha_t * x_t, t ascending), so the
// positions of min / max are the forward's.  A frame is one flat run of HW * C floats; a thread takes V consecutive ones
// (V = 4 with 16-byte accesses when every stride allows it, else 1).
// Launch 1, per block b: mn_b, mx_b, how many of its elements equal each, S_b = sum g_j, T_b = sum g_j (D_j - mn_b) (against
// the BLOCK's minimum: no cancellation).  Launch 2 folds the records of its sample: sum_j g_j (D_j - mn) = sum_b T_b +
// (mn_b - mn) S_b.  Summation order, fixed (no atomics, two runs are bitwise equal): a thread over its elements ascending;
// the 64 lanes of a wave in the butterfly of wave_reduce_sum; the four waves ascending; the blocks ascending.
struct DynBwdParams {
  const float* g;            // [N][HW][Cpad]
  const float* frames;
  const float* frames2;
  long long sample_stride, frame_stride;
  float* d_frames;
  float* d_frames2;
  long long d_sample_stride, d_frame_stride;
  int acc1, acc2;
  int N, K, C, Cpad;
  long long total;           // HW * C
  int nblk;
  float* rec;                // [N][nblk][8]
  float alpha[DYN_MAXK];
};

__device__ __forceinline__ const float* dynb_frame(const DynBwdParams& p, int n, int t) {
  if (p.frames2 && t == 1) return p.frames2 + (long long)n * p.total;
  return p.frames + (long long)n * p.sample_stride + (long long)t * p.frame_stride;
}

// D and g of this thread's V elements (invalid ones: ok[k] = false, g = 0)
template <int V>
__device__ __forceinline__ void dynb_load(const DynBwdParams& p, int n, long long e0, float (&D)[V], float (&gv)[V], bool (&ok)[V]) {
#pragma unroll
  for (int k = 0; k < V; ++k) {
    D[k] = 0.f;
    gv[k] = 0.f;
    ok[k] = e0 + k < p.total;
  }
  if (!ok[0]) return;
  for (int t = 0; t < p.K; ++t) {
    const float w = p.alpha[t];
    const float* src = dynb_frame(p, n, t) + e0;
    if constexpr (V == 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(src);
      D[0] += w * v.x;
      D[1] += w * v.y;
      D[2] += w * v.z;
      D[3] += w * v.w;
    } else {
      D[0] += w * src[0];
    }
  }
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const long long e = e0 + k;
    const long long px = e / p.C;
    gv[k] = p.g[((long long)n * (p.total / p.C) + px) * p.Cpad + (int)(e - px * p.C)];
  }
}

__device__ __forceinline__ float block_sum_ordered(float v, float* sm) {      // lanes: butterfly; waves ascending
  v = wave_reduce_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sm[0] + sm[1]) + sm[2]) + sm[3];
}

template <int V>
__global__ __launch_bounds__(256) void dynimg_bwd_reduce_kernel(const DynBwdParams p) {
  __shared__ float sm[4], smn[4], smx[4];
  const int n = blockIdx.y;
  const long long e0 = ((long long)blockIdx.x * 256 + threadIdx.x) * V;
  float D[V], gv[V];
  bool ok[V];
  dynb_load<V>(p, n, e0, D, gv, ok);
  float mn = INFINITY, mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < V; ++k)
    if (ok[k]) {
      mn = fminf(mn, D[k]);
      mx = fmaxf(mx, D[k]);
    }
  mn = wave_reduce_min(mn);
  mx = wave_reduce_max(mx);
  if ((threadIdx.x & 63) == 0) {
    smn[threadIdx.x >> 6] = mn;
    smx[threadIdx.x >> 6] = mx;
  }
  __syncthreads();
  mn = fminf(fminf(smn[0], smn[1]), fminf(smn[2], smn[3]));
  mx = fmaxf(fmaxf(smx[0], smx[1]), fmaxf(smx[2], smx[3]));
  float cmin = 0.f, cmax = 0.f, s = 0.f, tb = 0.f;
#pragma unroll
  for (int k = 0; k < V; ++k)
    if (ok[k]) {
      cmin += D[k] == mn ? 1.f : 0.f;
      cmax += D[k] == mx ? 1.f : 0.f;
      s += gv[k];
      tb += gv[k] * (D[k] - mn);
    }
  cmin = block_sum_ordered(cmin, sm);      // (counts <= 1024: exact)
  cmax = block_sum_ordered(cmax, sm);
  s = block_sum_ordered(s, sm);
  tb = block_sum_ordered(tb, sm);
  if (threadIdx.x == 0) {
    float* r = p.rec + ((long long)n * p.nblk + blockIdx.x) * 8;
    r[0] = mn; r[1] = mx; r[2] = cmin; r[3] = cmax; r[4] = s; r[5] = tb;
  }
}

template <int V>
__global__ __launch_bounds__(256) void dynimg_bwd_apply_kernel(const DynBwdParams p) {
  __shared__ float s_par[5];      // mn, mx, r, what a minimum takes, what a maximum gives
  const int n = blockIdx.y;
  if (threadIdx.x == 0) {
    const float* rec = p.rec + (long long)n * p.nblk * 8;
    float mn = INFINITY, mx = -INFINITY;
    for (int b = 0; b < p.nblk; ++b) {
      mn = fminf(mn, rec[b * 8]);
      mx = fmaxf(mx, rec[b * 8 + 1]);
    }
    float nmin = 0.f, nmax = 0.f, S = 0.f, T = 0.f;      // blocks ascending
    for (int b = 0; b < p.nblk; ++b) {
      const float* r = rec + b * 8;
      if (r[0] == mn) nmin += r[2];
      if (r[1] == mx) nmax += r[3];
      S += r[4];
      T += r[5] + (r[0] - mn) * r[4];
    }
    const float rng = mx - mn + 1e-6f;
    const float A = T / rng;                 // sum_j g_j out_j
    s_par[0] = mn;
    s_par[1] = mx;
    s_par[2] = rng;
    s_par[3] = ((A - S) / rng) / nmin;       // what every minimum takes
    s_par[4] = (A / rng) / nmax;             // what every maximum gives
  }
  __syncthreads();
  const float mn = s_par[0], mx = s_par[1], rng = s_par[2], cmn = s_par[3], cmx = s_par[4];
  const long long e0 = ((long long)blockIdx.x * 256 + threadIdx.x) * V;
  float D[V], gv[V];
  bool ok[V];
  dynb_load<V>(p, n, e0, D, gv, ok);
  if (!ok[0]) return;
  float dD[V];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    float d = gv[k] / rng;
    if (D[k] == mn) d += cmn;
    if (D[k] == mx) d -= cmx;
    dD[k] = d;
  }
  for (int t = 0; t < p.K; ++t) {
#pragma clang fp contract(off)      // accumulate = ONE float32 addition of the value the overwriting form stores (no fma with alpha_t)
    const bool second = p.frames2 && t == 1;
    float* dst = second ? p.d_frames2 : p.d_frames;
    if (!dst) continue;
    dst += second ? (long long)n * p.total + e0 : (long long)n * p.d_sample_stride + (long long)t * p.d_frame_stride + e0;
    const int acc = second ? p.acc2 : p.acc1;
    const float w = p.alpha[t];
    if constexpr (V == 4) {
      f32x4 o = {w * dD[0], w * dD[1], w * dD[2], w * dD[3]};
      if (acc) {
        const f32x4 old = *reinterpret_cast<const f32x4*>(dst);
        o = f32x4{old.x + o.x, old.y + o.y, old.z + o.z, old.w + o.w};
      }
      *reinterpret_cast<f32x4*>(dst) = o;
    } else {
      const float o = w * dD[0];
      dst[0] = acc ? dst[0] + o : o;
    }
  }
}

extern "C" int64_t geeco_dynimg_bwd_ws_bytes(int N, int64_t HW, int C) {
  return (int64_t)N * (cdiv64(HW * C, 256) + 1) * 8 * 4;      // one record per 256 elements at most (V = 1)
}

extern "C" int geeco_dynimg_bwd(const float* g, const float* frames, const float* frames2, int64_t sample_stride,
                                int64_t frame_stride, const float* alpha_host, int N, int K, int64_t HW, int C, int Cpad,
                                float* d_frames, int64_t d_sample_stride, int64_t d_frame_stride, int accumulate,
                                float* d_frames2, int accumulate2, void* ws, void* stream) {
  GEECO_CHECK_ARG(g && frames && alpha_host && ws && (d_frames || d_frames2), "dynimg_bwd: null pointer");
  GEECO_CHECK_ARG(K >= 1 && K <= DYN_MAXK, "dynimg_bwd: K=%d outside 1..%d", K, DYN_MAXK);
  GEECO_CHECK_ARG(N >= 1 && N <= 65535 && HW >= 1 && C >= 1 && C <= Cpad && Cpad <= 8, "dynimg_bwd: bad dims");
  GEECO_CHECK_ARG(!frames2 || K == 2, "dynimg_bwd: frames2 only with K == 2");
  GEECO_CHECK_ARG(!d_frames2 || frames2, "dynimg_bwd: d_frames2 only in the two-frame form");
  DynBwdParams p = {};
  p.g = g; p.frames = frames; p.frames2 = frames2; p.sample_stride = sample_stride; p.frame_stride = frame_stride;
  p.d_frames = d_frames; p.d_frames2 = d_frames2; p.d_sample_stride = d_sample_stride; p.d_frame_stride = d_frame_stride;
  p.acc1 = accumulate; p.acc2 = accumulate2; p.N = N; p.K = K; p.C = C; p.Cpad = Cpad; p.total = HW * C; p.rec = (float*)ws;
  for (int t = 0; t < K; ++t) p.alpha[t] = alpha_host[t];
  auto al16 = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
  const bool vec = p.total % 4 == 0 && sample_stride % 4 == 0 && frame_stride % 4 == 0 && d_sample_stride % 4 == 0 &&
                   d_frame_stride % 4 == 0 && al16(frames) && al16(frames2) && al16(d_frames) && al16(d_frames2);
  const int V = vec ? 4 : 1;
  p.nblk = (int)cdiv64(p.total, 256 * V);
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((unsigned)p.nblk, (unsigned)N);
  if (vec) {
    hipLaunchKernelGGL(dynimg_bwd_reduce_kernel<4>, grid, dim3(256), 0, s, p);
    GEECO_LAUNCH_CHECK();
    hipLaunchKernelGGL(dynimg_bwd_apply_kernel<4>, grid, dim3(256), 0, s, p);
  } else {
    hipLaunchKernelGGL(dynimg_bwd_reduce_kernel<1>, grid, dim3(256), 0, s, p);
    GEECO_LAUNCH_CHECK();
    hipLaunchKernelGGL(dynimg_bwd_apply_kernel<1>, grid, dim3(256), 0, s, p);
  }
  GEECO_LAUNCH_CHECK();
  return 0;
}
