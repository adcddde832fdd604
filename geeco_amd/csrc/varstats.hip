// Opt-in per-variable statistics of the gradient, the parameters and the update direction: what a logging step reports
// of each variable of the arena.  Two launches, read-only on the four arenas, never part of a captured step.  The record and the
// calling convention: include/geeco_hip.h (geeco_variable_stats).
#include "geeco_common.h"

// ---- the reduction order (the tests count their roundings from it) ----------------------------------
// A variable is cut into chunks of CH = GEECO_VARSTATS_CHUNK elements from its own first element (its last chunk is shorter); a chunk
// never straddles two variables and holds no pad.
// Pass 1, one 256-thread block per chunk.  Thread t owns the elements 4 (t + 256 j) .. + 3 of the chunk, j = 0..3, and folds them in
//   ascending offset order into its own running values: a sum by one addition per element, a sum of squares by one FMA per element
//   (x * x is not rounded on its own), extrema by min / max, counts by integer additions.  Then, per value, the wave butterfly
//   (6 levels of xor-shuffles, offsets 32 .. 1) and the four wave results left to right: ((w0 + w1) + w2) + w3.  That is at most
//   16 + 6 + 3 = 25 additions on the path of any element, as in csrc/clip.hip.  One partial record per chunk goes to the workspace.
//   The classes are counted with LDS integer atomics, one table per wave, the four tables added by 160 threads: integer addition is
//   order-free, so the counts do not depend on the order the atomics land in.
// Pass 2, one 256-thread block per variable.  Thread t folds the partials t, t + 256, ... of the variable's chunks in ascending
//   order (ceil(chunks / 256) additions), then the same butterfly and the same left-to-right sum of the wave results: + 6 + 3.
//   The class counts of all its chunks are added per class with LDS integer atomics (int64), all 256 threads side by side.
// There is no float atomic anywhere.  An element's VALUES do not depend on how it was loaded (16-byte or scalar load, whichever
// piece holds its gradient), so the record is bitwise the same for any partition of the gradient into pieces and from call to call.
//
// What is in no sum: an element whose exponent field is 255 (NaN, +-inf) is counted in `nonfinite` and skipped, so one NaN does not
// poison the record of its variable (deliberately unlike geeco_clip_scale).  A finite x with x * x beyond float32 still makes the sum
// of squares +inf: the sums are float32.
#define VS_CH GEECO_VARSTATS_CHUNK
#define VS_NCLS GEECO_VARSTATS_CLASSES
static_assert(VS_CH == 4096, "a chunk is four float4s per thread of a 256-thread block");
#define VS_NF 10                  // float words of a partial record
#define VS_NI 6                   // integer words behind them
#define VS_HIST (4 * VS_NCLS)     // gradient neg, gradient pos, parameter neg, parameter pos
#define VS_WORDS 180              // VS_NF + VS_NI + VS_HIST, padded to a multiple of 4 words
static_assert(VS_NF + VS_NI + VS_HIST <= VS_WORDS && VS_WORDS % 4 == 0, "partial record");
// float words: 0 g sum, 1 g sumsq, 2 g min, 3 g max, 4 p sum, 5 p sumsq, 6 p min, 7 p max, 8 u sumsq, 9 u max
// integer words: 10 g covered, 11 g non-finite, 12 g zeros, 13 p non-finite, 14 p zeros, 15 u non-finite

struct VsSegs {
  const float* g[GEECO_ADAM_SEGMENTS_MAX];
  long long off[GEECO_ADAM_SEGMENTS_MAX];
  long long cnt[GEECO_ADAM_SEGMENTS_MAX];
  int n;
};

struct VsTally {
  float sum, sumsq, mn, mx;
  unsigned nonfinite, zeros;
};

__device__ __forceinline__ void vs_tally(VsTally& t, float x, unsigned* hist) {
  const unsigned bits = __float_as_uint(x), ex = (bits >> 23) & 0xffu;
  if (ex == 255u) {
    ++t.nonfinite;
    return;
  }
  t.sum += x;
  t.sumsq = fmaf(x, x, t.sumsq);
  t.mn = fminf(t.mn, x);
  t.mx = fmaxf(t.mx, x);
  if ((bits & 0x7fffffffu) == 0u) {
    ++t.zeros;
  } else {
    int e = (int)ex - 127;
    e = e < -32 ? -32 : (e > 7 ? 7 : e);
    atomicAdd(&hist[((bits >> 31) ? 0 : VS_NCLS) + e + 32], 1u);
  }
}

__device__ __forceinline__ unsigned wave_reduce_sum_u32(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned long long wave_reduce_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void varstats_chunk_kernel(const float* __restrict__ p, const float* __restrict__ m, const float* __restrict__ v,
                                                             const VsSegs s, float gscale, float eps, const long long* __restrict__ chunks,
                                                             unsigned* __restrict__ ws) {
  __shared__ unsigned hist[4][VS_HIST];
  __shared__ float swf[4][VS_NF];
  __shared__ unsigned swi[4][VS_NI];
  for (int i = threadIdx.x; i < 4 * VS_HIST; i += 256) (&hist[0][0])[i] = 0u;
  __syncthreads();
  const int wave = threadIdx.x >> 6;
  const long long base = chunks[2 * (long long)blockIdx.x];        // a multiple of 4: the variable's offset is, and so is CH
  const int cnt = (int)chunks[2 * (long long)blockIdx.x + 1];      // 1 .. CH
  const float inf = __uint_as_float(0x7f800000u);
  VsTally tg = {0.f, 0.f, inf, -inf, 0u, 0u}, tp = {0.f, 0.f, inf, -inf, 0u, 0u};
  float u_sumsq = 0.f, u_max = 0.f;
  unsigned u_nonfinite = 0u, covered = 0u;
#pragma unroll 1      // (the piece lookup is 8 unrolled cases, as in csrc/clip.hip)
  for (int j = 0; j < VS_CH / 1024; ++j) {
    const int r0 = 4 * ((int)threadIdx.x + 256 * j);
    if (r0 >= cnt) break;
    const int lanes = cnt - r0 >= 4 ? 4 : cnt - r0;       // the chunk's tail: 1..3 elements, loaded one by one (what follows is pad or slack)
    const long long e = base + r0;
    float ge[4] = {0.f, 0.f, 0.f, 0.f};
    bool have[4] = {false, false, false, false};
#pragma unroll
    for (int k = 0; k < GEECO_ADAM_SEGMENTS_MAX; ++k) {
      if (k >= s.n) break;
      const long long r = e - s.off[k], pc = s.cnt[k];    // element e is element r of piece k
      if (r <= -4 || r >= pc) continue;
      const float* __restrict__ gs = s.g[k];
      if (lanes == 4 && r >= 0 && r + 4 <= pc && (r & 3) == 0 && ((uintptr_t)gs & 15) == 0) {
        const f32x4 gv = reinterpret_cast<const f32x4*>(gs)[r >> 2];
        ge[0] = gv.x; ge[1] = gv.y; ge[2] = gv.z; ge[3] = gv.w;
        have[0] = have[1] = have[2] = have[3] = true;
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const long long rc = r + c;
          if (c < lanes && rc >= 0 && rc < pc) {          // tested against the piece's count before the address is formed
            ge[c] = gs[rc];
            have[c] = true;
          }
        }
      }
    }
    float pe[4] = {0.f, 0.f, 0.f, 0.f}, me[4] = {0.f, 0.f, 0.f, 0.f}, ve[4] = {0.f, 0.f, 0.f, 0.f};
    if (lanes == 4) {
      const f32x4 pv = reinterpret_cast<const f32x4*>(p)[e >> 2], mv = reinterpret_cast<const f32x4*>(m)[e >> 2],
                  vv = reinterpret_cast<const f32x4*>(v)[e >> 2];
      pe[0] = pv.x; pe[1] = pv.y; pe[2] = pv.z; pe[3] = pv.w;
      me[0] = mv.x; me[1] = mv.y; me[2] = mv.z; me[3] = mv.w;
      ve[0] = vv.x; ve[1] = vv.y; ve[2] = vv.z; ve[3] = vv.w;
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < lanes) {
          pe[c] = p[e + c];
          me[c] = m[e + c];
          ve[c] = v[e + c];
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c >= lanes) continue;
      if (have[c]) {
        ++covered;
        vs_tally(tg, __fmul_rn(ge[c], gscale), &hist[wave][0]);      // the product rounded on its own: its bits are what is classed
      }
      vs_tally(tp, pe[c], &hist[wave][2 * VS_NCLS]);
      const float u = me[c] / (sqrtf(ve[c]) + eps);
      if (((__float_as_uint(u) >> 23) & 0xffu) == 255u) {
        ++u_nonfinite;
      } else {
        u_sumsq = fmaf(u, u, u_sumsq);
        u_max = fmaxf(u_max, fabsf(u));
      }
    }
  }
  float f[VS_NF] = {tg.sum, tg.sumsq, tg.mn, tg.mx, tp.sum, tp.sumsq, tp.mn, tp.mx, u_sumsq, u_max};
  unsigned q[VS_NI] = {covered, tg.nonfinite, tg.zeros, tp.nonfinite, tp.zeros, u_nonfinite};
#pragma unroll
  for (int i = 0; i < VS_NF; ++i) {
    const bool is_min = i == 2 || i == 6, is_max = i == 3 || i == 7 || i == 9;
    f[i] = is_min ? wave_reduce_min(f[i]) : (is_max ? wave_reduce_max(f[i]) : wave_reduce_sum(f[i]));
  }
#pragma unroll
  for (int i = 0; i < VS_NI; ++i) q[i] = wave_reduce_sum_u32(q[i]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int i = 0; i < VS_NF; ++i) swf[wave][i] = f[i];
#pragma unroll
    for (int i = 0; i < VS_NI; ++i) swi[wave][i] = q[i];
  }
  __syncthreads();      // (also: every wave's class counts have landed)
  unsigned* out = ws + (long long)blockIdx.x * VS_WORDS;
  if (threadIdx.x < VS_NF) {
    const int i = threadIdx.x;
    const bool is_min = i == 2 || i == 6, is_max = i == 3 || i == 7 || i == 9;
    const float a = swf[0][i], b = swf[1][i], c = swf[2][i], d = swf[3][i];
    const float r = is_min ? fminf(fminf(fminf(a, b), c), d) : (is_max ? fmaxf(fmaxf(fmaxf(a, b), c), d) : ((a + b) + c) + d);
    out[i] = __float_as_uint(r);
  } else if (threadIdx.x < VS_NF + VS_NI) {
    const int i = threadIdx.x - VS_NF;
    out[VS_NF + i] = swi[0][i] + swi[1][i] + swi[2][i] + swi[3][i];
  } else if (threadIdx.x >= 64 && threadIdx.x < 64 + VS_HIST) {
    const int h = threadIdx.x - 64;
    out[VS_NF + VS_NI + h] = hist[0][h] + hist[1][h] + hist[2][h] + hist[3][h];
  }
}

__global__ __launch_bounds__(256) void varstats_fold_kernel(const unsigned* __restrict__ ws, const long long* __restrict__ table,
                                                            geeco_varstats_record* __restrict__ out) {
  __shared__ float swf[4][VS_NF];
  __shared__ unsigned long long swi[4][VS_NI];
  __shared__ unsigned long long hist[VS_HIST];
  if (threadIdx.x < VS_HIST) hist[threadIdx.x] = 0ull;      // (the barrier behind the wave results below orders it before the first atomic)
  const long long c0 = table[2 * (long long)blockIdx.x], nc = table[2 * (long long)blockIdx.x + 1];
  const unsigned* part = ws + c0 * VS_WORDS;
  const float inf = __uint_as_float(0x7f800000u);
  float f[VS_NF] = {0.f, 0.f, inf, -inf, 0.f, 0.f, inf, -inf, 0.f, 0.f};
  unsigned long long q[VS_NI] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
  for (long long c = threadIdx.x; c < nc; c += 256) {
    const unsigned* w = part + c * VS_WORDS;
#pragma unroll
    for (int i = 0; i < VS_NF; ++i) {
      const bool is_min = i == 2 || i == 6, is_max = i == 3 || i == 7 || i == 9;
      const float x = __uint_as_float(w[i]);
      f[i] = is_min ? fminf(f[i], x) : (is_max ? fmaxf(f[i], x) : f[i] + x);
    }
#pragma unroll
    for (int i = 0; i < VS_NI; ++i) q[i] += w[VS_NF + i];
  }
#pragma unroll
  for (int i = 0; i < VS_NF; ++i) {
    const bool is_min = i == 2 || i == 6, is_max = i == 3 || i == 7 || i == 9;
    f[i] = is_min ? wave_reduce_min(f[i]) : (is_max ? wave_reduce_max(f[i]) : wave_reduce_sum(f[i]));
  }
#pragma unroll
  for (int i = 0; i < VS_NI; ++i) q[i] = wave_reduce_sum_u64(q[i]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int i = 0; i < VS_NF; ++i) swf[threadIdx.x >> 6][i] = f[i];
#pragma unroll
    for (int i = 0; i < VS_NI; ++i) swi[threadIdx.x >> 6][i] = q[i];
  }
  __syncthreads();
  geeco_varstats_record* rec = out + blockIdx.x;
  if (threadIdx.x == 0) {
    float r[VS_NF];
#pragma unroll
    for (int i = 0; i < VS_NF; ++i) {
      const bool is_min = i == 2 || i == 6, is_max = i == 3 || i == 7 || i == 9;
      const float a = swf[0][i], b = swf[1][i], c = swf[2][i], d = swf[3][i];
      r[i] = is_min ? fminf(fminf(fminf(a, b), c), d) : (is_max ? fmaxf(fmaxf(fmaxf(a, b), c), d) : ((a + b) + c) + d);
    }
    unsigned long long k[VS_NI];
#pragma unroll
    for (int i = 0; i < VS_NI; ++i) k[i] = swi[0][i] + swi[1][i] + swi[2][i] + swi[3][i];
    rec->grad_covered = (int64_t)k[0];
    rec->grad.nonfinite = (int64_t)k[1];
    rec->grad.zeros = (int64_t)k[2];
    rec->grad.sum = r[0]; rec->grad.sumsq = r[1]; rec->grad.min = r[2]; rec->grad.max = r[3];
    rec->param.nonfinite = (int64_t)k[3];
    rec->param.zeros = (int64_t)k[4];
    rec->param.sum = r[4]; rec->param.sumsq = r[5]; rec->param.min = r[6]; rec->param.max = r[7];
    rec->update_nonfinite = (int64_t)k[5];
    rec->update_sumsq = r[8];
    rec->update_max_abs = r[9];
  }
  // the classes: wave w walks the chunks w, w + 4, ..., its lanes on consecutive words of the chunk's record (independent loads), and
  // adds what is not zero per class with LDS integer atomics
  for (long long c = threadIdx.x >> 6; c < nc; c += 4) {
    const unsigned* w = part + c * VS_WORDS + VS_NF + VS_NI;
#pragma unroll
    for (int h = threadIdx.x & 63; h < VS_HIST; h += 64) {
      const unsigned x = w[h];
      if (x) atomicAdd(&hist[h], (unsigned long long)x);
    }
  }
  __syncthreads();
  if (threadIdx.x < VS_HIST) {
    const int h = threadIdx.x;
    geeco_varstats_tensor* t = h < 2 * VS_NCLS ? &rec->grad : &rec->param;
    const int hh = h % (2 * VS_NCLS);
    (hh < VS_NCLS ? t->neg : t->pos)[hh % VS_NCLS] = (int64_t)hist[h];
  }
}

extern "C" int64_t geeco_variable_stats_ws_bytes(int64_t nchunks) { return nchunks >= 1 ? nchunks * (int64_t)(VS_WORDS * sizeof(unsigned)) : 0; }

extern "C" int geeco_variable_stats(const float* p, const float* m, const float* v, const geeco_adam_segment* segs, int nseg, int64_t n,
                                    float grad_scale, float eps, const int64_t* var_off, const int64_t* var_cnt, int nvar,
                                    const int64_t* table, int64_t nchunks, void* ws, geeco_varstats_record* out, void* stream) {
  GEECO_CHECK_ARG(p && m && v && segs && var_off && var_cnt && table && ws && out, "variable_stats: null pointer");
  GEECO_CHECK_ARG((((uintptr_t)p | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ws) & 15) == 0 && (((uintptr_t)table | (uintptr_t)out) & 7) == 0,
                  "variable_stats: the arenas and the workspace must be 16-byte aligned, the table and the records 8-byte aligned");
  GEECO_CHECK_ARG(n >= 1 && nvar >= 1, "variable_stats: an arena of %lld floats with %d variables (at least 1 each)", (long long)n, nvar);
  GEECO_CHECK_ARG(nseg >= 1 && nseg <= GEECO_ADAM_SEGMENTS_MAX, "variable_stats: %d pieces of the gradient (1..%d)", nseg, GEECO_ADAM_SEGMENTS_MAX);
  GEECO_CHECK_ARG(eps >= 0.f && eps <= 3.402823466e38f, "variable_stats: eps %g is negative or not finite", (double)eps);
  int64_t chunks = 0;
  for (int i = 0; i < nvar; ++i) {
    GEECO_CHECK_ARG(var_off[i] >= 0 && (var_off[i] & 3) == 0 && var_cnt[i] >= 1 && var_cnt[i] <= n - var_off[i],
                    "variable_stats: variable %d: offset %lld is no multiple of 4, count %lld < 1, or the span lies outside the arena of %lld floats",
                    i, (long long)var_off[i], (long long)var_cnt[i], (long long)n);
    for (int q = 0; q < i; ++q)
      GEECO_CHECK_ARG(var_off[i] >= var_off[q] + var_cnt[q] || var_off[q] >= var_off[i] + var_cnt[i], "variable_stats: variables %d and %d overlap", q, i);
    chunks += cdiv64(var_cnt[i], VS_CH);
  }
  GEECO_CHECK_ARG(chunks == nchunks && nchunks <= 0x7fffffffll, "variable_stats: the variables make %lld chunks, the table is said to hold %lld",
                  (long long)chunks, (long long)nchunks);
  VsSegs s = {};
  s.n = nseg;
  for (int k = 0; k < nseg; ++k) {
    GEECO_CHECK_ARG(segs[k].g && ((uintptr_t)segs[k].g & 3) == 0 && segs[k].p_off >= 0 && segs[k].count >= 1 && segs[k].count <= n - segs[k].p_off,
                    "variable_stats: piece %d: null or misaligned gradients, or [offset, offset + count) outside the arena of %lld floats", k,
                    (long long)n);
    for (int q = 0; q < k; ++q)
      GEECO_CHECK_ARG(segs[k].p_off >= segs[q].p_off + segs[q].count || segs[q].p_off >= segs[k].p_off + segs[k].count,
                      "variable_stats: pieces %d and %d overlap", q, k);
    s.g[k] = segs[k].g;
    s.off[k] = segs[k].p_off;
    s.cnt[k] = segs[k].count;
  }
  hipLaunchKernelGGL(varstats_chunk_kernel, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream, p, m, v, s, grad_scale, eps,
                     (const long long*)table + 2 * (long long)nvar, (unsigned*)ws);
  GEECO_LAUNCH_CHECK();
  hipLaunchKernelGGL(varstats_fold_kernel, dim3((unsigned)nvar), dim3(256), 0, (hipStream_t)stream, (const unsigned*)ws, (const long long*)table, out);
  GEECO_LAUNCH_CHECK();
  return 0;
}
