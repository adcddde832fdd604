// Perturbation attributions: occlusion sensitivity and RISE (geeco_amd/perturbation.py).  Hide a region of the input,
// run the model's own forward, see how far the command moves -- no backward.  What is here are the streaming stages around that
// forward, on the launch path and the group loop of attr_stream.h, which attribution.hip shares:
//   1. perturb_apply:       dst = x where o == 0, fill where o == 1, x + o (fill - x) otherwise    the occluded input;
//   2. perturb_score:       d[n] = sum_j w_j (p[n][j] - p0[n][j])^2                                how far the command moved;
//   3. perturb_accumulate:  num += d[n] o, den += o  where o != 0                                   the running sums per pixel;
//   4. perturb_finish:      saliency = den > 0 ? num / den : +0.
// o(step, sample, y, x) in [0, 1], the occlusion weight, is shared by the frames and channels of a pixel; it is never stored: 1. and 3.
// recompute it with ONE device function (perturb_weight) from the step's description, so the two cannot disagree.  HBM-streaming,
// wave64, grid-stride within a sample (blockIdx.y = sample, so the random bits of a RISE mask are formed once per block, in LDS),
// 16-byte accesses where pointers and sizes allow, one float per access otherwise, no atomics.  Every float32 operation is rounded
// on its own (attr_stream.h), so every path gives numpy's float32 bits (tests/_perturbation_ref.py).
#include "geeco_common.h"
#include "philox_normal.h"
#include "attr_stream.h"

#define PT_MAXBITS 1024      // (g + 1)^2 keep-bits, g <= 31

// One step of one launch, by value: the image, the step's patch (occlusion) or the mask grid and the generator's words (RISE).
struct PerturbStep {
  int H, W;
  int y0, y1, x0, x1;          // occlusion: the step's patch, rows [y0, y1) x columns [x0, x1), clipped to the image
  int g, ch, cw;               // RISE: grid, cell height and width
  float inv_ch, inv_cw;        // 1 / ch, 1 / cw rounded to float32 (formed on the host)
  unsigned threshold, k0, k1, step;
  int sample0;                 // the sample the launch's first sample is in the generator's numbering
};

// RISE: the keep-bits and the shift of ``sample`` at the step, once per block.  Word i (i < (g + 1)^2 + 2) is output i % 4 of the
// Philox counter (i / 4, sample, step, 1) under the key words (k0, k1); see include/geeco_hip.h.
template <bool RISE>
__device__ __forceinline__ void perturb_prepare(const PerturbStep& s, int sample, float* keep, int* shift) {
  if (!RISE) return;
  const int nb = (s.g + 1) * (s.g + 1), calls = (nb + 2 + 3) >> 2;
  for (int q = threadIdx.x; q < calls; q += AT_THREADS) {
    unsigned w[4];
    philox4x32_10((unsigned)q, (unsigned)sample, s.step, 1u, s.k0, s.k1, w);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = 4 * q + j;
      if (i < nb) keep[i] = w[j] < s.threshold ? 1.f : 0.f;
      else if (i == nb) shift[0] = (int)(w[j] % (unsigned)s.ch);
      else if (i == nb + 1) shift[1] = (int)(w[j] % (unsigned)s.cw);
    }
  }
  __syncthreads();
}

// THE occlusion weight of pixel (y, x).  Occlusion: 1 inside the patch, 0 outside.  RISE: 1 - the bilinear interpolation of the
// keep-bits at ((y + dy) / ch, (x + dx) / cw), in the order the header states.
template <bool RISE>
__device__ __forceinline__ float perturb_weight(const PerturbStep& s, const float* keep, const int* shift, int y, int x) {
  if (!RISE) return (y >= s.y0 && y < s.y1 && x >= s.x0 && x < s.x1) ? 1.f : 0.f;
  const int yy = y + shift[0], xx = x + shift[1];
  const int r = yy / s.ch, c = xx / s.cw;
  const float fy = at_mul((float)(yy - r * s.ch), s.inv_ch), fx = at_mul((float)(xx - c * s.cw), s.inv_cw);
  const int r1 = r < s.g ? r + 1 : s.g, c1 = c < s.g ? c + 1 : s.g, g1 = s.g + 1;
  const float k00 = keep[r * g1 + c], k01 = keep[r * g1 + c1], k10 = keep[r1 * g1 + c], k11 = keep[r1 * g1 + c1];
  const float top = at_add(k00, at_mul(fx, at_sub(k01, k00))), bot = at_add(k10, at_mul(fx, at_sub(k11, k10)));
  return at_sub(1.f, at_add(top, at_mul(fy, at_sub(bot, top))));
}

// f(p0, np, o) for the units of four consecutive pixels p0 .. p0 + np - 1 of sample blockIdx.y that one thread owns (the last
// unit of HW may hold np < 4), o[j] their weights (0 past np): the sample's draws are prepared once per block, in LDS.
template <bool RISE, class F>
__device__ __forceinline__ void perturb_for_units(const PerturbStep& s, int HW, F&& f) {
  __shared__ float keep[RISE ? PT_MAXBITS : 1];
  __shared__ int shift[2];
  perturb_prepare<RISE>(s, s.sample0 + blockIdx.y, keep, shift);
  const int units = (HW + 3) >> 2;
  for (int u = blockIdx.x * AT_THREADS + threadIdx.x; u < units; u += gridDim.x * AT_THREADS) {
    const int p0 = u << 2, np = HW - p0 >= 4 ? 4 : HW - p0;
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int p = p0 + j, y = p / s.W;
      o[j] = j < np ? perturb_weight<RISE>(s, keep, shift, y, p - y * s.W) : 0.f;
    }
    f(p0, np, o);
  }
}

// ---- 1. the occluded input -----------------------------------------------------------------------------------------------------
// Tensors [N][frames][HW][C].  A thread owns units of four consecutive pixels of one sample (the last unit may hold fewer): their
// weights are formed once and serve every frame and channel, C groups of four elements per frame.
template <int C, bool V, bool RISE>
__global__ __launch_bounds__(AT_THREADS) void perturb_apply_kernel(float* __restrict__ dst, const float* __restrict__ x,
                                                                  const float* __restrict__ fill, long long period, int bv,
                                                                  PerturbStep s, int frames, int HW, long long n) {
  const long long base = (long long)blockIdx.y * frames * HW * C;
  const bool small = n <= 0xffffffffLL;
  perturb_for_units<RISE>(s, HW, [&](int p0, int np, const float o[4]) {
    const bool hidden = o[0] != 0.f || o[1] != 0.f || o[2] != 0.f || o[3] != 0.f;
    for (int f = 0; f < frames; ++f) {
      const long long e0 = base + ((long long)f * HW + p0) * C;
#pragma unroll
      for (int q = 0; q < C; ++q) {
        const long long e = e0 + 4 * q;
        const int left = np * C - 4 * q, cnt = left >= 4 ? 4 : left;
        if (cnt <= 0) continue;
        float xv[4], b[4] = {0.f, 0.f, 0.f, 0.f};
        attr_load4<V>(x, e, cnt, xv);
        if (hidden) {
          if (bv) attr_baseline4<true>(fill, period, small, e, cnt, b);
          else attr_baseline4<false>(fill, period, small, e, cnt, b);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float oj = o[(4 * q + j) / C];
            xv[j] = oj == 0.f ? xv[j] : (oj == 1.f ? b[j] : at_add(xv[j], at_mul(oj, at_sub(b[j], xv[j]))));
          }
        }
        attr_store4<V>(dst, e, cnt, xv);
      }
    }
  });
}

// The incremental form of the occlusion grid: dst holds the input of the previous step.  Only two patches change: the step's own
// (fill) and what the previous one hid outside it (the clean input again).  A thread owns one pixel of one of the two, all frames
// and channels; a pixel both patches hold is written once, by the step's own patch.  Copies and no arithmetic: the same bits as
// the whole rewrite.  (px0 .. py1: the previous patch.)
template <int C>
__global__ __launch_bounds__(AT_THREADS) void perturb_apply_patch_kernel(float* __restrict__ dst, const float* __restrict__ x,
                                                                        const float* __restrict__ fill, long long period, PerturbStep s,
                                                                        int py0, int py1, int px0, int px1, int frames, int HW,
                                                                        long long n) {
  const long long base = (long long)blockIdx.y * frames * HW * C;
  const bool small = n <= 0xffffffffLL;
  const int w_new = s.x1 - s.x0, a_new = (s.y1 - s.y0) * w_new, w_prev = px1 - px0, items = a_new + (py1 - py0) * w_prev;
  for (int i = blockIdx.x * AT_THREADS + threadIdx.x; i < items; i += gridDim.x * AT_THREADS) {
    int y, xx;
    const bool own = i < a_new;
    if (own) {
      y = s.y0 + i / w_new, xx = s.x0 + i % w_new;
    } else {
      y = py0 + (i - a_new) / w_prev, xx = px0 + (i - a_new) % w_prev;
      if (y >= s.y0 && y < s.y1 && xx >= s.x0 && xx < s.x1) continue;
    }
    for (int f = 0; f < frames; ++f) {
      const long long e0 = base + ((long long)f * HW + (long long)y * s.W + xx) * C;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const long long e = e0 + c;
        float v = x[e];
        if (own) v = fill ? fill[small ? (long long)((unsigned)e % (unsigned)period) : e % period] : 0.f;
        dst[e] = v;
      }
    }
  }
}

// ---- 2. the score --------------------------------------------------------------------------------------------------------------
// One thread per sample: j ascending from +0, difference, square, weight and sum each rounded on its own.
__global__ __launch_bounds__(64) void perturb_score_kernel(float* __restrict__ d, const float* __restrict__ preds,
                                                          const float* __restrict__ preds0, const float* __restrict__ w, int N, int OT) {
  const int n = blockIdx.x * 64 + threadIdx.x;
  if (n >= N) return;
  float acc = 0.f;
  for (int j = 0; j < OT; ++j) {
    const float t = at_sub(preds[(long long)n * OT + j], preds0[(long long)n * OT + j]);
    acc = at_add(acc, at_mul(w[j], at_mul(t, t)));
  }
  d[n] = acc;
}

// ---- 3. the running sums -------------------------------------------------------------------------------------------------------
// num, den [N][HW].  Where o == 0 the step adds nothing (a NaN score stays on the pixels its step hid); OVERWRITE: num and den are
// not read, and such a pixel starts at +0.
template <bool V, bool RISE, bool OVERWRITE>
__global__ __launch_bounds__(AT_THREADS) void perturb_accumulate_kernel(float* __restrict__ num, float* __restrict__ den,
                                                                       const float* __restrict__ d, PerturbStep s, int HW) {
  const float dn = d[blockIdx.y];
  const long long base = (long long)blockIdx.y * HW;
  perturb_for_units<RISE>(s, HW, [&](int p0, int np, const float o[4]) {
    float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 0.f, 0.f, 0.f};
    if (!OVERWRITE) {
      if (o[0] == 0.f && o[1] == 0.f && o[2] == 0.f && o[3] == 0.f) return;
      attr_load4<V>(num, base + p0, np, a);
      attr_load4<V>(den, base + p0, np, b);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (o[j] != 0.f) a[j] = at_add(a[j], at_mul(dn, o[j])), b[j] = at_add(b[j], o[j]);
    attr_store4<V>(num, base + p0, np, a);
    attr_store4<V>(den, base + p0, np, b);
  });
}

// ---- 4. the finish -------------------------------------------------------------------------------------------------------------
template <bool V>
__global__ __launch_bounds__(AT_THREADS) void perturb_finish_kernel(float* __restrict__ saliency, const float* __restrict__ num,
                                                                   const float* __restrict__ den, long long n) {
  attr_for_groups4(n, [&](long long e, int cnt) {
    float a[4], b[4], o[4];
    attr_load4<V>(num, e, cnt, a);
    attr_load4<V>(den, e, cnt, b);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = b[j] > 0.f ? a[j] / b[j] : 0.f;
    attr_store4<V>(saliency, e, cnt, o);
  });
}

// ---- the host side -------------------------------------------------------------------------------------------------------------
static int grid_positions(int size, int patch, int stride) { return patch >= size ? 1 : cdiv(size - patch, stride) + 1; }

// checks the description; fills what a step's launch needs (the patch of ``step`` for occlusion) and the grid (Gy, Gx; 0, 0 for RISE)
static int perturb_step(const char* who, const void* desc_, int64_t step, int sample0, PerturbStep* s, int* Gy, int* Gx) {
  const geeco_perturb_desc* d = static_cast<const geeco_perturb_desc*>(desc_);
  GEECO_CHECK_ARG(d, "%s: null description", who);
  GEECO_CHECK_ARG(d->method == GEECO_PERTURB_OCCLUSION || d->method == GEECO_PERTURB_RISE, "%s: method=%d", who, d->method);
  GEECO_CHECK_ARG(d->H >= 1 && d->W >= 1 && (int64_t)d->H * d->W <= (int64_t)1 << 28, "%s: H=%d, W=%d", who, d->H, d->W);
  GEECO_CHECK_ARG(step >= 0 && step <= 0x7fffffff && sample0 >= 0, "%s: step=%lld, sample0=%d must be >= 0", who, (long long)step, sample0);
  *s = PerturbStep{};
  s->H = d->H, s->W = d->W, s->step = (unsigned)step, s->sample0 = sample0;
  s->k0 = (unsigned)d->key, s->k1 = (unsigned)(d->key >> 32);
  s->g = s->ch = s->cw = 1;
  *Gy = *Gx = 0;
  if (d->method == GEECO_PERTURB_OCCLUSION) {
    GEECO_CHECK_ARG(d->ph >= 1 && d->pw >= 1 && d->sy >= 1 && d->sx >= 1, "%s: patch %d x %d, stride %d x %d must be >= 1", who, d->ph,
                    d->pw, d->sy, d->sx);
    const int ph = std::min(d->ph, d->H), pw = std::min(d->pw, d->W);      // a patch larger than the image is clipped to it
    *Gy = grid_positions(d->H, ph, d->sy), *Gx = grid_positions(d->W, pw, d->sx);
    GEECO_CHECK_ARG(step < (int64_t)*Gy * *Gx, "%s: step=%lld outside the grid of %d x %d positions", who, (long long)step, *Gy, *Gx);
    const int j = (int)(step / *Gx), i = (int)(step % *Gx);
    s->y0 = (int)std::min<int64_t>((int64_t)j * d->sy, d->H - ph), s->x0 = (int)std::min<int64_t>((int64_t)i * d->sx, d->W - pw);
    s->y1 = s->y0 + ph, s->x1 = s->x0 + pw;
  } else {
    GEECO_CHECK_ARG(d->grid >= 2 && d->grid <= 31, "%s: grid=%d outside 2..31", who, d->grid);
    GEECO_CHECK_ARG(d->keep_threshold >= 1, "%s: keep_threshold=0 keeps nothing", who);
    s->g = d->grid, s->ch = cdiv(d->H, d->grid), s->cw = cdiv(d->W, d->grid);
    s->inv_ch = 1.0f / (float)s->ch, s->inv_cw = 1.0f / (float)s->cw;
    s->threshold = d->keep_threshold;
  }
  return 0;
}

// blocks per sample: about AT_MAX_BLOCKS in all, at least one
static dim3 sample_grid(int items, int N) {
  const int per = std::max(1, AT_MAX_BLOCKS / N);
  return dim3((unsigned)std::min(cdiv(items, AT_THREADS), per), (unsigned)N);
}

extern "C" int64_t geeco_perturb_desc_sizeof(void) { return (int64_t)sizeof(geeco_perturb_desc); }

extern "C" int geeco_perturb_patch(const void* desc, int step, int32_t* out) {
  PerturbStep s;
  int Gy, Gx;
  GEECO_CHECK_ARG(out, "perturb_patch: null pointer");
  if (int rc = perturb_step("perturb_patch", desc, step, 0, &s, &Gy, &Gx)) return rc;
  out[0] = Gy, out[1] = Gx, out[2] = s.y0, out[3] = s.y1, out[4] = s.x0, out[5] = s.x1;
  return 0;
}

extern "C" int geeco_perturb_apply(float* dst, const float* x, const float* fill, int64_t fill_period, const void* desc, int step,
                                   int prev_step, int sample0, int N, int frames, int C, void* stream) {
  GEECO_CHECK_ARG(dst && x, "perturb_apply: null pointer");
  GEECO_CHECK_ARG(N >= 1 && N <= 65535 && frames >= 1 && frames <= 1 << 16, "perturb_apply: N=%d (1..65535), frames=%d", N, frames);
  GEECO_CHECK_ARG(C >= 1 && C <= 4, "perturb_apply: C=%d outside 1..4", C);
  PerturbStep s, prev;
  int Gy, Gx, pGy, pGx;
  if (int rc = perturb_step("perturb_apply", desc, step, sample0, &s, &Gy, &Gx)) return rc;
  GEECO_CHECK_ARG(prev_step >= -1, "perturb_apply: prev_step=%d (-1: the whole input)", prev_step);
  const bool rise = Gy == 0, patch = !rise && prev_step >= 0;
  if (patch)
    if (int rc = perturb_step("perturb_apply (prev_step)", desc, prev_step, sample0, &prev, &pGy, &pGx)) return rc;
  const int HW = s.H * s.W;
  const long long n = (long long)N * frames * HW * C;
  if (int rc = check_baseline("perturb_apply", fill, fill_period, n)) return rc;
  GEECO_CHECK_ARG(attr_aligned<4>(dst, x), "perturb_apply: dst and x must be 4-byte aligned");
  GEECO_CHECK_ARG(attr_apart(dst, 4 * (uintptr_t)n, x, 4 * (uintptr_t)n), "perturb_apply: dst overlaps x (the clean input is read by every step)");
  const long long period = fill ? fill_period : 1;
  hipStream_t st = (hipStream_t)stream;
  if (patch) {
    const int items = (s.y1 - s.y0) * (s.x1 - s.x0) + (prev.y1 - prev.y0) * (prev.x1 - prev.x0);
    const dim3 grid = sample_grid(items, N);
    attr_channels(C, [&](auto C_) {
      geeco_note_kernel("perturb_apply_patch_kernel<%d>", C_());
      hipLaunchKernelGGL((perturb_apply_patch_kernel<C_()>), grid, dim3(AT_THREADS), 0, st, dst, x, fill, period, s, prev.y0, prev.y1,
                         prev.x0, prev.x1, frames, HW, n);
    });
    GEECO_LAUNCH_CHECK();
    return 0;
  }
  // 16-byte accesses: every frame of every sample starts on a multiple of four floats
  const bool frames_aligned = ((long long)HW * C) % 4 == 0;
  const bool v = frames_aligned && attr_aligned<16>(dst, x);
  const int bv = frames_aligned && fill && fill_period % 4 == 0 && attr_aligned<16>(fill);
  const dim3 grid = sample_grid((HW + 3) >> 2, N);
  attr_channels(C, [&](auto C_) {
    attr_select([&](auto V, auto R) {
      geeco_note_kernel("perturb_apply_kernel<%d, %s, %s>", C_(), attr_tf(V()), attr_tf(R()));
      hipLaunchKernelGGL((perturb_apply_kernel<C_(), V(), R()>), grid, dim3(AT_THREADS), 0, st, dst, x, fill, period, bv, s, frames, HW, n);
    }, v, rise);
  });
  GEECO_LAUNCH_CHECK();
  return 0;
}

extern "C" int geeco_perturb_score(float* d, const float* preds, const float* preds0, const float* w, int N, int OT, void* stream) {
  GEECO_CHECK_ARG(d && preds && preds0 && w, "perturb_score: null pointer");
  GEECO_CHECK_ARG(N >= 1 && OT >= 1 && OT <= 1 << 16, "perturb_score: N=%d, OT=%d must be >= 1", N, OT);
  GEECO_CHECK_ARG(attr_aligned<4>(d, preds, preds0, w), "perturb_score: every pointer must be 4-byte aligned");
  geeco_note_kernel("perturb_score_kernel");
  hipLaunchKernelGGL(perturb_score_kernel, dim3((unsigned)cdiv(N, 64)), dim3(64), 0, (hipStream_t)stream, d, preds, preds0, w, N, OT);
  GEECO_LAUNCH_CHECK();
  return 0;
}

extern "C" int geeco_perturb_accumulate(float* num, float* den, const float* d, const void* desc, int step, int sample0, int N,
                                        int overwrite, void* stream) {
  GEECO_CHECK_ARG(num && den && d, "perturb_accumulate: null pointer");
  GEECO_CHECK_ARG(N >= 1 && N <= 65535, "perturb_accumulate: N=%d outside 1..65535", N);
  PerturbStep s;
  int Gy, Gx;
  if (int rc = perturb_step("perturb_accumulate", desc, step, sample0, &s, &Gy, &Gx)) return rc;
  const bool rise = Gy == 0;
  const int HW = s.H * s.W;
  GEECO_CHECK_ARG(attr_aligned<4>(num, den, d), "perturb_accumulate: every pointer must be 4-byte aligned");
  const uintptr_t bytes = 4 * (uintptr_t)N * HW, d_bytes = 4 * (uintptr_t)N;
  GEECO_CHECK_ARG(attr_apart(num, bytes, den, bytes), "perturb_accumulate: num overlaps den");
  GEECO_CHECK_ARG(attr_apart(num, bytes, d, d_bytes) && attr_apart(den, bytes, d, d_bytes), "perturb_accumulate: d overlaps num or den");
  const dim3 grid = sample_grid((HW + 3) >> 2, N);
  attr_select([&](auto V, auto R, auto O) {
    geeco_note_kernel("perturb_accumulate_kernel<%s, %s, %s>", attr_tf(V()), attr_tf(R()), attr_tf(O()));
    hipLaunchKernelGGL((perturb_accumulate_kernel<V(), R(), O()>), grid, dim3(AT_THREADS), 0, (hipStream_t)stream, num, den, d, s, HW);
  }, HW % 4 == 0 && attr_aligned<16>(num, den), rise, overwrite != 0);
  GEECO_LAUNCH_CHECK();
  return 0;
}

extern "C" int geeco_perturb_finish(float* saliency, const float* num, const float* den, int64_t n, void* stream) {
  GEECO_CHECK_ARG(saliency && num && den, "perturb_finish: null pointer");
  GEECO_CHECK_ARG(n >= 1, "perturb_finish: n=%lld must be >= 1", (long long)n);
  GEECO_CHECK_ARG(attr_aligned<4>(saliency, num, den), "perturb_finish: every pointer must be 4-byte aligned");
  const uintptr_t bytes = 4 * (uintptr_t)n;
  GEECO_CHECK_ARG(attr_apart(saliency, bytes, num, bytes) && attr_apart(saliency, bytes, den, bytes), "perturb_finish: saliency overlaps num or den");
  const unsigned grid = attr_grid((n + 3) >> 2);
  attr_select([&](auto V) {
    geeco_note_kernel("perturb_finish_kernel<%s>", attr_tf(V()));
    hipLaunchKernelGGL(perturb_finish_kernel<V()>, dim3(grid), dim3(AT_THREADS), 0, (hipStream_t)stream, saliency, num, den, (long long)n);
  }, attr_aligned<16>(saliency, num, den));
  GEECO_LAUNCH_CHECK();
  return 0;
}
