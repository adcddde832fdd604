// The learning-rate schedules (geeco_lr_schedule): lr as a function of the number of completed updates s, in double,
// from the parameters as the device holds them.  One home for the arithmetic: the two kernels that do the optimiser's prepare work
// under a schedule (adam_prepare_schedule_kernel, lr_schedule.hip; wgrad_reduce_batch_schedule_kernel, conv_wgrad.hip) and the host
// entry point geeco_lr_schedule_eval all call lr_schedule_at; the host checks every entry point makes are here too.
#pragma once
#include <math.h>

#include "geeco_common.h"

// lr(s), s >= 0 the updates completed before this one (TF 1.15's global_step as tf.train.*_decay sees it).  The schedule may be a
// by-value kernel argument: it is read with static indices only (the piecewise lookup is eight unrolled selects; a dynamic index
// would copy the struct to scratch).
__host__ __device__ __forceinline__ double lr_schedule_at(const geeco_lr_schedule& sc, long long s) {
  const long long w = sc.warmup_steps;
  const bool piecewise = sc.kind == GEECO_LR_PIECEWISE;
  if (s < w)      // linear warm-up to the schedule's value at its own step 0; the fraction first: the last step (s = w - 1) is that value exactly
    return (double)(piecewise ? sc.values[0] : sc.base_lr) * ((double)(s + 1) / (double)w);
  const long long u = s - w;
  const double base = (double)sc.base_lr;
  if (piecewise) {
    // values[i] for the first i with u <= boundaries[i], else values[n]: boundaries increase strictly, so the last i with
    // u > boundaries[i] names it
    float v = sc.values[0];
#pragma unroll
    for (int i = 0; i < GEECO_LR_BOUNDARIES_MAX; ++i)
      if (i < sc.n_boundaries && u > sc.boundaries[i]) v = sc.values[i + 1];
    return (double)v;
  }
  if (sc.kind == GEECO_LR_EXPONENTIAL) {
    const long long ds = sc.decay_steps;
    const double e = sc.staircase ? (double)(u / ds) : (double)u / (double)ds;
    return base * pow((double)sc.decay_rate, e);
  }
  if (sc.kind == GEECO_LR_COSINE) {
    const long long ds = sc.decay_steps;
    const double a = (double)sc.alpha;
    return base * ((1.0 - a) * 0.5 * (1.0 + cos(3.14159265358979323846 * (double)(u < ds ? u : ds) / (double)ds)) + a);
  }
  return base;      // GEECO_LR_CONSTANT
}

// tf.train.AdamOptimizer's lr_t for the counter t after the increment, as adam_prepare_kernel (misc.hip) forms it from a constant
__host__ __device__ __forceinline__ float adam_lr_t(double lr, float b1, float b2, long long t) {
  const double b1t = pow((double)b1, (double)t), b2t = pow((double)b2, (double)t);
  return (float)(lr * sqrt(1.0 - b2t) / (1.0 - b1t));
}

// The prepare work of one step under a schedule, by the one thread that does it: advances the counter, scal[0] = lr_t,
// scal[2] = lr(s) (scal[1] is the arena's sum of squares and is left alone).
__device__ __forceinline__ void adam_prepare_schedule_step(long long* step, const geeco_lr_schedule& sc, float b1, float b2, float* scal) {
  const long long t = *step + 1;
  *step = t;
  const double lr = lr_schedule_at(sc, t - 1);
  scal[0] = adam_lr_t(lr, b1, b2, t);
  scal[2] = (float)lr;
}

static inline bool lr_rate_ok(float x) { return x >= 0.f && x <= 3.402823466e38f; }      // finite and not negative (false for NaN)

// the argument checks of every entry point that takes a schedule, before any launch
static int check_lr_schedule(const char* what, const geeco_lr_schedule* sc) {
  GEECO_CHECK_ARG(sc, "%s: null pointer (schedule)", what);
  GEECO_CHECK_ARG(sc->kind == GEECO_LR_CONSTANT || sc->kind == GEECO_LR_EXPONENTIAL || sc->kind == GEECO_LR_COSINE ||
                      sc->kind == GEECO_LR_PIECEWISE,
                  "%s: unknown kind %d of schedule (0 constant, 1 exponential, 2 cosine, 3 piecewise)", what, sc->kind);
  GEECO_CHECK_ARG(sc->warmup_steps >= 0, "%s: warmup_steps=%lld is negative", what, (long long)sc->warmup_steps);
  if (sc->kind == GEECO_LR_PIECEWISE) {
    GEECO_CHECK_ARG(sc->n_boundaries >= 0 && sc->n_boundaries <= GEECO_LR_BOUNDARIES_MAX, "%s: n_boundaries=%d outside 0..%d", what,
                    sc->n_boundaries, GEECO_LR_BOUNDARIES_MAX);
    for (int i = 1; i < sc->n_boundaries; ++i)
      GEECO_CHECK_ARG(sc->boundaries[i] > sc->boundaries[i - 1], "%s: boundaries[%d]=%lld is not above boundaries[%d]=%lld (strictly increasing)",
                      what, i, (long long)sc->boundaries[i], i - 1, (long long)sc->boundaries[i - 1]);
    for (int i = 0; i <= sc->n_boundaries; ++i)
      GEECO_CHECK_ARG(lr_rate_ok(sc->values[i]), "%s: values[%d]=%g is not a finite number >= 0", what, i, (double)sc->values[i]);
    return 0;
  }
  GEECO_CHECK_ARG(lr_rate_ok(sc->base_lr), "%s: base_lr=%g is not a finite number >= 0", what, (double)sc->base_lr);
  if (sc->kind == GEECO_LR_EXPONENTIAL || sc->kind == GEECO_LR_COSINE)
    GEECO_CHECK_ARG(sc->decay_steps >= 1, "%s: decay_steps=%lld is below 1", what, (long long)sc->decay_steps);
  if (sc->kind == GEECO_LR_EXPONENTIAL)
    GEECO_CHECK_ARG(lr_rate_ok(sc->decay_rate) && sc->decay_rate > 0.f, "%s: decay_rate=%g is not a finite number > 0", what,
                    (double)sc->decay_rate);
  if (sc->kind == GEECO_LR_COSINE)
    GEECO_CHECK_ARG(sc->alpha >= 0.f && sc->alpha <= 1.f, "%s: alpha=%g is outside [0, 1]", what, (double)sc->alpha);
  return 0;
}
