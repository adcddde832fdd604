// Opt-in learning-rate schedules evaluated on the device from the step counter: geeco_adam_prepare under a schedule,
// and the same function on the host.  The arithmetic is lr_schedule.h's; the slab-sum launch that carries the prepare work under a
// schedule is in conv_wgrad.hip.
#include "lr_schedule.h"

// adam_prepare_kernel (misc.hip) with lr(s) of the schedule in place of the constant; scal[2] = lr(s).
__global__ void adam_prepare_schedule_kernel(long long* step, const geeco_lr_schedule sc, float b1, float b2, float* scal) {
  if (threadIdx.x == 0 && blockIdx.x == 0) adam_prepare_schedule_step(step, sc, b1, b2, scal);
}

extern "C" int geeco_adam_prepare_schedule(int64_t* global_step_dev, const geeco_lr_schedule* schedule, float beta1, float beta2,
                                           float* scal_dev, void* stream) {
  GEECO_CHECK_ARG(global_step_dev && scal_dev, "adam_prepare_schedule: null pointer");
  if (int rc = check_lr_schedule("adam_prepare_schedule", schedule)) return rc;
  hipLaunchKernelGGL(adam_prepare_schedule_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (long long*)global_step_dev, *schedule,
                     beta1, beta2, scal_dev);
  GEECO_LAUNCH_CHECK();
  return 0;
}

extern "C" int geeco_lr_schedule_eval(const geeco_lr_schedule* schedule, int64_t step, double* lr_out) {
  GEECO_CHECK_ARG(lr_out, "lr_schedule_eval: null pointer");
  if (int rc = check_lr_schedule("lr_schedule_eval", schedule)) return rc;
  GEECO_CHECK_ARG(step >= 0, "lr_schedule_eval: step=%lld is negative", (long long)step);
  *lr_out = lr_schedule_at(*schedule, (long long)step);
  return 0;
}
