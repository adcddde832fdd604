// What more than one of the dynamic-image files uses: dynimg.hip (the plain dynamic image), dynimg_goal.hip (the goal model's
// one-pass input stage) and predict_io.hip (which takes the window-length bound from here).
#pragma once
#include "geeco_common.h"

#define DYN_MAXK 64

struct DynParams {
  const float* frames;
  const float* frames2;
  const float* depth;      // optional 4th channel kept in its own tensor ([N][K][HW] / [N][HW]): RGB-D without packing
  const float* depth2;
  long long dsample_stride, dframe_stride;
  long long sample_stride, frame_stride;
  int N, K;
  long long HW;
  int C, Cpad;
  float* out;
  float* last;   // optional [N][HW][4]: the LAST frame of the stack channel-padded (conv1's input of the current frame)
  float* part;   // [N][nblk][2]
  int nblk;
  float alpha[DYN_MAXK];
  // DIFF (geeco_goal_dynimgs_fwd): the pair image alpha2[0] * last frame + alpha2[1] * target (graph.py:397-400) from the same pass:
  // the last frame is in registers anyway, so the pair image costs one read of the target instead of a launch that reads both
  const float* tgt;       // [N][HW][3]
  const float* tgt_depth; // [N][HW] (DEPTH)
  float* diff_out;        // [N][HW][4]
  float* part2;           // [N][nblk][2]
  float alpha2[2];
  // U8 (geeco_goal_dynimgs_u8_fwd): the RGB frames are the recorder's uint8 values, still in the episode's resident frames:
  // win[n] = address of the first frame of window n ([K][HW][3] bytes, consecutive frames), tgt_u8[n] = its target frame
  const unsigned char* const* win;
  const unsigned char* const* tgt_u8;
};

__device__ __forceinline__ const float* dyn_frame_ptr(const DynParams& p, int n, int t) {
  if (p.frames2 && t == 1) return p.frames2 + (long long)n * p.HW * p.C;
  return p.frames + (long long)n * p.sample_stride + (long long)t * p.frame_stride;
}

__device__ __forceinline__ void block_minmax_store(float mn, float mx, float* dst) {
  __shared__ float smn[4], smx[4];
  mn = wave_reduce_min(mn);
  mx = wave_reduce_max(mx);
  const int wid = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    smn[wid] = mn;
    smx[wid] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    dst[0] = fminf(fminf(smn[0], smn[1]), fminf(smn[2], smn[3]));
    dst[1] = fmaxf(fmaxf(smx[0], smx[1]), fmaxf(smx[2], smx[3]));
  }
}
