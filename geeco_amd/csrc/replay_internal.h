// What both episode-replay files use: replay.hip (the window states of every replay class, the errors) and replay_dynimg.hip (the
// image stage of the dynamic-image controllers).
#pragma once
#include "dynimg_internal.h"      // DYN_MAXK

#define RP_THREADS 256
#define RP_MAXK DYN_MAXK          // the window lengths the predictors take
#define RP_MAX_BLOCKS 2048        // 8 blocks of 256 threads per CU: the grid-stride loops take the rest

// the window arguments every entry point over an episode takes: K steps, the windows [t0, t1) of T frames, N rows per step
static int check_replay_windows(const char* what, int T, int t0, int t1, int N, int K) {
  GEECO_CHECK_ARG(K >= 1 && K <= RP_MAXK, "%s: K=%d outside 1..%d", what, K, RP_MAXK);
  GEECO_CHECK_ARG(T >= 1 && t0 >= 0 && t0 < t1 && t1 <= T, "%s: windows [%d, %d) outside the %d frames", what, t0, t1, T);
  GEECO_CHECK_ARG(N >= t1 - t0, "%s: N=%d rows per step for %d windows", what, N, t1 - t0);
  return 0;
}
