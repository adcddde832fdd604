// The decoder-state columns of the three window modes (GEECO_PREDICT_FEAT_*), per cell:
//   PLAIN [feat | jnt],  CONSTANT [feat | jnt | tgt],  RESIDUAL [tgt - feat | jnt]
// with feat / tgt of ch columns and jnt of J.  One home for the layout and for the argument checks of the kernels that write or
// read such rows: push_features_kernel (predict_io.hip), window_states_fwd_kernel and window_states_bwd_kernel
// (shared_frames.hip).  A header of its own rather than a section of decoder_internal.h: none of its users is a decoder file, and
// the decoder's own concat (fill_concat, decoder_concat.hip) is the general nfeat / jnt_pos form these modes are special cases of.
// The per-unit store and the joint-state tiling stay written out in the two forward kernels, with their columns from here: as
// shared inline functions they gave other device code (profiles/ingest_one_copy/README.md), which nobody has timed.
#pragma once
#include "geeco_common.h"

// I = int in the kernels, int64_t in the host checks (where ch + J + ch is formed before anything bounds J)
template <typename I>
struct StateLayout {
  I Ctot;            // columns of one cell
  I jnt_off;         // first joint-state column of a cell
  I tgt_off;         // where the target's features go relative to the frame's: behind jnt (CONSTANT), onto them (RESIDUAL)
  float feat_sign;   // d(state) / d(frame feature): -1 in RESIDUAL (the state holds tgt - feat)
};

template <typename I>
__host__ __device__ __forceinline__ StateLayout<I> state_layout(int mode, I ch, I J) {
  return {ch + J + (mode == GEECO_PREDICT_FEAT_CONSTANT ? ch : 0), ch, mode == GEECO_PREDICT_FEAT_CONSTANT ? ch + J : 0,
          mode == GEECO_PREDICT_FEAT_RESIDUAL ? -1.f : 1.f};
}

// the argument checks every entry point over such rows makes
static int check_state_layout(const char* what, int mode, int cells, int ch, int J, int64_t state_stride) {
  GEECO_CHECK_ARG(mode == GEECO_PREDICT_FEAT_PLAIN || mode == GEECO_PREDICT_FEAT_CONSTANT || mode == GEECO_PREDICT_FEAT_RESIDUAL,
                  "%s: mode=%d must be 0 (plain), 1 (constant) or 2 (residual)", what, mode);
  GEECO_CHECK_ARG(cells >= 1 && ch >= 1 && J >= 1 && (int64_t)cells * ch <= (1 << 24), "%s: cells=%d ch=%d J=%d", what, cells, ch, J);
  const int64_t Ctot = state_layout<int64_t>(mode, ch, J).Ctot;
  GEECO_CHECK_ARG(state_stride >= cells * Ctot, "%s: state_stride=%lld below cells * %lld columns", what, (long long)state_stride,
                  (long long)Ctot);
  return 0;
}
