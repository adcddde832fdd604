// Shared by the LDS-halo kernel files (conv_halo_*.hip, conv_wgrad_halo.hip, conv_dgrad_lds.hip): barriers, LDS-DMA pointer
// types and zero page, streaming stores, the dev stamp macro, and the slicing of the persistent encoder-bottom kernels.
//
// The conv_halo_*.hip files hold the LDS-halo kernels for the two big-spatial / small-channel layers of the encoder:
//   conv1: 3x3, stride 1,  4 -> 32 channels (RGB padded to 4)     graph.py:76-80
//   conv2: 3x3, stride 2, 32 -> 48 channels                        graph.py:81-85
// (reference src/models/e2evmc/graph.py; backward = autodiff via estimator.py:243-244).
//
// Why a second kernel family: at Cout = 32/48 the gather-GEMM of conv_gemm.hip moves
// 9*Cin*4 bytes of gathered input per output pixel for 2*9*Cin*Cout FLOP = Cout/2 FLOP per byte
// (24 FLOP/B for conv2): the L1/TA load path, not the MFMA pipe, sets its speed (PMC: 55 % MFMA
// busy, 1.6-3x HBM over-fetch).  Here a block stages the input HALO of its output tile in LDS once
// and every tap reads its fragments from there (2.25x fewer bytes for stride 2, 9x for stride 1),
// the kernel weights stay resident in LDS for the block's lifetime (persistent blocks walk the
// tiles), and the next tile's halo is fetched behind the current tile's MFMAs (conv2 forward:
// straight into LDS by LDS-DMA; the gradient kernels: through registers).
//
// MFMA: v_mfma_f32_16x16x4_f32, roles as in conv_gemm.hip (row i = output channel, column j =
// pixel) so every lane owns 4 consecutive NHWC channels of one pixel.
#pragma once
#include "geeco_common.h"
#include "conv_wgrad_plan.h"

// Workgroup barrier that waits for this wave's LDS traffic only.  __syncthreads() also drains the
// vector-memory counter (vmcnt(0)), which would expose the latency of the epilogue's global stores
// and of the next tile's prefetch loads once per tile (cdna_hip_programming.md, "Pipelining across
// barriers").  The "memory" clobber keeps the compiler from moving LDS accesses across it.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Barrier that also retires this wave's LDS-DMA (global_load_lds) writes before anyone reads them.
__device__ __forceinline__ void dma_barrier() { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// s_waitcnt vmcnt(N): at most N of this wave's vector-memory operations (LDS-DMA pieces) stay in flight
template <int N>
__device__ __forceinline__ void wait_vm_imm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

typedef __attribute__((address_space(1))) const void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

// g_zero_page: source of the LDS-DMA lanes that fall outside the image (TF SAME zero padding).  Every translation unit has
// its own (without relocatable device code two files cannot share a __device__ variable).  The compiler addresses a static
// page and an externally visible one with different instructions; the conv_halo_*.hip kernels were measured with the
// external form, so those files name their page before they include this header (#define GEECO_ZERO_PAGE
// g_zero_page_<file>: distinct symbols at link time).
#ifdef GEECO_ZERO_PAGE
__device__ float GEECO_ZERO_PAGE[64];
#define g_zero_page GEECO_ZERO_PAGE
#else
[[maybe_unused]] static __device__ float g_zero_page[64];
#endif

// Output stores of the big layers.  Bit SITE of GEECO_NT selects a non-temporal store (the tensor is far larger than the
// caches and streams to HBM: measured on conv1's 805 MB output, 207 -> 190 us); sites: 0 conv1 fwd, 1 conv2 fwd,
// 2 conv3 fwd, 3 conv3 dgrad.
#ifndef GEECO_NT
#define GEECO_NT 1
#endif
template <int SITE>
__device__ __forceinline__ void stream_store(float* dst, const f32x4& v) {
  if constexpr ((GEECO_NT >> SITE) & 1)
    __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(dst));
  else
    *reinterpret_cast<f32x4*>(dst) = v;
}

// Dev instrumentation (-DGEECO_STAMPS builds only, scripts/dev/*stamps.py): in-kernel s_memtime timelines, [row][2 waves][64]
// per launch: wave 0 and wave 4 of a block write stamp i of `row` (a block or slice index; negative: no stamp).  The launchers
// arm p.stamps with geeco_arm_halo_stamps() (buffer and geeco_debug_dump_halo_stamps: conv_halo_s2_fwd.hip).
#ifdef GEECO_STAMPS
unsigned long long* geeco_arm_halo_stamps();
#define HALO_STAMP(row, i)                                                                               \
  do {                                                                                                   \
    const long long row_ = (row);                                                                        \
    if (lane == 0 && wid < 8 && (wid & 3) == 0 && row_ >= 0 && p.stamps && (i) < 64)                     \
      p.stamps[(row_ * 2 + (wid >> 2)) * 64 + (i)] = __builtin_amdgcn_s_memtime();                       \
  } while (0)
#else
static inline unsigned long long* geeco_arm_halo_stamps() { return nullptr; }
#define HALO_STAMP(row, i)
#endif

// Persistent one-block-per-CU kernels of the encoder bottom (conv2's filter gradient, the fused conv2-dgrad + conv1-wgrad):
// slices per encoder.  The entry points' `reserved_cus` argument k leaves k CUs free for a collective that runs beside them (data parallel:
// the early gradient bucket is reduced while these two kernels run; a grid that occupies every CU would make the
// collective's workgroups wait for - or delay - the persistent blocks).  The workspace is sized for k = 0.
// conv_wgrad_plan.h holds the slicing itself (BottomSlices, bottom_slices_on: plain C++ that the host tests evaluate); here only
// the CU count of the call being served.
static BottomSlices bottom_slices(int groups, long long T, bool for_ws = false) {
  return bottom_slices_on(WGRAD_CUS - (for_ws ? 0 : geeco_call_reserved_cus()), groups, T, for_ws);
}

// tile grid of one encoder and its slicing over the persistent blocks (HaloWgradParams; the fused bottom takes its own from
// fused_bottom_launch_plan)
template <class P>
static BottomSlices fill_bottom_geometry(P& p, int groups, int N, int H, int W, int tiles_x, int tiles_y) {
  p.N = N; p.H = H; p.W = W; p.Ho = H / 2; p.Wo = W / 2;
  p.tiles_x = tiles_x; p.tiles_y = tiles_y;
  p.tiles_per_group = N * tiles_x * tiles_y;
  const BottomSlices bs = bottom_slices(groups, p.tiles_per_group);
  p.S = bs.S; p.S0 = bs.S0; p.per = bs.per; p.groups = groups;
  return bs;
}
