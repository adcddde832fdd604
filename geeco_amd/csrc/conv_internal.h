// Internal (non-ABI) functions the conv files call across translation units.  The file that defines one and every file that
// calls it include this header, so a signature that drifts is a compile error instead of a link error.
//
// geeco_try_*: launch the layer if the file's kernels serve the shape.  Returns 0 or an error code; *handled = 1 if it
// was launched, 0 if the shape is not covered (the caller goes on to the next kernel family).
// geeco_*_handles: would geeco_try_* take the shape?  (Forward and input gradient: conv_halo_plan.h, plain C++ that the host tests
// evaluate.)  geeco_*_ws_bytes: slab workspace it needs (0: shape not covered).
#pragma once
#include "geeco_common.h"
#include "conv_halo_plan.h"

// conv_halo_conv1.hip
int geeco_try_conv1_fwd(const float* x, const float* w, const float* b, float* y, int groups, int64_t gs_x,
                        int64_t gs_w, int64_t gs_b, int64_t gs_y, int N, int H, int W, int Cin, int Cout, int stride,
                        int relu, hipStream_t stream, int* handled);
int64_t geeco_conv1_wgrad_ws_bytes(int groups, int Cin, int Cout, int stride);
int geeco_try_conv1_wgrad(const float* x, const float* dz, float* dw, float* db, int groups, int64_t gs_x,
                          int64_t gs_dz, int64_t gs_dw, int64_t gs_db, int N, int H, int W, int Cin, int Cout,
                          int stride, void* ws, hipStream_t stream, int* handled);

// conv_halo_s2_fwd.hip
int geeco_try_halo_fwd(const float* x, const float* w, const float* b, float* y, int groups, int64_t gs_x,
                       int64_t gs_w, int64_t gs_b, int64_t gs_y, int N, int H, int W, int Cin, int Cout, int stride,
                       int relu, hipStream_t stream, int* handled);

// conv_halo_s2_bwd.hip
int64_t geeco_halo_wgrad_ws_bytes(int groups, int N, int H, int W, int Cin, int Cout, int stride);
int geeco_try_halo_wgrad(const float* x, const float* dz, float* dw, float* db, int groups, int64_t gs_x,
                         int64_t gs_dz, int64_t gs_dw, int64_t gs_db, int N, int H, int W, int Cin, int Cout,
                         int stride, void* ws, hipStream_t stream, int* handled);
int geeco_try_halo_dgrad(const float* dz, const float* w_hwio, const float* ymask, float* dx, int groups,
                         int64_t gs_dz, int64_t gs_w, int64_t gs_dx, int N, int H, int W, int Cin, int Cout,
                         int stride, hipStream_t stream, int* handled);

// conv_wgrad_halo.hip
int64_t geeco_wgrad_lds_ws_bytes(int groups, int N, int H, int W, int Cin, int Cout, int stride);
int geeco_try_wgrad_lds(const float* x, const float* dz, float* dw, float* db, int groups, int64_t gs_x, int64_t gs_dz,
                        int64_t gs_dw, int64_t gs_db, int N, int H, int W, int Cin, int Cout, int stride, void* ws,
                        hipStream_t stream, int* handled);

// conv_dgrad_lds.hip
int geeco_try_dgrad_lds(const float* dz, const float* w_hwio, const float* ymask, float* dx, int groups, int64_t gs_dz,
                        int64_t gs_w, int64_t gs_dx, int N, int H, int W, int Cin, int Cout, int stride,
                        hipStream_t stream, int* handled);

// conv_wgrad.hip: sums the S slabs of every group in a fixed order into dw / db (or records the sum: geeco_set_pending_reduce)
void geeco_launch_wgrad_reduce(const float* part, float* dw, float* db, long long gs_dw, long long gs_db, int S,
                               long long KC, int Cout, int groups, hipStream_t s);
