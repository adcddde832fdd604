// Prints every field that determines a gather-GEMM launch (geeco_amd/csrc/conv_gemm_plan.h) for a fixed sweep of shapes: the
// eight encoder layers, forward and input gradient, at 136 x 136, 256 x 256 and 135 x 135 inputs, 1..3 encoders, 1 / 5 / 32 / 96
// frames.  tests/test_conv_plan_cpu.py builds it with -fsanitize=address,undefined and compares the output byte for byte with
// conv_plan_table.txt, which was recorded from the planning code of the commit before the header existed (moved, not yet
// deduplicated: profiles/conv_gemm_split/README.md).  A host program: it needs no GPU and is not loaded into Python.
#include <stdio.h>
#include "conv_gemm_plan.h"

static const int kFilters[8] = {32, 48, 64, 128, 192, 256, 256, 256};
static const int kStrides[8] = {1, 2, 2, 2, 2, 2, 2, 2};
static float g_operand[4];     // the operands are only compared with NULL

static void print_classes(const ConvGemmParams& p) {
  printf(" ncls=%d", p.ncls);
  for (int c = 0; c < p.ncls; ++c) printf(" [M=%lld ntaps=%d tile0=%d]", p.cls[c].M, p.cls[c].ntaps, p.cls[c].tile0);
}

// what launch_conv_gemm does between the problem and the launch (the workspace is given whenever the plan asks for one)
static void print_launch(ConvGemmParams& p, int groups) {
  const ConvPlan pl = conv_plan(p, groups);
  p.ksplit = pl.ksplit; p.groups = groups;
  const ConvGemmGrid gr = conv_gemm_grid(p, pl.bm, pl.bn, groups);
  printf(" bm=%d bn=%d ksplit=%d ws=%lld", pl.bm, pl.bn, pl.ksplit, (long long)conv_ws_bytes(p, groups));
  print_classes(p);
  printf(" rot=%d grid=%dx%dx%d ut=%d bt=%d rows_ok=%d", p.rot, gr.gx, gr.gy, gr.gz, (int)gr.ut, p.bt, conv_rows_beyond_32bit(p) == 0);
}

int main() {
  const int inputs[3] = {136, 256, 135}, frames[4] = {1, 5, 32, 96};
  for (int in : inputs)
    for (int G = 1; G <= 3; ++G)
      for (int N : frames) {
        int H = in, W = in, Cin = 4;
        for (int l = 0; l < 8; ++l) {
          const int Cout = kFilters[l], s = kStrides[l];
          printf("fwd in=%d G=%d N=%d conv%d %dx%dx%d->%d s%d:", in, G, N, l + 1, H, W, Cin, Cout, s);
          ConvGemmParams f = {};
          conv_fwd_problem(&f, g_operand, g_operand, g_operand, g_operand, 1, 1, 1, 1, N, H, W, Cin, Cout, s, 1);
          print_launch(f, G);
          printf("\ndgrad in=%d G=%d N=%d conv%d %dx%dx%d->%d s%d:", in, G, N, l + 1, H, W, Cin, Cout, s);
          ConvGemmParams d = {};
          conv_dgrad_problem(&d, g_operand, g_operand, nullptr, g_operand, g_operand, 1, 1, 0, 1, N, H, W, Cin, Cout, s);
          printf(" w=%d", d.w != nullptr);
          print_launch(d, G);
          // the top-of-the-backward form (geeco_conv_top_bwd): the same problem as a range of block indices of one 1-D grid
          ConvGemmParams t = {};
          conv_dgrad_problem(&t, g_operand, g_operand, nullptr, g_operand, g_operand, 1, 1, 0, 1, N, H, W, Cin, Cout, s);
          const ConvPlan pl = conv_plan(t, G);
          if (s == 2 && t.w && t.ncls && pl.bm == 64 && pl.bn == 64) {
            t.ksplit = pl.ksplit; t.groups = G;
            const ConvGemmGrid gr = conv_gemm_grid(t, 64, 64, G);
            printf(" top: gx=%d gy=%d blocks=%lld ut=%d rot=%d", gr.gx, gr.gy, (long long)gr.gx * gr.gy * gr.gz, (int)gr.ut, t.rot);
            for (int c = 0; c < t.ncls; ++c) printf(" tile0=%d", t.cls[c].tile0);
          }
          printf("\n");
          int pad;
          same_pad(H, 3, s, &H, &pad);
          same_pad(W, 3, s, &W, &pad);
          Cin = Cout;
        }
      }
  return 0;
}
