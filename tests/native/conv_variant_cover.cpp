// Which launch variants of the gather GEMM (geeco_amd/csrc/conv_gemm.hip) the cases of conv_gemm_cases.txt run, and which ones
// the model reaches.  A variant key is everything that selects code in a launch:
//   dir, BM x BN (the tile instantiation), ut (uniform tap: C % 16 == 0), split (S > 1: slabs + the slab-sum launch), ncls (parity
//   classes), rot0 (rot == 0: no class rotation), uneqM (classes of unequal row counts), ragged (a class whose rows do not fill
//   its last M tile).
// Output, read by tests/test_conv_cover_cpu.py:
//   (a) "case <the case's fields and flags> | <key> S=<factor the launch runs> planS=<factor the plan asks for>" per case of the
//       list (argv[1]); S is 1 where the case gives no workspace (launch_conv_gemm's ksplit = 1 fallback);
//   (b) "sweep <key>" once per key, and "sweepS <factor>" once per split factor, of the eight encoder layers, forward for
//       N = 1..512 and input gradient for N = 1..96, at inputs 136 / 144 / 256 with 1..3 encoders.
// The sweep treats every layer as the gather GEMM's.  That is a superset of what the family order of conv_gemm.hip lets through
// (the LDS-halo, conv1 and LDS-staged kernels take some of these layers first), so this program need not copy the *_handles
// predicates out of the .hip files; the only layers left out are those the entry points reject (conv1's input gradient:
// Cin = 4 is not a multiple of 16, and the model never asks for it).
// A host program (tests/native/conv_plan_table.cpp's style): built with -fsanitize=address,undefined, never loaded into Python.
#include <stdio.h>
#include <string.h>
#include <set>
#include <string>
#include "conv_gemm_plan.h"

static const int kFilters[8] = {32, 48, 64, 128, 192, 256, 256, 256};
static const int kStrides[8] = {1, 2, 2, 2, 2, 2, 2, 2};
static float g_operand[4];     // the operands are only compared with NULL

struct Variant {
  std::string key;
  int plan_s;
};

// what launch_conv_gemm does between the problem and the launch
static Variant variant_of(bool fwd, int G, int N, int H, int W, int Cin, int Cout, int s, bool ws) {
  ConvGemmParams p = {};
  if (fwd)
    conv_fwd_problem(&p, g_operand, g_operand, g_operand, g_operand, 1, 1, 1, 1, N, H, W, Cin, Cout, s, 1);
  else
    conv_dgrad_problem(&p, g_operand, g_operand, g_operand, g_operand, g_operand, 1, 1, 1, 1, N, H, W, Cin, Cout, s);
  const ConvPlan pl = conv_plan(p, G);
  p.ksplit = ws ? pl.ksplit : 1;
  p.groups = G;
  const ConvGemmGrid gr = conv_gemm_grid(p, pl.bm, pl.bn, G);
  bool uneq = false, ragged = false;
  for (int c = 0; c < p.ncls; ++c) {
    uneq = uneq || p.cls[c].M != p.cls[0].M;
    ragged = ragged || p.cls[c].M % pl.bm != 0;
  }
  char buf[160];
  snprintf(buf, sizeof buf, "%s %dx%d ut=%d split=%d ncls=%d rot0=%d uneqM=%d ragged=%d", fwd ? "fwd" : "dgrad", pl.bm, pl.bn,
           (int)gr.ut, p.ksplit > 1, p.ncls, p.rot == 0, (int)uneq, (int)ragged);
  return Variant{buf, pl.ksplit};
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: conv_variant_cover conv_gemm_cases.txt\n");
    return 2;
  }
  FILE* f = fopen(argv[1], "r");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  char line[512];
  while (fgets(line, sizeof line, f)) {
    char* bar = strchr(line, '|');
    if (line[0] == '#' || line[0] == '\n' || !bar) continue;
    *bar = 0;
    size_t n = strlen(line);
    while (n && (line[n - 1] == ' ' || line[n - 1] == '\t')) line[--n] = 0;
    char fields[512];
    strcpy(fields, line);      // strtok below cuts the flags apart
    char dir[16];
    int G, N, H, W, Cin, Cout, s, used = 0;
    if (sscanf(line, "%15s %d %d %d %d %d %d %d%n", dir, &G, &N, &H, &W, &Cin, &Cout, &s, &used) != 8 ||
        (strcmp(dir, "fwd") != 0 && strcmp(dir, "dgrad") != 0)) {
      fprintf(stderr, "bad case line: %s\n", line);
      return 2;
    }
    bool ws = false;
    for (char* tok = strtok(line + used, " \t\n"); tok; tok = strtok(nullptr, " \t\n")) ws = ws || strcmp(tok, "ws") == 0;
    const Variant v = variant_of(strcmp(dir, "fwd") == 0, G, N, H, W, Cin, Cout, s, ws);
    printf("case %s | %s S=%d planS=%d\n", fields, v.key.c_str(), ws ? v.plan_s : 1, v.plan_s);
  }
  fclose(f);

  std::set<std::string> keys;
  std::set<int> factors;
  const int inputs[3] = {136, 144, 256};
  for (int in : inputs)
    for (int G = 1; G <= 3; ++G)
      for (int N = 1; N <= 512; ++N) {
        int H = in, W = in, Cin = 4;
        for (int l = 0; l < 8; ++l) {
          const int Cout = kFilters[l], s = kStrides[l];
          Variant v = variant_of(true, G, N, H, W, Cin, Cout, s, true);
          keys.insert(v.key);
          if (v.plan_s > 1) factors.insert(v.plan_s);
          if (N <= 96 && Cin % 16 == 0) {
            v = variant_of(false, G, N, H, W, Cin, Cout, s, true);
            keys.insert(v.key);
            if (v.plan_s > 1) factors.insert(v.plan_s);
          }
          int pad;
          same_pad(H, 3, s, &H, &pad);
          same_pad(W, 3, s, &W, &pad);
          Cin = Cout;
        }
      }
  for (const std::string& k : keys) printf("sweep %s\n", k.c_str());
  for (int s : factors) printf("sweepS %d\n", s);
  return 0;
}
