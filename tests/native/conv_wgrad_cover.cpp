// Which launch variants of the filter gradient (geeco_conv3x3_wgrad: geeco_amd/csrc/conv_wgrad_plan.h) the cases of
// conv_wgrad_cases.txt run, and which ones the models reach.  A launch is described by
//   family (halo / conv1 / lds / generic, the dispatcher's order), the kernel instantiation as geeco_note_kernel names it,
//   S (slabs per group), reduce (the slab-sum kernel behind it: split / plain / none), slice_px (the most output pixels one
//   slice accumulates), remainder (the halo kernel's remainder-block form).
// and its key is (family, instantiation, reduce, S == 1 or S > 1, regular or remainder-block form).
// Output, read by tests/test_conv_wgrad_cover_cpu.py:
//   (a) "case <the case's fields and flags> | <family> <instantiation> S=.. reduce=.. slice_px=.. [remainder] [unreached]" per
//       case of the list (argv[1]); unreached: no shape of the sweep runs the case's instantiation;
//   (b) "sweep <key>" once per key of the sweep: the eight encoder layers at inputs 136 / 144 / 256 with 1..3 encoders and
//       1..512 frames, every layer taken as EACH family that can serve its shape would serve it (the dispatcher's own choice and
//       the families behind it in the order: a superset of what the order lets through, so a change of one family's
//       predicate cannot silently hand a layer to a variant without a case);
//   (c) "inst <instantiation>" once per instantiation the dispatcher can choose at all: the six LDS variants, the four generic
//       tiles, conv1's kernel, the halo kernel, both slab-sum kernels.
// A host program (tests/native/conv_variant_cover.cpp's style): built with -fsanitize=address,undefined, never loaded into Python.
#include <stdio.h>
#include <string.h>
#include <set>
#include <string>
#include "conv_wgrad_plan.h"

static const int kFilters[8] = {32, 48, 64, 128, 192, 256, 256, 256};
static const int kStrides[8] = {1, 2, 2, 2, 2, 2, 2, 2};
static const char* kFamily[4] = {"halo", "conv1", "lds", "generic"};

// the names the launchers note (conv_wgrad_halo.hip: launch_wgrad_lds's template arguments per variant; conv_wgrad.hip's switch);
// tests/test_conv_wgrad_variants_gpu.py holds them against the trace of the launches
static std::string lds_name(int variant) {
  switch (variant) {
    case 1: return "conv_s2_wgrad_lds_kernel<3, 4, 1, 2, 16, 14, false, 2, 3>";
    case 4: return "conv_s2_wgrad_lds_kernel<3, 4, 1, 4, 8, 14, false, 2, 3>";
    case 2: return "conv_s2_wgrad_lds_kernel<4, 2, 2, 2, 16, 16, true, 2, 2>";
    case 5: return "conv_s2_wgrad_lds_kernel<2, 4, 2, 4, 8, 10, false, 2, 2>";
    case 6: return "conv_s2_wgrad_lds_kernel<4, 2, 3, 4, 8, 16, true, 2, 2>";
    default: return "conv_s2_wgrad_lds_kernel<4, 2, 2, 4, 8, 16, true, 2, 2>";
  }
}

static std::string generic_name(int BC) {
  char buf[64];
  snprintf(buf, sizeof buf, "conv_wgrad_kernel<64, %d, %d>", BC, BC >= 48 ? 32 : 64);
  return buf;
}

static std::string main_name(const WgradLaunchPlan& l) {
  switch (l.family) {
    case WGRAD_FAMILY_HALO: return "conv_s2_halo_wgrad_kernel<32, 48>";
    case WGRAD_FAMILY_CONV1: return "conv1_halo_wgrad_kernel";
    case WGRAD_FAMILY_LDS: return lds_name(l.variant);
    default: return generic_name(l.variant);
  }
}

static const char* reduce_form(const WgradLaunchPlan& l) { return !l.reduce ? "none" : l.reduce_split ? "split" : "plain"; }

static std::string key_of(const WgradLaunchPlan& l) {
  return std::string(kFamily[l.family]) + " " + main_name(l) + " reduce=" + reduce_form(l) + (l.S > 1 ? " S>1" : " S=1") +
         (l.remainder ? " remainder" : " regular");
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: conv_wgrad_cover conv_wgrad_cases.txt\n");
    return 2;
  }
  // ---- the sweep ------------------------------------------------------------------------------------------------------
  std::set<std::string> keys, reached;
  const int inputs[3] = {136, 144, 256};
  for (int in : inputs)
    for (int G = 1; G <= 3; ++G)
      for (int N = 1; N <= 512; ++N) {
        int H = in, W = in, Cin = 4;
        for (int l = 0; l < 8; ++l) {
          const int Cout = kFilters[l], s = kStrides[l];
          const int first = (int)wgrad_family(G, N, H, W, Cin, Cout, s);
          for (int f = first; f < 4; ++f) {
            WgradLaunchPlan lp;
            if (!wgrad_launch_plan((WgradFamily)f, WGRAD_CUS, G, N, H, W, Cin, Cout, s, &lp)) continue;
            keys.insert(key_of(lp));
            reached.insert(main_name(lp));
            if (lp.reduce) reached.insert(lp.reduce_split ? "wgrad_reduce_kernel<true>" : "wgrad_reduce_kernel<false>");
          }
          int pad;
          same_pad(H, 3, s, &H, &pad);
          same_pad(W, 3, s, &W, &pad);
          Cin = Cout;
        }
      }

  // ---- the cases -----------------------------------------------------------------------------------------------------
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
    int G, N, H, W, Cin, Cout, s;
    if (sscanf(line, "%d %d %d %d %d %d %d", &G, &N, &H, &W, &Cin, &Cout, &s) != 7 || G < 1 || N < 1 || H < 1 || W < 1 || s < 1 ||
        Cin < 4 || Cin % 4 != 0 || Cout % 16 != 0 || Cout < 16) {
      fprintf(stderr, "bad case line: %s\n", line);
      return 2;
    }
    WgradLaunchPlan lp;
    if (!wgrad_launch_plan(wgrad_family(G, N, H, W, Cin, Cout, s), WGRAD_CUS, G, N, H, W, Cin, Cout, s, &lp)) {
      fprintf(stderr, "no family serves: %s\n", line);
      return 2;
    }
    printf("case %s | %s %s S=%d reduce=%s slice_px=%lld%s%s\n", line, kFamily[lp.family], main_name(lp).c_str(), lp.S,
           reduce_form(lp), lp.slice_px, lp.remainder ? " remainder" : "", reached.count(main_name(lp)) ? "" : " unreached");
  }
  fclose(f);

  for (const std::string& k : keys) printf("sweep %s\n", k.c_str());
  const int lds_variants[6] = {1, 2, 3, 4, 5, 6}, generic_tiles[4] = {64, 48, 32, 16};
  for (int v : lds_variants) printf("inst %s\n", lds_name(v).c_str());
  for (int bc : generic_tiles) printf("inst %s\n", generic_name(bc).c_str());
  printf("inst conv1_halo_wgrad_kernel\ninst conv_s2_halo_wgrad_kernel<32, 48>\n");
  printf("inst wgrad_reduce_kernel<true>\ninst wgrad_reduce_kernel<false>\n");
  return 0;
}
