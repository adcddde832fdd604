// Which launch variants of the LDS-halo and LDS-staged forwards and input gradients (geeco_amd/csrc/conv_halo_plan.h) the cases of
// conv_halo_cases.txt run, and which ones the models reach.  A launch is described by
//   family (lds: conv_dgrad_lds.hip; halo: conv_halo_s2_fwd.hip / conv_halo_s2_bwd.hip; conv1: conv_halo_conv1.hip; gemm: the
//   shape is left to the gather GEMM), the kernel instantiation as geeco_note_kernel names it, items (items or tiles of the
//   launch), blocks, rounds (the most items one block takes), cross (the boundaries some block's walk crosses between two of its
//   items: frame, cib = ci block, enc = encoder; none), empty (blocks whose range is empty)
// and its key is (family, instantiation, one round or several, mask form): none / mask / fields for a gradient, plain / fields /
// bits for a forward.
// Output, read by tests/test_conv_halo_cover_cpu.py:
//   (a) "case <the case's fields and flags> | <family> <instantiation> items=.. blocks=.. rounds=.. cross=.. empty=.." per case
//       of the list (argv[1]); "| gemm" for a shape these dispatchers decline;
//   (b) "sweep <key>" once per key of the sweep: the eight encoder layers at inputs 136 / 144 / 256 with 1..3 encoders and
//       1..512 frames, forward and input gradient, in every mask form the entry points of the layer's family take;
//   (c) "inst <instantiation>" once per instantiation these dispatchers can choose at all.
// A host program (tests/native/conv_wgrad_cover.cpp's style): built with -fsanitize=address,undefined, never loaded into Python.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <set>
#include <string>
#include <vector>
#include "conv_halo_plan.h"

static const int kFilters[8] = {32, 48, 64, 128, 192, 256, 256, 256};
static const int kStrides[8] = {1, 2, 2, 2, 2, 2, 2, 2};

struct Launch {
  std::string family, inst;      // family "gemm": declined
  long long items = 0;
  long long blocks = 0;
  long long rounds = 0;
  bool frame = false, cib = false, enc = false;
  long long empty = 0;
};

static std::string fmt(const char* f, int a, int b, int c = 0, int d = 0, int e = 0) {
  char buf[96];
  snprintf(buf, sizeof buf, f, a, b, c, d, e);
  return buf;
}

// blocks that take the items b, b + blocks, ... of `items`, an item being (encoder, ci block, tile) with the tile fastest
// (conv_s2_dgrad_lds_kernel's decode; conv1's forward with n_cib = 1 and one grid row per encoder)
static void strided_walk(Launch& l, long long items, long long blocks, int n_cib, long long tiles_per_group, long long tiles_per_frame,
                         bool detail) {
  const long long per_g = n_cib * tiles_per_group;
  l.rounds = (items + blocks - 1) / blocks;
  if (!detail) return;      // the sweep asks for the rounds only
  for (long long b = 0; b < blocks; ++b)
    for (long long it = b; it + blocks < items; it += blocks) {
      const long long nx = it + blocks;
      const long long g0 = it / per_g, g1 = nx / per_g;
      const long long c0 = (it - g0 * per_g) / tiles_per_group, c1 = (nx - g1 * per_g) / tiles_per_group;
      const long long f0 = ((it - g0 * per_g) % tiles_per_group) / tiles_per_frame, f1 = ((nx - g1 * per_g) % tiles_per_group) / tiles_per_frame;
      if (g0 != g1) l.enc = true;
      if (c0 != c1) l.cib = true;
      if (f0 != f1) l.frame = true;
    }
}

// blocks that take the tiles [b per, (b + 1) per) of the grid (the stride-2 halo kernels)
static void range_walk(Launch& l, const HaloTileGrid& t, bool detail) {
  const long long per = halo_tiles_per_block(t.ntiles, t.blocks);
  const long long per_frame = (long long)t.tiles_x * t.tiles_y;
  l.items = t.ntiles; l.blocks = t.blocks; l.rounds = per;
  if (!detail) return;
  for (long long b = 0; b < t.blocks; ++b) {
    const long long first = b * per, end = first + per < t.ntiles ? first + per : t.ntiles;
    if (first >= end) {
      ++l.empty;
      continue;
    }
    for (long long i = first; i + 1 < end; ++i) {
      if (i / t.tiles_per_group != (i + 1) / t.tiles_per_group) l.enc = true;
      if (i / per_frame != (i + 1) / per_frame) l.frame = true;
    }
  }
}

static Launch dgrad_launch(int G, int N, int H, int W, int Cin, int Cout, int s, bool fields, int reserved, bool detail = false) {
  Launch l;
  const ConvFamily fam = conv_dgrad_family(H, W, Cin, Cout, s);
  if (fam == CONV_HALO) {
    l.family = "halo";
    const bool conv3 = Cin == 48;
    l.inst = conv3 ? std::string("conv_s2_halo_dgrad_chunked_kernel<48, 64, ") + (fields ? "true>" : "false>") : "conv_s2_halo_dgrad_kernel<32, 48>";
    range_walk(l, halo_dgrad_grid(G, N, H, W, conv3 ? reserved : 0), detail);
    return l;
  }
  if (fam == CONV_DGRAD_LDS) {
    const DgradLdsPlan pl = dgrad_lds_plan(G, N, H, W, Cin, Cout, s);
    if (pl.variant != DGRAD_LDS_NONE) {
      l.family = "lds";
      l.inst = fmt("conv_s2_dgrad_lds_kernel<%d, %d, %d, %d, %d>", pl.PR, pl.PC, pl.FR, pl.NCIT, pl.NW);
      l.items = pl.items; l.blocks = pl.blocks;
      strided_walk(l, pl.items, pl.blocks, pl.n_cib, pl.tiles_per_group, (long long)pl.tiles_y * pl.tiles_x, detail);
      return l;
    }
  }
  l.family = "gemm";
  return l;
}

static Launch fwd_launch(int G, int N, int H, int W, int Cin, int Cout, int s, bool rgb, bool detail = false) {
  Launch l;
  const ConvFamily fam = conv_fwd_family(H, W, Cin, Cout, s);
  if (fam == CONV_HALO) {
    l.family = "halo";
    l.inst = Cin == 32 ? "conv_s2_halo_fwd_ws_kernel<32, 48, 4>" : "conv_s2_halo_fwd_chunked_kernel<48, 64>";
    range_walk(l, halo_fwd_grid(G, N, H, W), detail);
    return l;
  }
  if (fam == CONV_CONV1) {
    l.family = "conv1";
    l.inst = rgb ? "conv1_halo_fwd_kernel<true>" : "conv1_halo_fwd_kernel<false>";
    const HaloTileGrid t = conv1_fwd_grid(G, N, H, W);
    l.items = t.ntiles; l.blocks = (long long)t.blocks * t.grid_y;
    // every encoder has its own grid row: one encoder's walk, never across encoders
    strided_walk(l, t.tiles_per_group, t.blocks, 1, t.tiles_per_group, (long long)t.tiles_x * t.tiles_y, detail);
    return l;
  }
  l.family = "gemm";
  return l;
}

static std::string key_of(const Launch& l, const char* form) {
  return l.family + " " + l.inst + (l.rounds > 1 ? " several " : " one ") + form;
}

static std::string text_of(const Launch& l) {
  if (l.family == "gemm") return "gemm";
  std::string cross;
  if (l.frame) cross += "frame";
  if (l.cib) cross += std::string(cross.empty() ? "" : "+") + "cib";
  if (l.enc) cross += std::string(cross.empty() ? "" : "+") + "enc";
  if (cross.empty()) cross = "none";
  char buf[160];
  snprintf(buf, sizeof buf, " items=%lld blocks=%lld rounds=%lld cross=%s empty=%lld", l.items, l.blocks, l.rounds, cross.c_str(), l.empty);
  return l.family + " " + l.inst + buf;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: conv_halo_cover conv_halo_cases.txt\n");
    return 2;
  }
  // ---- the sweep ------------------------------------------------------------------------------------------------------
  std::set<std::string> keys;
  const int inputs[3] = {136, 144, 256};
  for (int in : inputs)
    for (int G = 1; G <= 3; ++G)
      for (int N = 1; N <= 512; ++N) {
        int H = in, W = in, Cin = 4;
        for (int l = 0; l < 8; ++l) {
          const int Cout = kFilters[l], s = kStrides[l];
          Launch f = fwd_launch(G, N, H, W, Cin, Cout, s, false);
          if (f.family == "halo") {
            keys.insert(key_of(f, "plain"));
            keys.insert(key_of(f, "fields"));
          } else if (f.family == "conv1") {
            keys.insert(key_of(f, "plain"));
            keys.insert(key_of(f, "bits"));
            keys.insert(key_of(fwd_launch(G, N, H, W, Cin, Cout, s, true), "bits"));
          }
          if (l > 0) {
            Launch d = dgrad_launch(G, N, H, W, Cin, Cout, s, false, 0);
            if (d.family != "gemm") {
              keys.insert(key_of(d, "none"));
              keys.insert(key_of(d, "mask"));
              // sign fields: conv3's chunked kernel (another instantiation) and every LDS-staged one (Cin % 32 == 0)
              if (d.family == "lds") keys.insert(key_of(d, "fields"));
              if (d.family == "halo" && Cin == 48) keys.insert(key_of(dgrad_launch(G, N, H, W, Cin, Cout, s, true, 0), "fields"));
            }
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
    char dir[16] = {0};
    int G, N, H, W, Cin, Cout, s, used = 0;
    if (sscanf(line, "%15s %d %d %d %d %d %d %d%n", dir, &G, &N, &H, &W, &Cin, &Cout, &s, &used) != 8 || G < 1 || N < 1 || H < 1 ||
        W < 1 || s < 1 || Cin < 4 || Cin % 4 != 0 || Cout % 16 != 0 || Cout < 16 || (strcmp(dir, "fwd") && strcmp(dir, "dgrad"))) {
      fprintf(stderr, "bad case line: %s\n", line);
      return 2;
    }
    bool fields = false, rgb = false;
    int reserved = 0;
    std::vector<char> rest(line + used, line + n + 1);
    for (char* tok = strtok(rest.data(), " \t"); tok; tok = strtok(nullptr, " \t")) {
      if (!strcmp(tok, "fields")) fields = true;
      else if (!strcmp(tok, "rgb")) rgb = true;
      else if (!strncmp(tok, "reserved=", 9)) reserved = atoi(tok + 9);
      else if (strcmp(tok, "mask") && strcmp(tok, "relu") && strcmp(tok, "bias") && strcmp(tok, "bits") && strcmp(tok, "hostonly")) {
        fprintf(stderr, "unknown flag %s: %s\n", tok, line);
        return 2;
      }
    }
    if (reserved < 0 || reserved > 128) {
      fprintf(stderr, "reserved outside 0..128: %s\n", line);
      return 2;
    }
    const Launch l = !strcmp(dir, "fwd") ? fwd_launch(G, N, H, W, Cin, Cout, s, rgb, true) : dgrad_launch(G, N, H, W, Cin, Cout, s, fields, reserved, true);
    printf("case %s | %s\n", line, text_of(l).c_str());
  }
  fclose(f);

  for (const std::string& k : keys) printf("sweep %s\n", k.c_str());
  printf("inst conv_s2_dgrad_lds_kernel<1, 16, 1, 4, 8>\ninst conv_s2_dgrad_lds_kernel<1, 16, 1, 2, 8>\n");
  printf("inst conv_s2_dgrad_lds_kernel<2, 8, 1, 2, 4>\ninst conv_s2_halo_dgrad_kernel<32, 48>\n");
  printf("inst conv_s2_halo_dgrad_chunked_kernel<48, 64, false>\ninst conv_s2_halo_dgrad_chunked_kernel<48, 64, true>\n");
  printf("inst conv_s2_halo_fwd_ws_kernel<32, 48, 4>\ninst conv_s2_halo_fwd_chunked_kernel<48, 64>\n");
  printf("inst conv1_halo_fwd_kernel<false>\ninst conv1_halo_fwd_kernel<true>\n");
  return 0;
}
