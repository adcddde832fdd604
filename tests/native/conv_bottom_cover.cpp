// Which launch forms of the fused encoder-bottom backward (conv2_dgrad_conv1_wgrad_kernel<CREAL, BITS>, geeco_amd/csrc/conv_halo_bottom.hip)
// the cases of conv_bottom_cases.txt run, and which ones the models reach.  A launch is described by
//   the instantiation as geeco_note_kernel names it, tiles (8 x 64 tiles per encoder), blocks, S (slabs per encoder), per (tiles
//   of a regular block), slice_px (per * 8 * 64), remainder / regular (the remainder-block form: one more block walks what every
//   encoder's regular blocks leave over, encoder after encoder), cross (the boundaries some block's walk crosses between two of
//   its tiles: frame; enc = the remainder block going from one encoder's segment to the next; none), empty (blocks with an
//   empty range)
// and its key is (instantiation class: mask or bits; regular or remainder; crossing kinds).
// Output, read by tests/test_conv_bottom_cover_cpu.py:
//   (a) "case <the case's fields and flags> | <instantiation> tiles=.. blocks=.. S=.. per=.. slice_px=.. remainder|regular cross=..
//       empty=.." per case of the list (argv[1]);
//   (b) "sweep <key>" once per key of the sweep: the models' launches (the sign-word entry point) at inputs 136 / 144 / 256 with
//       1..3 encoders, 1..512 frames and reserved_cus in {0, 16, 32} (the step runner's values);
//   (c) "inst <instantiation>" for each of the four.
// The walk also holds the plan itself: every tile of every encoder is in exactly one block's range, no block past the CUs of the
// call, no slab past the workspace.  A host program (tests/native/conv_wgrad_cover.cpp's style): built with
// -fsanitize=address,undefined, never loaded into Python.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <set>
#include <string>
#include <vector>
#include "conv_wgrad_plan.h"

struct Walk {
  bool frame = false, enc = false;
  long long empty = 0;
  long long covered = 0;      // tiles in some block's range, all encoders
};

// [first, end) of one block's range inside an encoder: crosses a frame when its first and last tile lie in different frames
static void range(Walk& w, long long first, long long end, long long per_frame) {
  if (first >= end) return;
  w.covered += end - first;
  if (first / per_frame != (end - 1) / per_frame) w.frame = true;
}

// the kernel's own decode (conv2_dgrad_conv1_wgrad_kernel: regular blocks S0 per encoder, then the remainder block's segments)
static Walk walk(const FusedBottomLaunchPlan& l, int groups) {
  Walk w;
  const long long per_frame = (long long)l.tiles_x * l.tiles_y, T = l.tiles;
  const int nreg = l.S0 * groups;
  for (int b = 0; b < l.blocks; ++b) {
    if (b < nreg) {
      const long long split = b % l.S0, first = split * l.per;
      const long long end = first + l.per < T ? first + l.per : T;
      if (first >= end) ++w.empty;
      range(w, first, end, per_frame);
    } else {
      long long nonempty = 0;
      for (int g = 0; g < groups; ++g) {
        const long long first = (long long)l.S0 * l.per;
        range(w, first, T, per_frame);
        if (first < T) ++nonempty;
      }
      if (nonempty == 0) ++w.empty;
      if (nonempty > 1) w.enc = true;
    }
  }
  return w;
}

static std::string cross_of(const Walk& w) {
  std::string c;
  if (w.frame) c += "frame";
  if (w.enc) c += std::string(c.empty() ? "" : "+") + "enc";
  return c.empty() ? "none" : c;
}

static std::string inst_name(int creal, bool bits) {
  char buf[64];
  snprintf(buf, sizeof buf, "conv2_dgrad_conv1_wgrad_kernel<%d, %s>", creal, bits ? "true" : "false");
  return buf;
}

// -> false when the plan breaks one of its own conditions
static bool plan_holds(const FusedBottomLaunchPlan& l, const Walk& w, int cus, int groups, const char* what) {
  const BottomSlices ws = bottom_slices_on(WGRAD_CUS, groups, 0, true);
  const bool ok = w.covered == (long long)l.tiles * groups && l.blocks <= cus && l.blocks >= 1 && l.S <= ws.S && l.per >= 1 &&
                  l.S == l.S0 + (l.remainder ? 1 : 0) && l.blocks == l.S0 * groups + (l.remainder ? 1 : 0);
  if (!ok) fprintf(stderr, "the plan does not hold: %s: tiles %d covered %lld blocks %d cus %d S %d\n", what, l.tiles, w.covered, l.blocks, cus, l.S);
  return ok;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: conv_bottom_cover conv_bottom_cases.txt\n");
    return 2;
  }
  // ---- the sweep ------------------------------------------------------------------------------------------------------
  std::set<std::string> keys;
  const int inputs[3] = {136, 144, 256}, reserved_of_the_runner[3] = {0, 16, 32};
  for (int in : inputs)
    for (int G = 1; G <= 3; ++G)
      for (int N = 1; N <= 512; ++N)
        for (int res : reserved_of_the_runner) {
          const FusedBottomLaunchPlan l = fused_bottom_launch_plan(WGRAD_CUS - res, G, N, in, in);
          const Walk w = walk(l, G);
          char what[96];
          snprintf(what, sizeof what, "sweep %d %d %d %d reserved=%d", G, N, in, in, res);
          if (!plan_holds(l, w, WGRAD_CUS - res, G, what)) return 1;
          keys.insert(std::string("bits ") + (l.remainder ? "remainder" : "regular") + " cross=" + cross_of(w));
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
    int G, N, H, W, C, used = 0;
    if (sscanf(line, "%d %d %d %d %d%n", &G, &N, &H, &W, &C, &used) != 5 || G < 1 || N < 1 || H < 2 || W < 2 || H % 2 || W % 2 ||
        (C != 3 && C != 4)) {
      fprintf(stderr, "bad case line: %s\n", line);
      return 2;
    }
    bool mask = false, bits = false, dz1 = false, pending = false;
    int reserved = 0;
    std::vector<char> rest(line + used, line + n + 1);
    for (char* tok = strtok(rest.data(), " \t"); tok; tok = strtok(nullptr, " \t")) {
      if (!strcmp(tok, "mask")) mask = true;
      else if (!strcmp(tok, "bits")) bits = true;
      else if (!strcmp(tok, "dz1")) dz1 = true;
      else if (!strcmp(tok, "pending")) pending = true;
      else if (!strncmp(tok, "reserved=", 9)) reserved = atoi(tok + 9);
      else {
        fprintf(stderr, "unknown flag %s: %s\n", tok, line);
        return 2;
      }
    }
    // exactly one mask form; dz1 is stored by the float-mask forms only; reserved CUs are an argument of the deferred form
    if (mask == bits || (dz1 && bits) || (reserved && !pending) || reserved < 0 || reserved > 128) {
      fprintf(stderr, "flags do not fit an entry point: %s\n", line);
      return 2;
    }
    const FusedBottomLaunchPlan l = fused_bottom_launch_plan(WGRAD_CUS - reserved, G, N, H, W);
    const Walk w = walk(l, G);
    if (!plan_holds(l, w, WGRAD_CUS - reserved, G, line)) return 1;
    printf("case %s | %s tiles=%d blocks=%d S=%d per=%d slice_px=%lld %s cross=%s empty=%lld\n", line, inst_name(C, bits).c_str(), l.tiles,
           l.blocks, l.S, l.per, l.slice_px, l.remainder ? "remainder" : "regular", cross_of(w).c_str(), w.empty);
  }
  fclose(f);

  for (const std::string& k : keys) printf("sweep %s\n", k.c_str());
  for (int c = 3; c <= 4; ++c)
    for (int b = 0; b < 2; ++b) printf("inst %s\n", inst_name(c, b != 0).c_str());
  return 0;
}
