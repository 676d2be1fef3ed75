// Stand-alone check of the per-wave K-segment skipping of k_extend128 (x128_skip_counts, romhighcontrast_amd/csrc/rom_fem_plan.h:
// the function the kernel calls), built with -fsanitize=address,undefined by tests/test_ext_wave_skip_host.py.  Plans
// 2x2 / N = 128 (row tiles), 3x3 / N = 64 (FLAT), 3x3 / N = 171 (FLAT, n1 = 170), 2x3 / N = 128, 4x4 / N = 256 and the wide cases
// of tests/sweep_truth.py with something to skip (2x2 / N = 171, 3x3 / N = 140: FLAT, n1 odd; 2x2 / N = 250: row tiles) and, for every
// block the 128-vertex kernel extends, every tile, wave column and side, checks by brute force over the wave's vertices that no
// K segment a vertex needs (FemPlan::GemmG::seg0 at the vertex's distance) lies in front of the wave's skip count, that the wave's
// count is never below the tile's and that every geometry has a (tile, wave, side) where it is larger.  Prints per geometry
//   "count <geometry> <tiling> executed_tile <a> needed_wave <b> tile_needed <c>"
// in units of one 8-wide segment of one wave column: a = what every wave multiplied while it followed its tile's walk (the zero
// half of an odd walk included), b = what the waves multiply now, c = the tile-level count without the zero half.
// Exit status 0 = no violation.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "rom_fem_plan.h"

static int failures = 0;
static const char* current = "";
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) {                                                               \
      ++failures;                                                                \
      fprintf(stderr, "%s: violated: %s (line %d)\n", current, #cond, __LINE__); \
    }                                                                            \
  } while (0)

template <bool FLAT>
static void check_tiling(const FemPlan& p, long long* executed_tile, long long* needed_wave, long long* tile_needed, long long* larger) {
  const int n1 = p.n1, N = p.N, nvert = n1 * n1, nct = (n1 + 127) / 128;
  const int ntile = FLAT ? (nvert + 127) / 128 : n1 * nct;
  for (int b : p.lr_blocks) {
    const BlockSide& sd = p.sides[b];
    const FemPlan::GemmG* gg[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int s = 0; s < 4; ++s) {
      if (sd.s[s].mode != 2) continue;
      for (const FemPlan::GemmG& cand : p.gemm_G)
        if (cand.off == sd.s[s].gtab) gg[s] = &cand;
      CHECK(gg[s] != nullptr && int(gg[s]->seg0.size()) == N + 1);
      if (!gg[s] || int(gg[s]->seg0.size()) != N + 1) return;
    }
    for (int tile = 0; tile < ntile; ++tile) {
      int tile_segs = 0;
      for (int wc = 0; wc < 4; ++wc) {
        int tsk[4], wsk[4];
        const bool has = x128_skip_counts<FLAT>(n1, N, tile, wc, sd.s[0], sd.s[1], sd.s[2], sd.s[3], tsk, wsk);
        // the wave's vertices, 1-based (i, j)
        std::vector<std::pair<int, int>> verts;
        for (int t = 32 * wc; t < 32 * wc + 32; ++t) {
          if (FLAT) {
            const int v = 128 * tile + t;
            if (v < nvert) verts.push_back({v / n1 + 1, v % n1 + 1});
          } else {
            const int j = 128 * (tile % nct) + 1 + t;
            if (j <= n1) verts.push_back({tile / nct + 1, j});
          }
        }
        CHECK(has == !verts.empty());
        tile_segs = 0;
        for (int s = 0; s < 4; ++s) {
          const int segs = x128_segs(sd.s[s]);
          CHECK(sd.s[s].mode == 2 ? segs >= 1 : segs == 0);
          CHECK(tsk[s] >= 0 && wsk[s] >= tsk[s] && wsk[s] <= (segs > 0 ? segs - 1 : 0));
          if (sd.s[s].mode != 2) continue;
          tile_segs += segs - tsk[s];
          if (has) *needed_wave += segs - wsk[s];
          if (has && wsk[s] > tsk[s]) ++*larger;
          for (const auto& ij : verts) {
            const int d = s == 0 ? ij.first : s == 1 ? N - ij.first : s == 2 ? ij.second : N - ij.second;
            CHECK(d >= 1 && d <= n1);
            const int need_from = gg[s]->seg0[d] < segs - 1 ? gg[s]->seg0[d] : segs - 1;  // first segment the vertex needs
            CHECK(need_from >= wsk[s]);
            CHECK(need_from >= tsk[s]);
          }
        }
        *executed_tile += 2 * ((tile_segs + 1) / 2);
        *tile_needed += tile_segs;
      }
    }
  }
}

int main() {
  const struct { int nrb, ncb, N; } geo[] = {{2, 2, 128}, {3, 3, 64}, {3, 3, 171}, {2, 3, 128}, {4, 4, 256},
                                             {2, 2, 171}, {3, 3, 140}, {2, 2, 250}};  // (the wide cases of tests/sweep_truth.py)
  for (const auto& g : geo) {
    char name[64];
    snprintf(name, sizeof(name), "%dx%d-N%d", g.nrb, g.ncb, g.N);
    current = name;
    FemSwitches sw{false, false, false, false, false, 1e-14L, false};
    FemPlan p;
    std::string err;
    if (rom_fem_plan(g.nrb, g.ncb, g.N, sw, &p, &err) != ROM_OK) {
      ++failures;
      fprintf(stderr, "%s: rom_fem_plan failed: %s\n", name, err.c_str());
      continue;
    }
    CHECK(!p.lr_blocks.empty());
    // the tiling rom_solve_batch picks (rom_fem_solve.hip)
    const int t_row = p.n1 * ((p.n1 + 127) / 128), t_flat = (p.n1 * p.n1 + 127) / 128;
    const bool flat = 100 * t_flat < 97 * t_row;
    long long executed_tile = 0, needed_wave = 0, tile_needed = 0, larger = 0;
    if (flat) check_tiling<true>(p, &executed_tile, &needed_wave, &tile_needed, &larger);
    else check_tiling<false>(p, &executed_tile, &needed_wave, &tile_needed, &larger);
    CHECK(larger > 0);  // (otherwise the GPU tests of the skipping prove nothing)
    CHECK(needed_wave < tile_needed && tile_needed <= executed_tile);
    printf("count %s %s executed_tile %lld needed_wave %lld tile_needed %lld\n", name, flat ? "flat" : "row", executed_tile,
           needed_wave, tile_needed);
    for (const BlockSide& bs : p.sides)
      for (const ExtSide& s : bs.s)
        if (s.mode == 2) {
          printf("thresholds %s rank %d:", name, s.r);
          for (int j = 0; j < EXT_THRESHOLDS; ++j) printf(" %d", int(s.thr[j]));
          printf("\n");
        }
    // the other tiling of the same plan must be safe too (the A/B build forces either one)
    long long x0 = 0, x1 = 0, x2 = 0, x3 = 0;
    if (flat) check_tiling<false>(p, &x0, &x1, &x2, &x3);
    else check_tiling<true>(p, &x0, &x1, &x2, &x3);
  }
  if (failures) fprintf(stderr, "%d violation(s)\n", failures);
  return failures ? 1 : 0;
}
