// Stand-alone check of the per-tile records of k_extend128 (X128Tile / x128_tile_plan, romhighcontrast_amd/csrc/rom_fem_plan.h; the
// tables FemPlan::x128_row and x128_flat that rom_fem_plan fills), built with -fsanitize=address,undefined by
// tests/test_x128_plan_host.py.  Plans 2x2 / N = 128 (row tiles), 3x3 / N = 64 (FLAT), 2x2 / N = 171 (FLAT, tiles inside one mesh
// row), 2x2 / N = 250 (two column tiles per mesh row, the last partly filled) and 5x4 / N = 64 (20 blocks: two launches) and, in BOTH
// tilings of every plan, for every (lr block, tile, wave column) holds the planner's record against
//   - a fresh call of x128_skip_counts (the function the kernel used to call): segment counts, first-segment offsets of both
//     operands, `has`;
//   - the wave's mask, built here bit by bit from its meaning (half h of the walk = segment tsk + k of side s; the wave multiplies
//     it iff it has a vertex and the segment is not in front of its own skip count), and the mask formula the kernel had;
//   - the tile's first vertex, the block, and the indexing of a launch: record [z0 + z][tile] belongs to block lr_blocks[z0 + z].
// Prints "records <geometry> lr <blocks> launches <n> row <tiles per block> flat <tiles per block> masked <records with a skipping wave>".
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
      if (++failures <= 20)                                                      \
        fprintf(stderr, "%s: violated: %s (line %d)\n", current, #cond, __LINE__); \
    }                                                                            \
  } while (0)

template <bool FLAT>
static long long check_tiling(const FemPlan& p, const std::vector<X128Tile>& table) {
  const int n1 = p.n1, N = p.N, nvert = n1 * n1, nct = (n1 + 127) / 128;
  const int ntile = FLAT ? (nvert + 127) / 128 : n1 * nct;
  const size_t seg_stride = size_t(n1) * n1 * 64;
  long long masked = 0;
  CHECK(table.size() == p.lr_blocks.size() * size_t(ntile));
  if (table.size() != p.lr_blocks.size() * size_t(ntile)) return 0;
  CHECK(reinterpret_cast<size_t>(table.data()) % 16 == 0 && sizeof(X128Tile) % 16 == 0);
  for (size_t z0 = 0; z0 < p.lr_blocks.size(); z0 += X128_BLOCKS)  // the launches of rom_solve_batch
    for (size_t z = 0; z < X128_BLOCKS && z0 + z < p.lr_blocks.size(); ++z) {
      const X128Tile* launch = table.data() + z0 * ntile;  // X128Head::plan of this launch
      const int b = p.lr_blocks[z0 + z];
      const BlockSide& sd = p.sides[b];
      for (int tile = 0; tile < ntile; ++tile) {
        const X128Tile& r = launch[z * ntile + tile];
        CHECK(r.block == b);
        const int v0 = 128 * tile;  // FLAT: the tile's first vertex
        CHECK(FLAT ? r.row == v0 / n1 && r.col == v0 % n1 : r.row == tile / nct + 1 && r.col == 128 * (tile % nct) + 1);
        int nseg = 0;
        bool any_skip = false;
        for (int wc = 0; wc < 4; ++wc) {
          int tsk[4], wsk[4];
          const bool has = x128_skip_counts<FLAT>(n1, N, tile, wc, sd.s[0], sd.s[1], sd.s[2], sd.s[3], tsk, wsk);
          nseg = 0;
          for (int s = 0; s < 4; ++s) {
            const int cnt = x128_segs(sd.s[s]) - tsk[s];
            CHECK(int(r.cnt[s]) == cnt);
            CHECK(r.offA[s] == unsigned(size_t(sd.s[s].off) * 8 + size_t(tsk[s]) * 64));
            CHECK(r.offB[s] == size_t(sd.s[s].gseg) * 8 + size_t(tsk[s]) * seg_stride);
            CHECK(sd.s[s].mode == 2 || cnt == 0);
            nseg += cnt;
          }
          // the mask from its meaning, half by half
          unsigned long long want = 0;
          int h = 0;
          for (int s = 0; s < 4; ++s)
            for (int k = 0; k < x128_segs(sd.s[s]) - tsk[s]; ++k, ++h)
              if (h < 64 && has && tsk[s] + k >= wsk[s]) want |= 1ull << h;
          if (nseg >= 64) want = ~0ull;  // (no mask for such a walk: the kernel multiplies everything)
          CHECK(r.live[wc] == want);
          if (nseg < 64) {  // ... and the formula the kernel had (X_LIVE)
            unsigned long long m = 0;
            int h0 = 0;
            for (int s = 0; s < 4; ++s) {
              const int cnt = x128_segs(sd.s[s]) - tsk[s];
              m |= ((1ull << cnt) - (1ull << (wsk[s] - tsk[s]))) << h0;
              h0 += cnt;
            }
            CHECK(r.live[wc] == (has ? m : 0ull));
            CHECK((r.live[wc] >> nseg) == 0);
            if (has && r.live[wc] != (nseg ? (1ull << nseg) - 1 : 0ull)) any_skip = true;
          }
        }
        CHECK(nseg > 0);
        masked += any_skip ? 1 : 0;
      }
    }
  return masked;
}

int main() {
  const struct { int nrb, ncb, N; bool flat; int launches; } geo[] = {
      {2, 2, 128, false, 1}, {3, 3, 64, true, 1}, {2, 2, 171, true, 1}, {2, 2, 250, false, 1}, {5, 4, 64, true, 2}};
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
    const int t_row = p.n1 * ((p.n1 + 127) / 128), t_flat = (p.n1 * p.n1 + 127) / 128;
    CHECK((100 * t_flat < 97 * t_row) == g.flat);  // the tiling rom_solve_batch picks (rom_fem_solve.hip)
    const int launches = (int(p.lr_blocks.size()) + X128_BLOCKS - 1) / X128_BLOCKS;
    CHECK(launches == g.launches);
    const long long m_row = check_tiling<false>(p, p.x128_row), m_flat = check_tiling<true>(p, p.x128_flat);
    CHECK((g.flat ? m_flat : m_row) > 0);  // (otherwise the masks of the tiling in use are all trivial)
    printf("records %s lr %zu launches %d row %d flat %d masked %lld\n", name, p.lr_blocks.size(), launches, t_row, t_flat,
           g.flat ? m_flat : m_row);
  }
  if (failures) fprintf(stderr, "%d violation(s)\n", failures);
  return failures ? 1 : 0;
}
