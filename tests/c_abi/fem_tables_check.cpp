// Stand-alone program behind tests/test_sweep_truth_host.py (test_system_fast_order_restated, test_wide_cases_reach_their_paths),
// built with -fsanitize=address,undefined: plans the geometries named on its command line (as PxQ-N<N>, default 3x3-N140 and
// 2x2-N128) and prints two lines per geometry.
//   "tables <geometry> gstotal <doubles> bytes <b> ...": the size of the segment-major extension tables (k_extend128's B operand:
//       rom_fem::gs_bytes = 8 gstotal) that enqueue_solve holds against 64 MiB when it chooses the workgroup order, the kinds of
//       its blocks and what the workspace of a sweep is computed from;
//   "paths <geometry> tiling <0 row | 1 flat> ...": which paths of k_extend128 the geometry's tiles take, summed over its compressed
//       blocks, from x128_skip_counts (rom_fem_plan.h, the function the kernel calls) in the tiling enqueue_solve picks:
//       tiles; flat tiles inside one mesh row (one_row), those of them that skip a K segment of side 2 or 3 (one_row_skip23), flat
//       tiles over exactly two mesh rows (two_rows) and over more (more_rows); waves with 1 .. 31 vertices (ragged_waves) and with
//       none (empty_waves); (tile, wave, side) where the wave skips more than its tile (wave_larger); the longest walk of a tile in
//       8-wide segments (max_walk: per-wave skipping needs fewer than 64).
// Exit status 0 = every plan succeeded.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "rom_fem_plan.h"

template <bool FLAT>
static void paths(const char* name, const FemPlan& p) {
  const int n1 = p.n1, N = p.N, nvert = n1 * n1, nct = (n1 + 127) / 128;
  const int ntile = FLAT ? (nvert + 127) / 128 : n1 * nct;
  long long tiles = 0, one_row = 0, one_row_skip23 = 0, two_rows = 0, more_rows = 0, ragged = 0, empty = 0, larger = 0;
  int max_walk = 0;
  for (int b : p.lr_blocks) {
    const BlockSide& sd = p.sides[b];
    for (int tile = 0; tile < ntile; ++tile) {
      ++tiles;
      int tsk[4], wsk[4];
      for (int wc = 0; wc < 4; ++wc) {
        const bool has = x128_skip_counts<FLAT>(n1, N, tile, wc, sd.s[0], sd.s[1], sd.s[2], sd.s[3], tsk, wsk);
        const int first = FLAT ? 128 * tile + 32 * wc : 128 * (tile % nct) + 32 * wc, end = FLAT ? nvert : n1;  // 0-based
        const int nv = first >= end ? 0 : end - first < 32 ? end - first : 32;
        if (has != (nv > 0)) {
          fprintf(stderr, "%s: tile %d wave %d: x128_skip_counts reports vertices %d, the wave has %d\n", name, tile, wc, int(has), nv);
          exit(1);
        }
        empty += nv == 0;
        ragged += nv > 0 && nv < 32;
        for (int s = 0; s < 4; ++s) larger += has && wsk[s] > tsk[s];
      }
      int walk = 0;
      for (int s = 0; s < 4; ++s) walk += x128_segs(sd.s[s]) - tsk[s];
      max_walk = walk > max_walk ? walk : max_walk;
      if (FLAT) {
        const int vt0 = 128 * tile, vend = vt0 + 127 < nvert - 1 ? vt0 + 127 : nvert - 1, rows = vend / n1 - vt0 / n1 + 1;
        one_row += rows == 1;
        one_row_skip23 += rows == 1 && (tsk[2] > 0 || tsk[3] > 0);
        two_rows += rows == 2;
        more_rows += rows > 2;
      }
    }
  }
  printf("paths %s tiling %d tiles %lld one_row %lld one_row_skip23 %lld two_rows %lld more_rows %lld ragged_waves %lld empty_waves %lld "
         "wave_larger %lld max_walk %d\n", name, int(FLAT), tiles, one_row, one_row_skip23, two_rows, more_rows, ragged, empty, larger,
         max_walk);
}

int main(int argc, char** argv) {
  const FemSwitches plain{false, false, false, false, false, 1e-14L, false};
  const char* dflt[] = {"", "3x3-N140", "2x2-N128"};
  if (argc < 2) {
    argc = 3;
    argv = const_cast<char**>(dflt);
  }
  int failures = 0;
  for (int i = 1; i < argc; ++i) {
    int nrb = 0, ncb = 0, N = 0;
    if (sscanf(argv[i], "%dx%d-N%d", &nrb, &ncb, &N) != 3) {
      fprintf(stderr, "%s: expected PxQ-N<N>\n", argv[i]);
      return 2;
    }
    FemPlan p;
    std::string err;
    if (rom_fem_plan(nrb, ncb, N, plain, &p, &err) != ROM_OK) {
      ++failures;
      fprintf(stderr, "%s: rom_fem_plan failed: %s\n", argv[i], err.c_str());
      continue;
    }
    printf("tables %s gstotal %lld bytes %lld n1 %d lr %zu gen %zu T %d slots %d nGa %d nGp %d lr_nch %d\n", argv[i], p.gstotal,
           p.gstotal * 8, p.n1, p.lr_blocks.size(), p.gen_blocks.size(), p.T, p.nslots, p.nGa, p.nGp, p.lr_nch);
    // the tiling enqueue_solve picks for 128 systems or more (rom_fem_solve.hip)
    const int t_row = p.n1 * ((p.n1 + 127) / 128), t_flat = (p.n1 * p.n1 + 127) / 128;
    if (100 * t_flat < 97 * t_row) paths<true>(argv[i], p);
    else paths<false>(argv[i], p);
  }
  return failures ? 1 : 0;
}
