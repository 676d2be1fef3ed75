// FemPlan: everything rom_fem_create decides on the host -- the interface layout, the symbolic tile Cholesky and every
// parameter-independent table the sweep kernels read -- as plain host vectors.  rom_fem_plan (rom_fem_plan.hip) fills
// it without touching the GPU or the environment; rom_fem_create (rom_fem_setup.hip) uploads it.
#pragma once
#include <string>
#include <vector>

#include "romhc_internal.h"

// ---- constants shared by the planner and the kernels (rom_fem_dev.h includes this header) -------------------------
constexpr int COEF_MAX = 64;   // term weights cached in LDS per pass
#ifndef PAIR_RING_
#define PAIR_RING_ 8
#endif
constexpr int PAIR_RING = PAIR_RING_;  // (term, block) pairs in flight in the single-tile assembly
constexpr int DENSE_GROUPS_MAX = 8;    // closed-form edges whose coefficient blocks k_solve1 builds
constexpr int EXT_ZERO_PAGE = 256;  // doubles of zeros behind FemDev::W (target of the lanes of k_extend128 that have nothing to load)
constexpr int EXT_THRESHOLDS = 7;   // distance thresholds of a compressed side (ExtSide::thr): K segments k_extend128 can skip
constexpr long double EXT_TRUNC_CUT = 1e-18L;  // a table column is dropped where its bound is below this share of the largest
constexpr int X128_BLOCKS = 16;     // blocks one k_extend128 launch extends (grid z)

// row of H0 that holds the extension from side s evaluated at interior vertex (i,j), 1-based
__host__ __device__ inline int h0_row(int s, int i, int j, int N, int n1) {
  int ii, jj;
  switch (s) {
    case 0: ii = i; jj = j; break;
    case 1: ii = N - i; jj = j; break;
    case 2: ii = j; jj = i; break;
    default: ii = N - j; jj = i; break;
  }
  return (ii - 1) * n1 + (jj - 1);
}

// leading 8-wide K segments of a compressed side that are zero at distance d from it (ExtSide::thr, ascending)
__host__ __device__ inline int x128_skip(const ExtSide& s, int d) {
  int n = 0;
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
  for (int j = 0; j < EXT_THRESHOLDS; ++j) n += d >= int(s.thr[j]) ? 1 : 0;
  return n;
}
// 8-wide K segments of a side that k_extend128 walks at most (0 for a side that is not compressed): the tables are padded
// to 16 per side, but only ceil((rank + 1) / 8) segments hold anything
__host__ __device__ inline int x128_segs(const ExtSide& s) {
  const int padded = 2 * s.nch, filled = (s.r + 1 + 7) / 8;
  return s.mode == 2 ? (padded < filled ? padded : filled) : 0;
}
// skip count of one side at distance d, clamped: the last segment (with 1/s) is always walked
__host__ __device__ inline int x128_skip_clamped(const ExtSide& s, int d) {
  const int n = x128_skip(s, d), last = x128_segs(s) - 1;
  return s.mode == 2 ? (n < last ? n : last) : 0;
}

// The K segments k_extend128 skips per side (0: i = 0, 1: i = N, 2: j = 0, 3: j = N) of vertex tile `tile` (tsk: the
// DMA walk starts behind them) and of the 32 consecutive vertices of its wave column wc = 0 .. 3 (wsk >= tsk: the wave
// multiplies nothing in front of them).  A distance is that of the nearest vertex; the tile is a mesh row's vertices
// 128 (tile % nct) + 1 .. + 128, or (FLAT) vertices 128 tile .. + 127 of the block's row-major numbering, where a range
// that spans two mesh rows meets both ends of one.  Returns false where the wave has no vertex at all (the tile pads).
template <bool FLAT>
__host__ __device__ inline bool x128_skip_counts(int n1, int N, int tile, int wc, const ExtSide& s0, const ExtSide& s1,
                                                 const ExtSide& s2, const ExtSide& s3, int tsk[4], int wsk[4]) {
  int dist0, dist1, dist2, dist3;  // the tile's
  int wd0, wd1, wd2, wd3;          // the wave's
  bool has;
  if (FLAT) {
    const int nvert = n1 * n1, vt0 = 128 * tile;
    const int vend = vt0 + 127 < nvert - 1 ? vt0 + 127 : nvert - 1, i_lo = vt0 / n1, i_hi = vend / n1;  // 0-based mesh rows of the tile
    const bool one_row = i_lo == i_hi;  // (else the tile meets both ends of a mesh row)
    dist0 = i_lo + 1;
    dist1 = N - (i_hi + 1);
    dist2 = one_row ? vt0 - i_lo * n1 + 1 : 1;
    dist3 = one_row ? N - (vend - i_hi * n1 + 1) : 1;
    const int v0 = vt0 + 32 * wc, v1 = v0 + 31 < vend ? v0 + 31 : vend;
    has = v0 <= vend;
    const int w_lo = has ? v0 / n1 : i_lo, w_hi = has ? v1 / n1 : i_hi;
    const bool w_one = w_lo == w_hi;
    wd0 = w_lo + 1;
    wd1 = N - (w_hi + 1);
    wd2 = w_one ? v0 - w_lo * n1 + 1 : 1;
    wd3 = w_one ? N - (v1 - w_hi * n1 + 1) : 1;
  } else {
    const int nct = (n1 + 127) / 128, iv = tile / nct + 1, jv0 = 128 * (tile % nct) + 1;
    dist0 = iv;
    dist1 = N - iv;
    dist2 = jv0;
    dist3 = N - (jv0 + 127 < n1 ? jv0 + 127 : n1);
    const int jw = jv0 + 32 * wc;
    has = jw <= n1;
    wd0 = iv;
    wd1 = N - iv;
    wd2 = jw;
    wd3 = N - (jw + 31 < n1 ? jw + 31 : n1);
  }
  tsk[0] = x128_skip_clamped(s0, dist0);
  tsk[1] = x128_skip_clamped(s1, dist1);
  tsk[2] = x128_skip_clamped(s2, dist2);
  tsk[3] = x128_skip_clamped(s3, dist3);
  wsk[0] = has ? x128_skip_clamped(s0, wd0) : tsk[0];
  wsk[1] = has ? x128_skip_clamped(s1, wd1) : tsk[1];
  wsk[2] = has ? x128_skip_clamped(s2, wd2) : tsk[2];
  wsk[3] = has ? x128_skip_clamped(s3, wd3) : tsk[3];
  return has;
}

// What a workgroup of k_extend128 needs to know about its (lr block, tile) before it can request its first operand bytes,
// and its waves' share of the walk: all of it depends on the geometry alone, so the planner works it out once (x128_tile_plan
// below, with the functions above) and the workgroup fetches it with one scalar load instead of walking the thresholds itself.
struct alignas(32) X128Tile {
  unsigned char cnt[4];        // K segments walked per side (x128_segs - tsk); a side with 0 is passed over
  int block;                   // the block (row-major, as in BlockSide / FemDev::sides)
  unsigned offA[4];            // first walked segment of the side's [z_f, 1/s_f] block: bytes from the system's interface vector
  unsigned long long offB[4];  // ... of the side's segment-major table: bytes from FemDev::Gs
  unsigned long long live[4];  // per wave column: bit h = the column multiplies half h of the walk (0: it has no vertex at all);
                               // all ones where the walk is too long for the mask (64 segments or more)
  int row, col;                // the tile's first vertex: mesh row and column, 1-based (iv, jv0); FLAT: 0-based
};
static_assert(sizeof(X128Tile) == 96, "three 32-byte scalar loads");

template <bool FLAT>
inline X128Tile x128_tile_plan(int n1, int N, int block, int tile, const BlockSide& sd) {
  X128Tile t{};
  t.block = block;
  const int nct = (n1 + 127) / 128;
  t.row = FLAT ? 128 * tile / n1 : tile / nct + 1;
  t.col = FLAT ? 128 * tile % n1 : 128 * (tile % nct) + 1;
  int tsk[4], wsk[4][4], nseg = 0;
  bool has[4];
  for (int wc = 0; wc < 4; ++wc) has[wc] = x128_skip_counts<FLAT>(n1, N, tile, wc, sd.s[0], sd.s[1], sd.s[2], sd.s[3], tsk, wsk[wc]);
  const size_t seg_stride = size_t(n1) * n1 * 64;  // bytes between the K segments of a table
  for (int s = 0; s < 4; ++s) {
    t.cnt[s] = (unsigned char)(x128_segs(sd.s[s]) - tsk[s]);
    t.offA[s] = unsigned(sd.s[s].off) * 8u + unsigned(tsk[s]) * 64u;
    t.offB[s] = size_t(sd.s[s].gseg) * 8 + size_t(tsk[s]) * seg_stride;
    nseg += t.cnt[s];
  }
  for (int wc = 0; wc < 4; ++wc) {
    unsigned long long m = 0;
    int h0 = 0;
    for (int s = 0; s < 4 && nseg < 64; ++s) {  // the side's halves h0 .. h0 + cnt - 1 hold its segments tsk .. : live from wsk on
      m |= ((1ull << t.cnt[s]) - (1ull << (wsk[wc][s] - tsk[s]))) << h0;
      h0 += t.cnt[s];
    }
    t.live[wc] = nseg >= 64 ? ~0ull : has[wc] ? m : 0ull;
  }
  return t;
}

// what rom_fem_create reads from the environment for the planner (ROMHC_NO_PREELIM, ROMHC_NO_COMPRESS,
// ROMHC_NO_LOWRANK_EXT, ROMHC_NO_EXT_LR, ROMHC_VERBOSE, ROMHC_COMPRESS_TOL, ROMHC_NO_EXT_TRUNC)
struct FemSwitches {
  bool no_preelim, no_compress, no_lowrank_ext, no_ext_lr, verbose;
  long double compress_tol;
  bool no_ext_trunc;  // keep the pivoted basis of the reduced unknowns and walk every K segment of the extension everywhere
};

struct FemPlan {
  // dimensions (named as in rom_fem; npre_all counts every closed-form edge, pre_edges only those recovered node by node)
  int nrb, ncb, N, n1, n1p, nr, nc, nG, nGp, nGa, nred, ncross, xb0, T, nslots, n_all_edges, npre_all;
  int64_t dim;
  int spos0, nsc, npairs = 0, wp0[5] = {}, ncoef, ncf, nctask, ndg, ndi, n_edges, lr_nch;
  bool fused1 = false;
  // one vector per device table (rom_fem::d_<name>, FemDev)
  std::vector<double> pool, pool_acc, dmat, Ptab, Bt, Qp, rho, Wz, g_red, vecs, cm;
  std::vector<GenTerm> terms;
  std::vector<TileDesc> desc;
  std::vector<int> alist, aoff, pairs, wmeta, s1_items, s1_citems, dweight, ditem_group, ditem_k, kmax, item_group, item_k, item_cf;
  std::vector<int> ctask, xred, scb, kptr, kpair, colptr, colrow, colti, vmap, scat, lr_blocks, gen_blocks, epos;
  std::vector<DenseGroup> dgroups;
  std::vector<RhsTerm> rhs_terms;
  std::vector<PreEdge> pre_edges;
  std::vector<ExpEdge> exps;
  std::vector<CoefGroup> groups;
  std::vector<BlockSide> sides;
  // k_extend128's per-tile records, [position in lr_blocks][tile], for its two tilings: mesh rows (n1 * ceil(n1 / 128) tiles
  // per block) and FLAT (ceil(n1^2 / 128))
  std::vector<X128Tile> x128_row, x128_flat;
  // inputs of the device-side builds: G + off = A0 * Bh^T (rows x rp), Gs + gsoff = k_repack_table(G + goff); A0 from Qp, rho
  // Rotated basis (entry non-empty): Bh[k] is zero in front of mode entry[k]; rows at distance d from the side need only
  // the K segments from seg0[d] on (thr: the same as thresholds, ExtSide::thr) -- the others hold columns bounded by `cut`
  // and are zeroed in G (k_mask_table)
  struct GemmG {
    std::vector<double> Bh; long long off; int rp;
    int r = 0;
    std::vector<int> entry, seg0;
    std::vector<long double> W;  // the rotated basis itself (n1 x r; host copy for the checks, not uploaded)
    unsigned short thr[8] = {0xffff, 0xffff, 0xffff, 0xffff, 0xffff, 0xffff, 0xffff, 0xffff};
    double cut = 0;
  };
  struct Repack { long long goff, gsoff; int ld, nseg, orient; };
  std::vector<GemmG> gemm_G;
  std::vector<Repack> repacks;
  long long gtotal = 0, gstotal = 0;
  // host copies and the work accounting (per snapshot solve)
  std::vector<int> ranks, slot_of, diag_slot;
  double ext_flops = 0, flops_solve = 0, bytes_solve = 0;
};

// ROM_OK, or ROM_ERR_INVALID with the reason in *error.  Host only: no HIP call, no environment variable.
int rom_fem_plan(int nrb, int ncb, int N, const FemSwitches& sw, FemPlan* out, std::string* error);
