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
constexpr int X128_BLOCKS = 16;     // blocks whose descriptors one k_extend128 launch takes by value (X128Args, rom_fem_dev.h)

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
