// Stand-alone check of the host planner (romhighcontrast_amd/csrc/rom_fem_plan.hip), built with -fsanitize=address,undefined
// by tests/test_fem_plan_host.py: plans the geometries of tests/sweep_truth.py::CASES and 3x3 / N = 24 under every planner
// switch, each twice, and checks what the sweep kernels assume about the tables.  Exit status 0 = no violation.
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

template <class T>
static bool same_bytes(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

// planning is deterministic whatever the host threads do: every vector of two plans has the same bytes
static void check_same(const FemPlan& a, const FemPlan& b) {
#define SAME(field) CHECK(same_bytes(a.field, b.field))
  SAME(pool); SAME(terms); SAME(desc); SAME(alist); SAME(aoff); SAME(pairs); SAME(pool_acc); SAME(wmeta); SAME(s1_items);
  SAME(s1_citems); SAME(dgroups); SAME(dweight); SAME(ditem_group); SAME(ditem_k); SAME(dmat); SAME(Ptab); SAME(Bt); SAME(Qp);
  SAME(rho); SAME(kmax); SAME(Wz); SAME(g_red); SAME(vecs); SAME(rhs_terms); SAME(pre_edges); SAME(exps); SAME(groups); SAME(cm);
  SAME(item_group); SAME(item_k); SAME(item_cf); SAME(ctask); SAME(xred); SAME(scb); SAME(kptr); SAME(kpair); SAME(colptr);
  SAME(colrow); SAME(colti); SAME(sides); SAME(vmap); SAME(scat); SAME(lr_blocks); SAME(gen_blocks); SAME(epos); SAME(ranks);
  SAME(slot_of); SAME(diag_slot);
#undef SAME
  CHECK(a.gemm_G.size() == b.gemm_G.size() && a.gtotal == b.gtotal && a.gstotal == b.gstotal);
  for (size_t i = 0; i < a.gemm_G.size() && i < b.gemm_G.size(); ++i)
    CHECK(same_bytes(a.gemm_G[i].Bh, b.gemm_G[i].Bh) && a.gemm_G[i].off == b.gemm_G[i].off && a.gemm_G[i].rp == b.gemm_G[i].rp);
  CHECK(a.repacks.size() == b.repacks.size());
  CHECK(a.nGp == b.nGp && a.nslots == b.nslots && a.fused1 == b.fused1 && a.flops_solve == b.flops_solve);
}

// the parts of the interface vector are pairwise disjoint and lie in [0, nGp)
static void check_layout(const FemPlan& p) {
  std::vector<int> used(size_t(p.nGp > 0 ? p.nGp : 0), 0);
  int outside = 0;
  auto claim = [&](int pos, int len) {
    for (int i = pos; i < pos + len; ++i) {
      if (i < 0 || i >= p.nGp) ++outside;
      else ++used[i];
    }
  };
  CHECK(p.exps.size() >= p.ranks.size());
  for (size_t i = 0; i < p.ranks.size() && i < p.exps.size(); ++i) {  // active edges, in elimination order: [zpos, zpos + rk)
    claim(p.exps[i].zpos, p.ranks[i]);
    CHECK(p.exps[i].zpos + p.ranks[i] <= p.nred);
  }
  CHECK(int(p.xred.size()) == p.ncross);
  for (int x : p.xred) {
    claim(x, 1);
    CHECK(x < p.nred);
  }
  for (int e = 0; e < p.n_all_edges; ++e) claim(p.nGa + e * p.n1p, p.n1p);  // nodal blocks
  for (const ExpEdge& ee : p.exps) CHECK(ee.npos >= p.nGa && ee.npos < p.xb0 && (ee.npos - p.nGa) % p.n1p == 0);
  for (const PreEdge& pe : p.pre_edges) CHECK(pe.pos >= p.nGa && pe.pos < p.xb0 && (pe.pos - p.nGa) % p.n1p == 0);
  CHECK(p.xb0 == p.nGa + p.n_all_edges * p.n1p);
  if (p.ncross > 0) claim(p.xb0, (p.ncross + TB - 1) / TB * TB);  // cross block
  for (const CoefGroup& g : p.groups) claim(g.cpos, g.w);         // [z, 1/s] blocks of the compressed edges
  claim(p.spos0, (p.nsc + BK - 1) / BK * BK);                     // scalar block
  CHECK(p.spos0 + (p.nsc + BK - 1) / BK * BK == p.nGp);
  CHECK(outside == 0);
  int overlaps = 0;
  for (int u : used) overlaps += u > 1;
  CHECK(overlaps == 0);
  CHECK(p.nGa == p.T * TB);
  CHECK(p.nred <= p.nGa);
  // vmap: injective on its entries >= 0, which are exactly the interface degrees of freedom
  CHECK(int(p.vmap.size()) == (p.nGp > 1 ? p.nGp : 1));
  std::vector<int> seen;
  for (int v : p.vmap)
    if (v >= 0) {
      CHECK(v < p.dim);
      seen.push_back(v);
    }
  CHECK(int(seen.size()) == p.n_all_edges * p.n1 + p.ncross && int(seen.size()) == p.nG);
  std::vector<char> hit(size_t(p.dim), 0);
  int twice = 0;
  for (int v : seen)
    if (v < p.dim) twice += hit[v]++ ? 1 : 0;
  CHECK(twice == 0);
  for (int s : p.scat) CHECK(s >= 0 && s < p.nGp && p.vmap[s] >= 0);
}

// what the kernels assume about the assembly encodings and the symbolic factorisation
static void check_kernel_assumptions(const FemPlan& p) {
  CHECK(int(p.desc.size()) == p.nslots && int(p.kptr.size()) == p.nslots + 1);
  CHECK(int(p.aoff.size()) == 4 * p.nslots + 1);
  for (size_t i = 0; i + 1 < p.aoff.size(); ++i) CHECK(p.aoff[i + 1] >= p.aoff[i] && (p.aoff[i + 1] - p.aoff[i]) % 8 == 0);
  CHECK(!p.aoff.empty() && p.alist.size() == 2 * (size_t(p.aoff.back()) + 128));
  for (size_t i = p.alist.size() >= 256 ? p.alist.size() - 256 : 0; i < p.alist.size(); i += 2)
    CHECK(p.alist[i] == 0 && p.alist[i + 1] == 1 << 17);
  for (size_t i = 0; i < p.alist.size(); i += 2)  // a piece is a kilobyte of the pool
    CHECK((p.alist[i + 1] >> 17) || (p.alist[i] >= 0 && size_t(p.alist[i]) + 7 * TB + 16 <= p.pool.size()));
  CHECK(p.npairs % 64 == 0 && p.pairs.size() == 2 * (size_t(p.npairs) + 64));
  if (p.fused1) {
    CHECK(p.T == 1 && p.nslots == 1);
    for (int w = 0; w < 4; ++w) CHECK(p.wp0[w + 1] >= p.wp0[w] && (p.wp0[w + 1] - p.wp0[w]) % PAIR_RING == 0);
    CHECK(p.wmeta.size() == size_t(p.wp0[4]) + 128);
    CHECK(p.pool_acc.size() == 256 * size_t(p.wp0[4]) + 2 * PAIR_RING * 256);
    CHECK(p.desc[0].t1 - p.desc[0].t0 < COEF_MAX && p.ndg <= DENSE_GROUPS_MAX && p.ndi <= 64 && p.rhs_terms.size() <= 64);
  }
  CHECK(p.pool.size() % 4096 == 0);
  for (const GenTerm& g : p.terms) {
    CHECK(0 <= g.r_lo && g.r_lo <= g.r_hi && g.r_hi <= 64 && 0 <= g.c_lo && g.c_lo <= g.c_hi && g.c_hi <= 64);
    CHECK(g.tab >= 0 && size_t(g.tab) < p.pool.size() / 4096);
  }
  for (const TileDesc& d : p.desc) CHECK(0 <= d.t0 && d.t0 <= d.t1 && size_t(d.t1) <= p.terms.size() && d.tj <= d.ti && d.ti < p.T);
  for (int k : p.kpair) CHECK(k >= 0 && k < p.nslots);
  CHECK(p.kpair.size() == 2 * size_t(p.kptr.empty() ? 0 : p.kptr.back()));
  CHECK(p.lr_blocks.size() + p.gen_blocks.size() == size_t(p.nrb * p.ncb) && int(p.sides.size()) == p.nrb * p.ncb);
  for (const FemPlan::GemmG& g : p.gemm_G)
    CHECK(g.off >= 0 && g.off + (long long)p.n1 * p.n1 * g.rp <= p.gtotal && g.Bh.size() == size_t(g.rp) * p.n1p);
  for (const FemPlan::Repack& r : p.repacks)
    CHECK(r.goff >= 0 && r.goff < p.gtotal && r.gsoff >= 0 && r.gsoff + (long long)r.nseg * p.n1 * p.n1 * 8 <= p.gstotal && 8 * r.nseg <= r.ld);
}

static void plan_case(const char* name, int nrb, int ncb, int N, FemSwitches sw) {
  current = name;
  FemPlan a, b;
  std::string err;
  if (rom_fem_plan(nrb, ncb, N, sw, &a, &err) != ROM_OK || rom_fem_plan(nrb, ncb, N, sw, &b, &err) != ROM_OK) {
    ++failures;
    fprintf(stderr, "%s: rom_fem_plan failed: %s\n", name, err.c_str());
    return;
  }
  check_same(a, b);
  check_layout(a);
  check_kernel_assumptions(a);
  printf("%-26s nGp %5d  T %2d  slots %3d  terms %4zu  fused1 %d  lr %2zu  gen %2zu\n", name, a.nGp, a.T, a.nslots, a.terms.size(),
         int(a.fused1), a.lr_blocks.size(), a.gen_blocks.size());
}

int main() {
  const FemSwitches plain{false, false, false, false, false, 1e-14L};
  const struct { int nrb, ncb, N; } geo[] = {{2, 2, 2},  {2, 2, 3}, {2, 2, 16}, {2, 2, 65}, {2, 2, 66}, {2, 2, 128},
                                             {1, 1, 8},  {1, 2, 128}, {1, 3, 7}, {2, 3, 40}, {3, 3, 24}, {5, 4, 33},
                                             {2, 2, 171}, {3, 3, 140}, {2, 2, 250}, {1, 2, 257}};
  for (const auto& g : geo) {
    char name[64];
    snprintf(name, sizeof(name), "%dx%d-N%d", g.nrb, g.ncb, g.N);
    plan_case(name, g.nrb, g.ncb, g.N, plain);
  }
  FemSwitches sw = plain;
  sw.no_preelim = true;
  plan_case("3x3-N24 no_preelim", 3, 3, 24, sw);
  sw = plain;
  sw.no_compress = true;
  plan_case("3x3-N24 no_compress", 3, 3, 24, sw);
  sw = plain;
  sw.no_lowrank_ext = true;
  plan_case("3x3-N24 no_lowrank_ext", 3, 3, 24, sw);
  sw = plain;
  sw.compress_tol = 1e-10L;
  plan_case("3x3-N24 compress_tol 1e-10", 3, 3, 24, sw);
  if (failures) fprintf(stderr, "%d violation(s)\n", failures);
  return failures ? 1 : 0;
}
