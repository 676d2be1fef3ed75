// Stand-alone check of the extension truncation of the host planner (romhighcontrast_amd/csrc/rom_fem_plan.hip), built with
// -fsanitize=address,undefined by tests/test_ext_trunc_host.py.  Plans 2x2 at N = 40, 64, 128 and 3x3 at N = 64 and checks
// the rotated basis, the echelon form of the stored sine coefficients, the distance thresholds and the bound of every table
// entry the mask zeroes; prints one "hash <geometry> <FNV-1a>" line per geometry for the plan with no_ext_trunc, which the
// Python side compares with the hashes recorded from the planner before the truncation existed.  Exit status 0 = no violation.
#include <cmath>
#include <cstdint>
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

// FNV-1a over every table and scalar of a plan in the form it had before the truncation (ExtSide field by field: the struct
// has grown since)
static uint64_t fnv(uint64_t h, const void* p, size_t n) {
  const unsigned char* b = static_cast<const unsigned char*>(p);
  for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
  return h;
}
template <class T>
static uint64_t fnv_vec(uint64_t h, const std::vector<T>& v) {
  const size_t n = v.size();
  h = fnv(h, &n, sizeof(n));
  return v.empty() ? h : fnv(h, v.data(), n * sizeof(T));
}
static uint64_t plan_hash(const FemPlan& p) {
  uint64_t h = 14695981039346656037ull;
#define HV(field) h = fnv_vec(h, p.field)
  HV(pool); HV(terms); HV(desc); HV(alist); HV(aoff); HV(pairs); HV(pool_acc); HV(wmeta); HV(s1_items);
  HV(s1_citems); HV(dgroups); HV(dweight); HV(ditem_group); HV(ditem_k); HV(dmat); HV(Ptab); HV(Bt); HV(Qp);
  HV(rho); HV(kmax); HV(Wz); HV(g_red); HV(vecs); HV(rhs_terms); HV(pre_edges); HV(exps); HV(groups); HV(cm);
  HV(item_group); HV(item_k); HV(item_cf); HV(ctask); HV(xred); HV(scb); HV(kptr); HV(kpair); HV(colptr);
  HV(colrow); HV(colti); HV(vmap); HV(scat); HV(lr_blocks); HV(gen_blocks); HV(epos); HV(ranks);
  HV(slot_of); HV(diag_slot);
#undef HV
  for (const BlockSide& b : p.sides)
    for (const ExtSide& s : b.s) {
      const int f[8] = {s.mode, s.off, s.nch, s.r, s.gtab, s.gseg, s.b0, s.b1};
      h = fnv(h, f, sizeof(f));
    }
  for (const FemPlan::GemmG& g : p.gemm_G) {
    h = fnv_vec(h, g.Bh);
    h = fnv(h, &g.off, sizeof(g.off));
    h = fnv(h, &g.rp, sizeof(g.rp));
  }
  for (const FemPlan::Repack& r : p.repacks) {
    const long long f[5] = {r.goff, r.gsoff, r.ld, r.nseg, r.orient};
    h = fnv(h, f, sizeof(f));
  }
  const long long sc[] = {p.nrb, p.ncb, p.N, p.n1, p.n1p, p.nr, p.nc, p.nG, p.nGp, p.nGa, p.nred, p.ncross, p.xb0, p.T, p.nslots,
                          p.n_all_edges, p.npre_all, p.dim, p.spos0, p.nsc, p.npairs, p.wp0[0], p.wp0[1], p.wp0[2], p.wp0[3], p.wp0[4],
                          p.ncoef, p.ncf, p.nctask, p.ndg, p.ndi, p.n_edges, p.lr_nch, p.fused1, p.gtotal, p.gstotal};
  h = fnv(h, sc, sizeof(sc));
  const double fl[] = {p.ext_flops, p.flops_solve, p.bytes_solve};
  return fnv(h, fl, sizeof(fl));
}

// rho_m(d) = sinh((N - d) phi_m) / sinh(N phi_m), cosh phi_m = 1 + lam_m / 2, in long double (m 0-based, d = 0 .. N)
static std::vector<long double> rho_table(int N) {
  const int n1 = N - 1;
  const long double PI = acosl(-1.0L);
  std::vector<long double> rho(size_t(n1) * (N + 1));
  for (int m = 0; m < n1; ++m) {
    const long double lam = 2.0L - 2.0L * cosl(PI * (m + 1) / N), phi = acoshl(1.0L + lam / 2.0L);
    const long double den = -expm1l(-2.0L * N * phi);
    for (int d = 0; d <= N; ++d) rho[size_t(m) * (N + 1) + d] = expl(-phi * d) * (-expm1l(-2.0L * (N - d) * phi)) / den;
  }
  return rho;
}

static int skipped(const unsigned short* thr, int d) {
  int n = 0;
  for (int j = 0; j < EXT_THRESHOLDS; ++j) n += d >= int(thr[j]);
  return n;
}

static void check_truncated(const FemPlan& p) {
  const int n1 = p.n1, N = p.N, n1p = p.n1p;
  const std::vector<long double> rho = rho_table(N);
  int with_fewer = 0, rotated = 0;
  double full_flops = 0;
  for (const FemPlan::GemmG& g : p.gemm_G) {
    const int r = g.r, nseg = (r + 1 + 7) / 8;
    CHECK(int(g.seg0.size()) == N + 1);
    if (g.entry.empty()) continue;
    ++rotated;
    CHECK(int(g.entry.size()) == r && g.W.size() == size_t(n1) * r && g.cut > 0);
    // W^T W = I: the basis is orthonormal to a few roundings of the long double it is built in -- far inside the fp64
    // rounding (1.1e-16) of the tables made from it
    long double worst = 0;
    for (int a = 0; a < r; ++a)
      for (int b = 0; b <= a; ++b) {
        long double s = 0;
        for (int i = 0; i < n1; ++i) s += g.W[size_t(i) * r + a] * g.W[size_t(i) * r + b];
        worst = std::max(worst, fabsl(s - (a == b ? 1.0L : 0.0L)));
      }
    CHECK(worst < 1e-16L);
    // echelon form, droppable directions first: the entry modes descend, the stored coefficients in front of them are zeros
    int nonzero_below = 0;
    for (int k = 0; k < r; ++k) {
      if (k > 0) CHECK(g.entry[k] < g.entry[k - 1]);
      CHECK(g.entry[k] >= 0 && g.entry[k] < n1);
      for (int m = 0; m < g.entry[k] && m < n1; ++m) nonzero_below += g.Bh[size_t(k) * n1p + m] != 0.0;
      if (g.entry[k] < n1) CHECK(g.Bh[size_t(k) * n1p + g.entry[k]] != 0.0);
    }
    CHECK(nonzero_below == 0);
    // thresholds: ascending, the same function of the distance as seg0, the last segment (1/s) always walked
    for (int j = 0; j + 1 < EXT_THRESHOLDS; ++j) CHECK(g.thr[j] <= g.thr[j + 1]);
    for (int d = 1; d <= n1; ++d) {
      CHECK(g.seg0[d] == skipped(g.thr, d) && g.seg0[d] >= 0 && g.seg0[d] <= nseg - 1);
      if (d > 1) CHECK(g.seg0[d] >= g.seg0[d - 1]);
      with_fewer += g.seg0[d] > 0;
    }
    // every entry the mask zeroes -- row at distance d, column k < 8 seg0[d] -- is bounded by the cut
    long double top = 0;
    int above = 0;
    for (int k = 0; k < r; ++k) {
      int dmin = n1 + 1;  // first distance at which column k is masked
      for (int d = n1; d >= 1; --d)
        if (k < 8 * g.seg0[d]) dmin = d;
      long double b1 = 0;
      for (int m = 0; m < n1; ++m) b1 += rho[size_t(m) * (N + 1) + 1] * fabsl((long double)g.Bh[size_t(k) * n1p + m]);
      top = std::max(top, b1);
      for (int d = dmin; d <= n1; ++d) {
        long double b = 0;
        for (int m = 0; m < n1; ++m) b += rho[size_t(m) * (N + 1) + d] * fabsl((long double)g.Bh[size_t(k) * n1p + m]);
        above += !(b < (long double)g.cut * (1.0L + 1e-12L));
      }
    }
    CHECK(above == 0);
    CHECK(fabsl((long double)g.cut - EXT_TRUNC_CUT * top) <= 1e-12L * (long double)g.cut);
  }
  CHECK(rotated > 0 && rotated == int(p.gemm_G.size()));
  CHECK(with_fewer > 0);  // (otherwise the GPU tests of the skipping prove nothing)
  for (const BlockSide& b : p.sides)
    for (const ExtSide& s : b.s) {
      if (s.mode != 2) continue;
      const FemPlan::GemmG* g = nullptr;
      for (const FemPlan::GemmG& cand : p.gemm_G)
        if (cand.off == s.gtab) g = &cand;
      CHECK(g != nullptr);
      if (!g) continue;
      CHECK(memcmp(s.thr, g->thr, sizeof(s.thr)) == 0 && s.r == g->r);
      full_flops += 2.0 * n1 * double(n1) * (s.r + 1);
    }
  CHECK(p.n_edges > 0 || p.ext_flops < full_flops);
}

static void check_plain(const char* name, const FemPlan& p) {
  for (const FemPlan::GemmG& g : p.gemm_G) {
    CHECK(g.entry.empty());
    for (int j = 0; j < 8; ++j) CHECK(g.thr[j] == 0xffff);
    for (int s : g.seg0) CHECK(s == 0);
  }
  for (const BlockSide& b : p.sides)
    for (const ExtSide& s : b.s)
      if (s.mode == 2)
        for (int j = 0; j < 8; ++j) CHECK(s.thr[j] == 0xffff);
  printf("hash %s %016llx\n", name, (unsigned long long)plan_hash(p));
}

int main() {
  const struct { int nrb, ncb, N; } geo[] = {{2, 2, 40}, {2, 2, 64}, {2, 2, 128}, {3, 3, 64}};
  for (const auto& g : geo) {
    char name[64];
    snprintf(name, sizeof(name), "%dx%d-N%d", g.nrb, g.ncb, g.N);
    current = name;
    FemSwitches sw{false, false, false, false, false, 1e-14L};
    FemPlan cut, plain;
    std::string err;
    if (rom_fem_plan(g.nrb, g.ncb, g.N, sw, &cut, &err) != ROM_OK) {
      ++failures;
      fprintf(stderr, "%s: rom_fem_plan failed: %s\n", name, err.c_str());
      continue;
    }
    check_truncated(cut);
    sw.no_ext_trunc = true;
    if (rom_fem_plan(g.nrb, g.ncb, g.N, sw, &plain, &err) != ROM_OK) {
      ++failures;
      fprintf(stderr, "%s: rom_fem_plan (no_ext_trunc) failed: %s\n", name, err.c_str());
      continue;
    }
    check_plain(name, plain);
    CHECK(cut.ext_flops <= plain.ext_flops && cut.nGp >= plain.nGp && cut.nred == plain.nred && cut.T == plain.T);
  }
  if (failures) fprintf(stderr, "%d violation(s)\n", failures);
  return failures ? 1 : 0;
}
