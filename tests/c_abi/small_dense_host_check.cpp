// The host-visible rules of the small dense layer on the CPU (run by tests/test_small_dense_layout_host.py under
// AddressSanitizer and UBSan): csrc/rom_small_dense_host.h compiled with a plain C++ compiler.  The LDS layouts of
// kb_small_eig and kb_pivchol_whiten against the byte counts their launchers used to compute by hand; the round-robin pair of
// a slot against the modular spelling kb_small_eig used to have; the rotation thresholds against the literal expression.
// Exit status 0, an empty stderr and a last line "OK" mean that every check passed.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "rom_small_dense_host.h"

static int g_failed = 0;
#define EXPECT(cond, ...)                           \
  do {                                              \
    if (!(cond)) {                                  \
      printf("FAILED %s:%d: ", __FILE__, __LINE__); \
      printf(__VA_ARGS__);                          \
      printf("\n");                                 \
      ++g_failed;                                   \
    }                                               \
  } while (0)

// ---- layouts ----------------------------------------------------------------------------------------------------------
struct Arr {
  const char* name;
  size_t off, bytes;
  bool is_double;
};

// the arrays in any order: inside [0, total), pairwise disjoint, doubles on 8-byte boundaries (ints on 4)
static void check_arrays(const char* who, int n, std::vector<Arr> a, size_t total) {
  std::sort(a.begin(), a.end(), [](const Arr& x, const Arr& y) { return x.off < y.off; });
  for (size_t i = 0; i < a.size(); ++i) {
    EXPECT(a[i].off % (a[i].is_double ? 8 : 4) == 0, "%s n = %d: %s at %zu is misaligned", who, n, a[i].name, a[i].off);
    const size_t end = a[i].off + a[i].bytes, next = i + 1 < a.size() ? a[i + 1].off : total;
    EXPECT(end <= next, "%s n = %d: %s [%zu, %zu) runs into %s at %zu", who, n, a[i].name, a[i].off, end,
           i + 1 < a.size() ? a[i + 1].name : "the end", next);
  }
}

static void check_layouts() {
  for (int n = 1; n <= 96; ++n) {
    const size_t ld = n | 1, half = (n + (n & 1)) / 2, N = n;
    {
      const SmallEigLds L(n);
      // the launcher's formula before the layout struct
      const size_t vec = (2 * half + 2 * N + 8) * sizeof(double) + (2 * half + N + 2) * sizeof(int);
      const size_t want = vec + 16 + 2 * N * ld * sizeof(double);
      EXPECT(L.bytes == want, "SmallEigLds(%d).bytes = %u, the launch had %zu", n, L.bytes, want);
      check_arrays("SmallEigLds", n,
                   {{"As", L.As, N * ld * 8, true},  {"Vt", L.Vt, N * ld * 8, true}, {"cs", L.cs, half * 8, true},
                    {"sn", L.sn, half * 8, true},    {"ev", L.ev, N * 8, true},      {"nu2", L.nu2, N * 8, true},
                    {"red", L.red, 8 * 8, true},     {"pp", L.pp, half * 4, false},  {"qq", L.qq, half * 4, false},
                    {"perm", L.perm, N * 4, false},  {"flag", L.flag, 4, false}},
                   L.bytes);
    }
    {
      const PivcholLds L(n);
      const size_t want = 2 * N * ld * sizeof(double) + 4 * sizeof(double) + (4 + N) * sizeof(int) + 16;
      EXPECT(L.bytes == want, "PivcholLds(%d).bytes = %u, the launch had %zu", n, L.bytes, want);
      check_arrays("PivcholLds", n,
                   {{"As", L.As, N * ld * 8, true},
                    {"Li", L.Li, N * ld * 8, true},
                    {"red", L.red, 4 * 8, true},
                    {"redi", L.redi, 4 * 4, false},
                    {"perm", L.perm, N * 4, false}},
                   L.bytes);
    }
  }
  // what the launchers opt in to
  EXPECT(SmallEigLds(96).bytes <= 160 * 1024, "SmallEigLds(96).bytes = %u", SmallEigLds(96).bytes);
  EXPECT(PivcholLds(96).bytes <= 160 * 1024 - 256, "PivcholLds(96).bytes = %u", PivcholLds(96).bytes);
  EXPECT(SE_LDS_MAX == 96 && SE_MAX == 1024 && SE_GRID_MAX == 2048, "the limits of the routes moved");
}

// ---- round-robin pairs ------------------------------------------------------------------------------------------------
static void check_pairs(int ne) {
  const int nm1 = ne - 1, half = ne / 2;
  std::vector<int> met(size_t(ne) * ne, 0);
  for (int r = 0; r < nm1; ++r) {
    std::vector<int> used(ne, 0);
    for (int k = 0; k < half; ++k) {
      const JacobiPair pr = jacobi_pair(k, r, nm1);
      // kb_small_eig's earlier spelling
      int p = k == 0 ? ne - 1 : (r + k) % (ne - 1), q = k == 0 ? r : (r - k + ne - 1) % (ne - 1);
      if (p > q) std::swap(p, q);
      EXPECT(pr.p == p && pr.q == q, "ne = %d round %d slot %d: (%d, %d), the modular form gives (%d, %d)", ne, r, k, pr.p, pr.q, p, q);
      if (k == 0) EXPECT(pr.p == r && pr.q == ne - 1, "ne = %d round %d: slot 0 holds (%d, %d)", ne, r, pr.p, pr.q);
      if (!(0 <= pr.p && pr.p < pr.q && pr.q < ne)) {
        EXPECT(false, "ne = %d round %d slot %d: (%d, %d) is no sorted pair below ne", ne, r, k, pr.p, pr.q);
        continue;
      }
      used[pr.p] += 1;
      used[pr.q] += 1;
      met[size_t(pr.p) * ne + pr.q] += 1;
    }
    for (int i = 0; i < ne; ++i) EXPECT(used[i] == 1, "ne = %d round %d: index %d is in %d pairs", ne, r, i, used[i]);
  }
  long long pairs = 0;
  for (int p = 0; p < ne; ++p)
    for (int q = p + 1; q < ne; ++q) {
      EXPECT(met[size_t(p) * ne + q] == 1, "ne = %d: a sweep meets (%d, %d) %d times", ne, p, q, met[size_t(p) * ne + q]);
      pairs += met[size_t(p) * ne + q];
    }
  EXPECT(pairs == (long long)ne * (ne - 1) / 2, "ne = %d: %lld pairs in a sweep", ne, pairs);
}

// ---- thresholds, noise levels, ranking --------------------------------------------------------------------------------
static void check_rules() {
  const int orders[] = {1, 8, 9, 96, 2048};
  const double dmaxs[] = {0.0, 1e-280, 1.0, 3.5e7, 1e300};
  for (int n : orders)
    for (int gram_like = 0; gram_like <= 2; ++gram_like)
      for (double dmax : dmaxs) {
        const double tol2 = jacobi_tol2(n, gram_like), floor_abs = jacobi_floor(dmax);
        const double tol = (gram_like == 2 ? 16.0 : double(n > 8 ? n : 8)) * 1.1e-16;
        EXPECT(tol2 == tol * tol, "jacobi_tol2(%d, %d) = %a, literally %a", n, gram_like, tol2, tol * tol);
        EXPECT(floor_abs == fmax(1e-300, 1e-40 * dmax), "jacobi_floor(%g) = %a", dmax, floor_abs);
      }
  EXPECT(jacobi_tol2(1, 0) == jacobi_tol2(8, 1) && jacobi_tol2(9, 1) > jacobi_tol2(8, 1),
         "the threshold grows with n from 8 on");
  EXPECT(jacobi_tol2(2048, 2) == jacobi_tol2(1, 2), "the tight threshold does not depend on n");
  EXPECT(jacobi_nu2_init(0, -3.0, 7.0) == 7.0 && jacobi_nu2_init(1, -3.0, 7.0) == 3.0 && jacobi_nu2_init(2, -3.0, 7.0) == 3.0,
         "jacobi_nu2_init: max |a_ii| for a general matrix, |a_ii| for a Gram-like one");
  // descending, ties by index: the order of a stable sort
  const std::vector<double> ev = {2.0, 5.0, 2.0, -1.0, 5.0, 0.0, 2.0};
  std::vector<int> perm(ev.size(), -1), want(ev.size());
  for (size_t i = 0; i < ev.size(); ++i) {
    perm[rank_descending(ev.data(), int(ev.size()), int(i))] = int(i);
    want[i] = int(i);
  }
  std::stable_sort(want.begin(), want.end(), [&](int a, int b) { return ev[a] > ev[b]; });
  EXPECT(perm == want, "rank_descending is not the stable descending order");
  // R_k B R_l^T: identities leave the block alone; a quarter turn on the rows swaps them with a sign
  double o00, o01, o10, o11;
  jacobi_block_update(1.0, 0.0, 1.0, 0.0, 1.0, 2.0, 3.0, 4.0, o00, o01, o10, o11);
  EXPECT(o00 == 1.0 && o01 == 2.0 && o10 == 3.0 && o11 == 4.0, "jacobi_block_update with (c, s) = (1, 0) twice");
  jacobi_block_update(0.0, 1.0, 1.0, 0.0, 1.0, 2.0, 3.0, 4.0, o00, o01, o10, o11);
  EXPECT(o00 == -3.0 && o01 == -4.0 && o10 == 1.0 && o11 == 2.0, "jacobi_block_update with a quarter turn of the rows");
  jacobi_block_update(1.0, 0.0, 0.0, 1.0, 1.0, 2.0, 3.0, 4.0, o00, o01, o10, o11);
  EXPECT(o00 == -2.0 && o01 == 1.0 && o10 == -4.0 && o11 == 3.0, "jacobi_block_update with a quarter turn of the columns");
}

int main() {
  check_layouts();
  for (int ne = 2; ne <= 98; ne += 2) check_pairs(ne);
  check_pairs(2048);
  check_rules();
  printf("LAYOUT small_eig %u pivchol %u\n", SmallEigLds(96).bytes, PivcholLds(96).bytes);
  if (g_failed) {
    printf("%d checks FAILED\n", g_failed);
    return 1;
  }
  printf("OK\n");
  return 0;
}
