// The host side of the map entry points on the CPU (run by tests/test_map_host.py under AddressSanitizer and UBSan):
// the block checks of csrc/rom_block.h, message for message and with the extents that wrap a size_t, and the host arithmetic
// of rom_poly_fit (csrc/rom_poly_host.h) on integer inputs whose exact answers are representable.  The exponent rows and the
// factor tables are printed for the pytest side to compare; everything else is checked here.  Exit status 0 and an empty
// stderr mean that every check passed.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "rom_block.h"
#include "rom_poly_host.h"

static char g_error[512];
void rom_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof g_error, fmt, ap);
  va_end(ap);
}

static int g_failed = 0;
#define EXPECT(cond, ...)                 \
  do {                                    \
    if (!(cond)) {                        \
      printf("FAILED %s:%d: ", __FILE__, __LINE__); \
      printf(__VA_ARGS__);                \
      printf("\n");                       \
      ++g_failed;                         \
    }                                     \
  } while (0)

// ---- block checks -----------------------------------------------------------------------------------------------------------
static const RomBlockNames XN = {"X", "ldx", "m"};

static void accepted(const char* what, size_t n, size_t off, int64_t ld, int cols, int64_t rows) {
  g_error[0] = 0;
  const int s = rom_check_block("t", XN, n, off, ld, cols, rows);
  EXPECT(s == ROM_OK && g_error[0] == 0, "%s: status %d, message '%s'", what, s, g_error);
}

static void refused(const char* what, const std::string& want, size_t n, size_t off, int64_t ld, int cols, int64_t rows) {
  g_error[0] = 0;
  const int s = rom_check_block("t", XN, n, off, ld, cols, rows);
  EXPECT(s == ROM_ERR_INVALID && want == g_error, "%s: status %d, message '%s', expected '%s'", what, s, g_error, want.c_str());
}

static std::string holds(size_t n, long long rows, int cols, size_t off, long long ld) {
  char b[256];
  snprintf(b, sizeof b, "t: X holds %zu doubles, %lld rows of %d at offset %zu with stride %lld need more", n, rows, cols, off, ld);
  return b;
}

static void check_blocks() {
  // the two messages as the GPU tests read them
  refused("stride", "t: ldx = 1 < m = 2", 400, 0, 1, 2, 50);
  refused("short", "t: X holds 400 doubles, 50 rows of 2 at offset 7 with stride 8 need more", 400, 7, 8, 2, 50);
  // a block that ends on the buffer's last double, and the same with one double fewer
  accepted("exact end", 7 + 49 * 8 + 2, 7, 8, 2, 50);
  refused("one short", holds(7 + 49 * 8 + 1, 50, 2, 7, 8), 7 + 49 * 8 + 1, 7, 8, 2, 50);
  accepted("packed", 100, 0, 2, 2, 50);
  refused("packed, offset 1", holds(100, 50, 2, 1, 2), 100, 1, 2, 2, 50);
  // the stride rule holds for one row too
  refused("ld = cols - 1", "t: ldx = 4 < m = 5", 400, 0, 4, 5, 10);
  refused("one row, ld < cols", "t: ldx = 1 < m = 2", 400, 0, 1, 2, 1);
  accepted("one row", 9, 7, 2, 2, 1);
  // extents that wrap a size_t: (rows - 1) ld, + cols, + off
  const int64_t two40 = int64_t(1) << 40, big = INT64_MAX;
  refused("2^40 rows of stride 2^24 + 1", holds(400, two40, 1, 0, (1 << 24) + 1), 400, 0, (1 << 24) + 1, 1, two40);
  refused("3 rows of stride 2^63 - 1", holds(400, 3, 2, 0, big), 400, 0, big, 2, 3);
  refused("5 rows of stride 2^62 (the product is 2^64)", holds(400, 5, 2, 0, int64_t(1) << 62), 400, 0, int64_t(1) << 62, 2, 5);
  refused("2^40 rows of stride 2^62", holds(400, two40, 1, 0, int64_t(1) << 62), 400, 0, int64_t(1) << 62, 1, two40);
  refused("offset SIZE_MAX - 1", holds(400, 1, 2, SIZE_MAX - 1, 2), 400, SIZE_MAX - 1, 2, 2, 1);
  refused("offset SIZE_MAX - 1, 50 rows", holds(400, 50, 2, SIZE_MAX - 1, 8), 400, SIZE_MAX - 1, 8, 2, 50);
  EXPECT(rom_block_span(50, 8, 2) == 394 && rom_block_span(1, 8, 2) == 2, "span");
  EXPECT(rom_block_span(3, big, 2) == SIZE_MAX && rom_block_span(0, 8, 2) == SIZE_MAX, "span of a block that does not exist");

  // overlap of [a, a + na) and [b, b + nb)
  static double buf[64];
  EXPECT(!rom_blocks_overlap(buf, 10, buf + 10, 10) && !rom_blocks_overlap(buf + 10, 10, buf, 10), "adjacent ranges");
  EXPECT(rom_blocks_overlap(buf, 11, buf + 10, 10) && rom_blocks_overlap(buf + 10, 10, buf, 11), "ranges that share one double");
  EXPECT(rom_blocks_overlap(buf, 40, buf + 10, 5) && rom_blocks_overlap(buf + 10, 5, buf, 40), "nested ranges");

  g_error[0] = 0;
  EXPECT(rom_check_rows("t", 1) == ROM_OK && rom_check_rows("t", int64_t(1) << 40) == ROM_OK && g_error[0] == 0, "rows accepted");
  EXPECT(rom_check_rows("t", 0) == ROM_ERR_INVALID && !strcmp(g_error, "t: M = 0 rows, at least 1"), "rows: '%s'", g_error);
  EXPECT(rom_check_rows("t", (int64_t(1) << 40) + 1) == ROM_ERR_INVALID, "rows above 2^40");
}

// ---- terms and factor tables ------------------------------------------------------------------------------------------------
static void print_terms(int m, int d, bool table) {
  std::vector<int> powers;
  poly_powers(m, d, powers);
  const long long P = poly_count(m, d);
  EXPECT(powers.size() == size_t(P) * m, "poly_powers(%d, %d): %zu entries, P = %lld", m, d, powers.size(), P);
  printf("POWERS %d %d %lld", m, d, P);
  for (int v : powers) printf(" %d", v);
  printf("\n");
  if (!table) return;
  const std::vector<unsigned char> tab = poly_factor_table(powers, m, d, int(P));
  EXPECT(tab.size() == size_t(PL_MAX) * PL_DMAX, "table size %zu", tab.size());
  printf("TABLE %d %d", m, d);
  for (unsigned char v : tab) printf(" %d", int(v));
  printf("\n");
}

// ---- Cholesky, the solve, the update ---------------------------------------------------------------------------------------
static int small(unsigned& s, int lo, int hi) {   // a fixed sequence of small integers
  s = s * 1664525u + 1013904223u;
  return lo + int((s >> 16) % unsigned(hi - lo + 1));
}

// G = L0 L0^T of order P (L0: small integers, a power-of-two diagonal); the factor of the leading rank x rank block must be
// that block of L0, and with B = G Z (Z integer) W = T^T Z for an integer T, exactly
static void check_solve(int P, int rank, int q) {
  unsigned s = 12345u + P;
  std::vector<double> L0(size_t(P) * P, 0.0), G(size_t(P) * P, 0.0), Z(size_t(rank) * q), B(size_t(rank) * q, 0.0), T(size_t(P) * P);
  for (int i = 0; i < P; ++i) {
    for (int j = 0; j < i; ++j) L0[size_t(i) * P + j] = small(s, -3, 3);
    L0[size_t(i) * P + i] = double(1 << small(s, 0, 2));
  }
  for (int i = 0; i < P; ++i)
    for (int j = 0; j < P; ++j)
      for (int k = 0; k < P; ++k) G[size_t(i) * P + j] += L0[size_t(i) * P + k] * L0[size_t(j) * P + k];
  for (double& v : Z) v = small(s, -5, 5);
  for (double& v : T) v = small(s, -4, 4);
  for (int i = 0; i < rank; ++i)
    for (int c = 0; c < q; ++c)
      for (int k = 0; k < rank; ++k) B[size_t(i) * q + c] += G[size_t(i) * P + k] * Z[size_t(k) * q + c];
  std::vector<long double> L;
  EXPECT(host_cholesky(L, G.data(), P, rank), "order %d, rank %d: not positive definite", P, rank);
  bool same = L.size() == size_t(rank) * rank;
  for (int i = 0; i < rank && same; ++i)
    for (int j = 0; j < rank; ++j) same = same && L[size_t(i) * rank + j] == (long double)L0[size_t(i) * P + j];
  EXPECT(same, "order %d, rank %d: the factor is not L0", P, rank);
  std::vector<long double> z(P);
  std::vector<double> W(size_t(q) * P, -1.0);
  poly_solve_w(P, q, rank, L, B.data(), T.data(), z.data(), W.data());
  bool exact = true;
  for (int c = 0; c < q; ++c)
    for (int t = 0; t < P; ++t) {
      double want = 0.0;
      for (int i = 0; i < rank; ++i) want += T[size_t(i) * P + t] * Z[size_t(i) * q + c];
      exact = exact && W[size_t(c) * P + t] == want;
    }
  EXPECT(exact, "order %d, rank %d: W is not T^T Z", P, rank);
}

static void check_not_positive() {
  std::vector<long double> L;
  const double zero_pivot[4] = {1.0, 1.0, 1.0, 1.0};       // second pivot 1 - 1 = 0
  const double negative_pivot[4] = {1.0, 2.0, 2.0, 1.0};   // second pivot 1 - 4 < 0
  const double nan_pivot[1] = {__builtin_nan("")};
  EXPECT(!host_cholesky(L, zero_pivot, 2, 2), "a zero pivot was accepted");
  EXPECT(!host_cholesky(L, negative_pivot, 2, 2), "a negative pivot was accepted");
  EXPECT(!host_cholesky(L, nan_pivot, 1, 1), "a NaN pivot was accepted");
}

static void check_update(int P, int rank, int r2) {
  unsigned s = 999u + P;
  std::vector<double> That(size_t(P) * P), T(size_t(P) * P), Tn(size_t(P) * P, -1.0);
  for (double& v : That) v = small(s, -6, 6);
  for (double& v : T) v = small(s, -6, 6);
  poly_update_t(P, rank, r2, That.data(), T.data(), Tn.data());
  bool exact = true;
  for (int i = 0; i < P; ++i)
    for (int c = 0; c < P; ++c) {
      double want = 0.0;
      if (i < r2)
        for (int r = 0; r < rank; ++r) want += That[size_t(i) * P + r] * T[size_t(r) * P + c];
      exact = exact && Tn[size_t(i) * P + c] == want && (i < r2 || !std::signbit(Tn[size_t(i) * P + c]));
    }
  EXPECT(exact, "update P = %d, rank %d, r2 = %d", P, rank, r2);
}

static void check_first_transform() {
  const double lam[3] = {4.0, 1.0, 0.0}, D[3] = {0.5, 2.0, 8.0};
  const double That[9] = {1.0, 0.0, 0.0, 3.0, 0.0, 5.0, 7.0, 7.0, 7.0};   // column 1 is zero in the first two rows
  double T[9], ratio = -1.0, dropped[3] = {-1.0, -1.0, -1.0};
  const int rank = poly_first_transform(3, lam, D, That, T, &ratio, dropped);
  bool scaled = true;
  for (int i = 0; i < 3; ++i)
    for (int c = 0; c < 3; ++c) scaled = scaled && T[i * 3 + c] == That[i * 3 + c] * D[c];
  EXPECT(rank == 2 && ratio == 0.25 && scaled, "first transform: rank %d, ratio %g", rank, ratio);
  EXPECT(dropped[0] == 0.0 && dropped[1] == 1.0 && dropped[2] == 0.0, "dropped flags %g %g %g", dropped[0], dropped[1], dropped[2]);
  const double none[3] = {0.0, -1.0, __builtin_nan("")};
  EXPECT(poly_first_transform(3, none, D, That, T, &ratio, dropped) == 0 && ratio == 0.25, "no positive pivot");
}

int main() {
  check_blocks();
  const int cases[6][2] = {{1, 1}, {2, 3}, {3, 2}, {16, 1}, {2, 8}, {4, 4}};
  for (const auto& c : cases) print_terms(c[0], c[1], (c[0] == 2 && c[1] == 3) || (c[0] == 3 && c[1] == 2));
  int d5 = 1;
  while (poly_count(5, d5 + 1) <= PL_MAX) ++d5;
  print_terms(5, d5, false);
  EXPECT(poly_count(16, 1) == 17 && poly_count(2, 8) == 45 && poly_count(4, 4) == 70 && poly_count(16, 8) == 735471, "poly_count");
  for (int P : {1, 2, 7, 96}) check_solve(P, P, P == 96 ? 5 : 3);
  check_solve(7, 4, 3);     // the leading block only
  check_solve(96, 61, 2);
  check_not_positive();
  check_update(7, 5, 3);
  check_update(96, 96, 95);
  check_update(2, 2, 1);
  check_first_transform();
  if (g_failed) {
    printf("FAILED %d checks\n", g_failed);
    return 1;
  }
  printf("OK\n");
  return 0;
}
