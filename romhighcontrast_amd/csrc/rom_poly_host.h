// The host arithmetic of rom_poly_fit / rom_poly_terms (rom_poly.hip): the terms of the feature space and their factor table,
// and the small dense steps between the passes, in extended precision.  Host only: no HIP type, compiles with a plain C++
// compiler.  Matrices are row-major; T, T^ and G have P columns, the factor L of a rank x rank block has rank.  (internal)
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

namespace {

constexpr int PL_MAX = 96;       // largest P (T + the slabs in 160 KB of LDS)
constexpr int PL_MMAX = 16, PL_DMAX = 8;
constexpr int PL_NOFAC = 255;

// the exponent rows of PolynomialFeatures(d).powers_: graded, combinations_with_replacement(range(m), k) in lexicographic order
long long poly_count(int m, int d) {
  long long p = 1;
  for (int k = 1; k <= d; ++k) p = p * (m + k) / k;   // C(m + k, k): exact at every step
  return p;
}

void poly_powers(int m, int d, std::vector<int>& powers) {
  powers.clear();
  std::vector<int> comb;
  for (int deg = 0; deg <= d; ++deg) {
    comb.assign(deg, 0);
    for (;;) {
      const size_t at = powers.size();
      powers.resize(at + m, 0);
      for (int v : comb) powers[at + v] += 1;
      int pos = deg - 1;
      while (pos >= 0 && comb[pos] == m - 1) --pos;
      if (pos < 0) break;
      const int v = comb[pos] + 1;
      for (int r = pos; r < deg; ++r) comb[r] = v;
    }
  }
}

// factor table of the P terms: row p lists the entries j d + alpha_j - 1 of the Legendre table whose product is term p, in
// input order, padded with PL_NOFAC to PL_DMAX; PL_MAX rows
std::vector<unsigned char> poly_factor_table(const std::vector<int>& powers, int m, int d, int P) {
  std::vector<unsigned char> tab(size_t(PL_MAX) * PL_DMAX, (unsigned char)PL_NOFAC);
  for (int p = 0; p < P; ++p) {
    int nf = 0;
    for (int j = 0; j < m; ++j)
      if (powers[size_t(p) * m + j] > 0) tab[size_t(p) * PL_DMAX + nf++] = (unsigned char)(j * d + powers[size_t(p) * m + j] - 1);
  }
  return tab;
}

// L L^T = A (r x r, row-major with stride ld, lower triangle read) in extended precision; false if a pivot is not positive
bool host_cholesky(std::vector<long double>& L, const double* A, int ld, int r) {
  L.assign(size_t(r) * r, 0.0L);
  for (int i = 0; i < r; ++i)
    for (int j = 0; j <= i; ++j) {
      long double s = A[size_t(i) * ld + j];
      for (int q = 0; q < j; ++q) s -= L[size_t(i) * r + q] * L[size_t(j) * r + q];
      if (i == j) {
        if (!(s > 0.0L)) return false;
        L[size_t(i) * r + i] = sqrtl(s);
      } else {
        L[size_t(i) * r + j] = s / L[size_t(j) * r + j];
      }
    }
  return true;
}

// The first pass's transform from the pivoted whitening T^ of the column-normalised Gram matrix (pivots lam, scalings D):
// T = T^ D, the rank (positive pivots), the ratio of the last pivot to the first, and dropped[c] = 1 for a term whose column of
// T^ is zero -- it never became a pivot.  A rank of 0 leaves T, the ratio and the flags alone.
int poly_first_transform(int P, const double* lam, const double* D, const double* That, double* T, double* piv_ratio, double* dropped) {
  int rank = 0;
  for (int i = 0; i < P; ++i) rank += lam[i] > 0.0 ? 1 : 0;
  if (rank < 1) return 0;
  *piv_ratio = lam[rank - 1] / lam[0];
  for (int i = 0; i < P; ++i)
    for (int c = 0; c < P; ++c) T[size_t(i) * P + c] = That[size_t(i) * P + c] * D[c];
  for (int c = 0; c < P; ++c) {
    bool used = false;
    for (int i = 0; i < rank && !used; ++i) used = That[size_t(i) * P + c] != 0.0;
    dropped[c] = used ? 0.0 : 1.0;
  }
  return rank;
}

// W = T^T G^-1 B on the leading rank x rank block: L the factor of G (host_cholesky), B rank x q, W q x P; z: rank scratch
void poly_solve_w(int P, int q, int rank, const std::vector<long double>& L, const double* B, const double* T, long double* z, double* W) {
  for (int c = 0; c < q; ++c) {
    for (int i = 0; i < rank; ++i) {
      long double s = B[size_t(i) * q + c];
      for (int r = 0; r < i; ++r) s -= L[size_t(i) * rank + r] * z[r];
      z[i] = s / L[size_t(i) * rank + i];
    }
    for (int i = rank - 1; i >= 0; --i) {
      long double s = z[i];
      for (int r = i + 1; r < rank; ++r) s -= L[size_t(r) * rank + i] * z[r];
      z[i] = s / L[size_t(i) * rank + i];
    }
    for (int t = 0; t < P; ++t) {
      long double s = 0.0L;
      for (int i = 0; i < rank; ++i) s += (long double)T[size_t(i) * P + t] * z[i];
      W[size_t(c) * P + t] = double(s);
    }
  }
}

// Tnew = T^ T: the leading r2 rows of T^ times the leading rank rows of T; the rows from r2 on are zero
void poly_update_t(int P, int rank, int r2, const double* That, const double* T, double* Tnew) {
  for (int i = 0; i < P; ++i)
    for (int c = 0; c < P; ++c) {
      long double s = 0.0L;
      if (i < r2)
        for (int r = 0; r < rank; ++r) s += (long double)That[size_t(i) * P + r] * T[size_t(r) * P + c];
      Tnew[size_t(i) * P + c] = double(s);
    }
}

}  // namespace
