// The small dense layer (rom_small_dense.hip) as its callers and its own kernels share it: the entry points, the limits of
// the routes, and the rules that the three Jacobi implementations (kb_small_eig, jacobi32_run, jacobi_grid) must state in the
// same words -- each written once here, for host and device alike.  (internal; no HIP call: compiles with a plain C++
// compiler, which is how tests/c_abi/small_dense_host_check.cpp checks it)
#pragma once
#include <cmath>
#include <cstddef>

#ifdef __HIPCC__
#define SD_HD __host__ __device__
#else
#define SD_HD
#endif

struct rom_ctx;

// ---- entry points and limits ----------------------------------------------------------------------------------------
enum { SE_EIG = 0, SE_WHITEN = 1, SE_LOWDIN = 2 };
// one workgroup with the matrix in LDS up to SE_LDS_MAX; SE_MAX: the limit of the public entries and of the modes per request
constexpr int SE_LDS_MAX = 96, SE_MAX = 1024;
// (the grid-wide Jacobi takes larger orders -- four buffers of n^2 doubles, n launches per sweep: ~1 s at 2048 -- as the
// whole-matrix fallback of the POD's Gram route)
constexpr int SE_GRID_MAX = 2048;
// A (n x n, symmetrised on entry) = sum_i lam_i q_i q_i^T: lam descending; T by mode (rows q_i^T, whitening rows, symmetric
// inverse square root).  tight (with gram_like): rotate down to |a_pq| <= 16 eps sqrt(a_pp a_qq) instead of n eps
int romb_small_eig(rom_ctx* ctx, int n, const double* A, int lda, double* lam, double* T, int ldt, int mode, double rel_tol,
                   bool gram_like = true, bool tight = false);
// rank-revealing whitening by pivoted Cholesky, n <= SE_LDS_MAX
int romb_pivchol_whiten(rom_ctx* ctx, int n, const double* A, int lda, double* lam, double* T, int ldt, double rel_tol);

// ---- the rules of the Jacobi sweeps ---------------------------------------------------------------------------------
// A rotation is applied when a_pq^2 > tol2 |a_pp a_qq|, |a_pq| > floor_abs and a_pq^2 > tol2 nu_p^2 nu_q^2.  gram_like:
// 0 general symmetric, 1 Gram-like, 2 Gram-like with the threshold 16 eps instead of max(n, 8) eps (romb_small_eig's
// `tight`: rom_pca_tall's own convergence test must lie above what the sweeps leave behind).  dmax = max |a_ii|.
SD_HD inline double jacobi_tol2(int n, int gram_like) {
  const double tol = (gram_like == 2 ? 16.0 : double(n > 8 ? n : 8)) * 1.1e-16;
  return tol * tol;
}
SD_HD inline double jacobi_floor(double dmax) { return fmax(1e-300, 1e-40 * dmax); }

// nu_i^2 at the start, the rounding noise of a_ii: |a_ii| for a Gram matrix of explicit rows, max |a_ii| for a general one
SD_HD inline double jacobi_nu2_init(int gram_like, double aii, double dmax) { return gram_like ? fabs(aii) : dmax; }

// The pair (p < q) of slot k in round r of the round-robin tournament over the even order ne = nm1 + 1, r < nm1, k < ne / 2:
// index ne - 1 stays in slot 0, the others move around it.  The slots of a round are disjoint and cover every index; the
// nm1 rounds of a sweep meet every pair once.
struct JacobiPair {
  int p, q;
};
SD_HD inline JacobiPair jacobi_pair(int k, int r, int nm1) {
  int p = r, q = nm1;
  if (k) {
    p = r + k;
    if (p >= nm1) p -= nm1;
    q = r - k;
    if (q < 0) q += nm1;
    if (p > q) { const int x = p; p = q; q = x; }
  }
  return {p, q};
}

// A <- J^T A J on the 2 x 2 block rows (p_k, q_k) x columns (p_l, q_l): B <- R_k B R_l^T, R = (c -s; s c).  The results go
// out through references on purpose: the device compiler fuses each difference and sum of two products into one product and
// one fma, WHICH product it keeps depends on the form the expressions reach it in, and a version that returned the four
// values in a struct fused the other way in jacobi32_run and kb_jgrid_round -- different last bits, one more sweep.
SD_HD inline void jacobi_block_update(double ck, double sk, double cl, double sl, double b00, double b01, double b10, double b11,
                                      double& o00, double& o01, double& o10, double& o11) {
  const double r00 = ck * b00 - sk * b10, r01 = ck * b01 - sk * b11;   // rows
  const double r10 = sk * b00 + ck * b10, r11 = sk * b01 + ck * b11;
  o00 = cl * r00 - sl * r01;                                           // columns
  o01 = sl * r00 + cl * r01;
  o10 = cl * r10 - sl * r11;
  o11 = sl * r10 + cl * r11;
}

// position of ev[i] in the descending order of ev[0..n) (stable: ties by index)
SD_HD inline int rank_descending(const double* ev, int n, int i) {
  int rank = 0;
  const double v = ev[i];
  for (int j = 0; j < n; ++j) rank += (ev[j] > v || (ev[j] == v && j < i)) ? 1 : 0;
  return rank;
}

// ---- dynamic LDS of the one-workgroup kernels: byte offsets of the arrays and the size of the launch, from n -----------
// kb_small_eig: matrix and eigenvector rows (n rows of ld = n | 1), then per slot of a round (half = ceil(n / 2)) cosine, sine
// and pair, per index eigenvalue, noise level and rank, the partials of a reduction and the sweep's flag
struct SmallEigLds {
  unsigned As, Vt, cs, sn, ev, nu2, red, pp, qq, perm, flag, bytes;
  SD_HD explicit SmallEigLds(int n) {
    const int half = (n + (n & 1)) / 2, mat = n * (n | 1) * 8;
    As = 0, Vt = As + mat;                                                       // doubles: two n x ld matrices,
    cs = Vt + mat, sn = cs + 8 * half;                                           // [half] per slot,
    ev = sn + 8 * half, nu2 = ev + 8 * n, red = nu2 + 8 * n;                     // [n] per index, [8] per wave
    pp = red + 8 * 8, qq = pp + 4 * half, perm = qq + 4 * half, flag = perm + 4 * n;   // ints: [half], [half], [n], [1]
    bytes = flag + 4 + 4 + 16;   // (rounded up past the flag: the size this launch has always had)
  }
};

// kb_pivchol_whiten: working matrix and L^-1 (n rows of ld = n | 1), the four waves' pivot candidates (value, index), the
// pivot order
struct PivcholLds {
  unsigned As, Li, red, redi, perm, bytes;
  SD_HD explicit PivcholLds(int n) {
    const int mat = n * (n | 1) * 8;
    As = 0, Li = As + mat, red = Li + mat;               // doubles: two n x ld matrices, [4]
    redi = red + 8 * 4, perm = redi + 4 * 4;             // ints: [4], [n]
    bytes = perm + 4 * n + 16;
  }
};
