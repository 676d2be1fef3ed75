// The basis stage behind the C-ABI: single-call operations for the projectors, the greedy and the POD.
//
// Reference counterparts: project_solutions (src/lib/SolutionsManagers.py:108-139), generate_fm_solutions (:88-106),
// orthonormalize_base (src/lib/ReducedBasis.py:18-21), ReducedBasisGreedy.build (:112-139), the PCA fit inside
// ReducedBasisPCA.build (:189-200).  Everything here runs on the device: small dense problems (symmetric eigenproblems
// of at most a few hundred unknowns, whitening) go to rom_small_dense.hip, selections
// (argmax of the greedy) stay in device memory, norms feed the next kernel through device scalars.  The host sees a
// status word at the end of a call -- and, in the POD, the handful of spectrum values its acceptance decisions need.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rom_ops.h"

#include "rom_basis_int.h"

// =====================================================================================================================
// small elementwise / indexing kernels
// =====================================================================================================================
__global__ void kb_fill(double* p, size_t n, double v) {
  for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) p[i] = v;
}

int romb_fill(rom_ctx* ctx, double* p, size_t n, double v) {
  if (n == 0) return ROM_OK;
  if (v == 0.0 && !std::signbit(v)) {  // (+0.0 only: -0.0 == 0.0, but its bits are not all zero)
    ROM_HIP(hipMemsetAsync(p, 0, n * sizeof(double), ctx->stream));
    return ROM_OK;
  }
  kb_fill<<<unsigned(std::min<size_t>((n + 255) / 256, 2048)), 256, 0, ctx->stream>>>(p, n, v);
  ROM_HIP(hipGetLastError());
  return ROM_OK;
}

__global__ void kb_identity(double* __restrict__ E, int k) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < k * k) E[i] = (i / k == i % k) ? 1.0 : 0.0;
}

int romb_onehot(rom_ctx* ctx, int k, double* out) {
  kb_identity<<<blocks_for(size_t(k) * k), 256, 0, ctx->stream>>>(out, k);
  ROM_HIP(hipGetLastError());
  return ROM_OK;
}

// B_total = h^2 in every inner entry (:177-185)
int romb_load_vector(rom_fem* f, double* out) { return romb_fill(f->ctx, out, size_t(f->dim), 1.0 / (double(f->N) * f->N)); }

__global__ void kb_ints_to_doubles(const int* __restrict__ src, double* __restrict__ dst, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = double(src[i]);
}

// ---- fixed-order sums of per-chunk partials (no floating-point atomics: the same bits on every call) -----------------
// Part[chunk] is ppad x ldp: a lower triangle in its leading columns and a rectangle from column ppad on.
// G[r][c] (P x P, with G != NULL) = sum over the chunks, in chunk order, of Part[chunk][max(r, c)][min(r, c)]: the reduction
// and the mirror in one; B[r][c0 + c] (P x q) = the same sum of Part[chunk][r][ppad + c], c < qg
__global__ void kb_partials_reduce(const double* __restrict__ Part, int chunks, int ppad, int ldp, int P, int qg,
                                   double* __restrict__ G, double* __restrict__ B, int q, int c0) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int ng = G ? P * P : 0;
  if (idx >= ng + P * qg) return;
  const size_t step = size_t(ppad) * ldp;
  const double* p;
  double* out;
  if (idx < ng) {
    const int r = idx / P, c = idx - r * P;
    p = Part + size_t(max(r, c)) * ldp + min(r, c);
    out = G + idx;
  } else {
    const int e = idx - ng, r = e / qg, c = e - r * qg;
    p = Part + size_t(r) * ldp + ppad + c;
    out = B + size_t(r) * q + c0 + c;
  }
  double s = 0.0;
  for (int ch = 0; ch < chunks; ++ch) s += p[ch * step];
  *out = s;
}

// out[j] = (sum over the chunks, in chunk order, of part[chunk][j]) / divisor, j < n (a plain sum: divisor = 1, exact)
__global__ void kb_partials_colsum(const double* __restrict__ part, int chunks, int n, double divisor, double* __restrict__ out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  double s = 0.0;
  for (int ch = 0; ch < chunks; ++ch) s += part[size_t(ch) * n + j];
  out[j] = s / divisor;
}

// counter-based generator (splitmix64 of seed and index): the same numbers whatever the launch shape
__device__ inline unsigned long long mix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
__device__ inline double u01(unsigned long long h) { return (double(h >> 11) + 0.5) * (1.0 / 9007199254740992.0); }

// gaussian != 0: standard normal (Box-Muller); else uniform in (-0.5, 0.5)
__global__ void kb_fill_random(double* p, size_t n, unsigned long long seed, int gaussian) {
  for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
    const unsigned long long h1 = mix64(seed * 0xD1342543DE82EF95ull + 2 * i), h2 = mix64(seed * 0xD1342543DE82EF95ull + 2 * i + 1);
    p[i] = gaussian ? sqrt(-2.0 * log(u01(h1))) * cos(6.283185307179586 * u01(h2)) : u01(h1) - 0.5;
  }
}

int romb_fill_random(rom_ctx* ctx, double* p, size_t n, unsigned long long seed, bool gaussian) {
  if (n == 0) return ROM_OK;
  kb_fill_random<<<unsigned(std::min<size_t>((n + 255) / 256, 4096)), 256, 0, ctx->stream>>>(p, n, seed, gaussian ? 1 : 0);
  ROM_HIP(hipGetLastError());
  return ROM_OK;
}

// out[i, :] = x[i, :] + s * f[i] * y[i, :]    (rows x dim; x may be null = 0)
__global__ void kb_rows_axpy(double* __restrict__ out, const double* __restrict__ x, const double* __restrict__ y,
                             const double* __restrict__ f, double s, long long dim) {
  const double a = s * f[blockIdx.y];
  const long long o = blockIdx.y * dim;
  for (long long j = blockIdx.x * (long long)blockDim.x + threadIdx.x; j < dim; j += (long long)gridDim.x * blockDim.x)
    out[o + j] = (x ? x[o + j] : 0.0) + a * y[o + j];
}

__global__ void kb_transpose(double* __restrict__ dst, long long ldd, const double* __restrict__ src, long long lds,
                             int rows, int cols) {
  const long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (idx >= (long long)rows * cols) return;
  const int r = int(idx / cols), c = int(idx % cols);
  dst[c * ldd + r] = src[r * lds + c];
}

int romb_transpose(rom_ctx* ctx, double* dst, long long ldd, const double* src, long long lds, int rows, int cols) {
  if (rows <= 0 || cols <= 0) return ROM_OK;
  kb_transpose<<<unsigned(((long long)rows * cols + 255) / 256), 256, 0, ctx->stream>>>(dst, ldd, src, lds, rows, cols);
  ROM_HIP(hipGetLastError());
  return ROM_OK;
}

// =====================================================================================================================
// orthonormalisation helpers (rows of a (b, dim) block)
// =====================================================================================================================
// X (b x dim) <- T X with T from the b x b Gram matrix X X^T: SE_WHITEN (rank revealing: dependent directions become
// zero rows) or SE_LOWDIN (rows stay individually close to what they were).  `rounds` repetitions (the second one
// removes what the squared condition number of the first Gram matrix left).  Y is a scratch block of the same size; the
// result ends in X.
int romb_gram_transform(rom_ctx* ctx, double* X, double* Y, int b, int64_t dim, int mode, double rel_tol, int rounds) {
  if (b <= 0) return ROM_OK;
  Tmp G, lam, T;
  ROM_TRY(G.get(ctx, size_t(b) * b));
  ROM_TRY(lam.get(ctx, b));
  ROM_TRY(T.get(ctx, size_t(b) * b));
  for (int r = 0; r < rounds; ++r) {
    ROM_TRY(rom_launch_gram(ctx, b, dim, X, dim, G, b));
    if (mode == SE_WHITEN && b <= SE_LDS_MAX) ROM_TRY(romb_pivchol_whiten(ctx, b, G, b, lam, T, b, r == 0 ? rel_tol : 1e-8));
    else ROM_TRY(romb_small_eig(ctx, b, G, b, lam, T, b, mode, r == 0 ? rel_tol : 1e-8));
    ROM_TRY(rom_launch_gemm_nn(ctx, b, dim, b, 1.0, T, b, X, dim, 0.0, Y, dim));
    ROM_HIP(hipMemcpyAsync(X, Y, size_t(b) * dim * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  }
  return ROM_OK;
}

// rows V[found : found + take] <- orthonormal and orthogonal to the orthonormal rows V[0 : found]: block Gram-Schmidt
// against the old rows (twice), symmetric orthonormalisation among the new ones
int romb_orthonormalize_against(rom_ctx* ctx, double* V, int found, int take, int64_t dim) {
  if (take <= 0) return ROM_OK;
  double* Vn = V + size_t(found) * dim;
  if (found > 0) {
    Tmp C;
    ROM_TRY(C.get(ctx, size_t(take) * found));
    for (int r = 0; r < 2; ++r) {
      ROM_TRY(rom_launch_gemm_nt(ctx, take, found, dim, 1.0, Vn, dim, V, dim, 0.0, C, found, "gemm_nt"));
      ROM_TRY(rom_launch_gemm_nn(ctx, take, dim, found, -1.0, C, found, V, dim, 1.0, Vn, dim));
    }
  }
  Tmp Y;
  ROM_TRY(Y.get(ctx, size_t(take) * dim));
  // (the new rows are orthonormal to ~1e-6 at worst -- lifted Gram modes -- and the symmetric orthonormalisation is second
  // order in that defect: one round)
  return romb_gram_transform(ctx, Vn, Y, take, dim, SE_LOWDIN, 1e-30, 1);
}

// kb_cgs_finish: v <- v / ||v||_2 (norm squared given on the device), zero row if the norm underflows or if what
// Gram-Schmidt left of the row is at roundoff of the row it was (nrm2[1]: its norm squared before; a dependent row --
// a1_dead in the Euclidean norm)
__global__ void kb_scale_by_inv_norm(double* __restrict__ v, long long dim, const double* __restrict__ nrm2) {
  const double n2 = nrm2[0];
  const double a = (!a1_dead(n2, nrm2[1]) && sqrt(n2) > 1e-300) ? 1.0 / sqrt(n2) : 0.0;
  for (long long j = blockIdx.x * (long long)blockDim.x + threadIdx.x; j < dim; j += (long long)gridDim.x * blockDim.x) v[j] *= a;
}

// orthonormalize_base (src/lib/ReducedBasis.py:18-21): rows of X -> Euclidean-orthonormal rows spanning the same NESTED
// subspaces (thin QR of X^T up to the sign of each row), by re-orthogonalised classical Gram-Schmidt; every step is a
// device operation, the norms never leave the device.
extern "C" int rom_orthonormalize_rows(rom_ctx* ctx, rom_buf* X, int64_t x_row0, int n, int64_t dim, rom_buf* Q, int64_t q_row0) {
  ROM_CHECK(ctx && X && Q, "rom_orthonormalize_rows: null argument");
  ROM_CHECK(n >= 0 && dim >= 1 && x_row0 >= 0 && q_row0 >= 0, "rom_orthonormalize_rows: bad sizes");
  ROM_CHECK(size_t(x_row0 + n) * dim <= X->n && size_t(q_row0 + n) * dim <= Q->n, "rom_orthonormalize_rows: rows out of range");
  if (n == 0) return ROM_OK;
  double* q = Q->p + q_row0 * dim;
  if (q != X->p + x_row0 * dim)
    ROM_HIP(hipMemcpyAsync(q, X->p + x_row0 * dim, size_t(n) * dim * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  Tmp h, nrm;
  ROM_TRY(h.get(ctx, n));
  ROM_TRY(nrm.get(ctx, 2));
  const unsigned grid = vector_grid(dim);
  for (int j = 0; j < n; ++j) {
    double* v = q + size_t(j) * dim;
    ROM_TRY(rom_launch_l2norm(ctx, v, 1, dim, nrm.p() + 1, false));  // the row as given: what "dependent" is measured against
    for (int r = 0; r < 2 && j > 0; ++r) {  // "twice is enough"
      ROM_TRY(rom_launch_gemm_nt(ctx, j, 1, dim, 1.0, q, dim, v, dim, 0.0, h, 1, "gemm_nt"));   // h = Q[:j] v
      ROM_TRY(rom_launch_gemm_nn(ctx, 1, dim, j, -1.0, h, j, q, dim, 1.0, v, dim));              // v -= h^T Q[:j]
    }
    ROM_TRY(rom_launch_l2norm(ctx, v, 1, dim, nrm, false));
    kb_scale_by_inv_norm<<<grid, 256, 0, ctx->stream>>>(v, dim, nrm);
    ROM_HIP(hipGetLastError());
  }
  return ROM_OK;
}

// nearly orthonormal rows -> orthonormal rows, each as close as possible to what it was (symmetric / Loewdin
// orthonormalisation: V <- (V V^T)^(-1/2) V, two rounds): the clean-up of modes that were expanded from another basis
extern "C" int rom_symmetric_orthonormalize(rom_ctx* ctx, rom_buf* V, int64_t v_row0, int n, int64_t dim) {
  ROM_CHECK(ctx && V, "rom_symmetric_orthonormalize: null argument");
  ROM_CHECK(n >= 0 && n <= SE_MAX && dim >= 1 && v_row0 >= 0 && size_t(v_row0 + n) * dim <= V->n, "rom_symmetric_orthonormalize: bad sizes");
  if (n == 0) return ROM_OK;
  Tmp Y;
  ROM_TRY(Y.get(ctx, size_t(n) * dim));
  return romb_gram_transform(ctx, V->p + v_row0 * dim, Y, n, dim, SE_LOWDIN, 1e-30, 2);
}

// rows V[found : found + rest] <- pseudo-random directions (seeded: deterministic) made orthonormal and orthogonal to the
// orthonormal rows V[0 : found]: how a mode request beyond what the data determine is completed (LAPACK and scikit-learn
// return SOME orthonormal directions there too)
extern "C" int rom_complete_orthonormal(rom_ctx* ctx, rom_buf* V, int64_t v_row0, int found, int rest, int64_t dim) {
  ROM_CHECK(ctx && V, "rom_complete_orthonormal: null argument");
  ROM_CHECK(found >= 0 && rest >= 0 && dim >= 1 && v_row0 >= 0 && size_t(v_row0 + found + rest) * dim <= V->n,
            "rom_complete_orthonormal: bad sizes");
  ROM_CHECK(int64_t(found) + rest <= dim && rest <= SE_MAX, "rom_complete_orthonormal: more rows than the space has dimensions");
  if (rest == 0) return ROM_OK;
  double* v = V->p + v_row0 * dim;
  ROM_TRY(romb_fill_random(ctx, v + size_t(found) * dim, size_t(rest) * dim, 0xc0de0000ull + unsigned(found), false));
  return romb_orthonormalize_against(ctx, v, found, rest, dim);
}

// =====================================================================================================================
// projectors
// =====================================================================================================================
// project_solutions (src/lib/SolutionsManagers.py:108-139): OUT_i = c_i C with (C A_1 C^T) c_i = C A_1 u_i
extern "C" int rom_project_h10(rom_fem* f, rom_buf* U, int64_t u_row0, int M, rom_buf* C, int64_t c_row0, int n,
                               rom_buf* OUT, int64_t out_row0) {
  ROM_CHECK(f && U && OUT && (C || n == 0), "rom_project_h10: null argument");
  ROM_CHECK(M >= 0 && n >= 0 && u_row0 >= 0 && c_row0 >= 0 && out_row0 >= 0, "rom_project_h10: negative size");
  ROM_CHECK(n <= 4096, "rom_project_h10: basis of %d vectors (at most 4096)", n);
  const int64_t dim = f->dim;
  ROM_CHECK(size_t(u_row0 + M) * dim <= U->n && size_t(out_row0 + M) * dim <= OUT->n && (n == 0 || size_t(c_row0 + n) * dim <= C->n),
            "rom_project_h10: rows out of range");
  rom_ctx* ctx = f->ctx;
  if (M == 0) return ROM_OK;
  double* out = OUT->p + out_row0 * dim;
  if (n == 0) return romb_fill(ctx, out, size_t(M) * dim, 0.0);  // (:109-111)
  const double* u = U->p + u_row0 * dim;
  const double* c = C->p + c_row0 * dim;
  Tmp AC, G, R, ones, coef;
  ROM_TRY(AC.get(ctx, size_t(n) * dim));
  ROM_TRY(G.get(ctx, size_t(n) * n));
  ROM_TRY(R.get(ctx, size_t(M) * n));
  ROM_TRY(ones.get(ctx, M));
  ROM_TRY(coef.get(ctx, size_t(M) * n));
  ROM_TRY(rom_launch_stencil_apply(f, nullptr, c, n, AC));                                           // A_1 C^T (:123)
  ROM_TRY(rom_launch_gemm_nt(ctx, n, n, dim, 1.0, AC, dim, c, dim, 0.0, G, n, "gemm_nt"));            // C A_1 C^T (:136)
  ROM_TRY(rom_launch_gemm_nt(ctx, M, n, dim, 1.0, u, dim, AC, dim, 0.0, R, n, "gemm_nt"));            // rhs (:113-124)
  ROM_TRY(romb_fill(ctx, ones, M, 1.0));
  ROM_HIP(hipMemsetAsync(ctx->d_status, 0, sizeof(int), ctx->stream));
  ROM_TRY(rom_launch_reduced_solve(ctx, n, n, 1, M, G, ones, R, 1, coef));                            // (:135-138)
  ROM_TRY(rom_launch_gemm_nn(ctx, M, dim, n, 1.0, coef, n, c, dim, 0.0, out, dim));                   // (:139)
  return read_status(ctx, "rom_project_h10");
}

// reduced tensor Ahat[b] = C A_b C^T (k, n, n) and b_hat = C B_total of generate_fm_solutions (:93-103)
int romb_reduced_tensor(rom_fem* f, const double* c, int n, double* AC, double* Ahat, double* bhat) {
  rom_ctx* ctx = f->ctx;
  const int k = f->nrb * f->ncb;
  const int64_t dim = f->dim;
  Tmp onehot, Bt;
  ROM_TRY(onehot.get(ctx, size_t(k) * k));
  ROM_TRY(Bt.get(ctx, dim));
  ROM_TRY(romb_onehot(ctx, k, onehot));
  for (int b = 0; b < k; ++b) {
    ROM_TRY(rom_launch_stencil_apply(f, onehot.p() + size_t(b) * k, c, n, AC));
    ROM_TRY(rom_launch_gemm_nt(ctx, n, n, dim, 1.0, AC, dim, c, dim, 0.0, Ahat + size_t(b) * n * n, n, "gemm_nt"));
  }
  ROM_TRY(romb_load_vector(f, Bt));
  return rom_launch_gemm_nt(ctx, n, 1, dim, 1.0, c, dim, Bt, dim, 0.0, bhat, 1, "gemm_nt");
}

// generate_fm_solutions (:88-106): OUT_m = c_m C with (sum_b a[m,b] C A_b C^T) c_m = C B_total
extern "C" int rom_galerkin_rom(rom_fem* f, rom_buf* a, int M, rom_buf* C, int64_t c_row0, int n, rom_buf* OUT, int64_t out_row0) {
  ROM_CHECK(f && a && OUT && (C || n == 0), "rom_galerkin_rom: null argument");
  ROM_CHECK(M >= 0 && n >= 0 && c_row0 >= 0 && out_row0 >= 0, "rom_galerkin_rom: negative size");
  ROM_CHECK(n <= 4096, "rom_galerkin_rom: basis of %d vectors (at most 4096)", n);
  const int64_t dim = f->dim;
  const int k = f->nrb * f->ncb;
  ROM_CHECK(size_t(M) * k <= a->n && size_t(out_row0 + M) * dim <= OUT->n && (n == 0 || size_t(c_row0 + n) * dim <= C->n),
            "rom_galerkin_rom: buffers too small");
  rom_ctx* ctx = f->ctx;
  if (M == 0) return ROM_OK;
  double* out = OUT->p + out_row0 * dim;
  if (n == 0) return romb_fill(ctx, out, size_t(M) * dim, 0.0);  // (:89-91)
  const double* c = C->p + c_row0 * dim;
  Tmp Ahat, bhat, coef, AC;
  ROM_TRY(Ahat.get(ctx, size_t(k) * n * n));
  ROM_TRY(bhat.get(ctx, n));
  ROM_TRY(coef.get(ctx, size_t(M) * n));
  ROM_TRY(AC.get(ctx, size_t(n) * dim));
  ROM_TRY(romb_reduced_tensor(f, c, n, AC, Ahat, bhat));
  ROM_HIP(hipMemsetAsync(ctx->d_status, 0, sizeof(int), ctx->stream));
  ROM_TRY(rom_launch_reduced_solve(ctx, n, n, k, M, Ahat, a->p, bhat, 0, coef));   // (:104-105)
  ROM_TRY(rom_launch_gemm_nn(ctx, M, dim, n, 1.0, coef, n, c, dim, 0.0, out, dim));  // (:106)
  return read_status(ctx, "rom_galerkin_rom");
}

// =====================================================================================================================
// strong greedy (src/lib/ReducedBasis.py:112-139)
// =====================================================================================================================
// The reference recomputes, in every iteration, the approximation of all M training snapshots in the current basis
// (H^1_0 projection or Galerkin ROM) and the H^1_0 norm of the differences.  Both depend on the SPAN of the basis only,
// so the span is carried as an A_1-orthonormal basis W (w_j^T A_1 w_i = delta_ij) and the projection residuals
//     R_m = u_m - sum_j p_mj w_j ,   p_mj = <u_m, w_j>_{A_1}
// are kept in HBM and UPDATED by one vector per iteration (modified Gram-Schmidt over the training block), ONE pass over
// the block per iteration.  With w_j = R_pick / ||R_pick||_A (the residual of the pick is already orthogonal to W; one
// re-orthogonalisation) and z_j = A_1 w_j, pass j
//     applies the PREVIOUS update          R_m <- R_m - p_{m,j-1} w_{j-1}        (read + write)
//     takes the exact norm of the result   N_m = ||R_m||_A^2                      (edge form, no cancellation)
//     and the new coefficient              p_mj = R_m . z_j
// so that the residual norm after update j is  ||R_m - p_mj w_j||_A^2 = N_m - p_mj^2  (w_j is A_1-orthogonal to R_m's
// complement): ONE step of Pythagoras from a norm that is exact -- its cancellation error is eps N_m, i.e. a relative
// error eps (||R_before|| / ||R_after||)^2 of the new norm, harmless unless a single basis vector takes a residual
// down by more than four orders of magnitude (rows that happens to -- the pick itself, duplicates of it -- are not the
// next maximum), and it does not accumulate: the next pass measures N_m afresh.
// The Galerkin approximation g_m = sum_j c_mj w_j differs from the projection inside span W only, so
//     ||u_m - g_m||_A^2 = ||R_m||_A^2 + sum_j (p_mj - c_mj)^2      (both terms >= 0)
// with c_m from the reduced systems in the W basis, whose tensor W A_b W^T grows by one row per iteration.
// The reference's dense contractions are O(n M dim) per iteration; this is one read and one write of the block.

// err[m] = sqrt(nrm2[m]); rel = err / h1; first maximum -> picks[it], maxerr[it]; one workgroup
__global__ __launch_bounds__(1024) void kb_greedy_select(int M, const double* __restrict__ err2, const double* __restrict__ extra2,
                                                         const double* __restrict__ h1, int it, int* __restrict__ picks,
                                                         double* __restrict__ maxerr) {
  __shared__ double bv[1024];
  __shared__ int bi[1024];
  double best = -1.0;
  int at = 0;
  for (int m = threadIdx.x; m < M; m += 1024) {
    const double e2 = err2[m] + (extra2 ? extra2[m] : 0.0);
    const double rel = sqrt(e2) / h1[m];
    if (rel > best) { best = rel; at = m; }  // ascending m per thread: keeps the first maximum
  }
  bv[threadIdx.x] = best;
  bi[threadIdx.x] = at;
  __syncthreads();
  for (int s = 512; s > 0; s >>= 1) {
    if (int(threadIdx.x) < s) {
      const double o = bv[threadIdx.x + s];
      const int oi = bi[threadIdx.x + s];
      if (o > bv[threadIdx.x] || (o == bv[threadIdx.x] && oi < bi[threadIdx.x])) { bv[threadIdx.x] = o; bi[threadIdx.x] = oi; }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    picks[it] = bi[0];
    maxerr[it] = bv[0];
  }
}

// w <- (Rs[pick] - pc w_prev) / ||.||_A, pc = p_prev[pick] (the one update the block in HBM does not hold yet);
// a pick whose residual is at roundoff of its snapshot (a duplicate) gives w = 0
__global__ void kb_take_pick(double* __restrict__ w, const double* __restrict__ Rs, const double* __restrict__ w_prev,
                             const double* __restrict__ p_prev, long long dim, const int* __restrict__ picks, int it,
                             const double* __restrict__ err2, const double* __restrict__ norm0sq, int* __restrict__ degenerate) {
  const int p = picks[it];
  const double e2 = err2[p];
  const bool dead = a1_dead(e2, norm0sq[p]);
  const double a = dead ? 0.0 : 1.0 / sqrt(e2);
  if (blockIdx.x == 0 && threadIdx.x == 0) degenerate[it] = dead ? 1 : 0;
  const double* r = Rs + (long long)p * dim;
  const double pc = w_prev ? p_prev[p] : 0.0;
  for (long long j = blockIdx.x * (long long)blockDim.x + threadIdx.x; j < dim; j += (long long)gridDim.x * blockDim.x)
    w[j] = a * (w_prev ? r[j] - pc * w_prev[j] : r[j]);
}

// w <- w / sqrt(nrm2) unless the vector is dead
__global__ void kb_renormalise(double* __restrict__ w, long long dim, const double* __restrict__ nrm2,
                               const int* __restrict__ degenerate, int it) {
  const double n2 = *nrm2;
  const double a = (degenerate[it] || !(n2 > 0.0)) ? 0.0 : 1.0 / sqrt(n2);
  for (long long j = blockIdx.x * (long long)blockDim.x + threadIdx.x; j < dim; j += (long long)gridDim.x * blockDim.x) w[j] *= a;
}

// The projection of a Gram-Schmidt round of w against the A_1-orthonormal rows W[0..j) (AW = A_1 W): t_i = <w_i, w>_A,
// w -= t^T W, nrm = ||w||_A^2
static int a1_project(rom_fem* f, const double* W, const double* AW, int j, double* w, double* t, double* nrm) {
  rom_ctx* ctx = f->ctx;
  const int64_t dim = f->dim;
  ROM_TRY(rom_launch_rowdot(ctx, AW, j, dim, w, t));                                    // t_i = <w_i, w>_A
  ROM_TRY(rom_launch_gemm_nn(ctx, 1, dim, j, -1.0, t, j, W, dim, 1.0, w, dim));         // w -= t^T W
  return rom_launch_h10norm(f, w, nullptr, 1, nrm, false);
}

// One Gram-Schmidt round, then w <- w / sqrt(nrm), or 0 when degenerate[it]: the re-orthogonalisation of the greedy and
// the second round of romb_a1_append.
static int romb_a1_reorth(rom_fem* f, const double* W, const double* AW, int j, double* w, double* t, double* nrm,
                   const int* degenerate, int it) {
  ROM_TRY(a1_project(f, W, AW, j, w, t, nrm));
  kb_renormalise<<<vector_grid(f->dim), 256, 0, f->ctx->stream>>>(w, f->dim, nrm, degenerate, it);
  ROM_HIP(hipGetLastError());
  return ROM_OK;
}

__global__ void kb_a1_decide(const double* __restrict__ nrm1, const double* __restrict__ norm0, int i, int* __restrict__ dead) {
  dead[i] = a1_dead(*nrm1, norm0[i]) ? 1 : 0;
}

int romb_a1_append(rom_fem* f, double* W, double* AW, int i, const double* norm0, double* t1, double* t2, double* nrm1,
                   double* nrm2, int* dead) {
  rom_ctx* ctx = f->ctx;
  const int64_t dim = f->dim;
  double* wi = W + size_t(i) * dim;
  if (i == 0) ROM_HIP(hipMemcpyAsync(nrm1, norm0, sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  else ROM_TRY(a1_project(f, W, AW, i, wi, t1, nrm1));
  kb_a1_decide<<<1, 1, 0, ctx->stream>>>(nrm1, norm0, i, dead);
  ROM_HIP(hipGetLastError());
  kb_renormalise<<<vector_grid(dim), 256, 0, ctx->stream>>>(wi, dim, nrm1, dead, i);
  ROM_HIP(hipGetLastError());
  if (i > 0) ROM_TRY(romb_a1_reorth(f, W, AW, i, wi, t2, nrm2, dead, i));
  return rom_launch_stencil_apply(f, nullptr, wi, 1, AW + size_t(i) * dim);  // z_i = A_1 w_i
}

// The pass of one greedy iteration over the training block (see above): d = Rs_m - p_prev[m] w_prev (written to Rout when
// there is a previous update), partial sums of ||d||_A^2 in edge form and of d . z.  Layout of k_h10_partial
// (rom_ops.hip): a thread owns a mesh column and walks down a slab of rows, every entry is read once, the halo row above
// the slab a second time; the east neighbour comes from the next lane, across waves through LDS, across workgroups by a
// load of the workgroup's last thread.  The update goes to a second buffer, not in place: halo entries belong to other
// workgroups.  partial: [2][M][nblk] (norms, dots).
// GU_SYS training rows per workgroup share the loads of w_prev and z (L2 resident, but two of the three loads per entry
// when every row fetches its own).  Measured at C4 (1024 x 262 144, ms per pass; tools/dev/ab_greedy.sh): GU_SYS x
// GU_UNROLL = 1 x 2..5: 1.15-1.17, 1 x 8: 1.59, 2 x 4: 1.46, 4 x 2: 1.58, 4 x 4: 2.28 (187 VGPRs) -- the pass lives on
// occupancy (waves in flight hide the HBM latency), not on fewer L2 reads, so the default shares nothing.
#ifndef GU_SYS_
#define GU_SYS_ 1
#endif
#ifndef GU_UNROLL_
#define GU_UNROLL_ 2
#endif
constexpr int GU_ROWS = 32, GU_UNROLL = GU_UNROLL_, GU_SYS = GU_SYS_;
template <bool PREV>
__global__ __launch_bounds__(256) void kb_greedy_pass(StencilGeom g, const double* __restrict__ Rs, double* __restrict__ Rout,
                                                      const double* __restrict__ w_prev, const double* __restrict__ p_prev,
                                                      const double* __restrict__ z, double* __restrict__ partial, int nblk, int M) {
  __shared__ double red[2][GU_SYS][4];
  __shared__ double west[2][4][GU_UNROLL][GU_SYS];  // first column of every wave, per row of the chunk (double buffered)
  const int m0 = blockIdx.z * GU_SYS;
  const double* u[GU_SYS];
  double* o[GU_SYS];
  double pm[GU_SYS];
  bool live[GU_SYS];
#pragma unroll
  for (int k = 0; k < GU_SYS; ++k) {
    const int mk = min(m0 + k, M - 1);  // (the last group repeats its last row; the repeats are neither stored nor reported)
    live[k] = m0 + k < M;
    u[k] = Rs + mk * g.dim;
    o[k] = PREV ? Rout + mk * g.dim : nullptr;
    pm[k] = PREV ? p_prev[mk] : 0.0;
  }
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int r0 = blockIdx.y * GU_ROWS, r1 = min(g.nr, r0 + GU_ROWS);
  const bool in = c < g.nc;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double s[GU_SYS], dt[GU_SYS], north[GU_SYS];
  {
    const long long i = (long long)(r0 - 1) * g.nc + c;
    const bool ok = in && r0 > 0;
    const double wn = (PREV && ok) ? w_prev[i] : 0.0;
#pragma unroll
    for (int k = 0; k < GU_SYS; ++k) {
      s[k] = dt[k] = 0.0;
      north[k] = ok ? (PREV ? u[k][i] - pm[k] * wn : u[k][i]) : 0.0;
    }
  }
  int buf = 0;
  for (int rb = r0; rb < r1; rb += GU_UNROLL, buf ^= 1) {
    double x[GU_SYS][GU_UNROLL], xe[GU_SYS][GU_UNROLL], zz[GU_UNROLL];
#pragma unroll
    for (int q = 0; q < GU_UNROLL; ++q) {
      const int r = rb + q;
      const long long i = (long long)r * g.nc + c;
      const bool ok = in && r < r1;
      const bool edge = threadIdx.x == 255 && c + 1 < g.nc && r < r1;
      const double wv = (PREV && ok) ? w_prev[i] : 0.0;
      const double we = (PREV && edge) ? w_prev[i + 1] : 0.0;
      zz[q] = ok ? z[i] : 0.0;
#pragma unroll
      for (int k = 0; k < GU_SYS; ++k) {
        x[k][q] = ok ? (PREV ? u[k][i] - pm[k] * wv : u[k][i]) : 0.0;
        xe[k][q] = edge ? (PREV ? u[k][i + 1] - pm[k] * we : u[k][i + 1]) : 0.0;
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int q = 0; q < GU_UNROLL; ++q)
#pragma unroll
        for (int k = 0; k < GU_SYS; ++k) west[buf][wave][q][k] = x[k][q];
    }
    // (uniform trip count: r0, r1 depend on the block only; the other buffer is read one barrier later.  The barrier
    // waits for the LDS writes only: __syncthreads() would also drain every global load in flight -- whatever the compiler
    // has hoisted from the next chunk -- once per four rows)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
    for (int q = 0; q < GU_UNROLL; ++q) {
      const int r = rb + q;
      const bool ok = in && r < r1;
#pragma unroll
      for (int k = 0; k < GU_SYS; ++k) {
        double east = __shfl_down(x[k][q], 1, 64);
        if (lane == 63) east = wave < 3 ? west[buf][wave + 1][q][k] : xe[k][q];
        if (ok) {
          if (PREV && live[k]) __builtin_nontemporal_store(x[k][q], &o[k][(long long)r * g.nc + c]);  // (read by the next pass only)
          if (c + 1 >= g.nc) east = 0.0;
          const double dh = x[k][q] - east, dv = x[k][q] - north[k];
          s[k] += dh * dh + dv * dv;
          if (c == 0) s[k] += x[k][q] * x[k][q];
          if (r == g.nr - 1) s[k] += x[k][q] * x[k][q];
          dt[k] += x[k][q] * zz[q];
          north[k] = x[k][q];
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < GU_SYS; ++k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      s[k] += __shfl_down(s[k], off, 64);
      dt[k] += __shfl_down(dt[k], off, 64);
    }
    if (lane == 0) {
      red[0][k][wave] = s[k];
      red[1][k][wave] = dt[k];
    }
  }
  __syncthreads();
  if (threadIdx.x < 2 * GU_SYS) {
    const int which = threadIdx.x / GU_SYS, k = threadIdx.x % GU_SYS;
    if (m0 + k < M) {
      const long long at_ = (which * (long long)M + m0 + k) * nblk + blockIdx.y * gridDim.x + blockIdx.x;
      partial[at_] = red[which][k][0] + red[which][k][1] + red[which][k][2] + red[which][k][3];
    }
  }
}

// N_m = sum of the norm partials, p_m = sum of the dot partials, err2_m = max(N_m - p_m^2, 0)
__global__ __launch_bounds__(256) void kb_greedy_finish(const double* __restrict__ partial, int nblk, int M,
                                                        double* __restrict__ p_new, double* __restrict__ err2) {
  __shared__ double red[2][4];
  double s = 0.0, d = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 256) {
    s += partial[blockIdx.x * (long long)nblk + i];
    d += partial[(M + blockIdx.x) * (long long)nblk + i];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s += __shfl_down(s, off, 64);
    d += __shfl_down(d, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = s;
    red[1][threadIdx.x >> 6] = d;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double N = red[0][0] + red[0][1] + red[0][2] + red[0][3], pp = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    p_new[blockIdx.x] = pp;
    err2[blockIdx.x] = fmax(N - pp * pp, 0.0);
  }
}

// row / column j of the reduced tensor (k, ld, ld) from col[i, b] = w_i^T A_b w_j (i <= j); a dead vector gets a unit
// diagonal and zero couplings, which keeps every reduced matrix positive definite and its coefficient at 0
__global__ void kb_grow_ahat(double* __restrict__ Ahat, int k, int ld, int j, const double* __restrict__ col,
                             const int* __restrict__ degenerate, int it) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (j + 1) * k) return;
  const int i = idx / k, b = idx % k;
  const bool dead = degenerate[it] != 0;
  const double v = dead ? (i == j ? 1.0 : 0.0) : col[idx];
  Ahat[(size_t(b) * ld + j) * ld + i] = v;
  Ahat[(size_t(b) * ld + i) * ld + j] = v;
}

// extra2[m] = sum_{j < n} (P[j, m] - c[m, j])^2   (P: row j = projection coefficients of basis vector j; c: packed n)
__global__ void kb_galerkin_gap(int M, int n, const double* __restrict__ P, const double* __restrict__ c,
                                double* __restrict__ extra2) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  double s = 0.0;
  for (int j = 0; j < n; ++j) {
    const double d = P[size_t(j) * M + m] - c[size_t(m) * n + j];
    s += d * d;
  }
  extra2[m] = s;
}

// mode 0: greedy for the H^1_0 projection error; 1: for the Galerkin error.  h1norm: the normalisation the caller passes
// as solutions2train_h1norm (M doubles on the host).  picks_out / max_err_out: n entries.
extern "C" int rom_greedy(rom_fem* f, rom_buf* U, int64_t u_row0, int M, rom_buf* a, const double* h1norm_host, int mode,
                          int n, int64_t* picks_out, double* max_err_out) {
  ROM_CHECK(f && U && h1norm_host && (picks_out || n == 0) && (max_err_out || n == 0), "rom_greedy: null argument");
  ROM_CHECK(mode == 0 || mode == 1, "rom_greedy: mode must be 0 (H10 projection) or 1 (Galerkin)");
  ROM_CHECK(mode == 0 || a, "rom_greedy: the Galerkin greedy needs the training parameters");
  ROM_CHECK(M >= 1 && M <= 65535 && n >= 0 && u_row0 >= 0, "rom_greedy: bad sizes (1 <= M <= 65535)");
  ROM_CHECK(n <= 2048, "rom_greedy: at most 2048 basis vectors");
  const int64_t dim = f->dim;
  const int k = f->nrb * f->ncb;
  ROM_CHECK(size_t(u_row0 + M) * dim <= U->n && (!a || size_t(M) * k <= a->n), "rom_greedy: buffers too small");
  if (n == 0) return ROM_OK;
  rom_ctx* ctx = f->ctx;
  const StencilGeom g = rom_make_geom(f->nrb, f->ncb, f->N);
  const double* u = U->p + u_row0 * dim;
  const int nb = std::max(n - 1, 1);  // basis vectors ever built
  Tmp Ra, Rb, W, AW, P, err2, norm0, h1, ipick, idead, maxerr, t, nrm, part, Ahat, bhat, cg, extra, ZB, col, onehot, Bt;
  ROM_TRY(Ra.get(ctx, size_t(M) * dim));
  ROM_TRY(Rb.get(ctx, size_t(M) * dim));
  ROM_TRY(W.get(ctx, size_t(nb) * dim));
  ROM_TRY(AW.get(ctx, size_t(nb) * dim));
  ROM_TRY(P.get(ctx, size_t(nb) * M));   // row j: p_mj = <R_m, w_j>_A, the projection coefficients
  ROM_TRY(err2.get(ctx, M));
  ROM_TRY(norm0.get(ctx, M));
  ROM_TRY(h1.get(ctx, M));
  ROM_TRY(ipick.get(ctx, n));   // n ints (picks) in a block of n doubles
  ROM_TRY(idead.get(ctx, n));   // n ints (1: the vector built from this pick is dead)
  ROM_TRY(maxerr.get(ctx, n));
  ROM_TRY(t.get(ctx, nb));
  ROM_TRY(nrm.get(ctx, 1));
  const dim3 ugrid((g.nc + 255) / 256, (g.nr + GU_ROWS - 1) / GU_ROWS, (M + GU_SYS - 1) / GU_SYS);
  const int nblk = int(ugrid.x * ugrid.y);
  ROM_TRY(part.get(ctx, 2 * size_t(M) * nblk));
  int* d_picks = reinterpret_cast<int*>(ipick.p());
  int* d_dead = reinterpret_cast<int*>(idead.p());
  double* d_maxerr = maxerr.p();
  if (mode == 1) {
    ROM_TRY(Ahat.get(ctx, size_t(k) * nb * nb));
    ROM_TRY(bhat.get(ctx, nb));
    ROM_TRY(cg.get(ctx, size_t(M) * nb));
    ROM_TRY(extra.get(ctx, M));
    ROM_TRY(ZB.get(ctx, size_t(k) * dim));
    ROM_TRY(col.get(ctx, size_t(nb) * k));
    ROM_TRY(onehot.get(ctx, size_t(k) * k));
    ROM_TRY(Bt.get(ctx, dim));
    ROM_TRY(romb_fill(ctx, Ahat, size_t(k) * nb * nb, 0.0));
    ROM_TRY(romb_load_vector(f, Bt));
    ROM_TRY(romb_onehot(ctx, k, onehot));
  }
  ROM_HIP(hipMemcpyAsync(h1.p(), h1norm_host, size_t(M) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  ROM_HIP(hipStreamSynchronize(ctx->stream));  // the caller's array is free again
  ROM_HIP(hipMemsetAsync(ctx->d_status, 0, sizeof(int), ctx->stream));
  ROM_HIP(hipMemsetAsync(ipick.p(), 0, size_t(n) * sizeof(double), ctx->stream));
  ROM_HIP(hipMemsetAsync(idead.p(), 0, size_t(n) * sizeof(double), ctx->stream));
  ROM_HIP(hipMemsetAsync(maxerr.p(), 0, size_t(n) * sizeof(double), ctx->stream));
  // empty basis (:120-129 with basis (0, 0)): the approximation is zero, the error of snapshot m is ||u_m||_A / h1_m --
  // the same kernel as rom_h10norm, so a caller that passes sm.H10norm(U) gets exactly 1.0 everywhere and index 0
  ROM_TRY(rom_launch_h10norm(f, u, nullptr, M, norm0, false));
  ROM_HIP(hipMemcpyAsync(err2.p(), norm0.p(), size_t(M) * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  kb_greedy_select<<<1, 1024, 0, ctx->stream>>>(M, err2, nullptr, h1, 0, d_picks, d_maxerr);
  ROM_HIP(hipGetLastError());
  const double* Rs = u;  // the block in HBM: all updates but the latest applied (the snapshots themselves are never written)
  double* bufs[2] = {Ra.p(), Rb.p()};
  const double *w_prev = nullptr, *p_prev = nullptr;
  const unsigned vgrid = vector_grid(dim);
  for (int it = 1; it < n; ++it) {
    const int j = it - 1;  // index of the basis vector built from pick it - 1
    double* wj = W.p() + size_t(j) * dim;
    double* zj = AW.p() + size_t(j) * dim;
    double* pj = P.p() + size_t(j) * M;
    kb_take_pick<<<vgrid, 256, 0, ctx->stream>>>(wj, Rs, w_prev, p_prev, dim, d_picks, it - 1, err2, norm0, d_dead);
    ROM_HIP(hipGetLastError());
    if (j > 0) ROM_TRY(romb_a1_reorth(f, W, AW, j, wj, t, nrm, d_dead, it - 1));  // one re-orthogonalisation, renormalise
    ROM_TRY(rom_launch_stencil_apply(f, nullptr, wj, 1, zj));                                // z = A_1 w
    {
      ROM_PROF(ctx, w_prev ? "greedy_pass" : "greedy_pass_first", 16.0 * double(M) * dim, (w_prev ? 16.0 : 8.0) * double(M) * dim);
      if (w_prev) {
        double* Rnext = bufs[it & 1];
        kb_greedy_pass<true><<<ugrid, 256, 0, ctx->stream>>>(g, Rs, Rnext, w_prev, p_prev, zj, part, nblk, M);
        Rs = Rnext;
      } else {
        kb_greedy_pass<false><<<ugrid, 256, 0, ctx->stream>>>(g, Rs, nullptr, nullptr, nullptr, zj, part, nblk, M);
      }
      kb_greedy_finish<<<M, 256, 0, ctx->stream>>>(part, nblk, M, pj, err2);
    }
    ROM_HIP(hipGetLastError());
    w_prev = wj;
    p_prev = pj;
    if (mode == 1) {
      ROM_TRY(rom_launch_stencil_apply_blocks(f, onehot, wj, ZB));                                       // A_b w_j, all b
      ROM_TRY(rom_launch_gemm_nt(ctx, j + 1, k, dim, 1.0, W, dim, ZB, dim, 0.0, col, k, "gemm_nt"));      // col[i, b] = w_i . A_b w_j
      kb_grow_ahat<<<unsigned(((j + 1) * k + 255) / 256), 256, 0, ctx->stream>>>(Ahat, k, nb, j, col, d_dead, it - 1);
      ROM_HIP(hipGetLastError());
      ROM_TRY(rom_launch_rowdot(ctx, wj, 1, dim, Bt, bhat.p() + j));                                      // w_j . B_total
      ROM_TRY(rom_launch_reduced_solve(ctx, j + 1, nb, k, M, Ahat, a->p, bhat, 0, cg));
      kb_galerkin_gap<<<unsigned((M + 255) / 256), 256, 0, ctx->stream>>>(M, j + 1, P, cg, extra);
      ROM_HIP(hipGetLastError());
    }
    kb_greedy_select<<<1, 1024, 0, ctx->stream>>>(M, err2, mode == 1 ? extra.p() : nullptr, h1, it, d_picks, d_maxerr);
    ROM_HIP(hipGetLastError());
  }
  // results: picks as doubles through one download
  Tmp outd;
  ROM_TRY(outd.get(ctx, 2 * size_t(n)));
  kb_ints_to_doubles<<<unsigned((n + 255) / 256), 256, 0, ctx->stream>>>(d_picks, outd, n);
  ROM_HIP(hipMemcpyAsync(outd.p() + n, d_maxerr, size_t(n) * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  std::vector<double> host(2 * size_t(n));
  ROM_TRY(download(ctx, outd, host.data(), host.size()));
  for (int i = 0; i < n; ++i) {
    picks_out[i] = int64_t(host[i]);
    max_err_out[i] = host[n + i];
  }
  return read_status(ctx, "rom_greedy");
}
