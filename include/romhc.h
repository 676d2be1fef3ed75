/*
 * romhc.h -- C-ABI of libromhc.so, the MI355X (gfx950) implementation of the
 * ROMHighContrast snapshot-generation + reduced-basis hot path.
 *
 * The reference (agussomacal/ROMHighContrast) has no FFI layer: its boundary for this path is
 * the Python API of src/lib/SolutionsManagers.py and src/lib/ReducedBasis.py.  Each entry point
 * below names the reference interface it replaces (file:line, relative to the reference tree).
 * The Python shim (romhighcontrast_amd/lib, re-exported as src.lib / lib) binds these
 * with ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; rom_last_error() returns a
 *     thread-local, NUL-terminated description of the last failure on this thread.
 *   - all floating point is IEEE fp64.  Bulk data lives in device buffers (rom_buf*), created
 *     and destroyed explicitly; host arrays are caller-owned and only touched by
 *     rom_buf_upload / rom_buf_download and the few *_host helpers.
 *   - snapshot matrices are row-major (n_rows, dim): row = one FE vector over the inner
 *     vertices in row-major (r, c) order -- exactly the reference's `solutions` arrays.
 *   - parameters `a` are row-major (M, nrb*ncb): a[m][p*ncb+q], p = block row (y), q = block
 *     column (x) -- the reference's a[m][p][q].
 *   - all work is enqueued on the context's HIP stream; functions that return host data
 *     synchronise that stream first.  One context per process per GPU.
 */
#ifndef ROMHC_H
#define ROMHC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rom_ctx rom_ctx; /* one GPU + stream + workspace            */
typedef struct rom_buf rom_buf; /* fp64 device buffer                      */
typedef struct rom_fem rom_fem; /* FE space of one (blocks_geometry, N)    */

#define ROM_OK 0
#define ROM_ERR_INVALID 1  /* bad argument                                              */
#define ROM_ERR_HIP 2      /* HIP runtime failure (message holds hipGetErrorString)     */
#define ROM_ERR_NOT_SPD 3  /* a pivot was <= 0: maps to scipy.linalg.LinAlgError         */
#define ROM_ERR_COMM 4     /* RCCL failure / librccl not loadable                        */
#define ROM_ERR_NOMEM 5

const char* rom_last_error(void);
int rom_version(void);

/* ---- context ------------------------------------------------------------------------- */
int rom_device_count(int* n);
int rom_init(int device, rom_ctx** out);
int rom_shutdown(rom_ctx* ctx);
int rom_synchronize(rom_ctx* ctx);
/* workspace budget (bytes) for the factor storage of rom_solve_batch; default 24 GiB */
int rom_set_workspace_limit(rom_ctx* ctx, size_t bytes);
int rom_device_name(rom_ctx* ctx, char* out, size_t cap);

/* HIP-event stopwatch on the context stream (bench.py's timed region) */
int rom_timer_start(rom_ctx* ctx);
int rom_timer_stop(rom_ctx* ctx, double* elapsed_ms);

/* per-kernel HIP-event profiling: when enabled every kernel launch of the library is
 * bracketed by an event pair on the launch stream; rom_profile_query sums them by name.
 * While it is enabled rom_solve_batch* keeps a sweep on ONE stream (otherwise geometries whose
 * reduced solve is the tile Cholesky run as two concurrent sub-batches, ROMHC_STREAMS), so
 * that a bracket times its kernel alone. */
int rom_profile_enable(rom_ctx* ctx, int on);
int rom_profile_reset(rom_ctx* ctx);
int rom_profile_count(rom_ctx* ctx, int* n_kernels);
int rom_profile_query(rom_ctx* ctx, int idx, char* name, size_t cap, double* total_ms, long* launches,
                      double* flops, double* bytes);

/* ---- device buffers ------------------------------------------------------------------- */
int rom_buf_alloc(rom_ctx* ctx, size_t n_doubles, rom_buf** out);
int rom_buf_free(rom_buf* b);
int rom_buf_size(rom_buf* b, size_t* n_doubles);
int rom_buf_upload(rom_buf* b, size_t offset, const double* host, size_t n);
int rom_buf_download(rom_buf* b, size_t offset, double* host, size_t n);
/* Page-locked host arrays for large results (process-wide pool, thread safe): generate_solutions
 * (src/lib/SolutionsManagers.py:64-68) returns the (M, dim) rows to the host, and rom_buf_download into such an
 * array runs at the PCIe rate (48 vs 11-25 GB/s) -- but pinning 533 MB takes 110 ms, so the Python shim only pins for
 * sizes it has seen repeatedly and otherwise takes what the pool has; the NumPy arrays it wraps around the blocks
 * give them back when they are collected. */
/* pooled_only != 0: hand out a block of the pool or *out = NULL (status 0), never pin new memory */
int rom_host_alloc(size_t n, int pooled_only, double** out);
int rom_host_free(double* p);
int rom_buf_fill(rom_buf* b, size_t offset, size_t n, double value);
int rom_buf_copy(rom_buf* dst, size_t dst_off, rom_buf* src, size_t src_off, size_t n);
/* *equal_host = 1 if the n doubles A[a_off ...] and B[b_off ...] have the same bits (how the Python layer checks that rows
 * handed back to it are still the image of the interface vectors it kept for them), else 0 */
int rom_buf_equal(rom_buf* A, size_t a_off, rom_buf* B, size_t b_off, size_t n, int* equal_host);
/* dst[i, :] = src[rows[i], :] for row length `dim` (host index list; used by the greedy) */
int rom_buf_gather_rows(rom_buf* dst, rom_buf* src, const int64_t* rows, int n_rows, size_t dim);

/* ---- FE space: SolutionsManagerFEM.__init__ (src/lib/SolutionsManagers.py:146-219) ------ */
/* Builds the parameter-independent tables of the substructured operator on the device
 * (unit-block sine basis, harmonic-extension matrix, Dirichlet-to-Neumann blocks, symbolic
 * tile Cholesky of the interface system).  Replaces the dense A_preassembled tensor. */
int rom_fem_create(rom_ctx* ctx, int nrb, int ncb, int N, rom_fem** out);
int rom_fem_destroy(rom_fem* fem);
int rom_fem_dims(rom_fem* fem, int* nr, int* nc, int64_t* dim, int* n_interface, int* n_tiles);
/* B_total (:177-185): dim doubles, host */
int rom_fem_load_vector_host(rom_fem* fem, double* B_out);

/* einsum('pqij,pq->ij') in stencil form (:19-23 / :187-215): for each of M parameters the
 * three stencil arrays diag[M,nr,nc], east[M,nr,nc-1], north[M,nr-1,nc]. */
int rom_assemble_batch(rom_fem* fem, rom_buf* a, int M, rom_buf* diag, rom_buf* east, rom_buf* north);

/* generate_solutions (:64-68) = map(galerkin (:17-40)) : U[row0+m, :] = A(a_m)^{-1} B_total.
 * Exact direct method (interface Schur complement + tile Cholesky + harmonic extension). */
int rom_solve_batch(rom_fem* fem, rom_buf* a, int M, rom_buf* U, int64_t row0);
/* The same sweep, only enqueued (no host synchronisation); a non-positive pivot -- the reference's
 * scipy LinAlgError case -- is latched on the device and reported by the next rom_solve_status()
 * (or rom_solve_batch()), which waits for the compute stream. */
int rom_solve_batch_async(rom_fem* fem, rom_buf* a, int M, rom_buf* U, int64_t row0);
int rom_solve_status(rom_ctx* ctx);
/* The sweep in two stages, for the multi-GPU exchange: a snapshot row is a fixed linear image of
 * its system's "interface vector" (reduced unknowns + coefficient blocks, rom_fem_reduced_stride() doubles:
 * 784 instead of 65,025 at 256x256 / 2x2).  Ranks all-gather the interface vectors and every rank expands all
 * of them; the expansion is deterministic, so the gathered snapshot block is bit-identical on every rank.
 * Both calls only enqueue work on the compute stream (rom_solve_status() reports a non-positive pivot). */
int rom_fem_reduced_stride(rom_fem* fem, int64_t* stride);
/* positions [nodal_begin, nodal_end) of an interface vector are outputs of the expansion (nodal edge values);
 * only the rest is read by it */
int rom_fem_reduced_layout(rom_fem* fem, int64_t* nodal_begin, int64_t* nodal_end);
/* 1 if rom_expand_batch_async is a LINEAR map of the interface vectors (it then ignores `a`): U = Y B^T with a fixed
 * B, so Gram matrices, means and POD modes of snapshots can be formed from Y alone (every geometry whose
 * closed-form edges are all kept in compressed form, e.g. 2x2/N>=16, 3x3/N=171, 4x4/N=256). */
int rom_fem_expansion_is_linear(rom_fem* fem, int* flag);
/* Compact form for the exchange (the all-gather before the SVD): the entries of an interface vector outside
 * its nodal part, rom_fem_compact_stride() doubles (272 of 784 at 256x256 / 2x2) -- all that has to travel, since the
 * expansion recomputes the nodal part.  pack: Yc[c_row0+m] <- Y[y_row0+m]; unpack: the inverse (nodal part zeroed).
 * Both only enqueue on the compute stream. */
int rom_fem_compact_stride(rom_fem* fem, int64_t* stride);
int rom_fem_pack_reduced_async(rom_fem* fem, rom_buf* Y, int64_t y_row0, int M, rom_buf* Yc, int64_t c_row0);
int rom_fem_unpack_reduced_async(rom_fem* fem, rom_buf* Yc, int64_t c_row0, int M, rom_buf* Y, int64_t y_row0);
int rom_solve_reduced_async(rom_fem* fem, rom_buf* a, int M, rom_buf* Y, int64_t y_row0);
int rom_expand_batch_async(rom_fem* fem, rom_buf* a, int M, rom_buf* Y, int64_t y_row0, rom_buf* U, int64_t row0);
/* flops / HBM bytes of the library's own algorithm for one snapshot solve, and the canonical
 * banded-Cholesky figures of SURVEY.md 8(d) for comparison */
int rom_solve_work(rom_fem* fem, double* flops_own, double* bytes_own, double* flops_banded,
                   double* bytes_banded);

/* Y[k,:] = A(coef) X[k,:], K rows.  mode 0: coef = a_one (k doubles, host) general blocks;
 * mode 1: unit coefficient (A_preassembled4h1_norm, :49).  (the C A_pq contractions, :93-101) */
int rom_stencil_apply(rom_fem* fem, const double* a_one_host, int unit, rom_buf* X, int64_t x_row0,
                      int K, rom_buf* Y, int64_t y_row0);

/* H10norm (:56-58): out[k] = sqrt(u_k^T A_1 u_k); out_host has K doubles.
 * If V != NULL computes the norm of (U[u_row0+k] - V[v_row0+k]) instead (greedy residuals,
 * src/lib/ReducedBasis.py:129). */
int rom_h10norm(rom_fem* fem, rom_buf* U, int64_t u_row0, rom_buf* V, int64_t v_row0, int K,
                double* out_host);
/* l2norm (:60-62) */
int rom_l2norm(rom_ctx* ctx, rom_buf* U, int64_t row0, int K, int64_t dim, double* out_host);

/* ---- dense fp64 contractions on MFMA (v_mfma_f64_16x16x4_f64) --------------------------- */
/* C[m,n] = alpha * sum_k A[m,k] B[n,k] + beta*C   (row-major, "NT": Gram / C A U^T).  rom_gemm_nt and rom_gemm_nn run a
 * product of more than 65535 * 64 rows in row blocks of that many (their 64-row tiles are one grid dimension). */
int rom_gemm_nt(rom_ctx* ctx, int64_t m, int64_t n, int64_t k, double alpha, rom_buf* A, size_t a_off,
                int64_t lda, rom_buf* B, size_t b_off, int64_t ldb, double beta, rom_buf* C, size_t c_off,
                int64_t ldc);
/* G[m,m] = A A^T (row-major A[m,k]): the snapshot Gram matrix of the POD; only the lower tiles are
 * computed on MFMA, the strict upper triangle is mirrored */
int rom_gram(rom_ctx* ctx, int64_t m, int64_t k, rom_buf* A, size_t a_off, int64_t lda, rom_buf* C, size_t c_off,
             int64_t ldc);
/* C[m,n] = alpha * sum_k A[m,k] B[k,n] + beta*C   (row-major, "NN": lift c_i . basis, :106/:139) */
int rom_gemm_nn(rom_ctx* ctx, int64_t m, int64_t n, int64_t k, double alpha, rom_buf* A, size_t a_off,
                int64_t lda, rom_buf* B, size_t b_off, int64_t ldb, double beta, rom_buf* C, size_t c_off,
                int64_t ldc);

/* batched reduced solves: for m<M: (sum_b w[m,b] * Ahat[b]) c_m = rhs[m or 0]  (n x n SPD).
 * Ahat: (kb, n, n); w: (M, kb); rhs: (M, n) if rhs_per_system else (n); out c: (M, n).
 * The reduced `galerkin` calls of generate_fm_solutions (:104-105) and project_solutions
 * (:135-138). */
int rom_reduced_solve_batch(rom_ctx* ctx, int n, int kb, int M, rom_buf* Ahat, rom_buf* w, rom_buf* rhs,
                            int rhs_per_system, rom_buf* c_out);

/* ---- helpers of the basis builders ------------------------------------------------------ */
int rom_buf_scale(rom_buf* b, size_t offset, size_t n, double alpha);
/* X[row0+m, :] -= mean over m (column means, kept in `mean`, dim doubles): the centring step of
 * sklearn PCA.fit called at src/lib/ReducedBasis.py:196 */
int rom_center_rows(rom_ctx* ctx, rom_buf* X, int64_t row0, int M, int64_t dim, rom_buf* mean);
/* X[row0+i, :] *= factors_host[i], i < rows: the 1/sigma scaling of the lifted POD modes (components_ of the PCA at
 * src/lib/ReducedBasis.py:196-197 have unit norm) */
int rom_rows_scale(rom_ctx* ctx, rom_buf* X, int64_t row0, int rows, int64_t dim, const double* factors_host);
/* every row times the sign of its entry of largest magnitude: sklearn's svd_flip(u_based_decision=False) inside the
 * same PCA call, which fixes the signs of `components_` */
int rom_rows_sign_flip(rom_ctx* ctx, rom_buf* X, int64_t row0, int rows, int64_t dim);
/* evaluate_solutions (src/lib/SolutionsManagers.py:221-244): P1 interpolation of K FE vectors at
 * npts points.  ix/iy = cell index of each point (searchsorted(points_c/points_r) - 1), tx/ty its
 * local coordinates in the cell; out_host is (K, npts). */
int rom_evaluate_points(rom_fem* fem, rom_buf* U, int64_t row0, int K, int npts, const int* ix_host,
                        const int* iy_host, const double* tx_host, const double* ty_host, double* out_host);
/* H^1_0 Riesz representers of P1 point evaluations (generate_riesz, src/lib/SolutionsManagers.py:70-86, the h10
 * branch the reference left unimplemented).  r_i = the (dim,) evaluation vector of point i, with exactly the locating
 * convention and the domain checks of rom_evaluate_points (so r_i is row i of generate_riesz(x, "l2")).
 * OMEGA[row0+i] = A_1^{-1} r_i for i < npts (OMEGA may be NULL: Gram only);
 * gram_host (npts x npts, row-major, may be NULL) = r_i^T A_1^{-1} r_j, symmetric to the bit.
 * A_1 is the 5-point Laplacian of the interior grid, diagonal in the 2-D sine basis: the representers are one sparse
 * -> spectral kernel and two MFMA products for all points (the sine tables are built once per FE space), G one Gram
 * product in spectral space.  A point whose three P1 weights all fall on the boundary has r_i = 0: omega_i = 0 and a
 * zero row / column of G.  One host synchronisation at the end. */
int rom_riesz_h10(rom_fem* fem, int npts, const int* ix_host, const int* iy_host, const double* tx_host,
                  const double* ty_host, rom_buf* OMEGA, int64_t row0, double* gram_host);
/* Greedy sensor selection for PBDW (the sampling question of the inverse-problem notebook, InverseProblemPipeline.ipynb;
 * the experiment draws uniform random points, src/experiments/HighContrast.py:155).
 * rom_riesz_norms_h10: out_host[i] = r_i^T A_1^{-1} r_i = ||omega_i||^2_{H^1_0} for npts points: the diagonal of
 * rom_riesz_h10's G, without G or the representers (vertex-pair Green tables built once per FE space, at most nine
 * table entries per point).  Same locating convention, domain check and boundary rule (a vanishing functional gives
 * exactly 0).  One host synchronisation. */
int rom_riesz_norms_h10(rom_fem* fem, int npts, const int* ix_host, const int* iy_host, const double* tx_host,
                        const double* ty_host, double* out_host);
/* Greedy selection (Binev, Cohen, Mula, Nichols 2018) of up to m of the ncand candidate points for PBDW on the span of
 * the n rows C[c_row0 ..): W = the A_1-orthonormal basis of that span (CGS2 with the dead-row rule of rom_error_curves: a
 * dead row gives a zero column of A), psi_k = the H^1_0-orthonormal basis of the picked points' representers in pick
 * order, Res[i,x] = (w_i - P_{W_k} w_i)(x), nu_x = ||omega_x||^2.  Criterion: mode 0 = collective OMP,
 * sum_i Res[i,x]^2 / nu_x; mode 1 = worst-case OMP, (sum_i alpha_i Res[i,x])^2 / nu_x with alpha a unit eigenvector of
 * A_k^T A_k for its smallest eigenvalue; 0 where nu_x = 0.  The pick is the first maximum.  1 <= n <= 128 (96 in mode 1),
 * 1 <= m <= 1024, ncand >= 1.  picks_out (m, int64; -1 past a stop), crit_out (m): best criterion per step,
 * A_out (m x n): A[k,i] = <psi_k, w_i>_{H^1_0}, alpha_out (m x n, mode 1, may be NULL): the direction used at step k,
 * info_host (4 doubles, may be NULL): dead basis rows, picks made, stop reason (0 m reached, 1 criterion below rel_tol x
 * the first step's, 2 no candidate with a positive criterion left), host synchronisations.  One host synchronisation at
 * the end. */
int rom_sensor_greedy(rom_fem* fem, rom_buf* C, int64_t c_row0, int n, int ncand, const int* ix_host, const int* iy_host,
                      const double* tx_host, const double* ty_host, int m, int mode, double rel_tol, int64_t* picks_out,
                      double* crit_out, double* A_out, double* alpha_out, double* info_host);

/* ---- the basis stage as single calls (rom_project_h10, rom_galerkin_rom, rom_greedy, rom_pod) --------
 * Each call enqueues all its kernels on the context's stream and waits for it once at its end (status word /
 * results); small dense problems (Gram matrices of the basis, projected eigenproblems, argmax of the greedy) are solved
 * on the device.  rom_pod additionally reads a few dozen spectrum values per pass to decide how many modes to accept. */
/* project_solutions (src/lib/SolutionsManagers.py:108-139): OUT[out_row0+m] = H^1_0-orthogonal projection of
 * U[u_row0+m] onto the span of the n rows C[c_row0 ...] (any full-rank rows; n = 0: zeros, :109-111).
 * ROM_ERR_NOT_SPD if C A_1 C^T is not positive definite (dependent rows). */
int rom_project_h10(rom_fem* fem, rom_buf* U, int64_t u_row0, int M, rom_buf* C, int64_t c_row0, int n, rom_buf* OUT,
                    int64_t out_row0);
/* generate_fm_solutions (:88-106): OUT[out_row0+m] = Galerkin reduced-order solution for a[m] (M x nrb*ncb) in the span
 * of the n rows of C (n = 0: zeros, :89-91) */
int rom_galerkin_rom(rom_fem* fem, rom_buf* a, int M, rom_buf* C, int64_t c_row0, int n, rom_buf* OUT, int64_t out_row0);
/* orthonormalize_base (src/lib/ReducedBasis.py:18-21): rows of X -> Euclidean-orthonormal rows of Q spanning the same
 * nested subspaces (the thin QR at :19 up to the sign of each row; a dependent row becomes zero).  Q may be X. */
int rom_orthonormalize_rows(rom_ctx* ctx, rom_buf* X, int64_t x_row0, int n, int64_t dim, rom_buf* Q, int64_t q_row0);
/* ReducedBasisGreedy.build (src/lib/ReducedBasis.py:112-139): strong greedy over the M training snapshots U[u_row0 ...]
 * in relative H^1_0 error; mode 0 = error of the H^1_0 projection (:122), 1 = error of the Galerkin ROM (:124, needs
 * the training parameters a, M x nrb*ncb).  h1norm_host: the M normalisations (solutions2train_h1norm, :129).
 * picks_out[i] = training index chosen in iteration i (first maximum, like np.argmax), max_err_out[i] = its relative
 * error, i < n.  Iteration 0 has the empty basis: with h1norm = rom_h10norm(U) every error is exactly 1.0 and the
 * pick is index 0, as in the reference. */
int rom_greedy(rom_fem* fem, rom_buf* U, int64_t u_row0, int M, rom_buf* a, const double* h1norm_host, int mode, int n,
               int64_t* picks_out, double* max_err_out);
/* H^1_0 error curves of the nested spans of the basis rows C[c_row0 .. +N) over the snapshots U[u_row0 .. +M), for every
 * dimension n = 0 .. N in one call (the statistics loop of the reference's experiment(), src/experiments/HighContrast.py:
 * 176-214, for all n at once):
 *   ERR[(0 * (N+1) + n) * M + m] = || u_m - P_n u_m ||_{H^1_0}      (P_n: A_1-orthogonal projector onto span C[0..n))
 *   ERR[(1 * (N+1) + n) * M + m] = || u_m - G_n(a_m) ||_{H^1_0}     (Galerkin ROM on span C[0..n); only when a != NULL,
 *                                                                    a: M x nrb*ncb parameters)
 * n = 0 is the empty basis (||u_m||).  Absolute errors: divide by the snapshot norms for the reference's relative ones.
 * Only the span counts: the call builds an A_1-orthonormal W row by row (two Gram-Schmidt rounds); a row whose residual
 * is at roundoff of its norm (the greedy's dead-vector rule) adds no direction, its curve is flat at that n.
 * P (M x N): p_mj = <u_m, w_j>_{A_1}, the coefficients of P_N u_m in W.  T (N x N, lower): C_i = sum_j T[i,j] w_j
 * (column j is 0 for a dependent row j).  info_host (4 doubles, may be NULL): dependent rows, Galerkin route
 * (-1 none, 0 reduced matrices in LDS, 1 in global memory: N > 64), passes over U, edge tiles per pass.
 * One host synchronisation at the end.  ROM_ERR_NOT_SPD if a reduced matrix has a non-positive pivot. */
int rom_error_curves(rom_fem* fem, rom_buf* U, int64_t u_row0, int M, rom_buf* C, int64_t c_row0, int N, rom_buf* a,
                     rom_buf* ERR, rom_buf* P, rom_buf* T, double* info_host);
/* PCA(n_components = n).fit (src/lib/ReducedBasis.py:196): leading n right singular vectors of the (M, dim) block
 * X[x_row0 ...] -- OVERWRITTEN when center != 0 (the column means are subtracted in place) -- into V[v_row0 ...] (n x dim, orthonormal rows,
 * scikit-learn's svd_flip(u_based_decision=False) signs) and their singular values into sigma_host (n).  Randomised
 * range-finder passes over the implicitly deflated block (thin products 2 b M dim, one power step, rows orthonormalised on
 * both sides of it: a pass resolves modes over seven orders of magnitude to LAPACK's own noise bound eps sigma_1 / sigma)
 * with a convergence rule per pass; when the first pass shows a spectrum that decays too slowly for that (its modes do not
 * separate from what lies beyond the sketch) the leading modes come from the M x M Gram matrix instead (MFMA, eigenpairs
 * iterated to convergence in M space) and the passes continue below its reach (1e-5 sigma_1).  Rayleigh-Ritz over the
 * collected modes; modes below 1e-13 sigma_1 do not exist in fp64 data and are completed with orthonormal directions of
 * singular value 0.  info_host (8 doubles or NULL): resolved modes, completed modes, Gram passes (0 or 1), sketch passes,
 * executed flops, 8 n M dim (the four thin products of a pass for the n modes alone), subspace iterations of the Gram
 * route, stop reason (0: all n modes resolved; 1: the spectrum reached the floor -- the completed modes are not determined
 * by the data; 2: a pass accepted nothing although the floor was not reached -- modes above it may be missing). */
int rom_pod(rom_ctx* ctx, rom_buf* X, int64_t x_row0, int M, int64_t dim, int n, int center, rom_buf* V, int64_t v_row0,
            double* sigma_host, double* info_host);
/* the same with the floor chosen by the caller: modes with sigma <= rel_floor * sigma_1 are not looked for (every sketch
 * pass over the block buys seven orders of magnitude; a reduced basis that is used to 1e-6 needs one pass).
 * rel_floor <= 1e-13 is rom_pod. */
int rom_pod_ex(rom_ctx* ctx, rom_buf* X, int64_t x_row0, int M, int64_t dim, int n, int center, double rel_floor, rom_buf* V,
               int64_t v_row0, double* sigma_host, double* info_host);
/* PCA(n_components = n).fit + .transform of a TALL block (src/experiments/NonLinearROM.py:34-41: 25,000 x 81): ALL the
 * information of the row-major (M, dim) block X[x_row0 ...], dim <= 1024, by a block one-sided Jacobi whose sweeps are Gram
 * matrices of the rotated data -- Y = Xc V^T, G = Y^T Y (dim x dim, from the DATA, never as V C V^T), Jacobi of G with the
 * relative stopping rule (rom_small_eig_host, gram_like = 2), V <- Q^T V -- until |g_ij| <= 64 eps max(d) max(d_i, d_j),
 * d_i = sqrt(g_ii), for all i != j (at most 6 passes; 3 are typical).  No sqrt(eps) floor as in a one-pass covariance
 * eigendecomposition: singular values come out to eps sigma_1 + M eps sigma_i over the whole fp64 range.
 * dim <= 96: one fused MFMA kernel per pass (rotation + Gram matrix + scores, the block read once).  Larger dim: rom_gemm_nt
 * + a TN Gram kernel; that form takes M <= 65535 * 64 rows and, unless S is given with n = dim, a temporary of M x dim doubles.
 * center != 0 subtracts the column means in place (X is OVERWRITTEN with the centred block, as in rom_pod).
 * V[v_row0 ...]: n x dim components, rows of a COMPLETE orthonormal basis (the rotation is square: nothing is completed
 * with random directions), scikit-learn's svd_flip(u_based_decision=False) signs.
 * S[s_row0 ...] (may be NULL): M x n scores Xc V^T (pca.transform).  mean (may be NULL): the dim column means (zeros when
 * center = 0).  sigma_host (n): the measured 2-norm of score column i, descending, also below the noise floor.
 * Meant for M >= dim, correct for any M >= 1 (a wide block has dim - rank modes at noise level); 0 <= n <= dim.
 * info_host (8 doubles or NULL): resolved modes #{sigma_i > 1e-13 sigma_1} among the n, passes over the block, Jacobi
 * decompositions, executed flops, largest |g_ij| / tol_ij of the last pass, stop reason (0 converged, 1 pass budget), host
 * synchronisations, 0.  Host synchronisations: one per pass, one at the end, one where the modes are put in order; for
 * dim > 96 the grid-wide Jacobi adds one per sweep and three per decomposition (DESIGN.md 5.6 gives typical counts).
 * Deterministic (fixed-order partial sums, no floating-point atomics).  NaN / Inf entries are an error, as in rom_pod. */
int rom_pca_tall(rom_ctx* ctx, rom_buf* X, int64_t x_row0, int M, int dim, int n, int center, rom_buf* V, int64_t v_row0,
                 rom_buf* S, int64_t s_row0, rom_buf* mean, double* sigma_host, double* info_host);
/* ---- the basis stage on a snapshot block held in FACTORED form ---------------------------------------------------------
 * A sweep gathered from several GPUs exists on every rank as interface vectors, not as rows (rom_comm_allgather_packed_
 * async); when rom_fem_expansion_is_linear() the rows are U = Y B^T with a fixed B, so the builders below work on the
 * (M, Kc) block of COMPACT interface vectors (Kc = rom_fem_compact_stride(); rom_fem_pack_reduced_async makes them) and
 * never form a row except the basis vectors they return.  Same reference bodies as the row calls above
 * (src/lib/ReducedBasis.py:112-139, :189-200); same contracts, same picks / modes up to rounding.
 * rom_fem_energy_map builds (once per FE space, cached on the fem) the geometry of the snapshots in those coordinates:
 * parts 1 = H^1_0 inner product (norms, greedy), 2 = the block forms u^T A_b v and the load functional (Galerkin greedy),
 * 4 = Euclidean inner product (POD); part 1 keeps the way back from its coordinates (rom_pod_h10_factored), 8 is accepted as
 * 1; the other calls build what they need themselves.  k_h10 / k_l2 (may be NULL): ranks. */
int rom_fem_energy_map(rom_fem* fem, int parts, int* k_h10, int* k_l2);
/* H10norm (src/lib/SolutionsManagers.py:56-58) of M snapshots from their compact interface vectors Yc[c_row0 ...] */
int rom_h10norm_factored(rom_fem* fem, rom_buf* Yc, int64_t c_row0, int M, double* out_host);
/* rom_greedy on compact interface vectors (M x Kc); a: M x nrb*ncb parameters (mode 1) */
int rom_greedy_factored(rom_fem* fem, rom_buf* Yc, int64_t c_row0, int M, rom_buf* a, const double* h1norm_host, int mode,
                        int n, int64_t* picks_out, double* max_err_out);
/* rom_pod on compact interface vectors (M x Kc, not modified): V[v_row0 ...] receives the n modes as ROWS (n x dim);
 * n <= 65535 (here and in rom_pod_h10_factored): ROM_ERR_INVALID beyond */
int rom_pod_factored(rom_fem* fem, rom_buf* Yc, int64_t c_row0, int M, int n, int center, rom_buf* V, int64_t v_row0,
                     double* sigma_host, double* info_host);
/* ---- the H^1_0 inner product in spectral form: POD in the energy norm -----------------------------------------------------
 * A_1 = S Lambda S with S = S_r (x) S_c the orthogonal 2-D sine transform of the interior grid and Lambda[j,k] = lam_r[j] +
 * lam_c[k] (the tables of rom_riesz_h10, built once per FE space).  The reference's greedy is parameterised by norm
 * (get_function_norm("l2" | "h10"), src/lib/ReducedBasis.py); its PCA (src/lib/ReducedBasis.py:189-200) is "optimal with
 * respect to L2" only (InverseProblemPipeline.ipynb, "Optimal in which sense?"): these calls fill the {POD} x {H^1_0} cell. */
/* OUT_i = Lambda^(post/2) o ( S_r (Lambda^(pre/2) o X_i) S_c ), i < K; pre, post in {-2,-1,0,1,2}; X not modified, OUT != X.
 * (pre, post) = (0,1): H^1_0 -> Euclidean coordinates; (-1,0): the way back; (0,-2) then (0,0): A_1^{-1} of dense rows.
 * X_i = row x_row0 + i as an nr x nc array.  Two MFMA products per row (the one over the grid rows a strided-batched kernel
 * with the scalings fused); no floating-point atomics: the same bits on every call with the same arguments and workspace limit.
 * Workspace: K x dim doubles, fewer rows at a time under rom_set_workspace_limit (the product over the columns may then take
 * another route of rom_gemm_nn: equal to rounding).  One host synchronisation at the end. */
int rom_sine_transform(rom_fem* fem, rom_buf* X, int64_t x_row0, int K, int pre, int post, rom_buf* OUT, int64_t out_row0);
/* rom_pod_ex in the H^1_0 inner product; X is NOT modified; rows of V are A_1-orthonormal, svd_flip sign on the returned rows.
 * The n-dimensional space that minimises sum_m ||x_m - P_n x_m||^2_{H^1_0}: the Euclidean POD (rom_pod_ex: same floor, same
 * completion, same NaN / Inf error) of the block in energy coordinates W_m = sqrt(Lambda) o (S_r X_m S_c) -- an M x dim
 * temporary, centred there when center != 0 -- with the modes taken back by v_i = S_r (Lambda^-1/2 o q_i) S_c.  sigma_host (n):
 * singular values of the block in the H^1_0 geometry (sum_{i>n} sigma_i^2 = the squared H^1_0 projection error of the whole
 * block); completed modes have sigma = 0.  info_host (8 doubles or NULL) as rom_pod, executed flops including the transforms. */
int rom_pod_h10(rom_fem* fem, rom_buf* X, int64_t x_row0, int M, int n, int center, double rel_floor, rom_buf* V, int64_t v_row0,
                double* sigma_host, double* info_host);
/* the same on compact interface vectors (M x Kc, not modified; rom_pod_factored with the H^1_0 coordinates of
 * rom_fem_energy_map, part 1, in place of the Euclidean ones): V[v_row0 ...] receives the n modes as ROWS (n x dim) */
int rom_pod_h10_factored(rom_fem* fem, rom_buf* Yc, int64_t c_row0, int M, int n, int center, rom_buf* V, int64_t v_row0,
                         double* sigma_host, double* info_host);
/* n nearly orthonormal rows of V -> orthonormal rows, each as close as possible to what it was: V <- (V V^T)^(-1/2) V */
int rom_symmetric_orthonormalize(rom_ctx* ctx, rom_buf* V, int64_t v_row0, int n, int64_t dim);
/* rows V[v_row0+found .. +found+rest) <- deterministic pseudo-random directions, orthonormal and orthogonal to the
 * orthonormal rows V[v_row0 .. +found): how rom_pod completes a request beyond what the data determine */
int rom_complete_orthonormal(rom_ctx* ctx, rom_buf* V, int64_t v_row0, int found, int rest, int64_t dim);
/* the device eigen-solver the calls above use for their small symmetric problems (cyclic Jacobi, one workgroup), for
 * n x n host matrices, n <= 1024: mode 0 T = eigenvector rows (eigenvalues descending in lam_host); 1 T = whitening
 * transform Lambda^-1/2 Q^T (rows with lambda <= rel_tol lambda_max zero); 2 T = Q Lambda^-1/2 Q^T; 3 (n <= 96) T =
 * the rank-revealing whitening transform [L_r^-1 0] P of the pivoted Cholesky factorisation P A P^T = L L^T (lam_host:
 * squared pivots), what the orthonormalisations of rom_pod use.
 * gram_like != 0: A is a Gram matrix of explicit rows (entries accurate relative to sqrt(a_pp a_qq): small eigenvalues
 * of graded matrices come out to high relative accuracy); 0: general symmetric matrix (absolute accuracy).  gram_like = 2:
 * the same with the rotation threshold 16 eps sqrt(a_pp a_qq) instead of n eps (what rom_pca_tall uses).  Test hook. */
int rom_small_eig_host(rom_ctx* ctx, int n, const double* A_host, int mode, double rel_tol, int gram_like,
                       double* lam_host, double* T_host);
/* ---- residual error bounds of the Galerkin ROM and the weak greedy (no truth snapshots) ------------------------------------
 * A(a) = sum_q a_q A_q (k = nrb*ncb blocks, A_q positive semidefinite, sum_q A_q = A_1), so for the Galerkin solution u_n(a)
 * on span C[0..n):   ||r|| / max_q a_q <= ||u(a) - u_n(a)||_{H^1_0} <= ||r|| / min_q a_q ,  r = f - A(a) u_n in the H^-1 norm.
 * With W the A_1-orthonormal basis of the span (CGS2, the dead-row rule of rom_error_curves), r = sum_j z_j g_j over the
 * P = 1 + k n functionals g_0 = f, g_{1+ik+q} = A_q w_i with z = (1, -c_i a_q), c the solution of the reduced system in W.
 * The handle keeps the g_j in H^-1 coordinates (rom_sine_transform (0, -1)) ORTHONORMALISED: g^_j = sum_i R_ij q_i with
 * Euclidean-orthonormal rows q_i, and ||r|| = ||R z||_2 -- the form z^T G z with the Gram matrix of the g^_j stops at
 * sqrt(eps) ||f|| and is never formed.  A functional whose remainder after two Gram-Schmidt rounds is below 1e-14 of its norm
 * adds no row (the g_j are rank deficient by construction).  The ordering is i-major: the first 1 + k n' functionals are
 * those of the nested basis n'.  No floating-point atomics anywhere: the same bits on a repeated call. */
typedef struct rom_resid rom_resid;
/* an empty estimator (n = 0: ||f||) for at most n_cap basis rows; workspace (2 n_cap + 2 k + P_cap) dim doubles */
int rom_resid_create(rom_fem* fem, int n_cap, rom_resid** out);
int rom_resid_destroy(rom_resid* h);
/* extend the basis by the rows C[c_row0 .. +rows) (not modified).  One host synchronisation per functional (k per row) and one
 * per row. */
int rom_resid_append(rom_resid* h, rom_buf* C, int64_t c_row0, int rows);
/* out8: rows n, live rows, P, rank, n_cap, k, dim, host synchronisations so far */
int rom_resid_query(rom_resid* h, int64_t* out8);
/* test hook, host copies: what = 0 R (rank x P), 1 Q (rank x dim), 2 the reduced tensor W A_q W^T (k x n x n, a dead direction
 * has a unit diagonal), 3 W f (n), 4 W (n x dim), 5 the rank after n' rows for n' = 0 .. n (n + 1), 6 dead flags (n).
 * count must be the size of the part. */
int rom_resid_download(rom_resid* h, int what, double* host, size_t count);
/* OUT[out_row0 .. +n) = W: u_n = c W through rom_gemm_nn with the COEF of rom_resid_eval */
int rom_resid_basis(rom_resid* h, rom_buf* OUT, int64_t out_row0);
/* DELTA[d_off + m] = weights[m] ||r(a_m)||_{H^-1} (weights NULL: 1) for the parameters a[a_row0 .. +M) (M x k) and the
 * nested basis of the first n <= built rows; n = 0 gives ||f||_{H^-1}.  COEF (may be NULL) receives c, the coordinates of
 * u_n in W (M x n from row coef_row0: ||u_n||_{H^1_0} = ||c||_2); without it the call takes M x n doubles of workspace.
 * Reduced solves: one launch per 2^18 parameters; then one MFMA kernel whose A operand z is formed as it is staged.
 * One host synchronisation.  ROM_ERR_NOT_SPD if a reduced matrix has a non-positive pivot. */
int rom_resid_eval(rom_resid* h, rom_buf* a, int64_t a_row0, int64_t M, int n, rom_buf* weights, rom_buf* DELTA, int64_t d_off,
                   rom_buf* COEF, int64_t coef_row0);
/* Weak greedy over the M parameters a (M x k) with a fresh handle h of capacity >= n_max.  Per step: evaluate all M with the
 * basis so far; the first maximum of weights[m] ||r(a_m)|| among the parameters not yet picked (np.argmax); stop when it is
 * <= rel_tol times the first step's; solve the picked parameter (rom_solve_batch) into BASIS[basis_row0 + step] -- raw
 * snapshots in pick order -- and append it to h.  picks_out / crit_out (n_max entries): picks and their criteria.
 * info_host (6 doubles or NULL): picks made, dead rows, stop reason (0 n_max, 1 rel_tol, 2 every parameter picked), final
 * rank, host synchronisations, the last criterion evaluated.  Workspace M (n_max + 1) doubles besides the handle's: no
 * M x dim block exists.  ROM_ERR_NOT_SPD as rom_resid_eval. */
int rom_weak_greedy(rom_fem* fem, rom_buf* a, int64_t M, rom_buf* weights, int n_max, double rel_tol, rom_resid* h,
                    rom_buf* BASIS, int64_t basis_row0, int64_t* picks_out, double* crit_out, double* info_host);

/* ---- polynomial maps between columns of a tall block (src/experiments/NonLinearROM.py:54-70,131-139) ------------------------
 * The least-squares fit of q target columns as polynomials of total degree <= d in m input columns over M rows: what the
 * reference's pipelines PolynomialFeatures(d) + LinearRegression compute (src/experiments/NonLinearROM.py:54-70,131-139), in
 * the basis of the P = C(m + d, d) products prod_j L_{alpha_j}(t_j), |alpha| <= d, of Legendre polynomials of t_j = (x_j - c_j)
 * / h_j (c_j, h_j: mid-range and half-range of input column j over the training rows; a constant column has t_j = 0).  The
 * same function space as scikit-learn's monomials -- the same fitted function whenever the problem has full rank -- without
 * their conditioning: the result does not depend on the scales of the input columns.  1 <= m <= 16, 1 <= d <= 8, P <= 96,
 * 1 <= q <= 1024, M >= 1.
 * Method: CholeskyQR in passes over the block, Gram matrices always from the data (as rom_pca_tall): G = Psi^T Psi and
 * B = Psi^T Y of Psi = Phi T^T by slabs of 32 rows in one MFMA kernel per pass and group of 96 target columns; pass 1 (T = I)
 * gives the rank-revealing whitening transform of the column-normalised G (rom_small_eig_host's mode 3); a term is DROPPED
 * there when its squared pivot is <= rcond^2 times the largest (rcond <= 0: sqrt(P eps), the noise level of a Cholesky
 * factorisation of a Gram matrix); pass 2 has G = I + delta and W = T^T G^-1 B; a further pass only while P |delta|_max > 1/3,
 * at most 4 passes.  When rank < P the result is a least-squares minimiser with the dropped terms' coefficients ZERO, not
 * scikit-learn's minimum-norm one.  No floating-point atomics: the same bits on a repeated call.  NaN / Inf among the training
 * inputs or targets are an error.  One host synchronisation per pass, one per re-whitening and one at the end. */
typedef struct rom_poly rom_poly;
/* (src/experiments/NonLinearROM.py:54-70,131-139) host only, no context: P = C(m+d,d) and (powers_out != NULL) the P x m
 * exponent rows in scikit-learn's order, PolynomialFeatures(d).powers_ */
int rom_poly_terms(int m, int d, int* P_out, int* powers_out);
/* (src/experiments/NonLinearROM.py:54-70,131-139: model.fit) X: M rows, m columns from element x_off with row stride ldx; Y
 * likewise (q columns).  Neither is modified.  info_host (8 doubles or NULL): P, rank, passes, |delta|_max of the accepted
 * pass, smallest kept / largest squared pivot of pass 1, executed flops, host synchronisations, stop reason (0 full rank,
 * 1 terms dropped, 2 pass budget reached). */
int rom_poly_fit(rom_ctx* ctx, rom_buf* X, size_t x_off, int64_t ldx, int m, rom_buf* Y, size_t y_off, int64_t ldy, int q,
                 int64_t M, int d, double rcond, rom_poly** out, double* info_host);
/* (src/experiments/NonLinearROM.py:54-70,131-139: model.predict and the error) OUT (may be NULL) <- prediction, or Yref -
 * prediction when Yref != NULL; sumsq_host (q, may be NULL): column sums of squares of what OUT receives (fixed-order
 * partials).  OUT == NULL requires sumsq_host != NULL.  OUT must not overlap X.  One host synchronisation. */
int rom_poly_predict(rom_poly* h, rom_buf* X, size_t x_off, int64_t ldx, int64_t M, rom_buf* OUT, size_t o_off, int64_t ldo,
                     rom_buf* Yref, size_t r_off, int64_t ldr, double* sumsq_host);
/* (src/experiments/NonLinearROM.py:54-70,131-139) out8: m, d, P, q, rank, M_train, passes, host synchronisations so far */
int rom_poly_query(rom_poly* h, int64_t* out8);
/* (src/experiments/NonLinearROM.py:54-70,131-139) host copies: what = 0 c (m), 1 h (m), 2 W (q x P: coefficients of the
 * Legendre products, LinearRegression.coef_ in that basis), 3 dropped flags of pass 1 (P).  count must be the size of the part. */
int rom_poly_download(rom_poly* h, int what, double* host, size_t count);
int rom_poly_destroy(rom_poly* h);

/* ---- MLP maps between columns of a tall block (src/experiments/NonLinearROM.py:54-70,138, src/lib/Estimators.py:75-97) ------
 * The "NN" entry of the reference's model list and the regressor of EstimatorNN: a fully connected network from m input columns
 * through 1 .. 3 hidden layers (tanh, logistic or relu; linear output) to q target columns over M rows.  Inputs are scaled as
 * in rom_poly_fit, t_j = (x_j - c_j) / h_j (a constant column has t_j = 0); with scale_targets the targets are centred by the
 * column mean and divided by the column standard deviation over the training rows (a constant column: its value and 1),
 * without it mean 0 and scale 1.  Loss (scikit-learn's): L(w) = 1/(2M) sum_rows |net(t) - y_scaled|^2 + alpha/(2M) sum_l
 * |W_l|_F^2, biases not penalised; prediction y_mean + y_scale net((x - c) / h).
 * Limits: 1 <= m <= 64, hidden widths 1 .. 64, 1 <= q <= 128, M >= 1, and TWO rules on the padded shape (every width, m
 * included, padded to a multiple of 16): sum_l K_l^pad N_l^pad <= 9216 doubles, and the LDS of the evaluation kernel at one
 * workgroup per CU <= 160 KB.  That kernel keeps the padded weights (row stride K^pad + 2), the biases and one 32-row slab
 * [A_0 | .. | A_L | Delta_1 | .. | Delta_L+1] (stride columns + 2) in LDS, + 5 KB of scalings and scratch.  The budget is
 * 9216, not 8192, because the widest output 1 -> 64 -> 128 is 16 x 64 + 64 x 128 = 9216 (150 KB of LDS: it fits); no budget
 * alone bounds the LDS (48 -> 32 -> 64 -> 16 -> 128 has 6656 padded weights and needs more than 160 KB, 16 -> 64 -> 64 -> 16
 * has 6144 and needs 129 KB), hence the second rule.  rom_mlp_layout reports both numbers.  ROM_ERR_INVALID outside the limits.
 * Optimiser: full-batch L-BFGS (two-loop recursion, gamma = s.y / y.y), first step min(1, 1/|g|_2) then 1, Armijo backtracking
 * (c1 = 1e-4, halving, 30 trials), a pair kept when s.y > 1e-10 |s| |y|, steepest descent with cleared memory when g.d >= 0;
 * stops at |g|_inf <= tol, at a relative loss decrease <= tol 1e-2 on two consecutive accepted iterations, at max_iter, or when
 * the line search is exhausted.  All of it runs on the device (one director workgroup between evaluations); the host enqueues
 * 16 (evaluation, reduction, director) sequences and reads a status word once per such batch.  No floating-point atomics: the
 * same bits on a repeated call.  NaN / Inf among the training inputs, targets or initial weights are an error. */
typedef struct rom_mlp rom_mlp;
/* (src/experiments/NonLinearROM.py:54-70,138, src/lib/Estimators.py:75-97) host only, no context; the single place of the
 * limits.  hidden: n_hidden widths.  out8: parameters P, padded weight doubles, LDS bytes of the evaluation kernel, LDS bytes
 * of the prediction kernel, weight layers n_hidden + 1, doubles of a workgroup's partial, weights among the parameters, 0.
 * offsets (2 (n_hidden + 1), or NULL): the offset of every W_l (row-major, outputs x inputs), then of every b_l, in the flat
 * parameter vector -- all W in layer order, then all b. */
int rom_mlp_layout(int m, int n_hidden, const int* hidden, int q, int64_t* out8, int64_t* offsets);
/* (src/experiments/NonLinearROM.py:54-70,138, src/lib/Estimators.py:75-97: model.fit) X, Y as in rom_poly_fit; neither is
 * modified.  activation: 0 tanh, 1 logistic, 2 relu.  w0_host: the P initial parameters in the layout above.  memory: L-BFGS
 * pairs, 1 .. 64.  max_iter = 0: the handle holds w0 and the scalings of the data.  info_host (8 doubles or NULL): iterations,
 * loss / gradient evaluations, final loss, final |g|_inf, stop reason (0 gradient tolerance, 1 loss stagnation, 2 iteration
 * budget, 3 line search failed), kernel launches, host synchronisations, executed flops (6 M sum K^pad N^pad per evaluation). */
int rom_mlp_fit(rom_ctx* ctx, rom_buf* X, size_t x_off, int64_t ldx, int m, rom_buf* Y, size_t y_off, int64_t ldy, int q, int64_t M,
                int n_hidden, const int* hidden, int activation, double alpha, int scale_targets, const double* w0_host,
                int max_iter, double tol, int memory, rom_mlp** out, double* info_host);
/* (src/experiments/NonLinearROM.py:54-70,138, src/lib/Estimators.py:75-97) L and its gradient (P doubles, the layout above) at
 * the handle's weights on any block of M rows, with the handle's scalings: what the optimiser evaluates.  One host
 * synchronisation. */
int rom_mlp_loss_grad(rom_mlp* h, rom_buf* X, size_t x_off, int64_t ldx, rom_buf* Y, size_t y_off, int64_t ldy, int64_t M,
                      double alpha, double* loss_host, double* grad_host);
/* (src/experiments/NonLinearROM.py:54-70,138, src/lib/Estimators.py:75-97: model.predict and the error) the contract of
 * rom_poly_predict: OUT (may be NULL) <- prediction, or Yref - prediction; sumsq_host (q, may be NULL): column sums of squares
 * of that, from fixed-order partials.  OUT == NULL requires sumsq_host.  OUT must not overlap X.  One host synchronisation. */
int rom_mlp_predict(rom_mlp* h, rom_buf* X, size_t x_off, int64_t ldx, int64_t M, rom_buf* OUT, size_t o_off, int64_t ldo,
                    rom_buf* Yref, size_t r_off, int64_t ldr, double* sumsq_host);
/* (src/experiments/NonLinearROM.py:54-70,138, src/lib/Estimators.py:75-97) out8: m, q, hidden layers, P, M_train, iterations,
 * kernel launches, host synchronisations so far */
int rom_mlp_query(rom_mlp* h, int64_t* out8);
/* (src/experiments/NonLinearROM.py:54-70,138, src/lib/Estimators.py:75-97) host copies: what = 0 w (P), 1 c (m), 2 h (m),
 * 3 y_mean (q), 4 y_scale (q), 5 the loss after every accepted iteration (iterations + 1).  count must be the size. */
int rom_mlp_download(rom_mlp* h, int what, double* host, size_t count);
int rom_mlp_destroy(rom_mlp* h);

/* ---- regression trees and bagged forests on columns of a tall block (src/experiments/NonLinearROM.py:54-70,136-137) ----------
 * What the reference's DecisionTreeRegressor() and RandomForestRegressor(n_estimators=10) compute: T multi-output CART trees
 * from m input columns (1 <= m <= 16) to q target columns (1 <= q <= 128) over M rows, 1 <= T <= 256, built LEVEL BY LEVEL
 * over all trees at once.  counts_host (T x M int32 >= 0, or NULL: all 1) are the bootstrap multiplicities of the rows per
 * tree; a row of count 0 does not exist for that tree; a tree without rows is an error.
 * Criterion: weighted MSE summed over the targets -- the candidate that maximises sum_k S_Lk^2 / n_L + S_Rk^2 / n_R, the sums
 * formed on targets shifted by the node's mean.  Candidates lie between consecutive distinct values lo < hi of one input among
 * the node's rows, both sides keeping a weighted count >= min_samples_leaf; threshold lo + (hi - lo) / 2 (lo if that is >=
 * hi); a row goes left iff x <= threshold.  Ties: largest gain, then lowest input, then lowest position.  A node is a leaf
 * iff n < min_samples_split, depth == max_depth (0: no limit), no valid candidate, or every target is constant over its rows.
 * Leaf value: weighted mean (bit for bit the row when the targets are constant).  Forest prediction: mean over the trees,
 * summed in tree order.  No floating-point atomics: the same bits on a repeated call.  NaN / Inf among the training inputs
 * or targets are an error.  One host synchronisation per level. */
typedef struct rom_tree rom_tree;
/* (src/experiments/NonLinearROM.py:54-70,136-137: model.fit) X, Y as in rom_poly_fit; neither is modified.  info_host (8
 * doubles or NULL): nodes, leaves, deepest level, levels run, kernel launches, host synchronisations, bytes of workspace, 0. */
int rom_tree_fit(rom_ctx* ctx, rom_buf* X, size_t x_off, int64_t ldx, int m, rom_buf* Y, size_t y_off, int64_t ldy, int q,
                 int64_t M, int T, const int32_t* counts_host, int max_depth, int min_samples_split, int min_samples_leaf,
                 rom_tree** out, double* info_host);
/* (src/experiments/NonLinearROM.py:54-70,136-137: model.predict and the error) as rom_poly_predict: OUT (may be NULL) <-
 * prediction, or Yref - prediction; sumsq_host (q, may be NULL): column sums of squares of that, from fixed-order partials.
 * OUT must not overlap X.  One host synchronisation. */
int rom_tree_predict(rom_tree* h, rom_buf* X, size_t x_off, int64_t ldx, int64_t M, rom_buf* OUT, size_t o_off, int64_t ldo,
                     rom_buf* Yref, size_t r_off, int64_t ldr, double* sumsq_host);
/* (src/experiments/NonLinearROM.py:54-70,136-137) out8: m, q, T, M_train, nodes in all trees, deepest level, kernel launches,
 * host synchronisations so far */
int rom_tree_query(rom_tree* h, int64_t* out8);
/* (src/experiments/NonLinearROM.py:54-70,136-137) host copies, the trees one after the other, each in breadth-first order:
 * what = 0 first node of each tree (T + 1), 1 input of the split (-1 at a leaf), 2 threshold, 3 left child (the right child is
 * left + 1; -1 at a leaf), 4 weighted count (one value per node each), 5 values (nodes x q).  count must be the size. */
int rom_tree_download(rom_tree* h, int what, double* host, size_t count);
int rom_tree_destroy(rom_tree* h);

/* ---- nearest rows of a tall library: the search of the library-based parameter estimation (src/lib/Estimators.py) ----------
 * For each of the K query rows of P, the t rows of the library Q (M rows) at the smallest squared Euclidean distance.  Q and P:
 * r columns from an element offset with a row stride, as in rom_poly_fit; neither is modified.  1 <= r <= 128, 1 <= t <= 8,
 * t <= M; K = 0 is a no-op.
 * dist2_host[k t + s] = sum_c (p_c - q_c)^2, formed from the original operands as differences (never a Gram expansion) by ONE
 * device function with one summation order: within (r + 2) eps (eps = 2^-52) relative of the exact value, exactly 0.0 for a
 * coincident row.  idx_host[k t .. + t) = the t rows that are smallest under the order (that value, row index), in that order:
 * bit for bit what an exhaustive scan with that function returns.  NaN / Inf in either operand: ROM_ERR_INVALID.  No floating-
 * point atomics: the same bits on a repeated call.
 * mode 0: screened search -- scores |q~|^2 - 2 p~ . q~ on operands shifted by the library's column means, one MFMA kernel that
 * writes only the minimum of every group of G = 32 rows and query (K x ceil(M / 32) doubles, the queries in passes when that
 * would exceed the workspace limit or 65535 tables (128 queries per table, 64 when r > 64)); per query the T' = t + 4 groups
 * of smallest minima are rescored exactly, and a certificate with a proven bound on the screen's error decides whether the
 * rows not rescored can be excluded; the queries it does not certify go to the exhaustive kernel.  mode 1 (test hook): the
 * exhaustive kernel for every query.
 * info_host (8 doubles or NULL): G, T', queries certified by the screen, queries sent to the exhaustive kernel, kernel launches,
 * host synchronisations, bytes of workspace, executed flops. */
int rom_nearest(rom_ctx* ctx, rom_buf* Q, size_t q_off, int64_t ldq, int64_t M, rom_buf* P, size_t p_off, int64_t ldp, int K, int r,
                int t, int mode, int64_t* idx_host, double* dist2_host, double* info_host);

/* ---- k-means on a tall block: the clustering of the local reduced bases (romhighcontrast_amd/local.py) --------------------------
 * Lloyd's algorithm on the M rows of X (r columns from an element offset with a row stride, as in rom_poly_fit; never modified)
 * against kc centroids.  Limits: 1 <= r <= 128, 1 <= kc <= 256, padded kc (to 16) x padded r (to 4) <= 8192 doubles -- (64, 128),
 * (128, 64) and (256, 32) are inside -- and kc <= M < 2^31; ROM_ERR_INVALID outside, and for NaN / Inf in the block or the
 * initial centroids.
 * The answer is defined as rom_nearest defines its own: dist2 = sum_c (x_c - c_c)^2 from the original operands by the ONE device
 * function of rom_nearest (differences first, one fma chain in column order: within (r + 2) eps relative of the exact value, 0.0
 * for a coincident row), and the label of a row is the centroid that is smallest under the order (that value, centroid index):
 * bit for bit what an exhaustive scan returns.  mode 1 (test hook and definition) is that scan; mode 0, the product path, is one
 * fused MFMA kernel per iteration -- screen scores |c~|^2 - 2 x~ . c~ on operands shifted by the column means mu of the block,
 * exact rescoring of every centroid within a proven bound of the smallest score, one-hot accumulation of the cluster sums and
 * counts -- and returns the same bits.  Update: c_j = mu + (sum of x - mu over the members, fixed order) / n_j; an empty cluster
 * keeps its centroid bit for bit and reports the count 0.
 * Iteration t assigns against C_t and updates to C_t+1.  It stops when no label changed (converged), when max_j |C_t+1,j -
 * C_t,j|^2 <= tol x (mean column variance of the block), or at max_iter; the call always ends with an assignment against the
 * centroids it returns, which labels, counts and the last inertia refer to.  The stop test runs on the device; the host
 * enqueues iterations in groups of 8 and reads one status word per group: host synchronisations <= 2 + ceil(iterations / 8).
 * No floating-point atomics: the same bits on a repeated call. */
typedef struct rom_kmeans rom_kmeans;
/* (local reduced bases: no counterpart in the reference) host only, no context; the single place of the limits and of the LDS
 * carve-up of the fused kernel.  out8: padded r, padded kc, LDS bytes of the fused kernel, rows of a slab (a workgroup's chunk
 * is a whole number of them), padded r + 1, row stride of the score / one-hot tile, doubles of a workgroup's partial,
 * accumulator tiles per wave. */
int rom_kmeans_layout(int r, int kc, int64_t* out8);
/* (local reduced bases) deterministic farthest-point start: rows_host[0] = the row nearest to the column means, rows_host[s] =
 * the row farthest from the rows chosen before it (largest minimum of dist2), the lowest row index among equals in both.  One
 * small kernel per centre, one host synchronisation. */
int rom_kmeans_init_maximin(rom_ctx* ctx, rom_buf* X, size_t x_off, int64_t ldx, int r, int64_t M, int kc, int64_t* rows_host);
/* (local reduced bases) init_host: kc x r initial centroids.  max_iter = 0: the handle holds the initial centroids and their
 * assignment.  info_host (8 doubles or NULL): iterations, converged (0 / 1), kernel launches, host synchronisations, bytes of
 * workspace, workgroup chunks, rows rescored beyond the first candidate (all passes), executed flops. */
int rom_kmeans_fit(rom_ctx* ctx, rom_buf* X, size_t x_off, int64_t ldx, int r, int64_t M, int kc, const double* init_host,
                   int max_iter, double tol, int mode, rom_kmeans** out, double* info_host);
/* (local reduced bases) labels (and dist2_host, inertia_host: either may be NULL) of any block of M rows against the handle's
 * centroids, by the same kernels.  One host synchronisation. */
int rom_kmeans_assign(rom_kmeans* h, rom_buf* X, size_t x_off, int64_t ldx, int64_t M, int mode, int32_t* labels_host,
                      double* dist2_host, double* inertia_host);
/* (local reduced bases) out8: r, kc, M_train, iterations, converged, stop reason (0 no label changed, 1 tolerance, 2 iteration
 * budget), kernel launches, host synchronisations so far */
int rom_kmeans_query(rom_kmeans* h, int64_t* out8);
/* (local reduced bases) host copies: what = 0 centroids (kc x r), 1 counts (kc), 2 inertia of the assignment of every iteration,
 * then of the final one (iterations + 1), 3 the shift mu (r), 4 labels of the training rows (M_train, as doubles).  count must
 * be the size of the part. */
int rom_kmeans_download(rom_kmeans* h, int what, double* host, size_t count);
int rom_kmeans_destroy(rom_kmeans* h);

/* ---- the polish of the library-based parameter estimation (romhighcontrast_amd/inverse.py::polish_parameters) ----------------
 * Levenberg-Marquardt in theta = log a for  min ||p - G_r c(theta)||^2 + perp2,  c(theta) = (sum_q e^theta_q Ahat_q)^-1 bhat,
 * for K queries from t starts each: the algorithm of polish_parameters (damping, acceptance, lambda schedule, eight trials, the
 * `still`, `tiny` and rounding-level rules, `converged`) in reduced sensor coordinates: with the compact SVD diag(w) E^T = U S V^T
 * of rank r, P (K rows of r from an element offset with a row stride) holds p = U^T (w y), Gr (r x n) = S V^T, and AUX (K x 2)
 * per query perp2 = ||(I - U U^T)(w y)||^2 and scale = max|w y| (NULL: 0 and max|p|).  Ahat (k, n, n) compact, bhat (n),
 * THETA0 (K, t, k) the starts, lo_host / hi_host (k each) the box.  One workgroup per (query, start) runs the whole iteration in
 * one launch; a second kernel keeps the start of smallest misfit per query (the lowest index among equals).
 * OUT row of query q (ldo >= k + n + 5 doubles apart, from out_off): theta (k) | c (n) | misfit = sqrt(|p - G_r c|^2 + perp2) |
 * sigma_min of the final Jacobian (one-sided Jacobi on its k columns) | converged (0 / 1) | iterations | start.
 * 1 <= n <= 64, 1 <= k <= 16, 1 <= r <= 64, 1 <= t <= 8: ROM_ERR_INVALID outside; K = 0 is a no-op; max_iter = 0 only evaluates
 * the starts.  A non-positive pivot of A(theta) in a trial rejects the trial, at a start it is ROM_ERR_NOT_SPD.  No input buffer
 * is modified; no floating-point atomics: the same bits on a repeated call.  One host synchronisation.
 * info8_host (8 doubles or NULL): kernel launches, host synchronisations, bytes of workspace, systems K t, LM iterations executed,
 * n x n factorisations executed (both summed on the device in integers), 0, 0. */
int rom_lm_polish(rom_ctx* ctx, int n, int k, int r, rom_buf* Ahat, rom_buf* bhat, rom_buf* Gr, rom_buf* P, size_t p_off, int64_t ldp,
                  int K, int t, rom_buf* THETA0, const double* lo_host, const double* hi_host, rom_buf* AUX, int max_iter,
                  double misfit_tol, rom_buf* OUT, size_t out_off, int64_t ldo, double* info8_host);

/* ---- posterior sampling of the parameters (romhighcontrast_amd/inverse.py::mcmc_host) ------------------------------------------
 * Which parameters are compatible with noisy data: adaptive random-walk Metropolis in theta = log a on the box [lo, hi]^k with a
 * uniform prior, for the potential Phi(theta) = ||p - G_r c(theta)||^2 in the reduced sensor coordinates of rom_lm_polish (Ahat,
 * bhat, Gr, P as there) and the log-posterior -invvar Phi / 2 inside the box; INVVAR (K) = 1 / sigma^2 per query, LPROP (K, k, k)
 * row-major lower triangular: the query's proposal factor L.  One CHAIN is a pair (query, chain index), K t of them, one workgroup
 * each with the loop over the steps inside the launch; the algorithm is mcmc_host's, step for step.  Step i (the global index,
 * step0 <= i < step0 + steps): k standard normals xi and a uniform u from Philox4x32-10 with the key (seed low word, seed high
 * word) and the counter (i, chain id low, chain id high, purpose), chain id = chain0 + the chain's index in the call -- purpose
 * j < ceil(k / 2): the Box-Muller pair (2 j, 2 j + 1) from the uniforms ((w0 >> 6) 2^26 + (w1 >> 6) + 0.5) 2^-52 and the same of
 * w2, w3; purpose 0xFFFFFFFF: u from w0, w1.  Proposal theta' = theta + e^ls L xi, a pinned coordinate (lo_q == hi_q) stays bit
 * for bit.  Outside the box: rejected without an evaluation, alpha = 0.  Inside: a non-positive pivot of A(theta') rejects with
 * alpha = 0; otherwise l = -invvar (Phi' - Phi) / 2, accepted iff log u < l, alpha = min(1, e^min(l, 0)).  i < burn:
 * ls += (i + 1)^-0.6 (alpha - 0.234), frozen afterwards.  i >= burn: the state enters the Welford mean and M2 (k x k) of theta,
 * the running mean of c, the smallest Phi with its theta; with SAMPLES and (i - burn) % thin == thin - 1 theta goes to slot
 * (i - burn) / thin of the chain (SAMPLES is [chain][slot][k] from smp_off; slots beyond `slots` are not written; NULL: none).
 * STATE row of a chain (lds apart, from s_off; rom_mcmc_layout): theta (k) | Phi | ls | mean (k) | M2 (k k) | mean of c (n) | kept |
 * accepted (both of the steps i >= burn) | outside | not_spd (of all steps) | Phi_min | theta_min (k).  With step0 == 0 only theta
 * is read, the start, and clipped to the box; otherwise the chain resumes from its row.  At most 1024 steps run per launch; a call
 * split at any step, here or by the caller through step0, returns the bits of the unsplit call.
 * 1 <= n <= 64, 1 <= k <= 16, 1 <= r <= 64, 1 <= t <= 8, K t <= 2^30, steps >= 0, burn >= 0, thin >= 1, step0 + steps <= 2^31:
 * ROM_ERR_INVALID outside; K = 0 is a no-op; steps = 0 leaves the clipped start and its Phi.  A start whose A(theta) is not positive
 * definite: ROM_ERR_NOT_SPD, its row NaN.  A query whose Phi at the start is NaN has a NaN row and no error.  No input buffer is
 * modified; no floating-point atomics: the same bits on a repeated call.  One host synchronisation.
 * seed: its 64 bits are the key (an unsigned seed above 2^63 is passed as the signed number of the same bits).
 * info8_host (8 doubles or NULL): kernel launches, host synchronisations, bytes of workspace, chains K t, steps taken, evaluations
 * of the model (both summed on the device in integers), 0, 0. */
/* out8: the row length, then the offsets of Phi, ls, mean, M2, the mean of c, kept (accepted, outside, not_spd follow it) and
 * Phi_min (theta_min follows it) */
int rom_mcmc_layout(int n, int k, int64_t* out8);
int rom_mcmc(rom_ctx* ctx, int n, int k, int r, rom_buf* Ahat, rom_buf* bhat, rom_buf* Gr, rom_buf* P, size_t p_off, int64_t ldp, int K,
             int t, rom_buf* INVVAR, rom_buf* LPROP, const double* lo_host, const double* hi_host, int64_t seed, int64_t chain0,
             int64_t step0, int steps, int burn, int thin, rom_buf* STATE, size_t s_off, int64_t lds, rom_buf* SAMPLES, size_t smp_off,
             int64_t slots, double* info8_host);

/* ---- sensor state estimation on the polynomial manifold (src/experiments/NonLinearROM.py:54-70, src/lib/ReducedBasis.py:65-70) ----
 * The decoder of a fitted rom_poly map, u(z) = mean + z V_known + g(z) V_unknown (the model of src/experiments/NonLinearROM.py:54-70),
 * fitted to point measurements instead of being given its known coordinates: the nonlinear counterpart of the linear state
 * estimation of src/lib/ReducedBasis.py:65-70.  With t = (z - c) / h and phi(t) the P = C(m + d, d) Legendre products of the map
 * (terms in rom_poly_terms order) the sensor image of the decoder is S phi(t); with the compact SVD diag(w) S = U Sigma V^T of
 * rank r, P (K rows of r from an element offset with a row stride) holds p = U^T (w y), Gr (r x P row-major) = Sigma V^T, and AUX
 * (K x 2) per query perp2 = ||(I - U U^T)(w y)||^2 and scale = max|w y| (NULL: 0 and max|p|).  Per query and start
 *     min over lo <= t <= hi of ||p - G_r phi(t)||^2 + perp2
 * by the Levenberg-Marquardt of rom_lm_polish (damping, acceptance, lambda schedule, eight trials, the `still`, `tiny` and
 * rounding-level rules, `converged`) with J = -G_r d phi / d t; romhighcontrast_amd/nonlinear.py::sense_scores is the same
 * algorithm on the host.  The residual p - G_r phi(t) and its squared norm are formed in double-double arithmetic and rounded once.  T0 (K, t, m) the starts, lo_host / hi_host (m each) the box; a coordinate with lo_j == hi_j is PINNED:
 * it stays at its clipped start bit for bit and has no column in J^T J or in the J whose sigma_min is reported.  One workgroup
 * per (query, start) runs the whole iteration in one launch (G_r d phi on fp64 MFMA); a second kernel keeps the start of smallest
 * misfit per query (the lowest index among equals).
 * OUT row of query q (ldo >= m + 5 doubles apart, from out_off): t (m) | misfit = sqrt(|p - G_r phi(t)|^2 + perp2) | sigma_min of
 * the final Jacobian's free columns (one-sided Jacobi; 0 when every coordinate is pinned) | converged (0 / 1) | iterations | start.
 * 1 <= m <= 16, 1 <= d <= 8, P <= 96, 1 <= r <= 96, 1 <= t <= 8: ROM_ERR_INVALID outside; K = 0 is a no-op; max_iter = 0 only
 * evaluates the clipped starts.  NaN / Inf in Gr, P or T0: ROM_ERR_INVALID.  A non-positive pivot of the damped system rejects
 * that trial.  No input buffer is modified; no floating-point atomics: the same bits on a repeated call.  One host synchronisation.
 * info8_host (8 doubles or NULL): kernel launches, host synchronisations, bytes of workspace, systems K t, LM iterations executed,
 * feature evaluations executed (both summed on the device in integers), 0, 0. */
int rom_poly_sense(rom_ctx* ctx, int m, int d, int r, rom_buf* Gr, rom_buf* P, size_t p_off, int64_t ldp, int K, int t, rom_buf* T0,
                   const double* lo_host, const double* hi_host, rom_buf* AUX, int max_iter, double misfit_tol, rom_buf* OUT,
                   size_t out_off, int64_t ldo, double* info8_host);

/* ---- sensor state estimation on the MLP manifold (src/experiments/NonLinearROM.py:54-70,138, src/lib/ReducedBasis.py:65-70) ----
 * rom_poly_sense for the decoder of a fitted rom_mlp map (the "NN" model of src/experiments/NonLinearROM.py:138): m inputs ->
 * n_hidden layers of hidden[l] units with the activation 0 tanh, 1 logistic, 2 relu -> a linear output layer.  With t = (z - c) / h
 * and a_L(t) the activations of the last hidden layer the sensor image of the decoder is S psi(t), psi = [1; t; a_L(t)] of length
 * 1 + m + H_L: the output layer and the scaling of the targets are part of S (romhighcontrast_amd/nonlinear.py::
 * mlp_sensing_matrix), so only the hidden layers reach the call.  WH holds them in the flat order of rom_mlp_layout without the
 * output layer: every W_l (outputs x inputs, row-major) in layer order, then every b_l.  Gr (r x (1 + m + H_L) row-major) = Sigma
 * V^T of the compact SVD diag(w) S = U Sigma V^T; P, AUX, T0, lo_host / hi_host, the iteration, pinned coordinates, the second
 * kernel and the OUT row  t (m) | misfit | sigma_min | converged | iterations | start  are those of rom_poly_sense, with
 * J = -G_r d psi / d t, d psi / d t = [0; I; D_L], D_0 = I, D_{l+1} = diag(sigma'(a_{l+1})) W_l D_l (the products W_l D_l and
 * G_r d psi on fp64 MFMA, psi in plain fp64, the residual and its squared norm in double-double arithmetic, rounded once);
 * romhighcontrast_amd/nonlinear.py::mlp_sense_scores is the same algorithm on the host.
 * 1 <= m <= 16, 1 <= n_hidden <= 3, 1 <= hidden[l] <= 64, activation in {0, 1, 2}, 1 <= r <= 96, 1 <= t <= 8: ROM_ERR_INVALID
 * outside; K = 0 is a no-op; max_iter = 0 only evaluates the clipped starts.  NaN / Inf in WH, Gr, P or T0: ROM_ERR_INVALID.  No
 * input buffer is modified; no floating-point atomics: the same bits on a repeated call.  Two launches, one host synchronisation.
 * info8_host (8 doubles or NULL): kernel launches, host synchronisations, bytes of workspace, systems K t, LM iterations executed,
 * forward passes of the hidden layers executed (both summed on the device in integers), 0, 0. */
int rom_mlp_sense(rom_ctx* ctx, int m, int n_hidden, const int* hidden, int activation, rom_buf* WH, int r, rom_buf* Gr, rom_buf* P,
                  size_t p_off, int64_t ldp, int K, int t, rom_buf* T0, const double* lo_host, const double* hi_host, rom_buf* AUX,
                  int max_iter, double misfit_tol, rom_buf* OUT, size_t out_off, int64_t ldo, double* info8_host);

/* ---- box-constrained least squares: linear state estimation that survives noise (src/lib/ReducedBasis.py:65-70) ----
 * The linear state estimation of src/lib/ReducedBasis.py:65-70 with the coefficients kept inside a box (constrained
 * stabilisation: the box the training snapshots' coefficients span).  For each of the K rows p of P (r columns from an element
 * offset with a row stride)
 *     min over lo <= c <= hi of ||p - G_r c||^2 + perp2
 * with Gr (r x n row-major, full column rank) shared by all rows and AUX (K x 2) per row perp2 and scale (NULL: 0; the scale is
 * not used) -- in reduced sensor coordinates Gr = Sigma V^T and p = U^T (w y) of the compact SVD diag(w) E^T = U Sigma V^T.
 * Stark-Parker bounded-variable least squares with every decision fixed; romhighcontrast_amd/inverse.py::bvls_host is the same
 * algorithm on the host.  Start: the unconstrained solution clipped to the box, what lands on a bound starts bound.  A pass
 * solves the least squares on the free columns with the bound ones moved to the right-hand side (L D L^T of the free block of
 * G^T G, one refinement step with the residual formed on the columns of Gr).  Feasible: it is taken, and with g = Gr^T (Gr c - p)
 * the bound variable of largest |g_j| / ||G_j|| among those whose multiplier has the wrong sign (g_j < 0 at lo, g_j > 0 at hi) is
 * freed, the lowest index among equals; none: the Karush-Kuhn-Tucker conditions hold, converged.  Infeasible: c moves along the
 * segment to the solution up to the first bound hit, and what hits it is bound.  A variable freed in one pass that leaves through
 * the same bound in the next is bound again and barred until another variable changes state.  At most max_iter passes
 * (max_iter = 0 returns the clipped start).  lo_host / hi_host (n each): lo_j == hi_j PINS c_j bit for bit; lo_j = -inf and
 * hi_j = +inf are allowed; lo_j > hi_j or NaN: ROM_ERR_INVALID.  One workgroup per row runs the whole iteration in one launch,
 * after one kernel that forms G^T G.
 * OUT row of p (ldo >= n + 4 doubles apart, from out_off): c (n) | misfit = sqrt(|p - G_r c|^2 + perp2) | number of bound
 * variables | converged (0 / 1) | passes.  BOUND (K x n doubles, or NULL): -1 at lo, +1 at hi, 0 free; a pinned coordinate -1.
 * 1 <= n <= 64, n <= r <= 96: ROM_ERR_INVALID outside, OUT unwritten; K = 0 is a no-op.  NaN / Inf in Gr or P, or a Gr without
 * full column rank: ROM_ERR_INVALID, reported once.  No input buffer is modified; no floating-point atomics: the same bits on a
 * repeated call.  Two launches, one host synchronisation.
 * info8_host (8 doubles or NULL): kernel launches, host synchronisations, bytes of workspace, systems K, passes executed,
 * factorisations executed (both summed on the device in integers), 0, 0. */
int rom_bvls(rom_ctx* ctx, int n, int r, rom_buf* Gr, rom_buf* P, size_t p_off, int64_t ldp, int K, const double* lo_host,
             const double* hi_host, rom_buf* AUX, int max_iter, rom_buf* OUT, size_t out_off, int64_t ldo, rom_buf* BOUND,
             double* info8_host);

/* ---- sensor state estimation with local reduced spaces: model selection by the PDE residual ----
 * Cohen, Dahmen, Mula, Nichols, "Nonlinear reduced models for state and parameter estimation" (SIAM/ASA JUQ 10, 2022): the linear
 * estimate is computed in each of kc local spaces, and the one whose residual, minimised over the cluster's parameter box, is
 * smallest is kept; the minimiser is a parameter estimate.  romhighcontrast_amd/inverse.py::local_select_host is the same
 * algorithm on the host.  For measurement vector i (row i of P: kc blocks of r reduced measurements, block j = p_ij, from an
 * element offset with a row stride) and cluster j:
 *   1. c_ij = argmin over c_lo[j] <= c <= c_hi[j] of ||p_ij - G_j c||, G_j (r x n row-major, full column rank) block j of GR:
 *      the iteration of rom_bvls; misfit_ij = ||p_ij - G_j c_ij||.
 *   2. B_ij[:, q] = sum_i' c_ij[i'] R_j[:, 1 + i' k + q] (rank x k), R_j (rank x (1 + k n) row-major, the residual table of
 *      rom_resid_download what = 0, padded with zero rows to the common rank) block j of RT, rho_j = R_j[:, 0]:
 *      ||r(a; c_ij W_j)||_H^-1 = ||rho_j - B_ij a|| for every a.
 *   3. S_ij = min over a_lo[j] <= a <= a_hi[j] of ||rho_j - B_ij a||, the same iteration on B_ij (k unknowns); a_ij its minimiser.
 *   4. label_i = the j of smallest (S_ij, j) among the systems of status 0 whose S is a number, or -1 when there is none.
 * The boxes are host arrays, kc x n (c_lo, c_hi) and kc x k (a_lo, a_hi), with the rules of rom_bvls (lo == hi pins, infinite
 * bounds allowed, lo > hi or NaN: ROM_ERR_INVALID).  max_iter bounds the passes of either solve; negative: 5 n + 10 and 5 k + 10.
 * OUT row i kc + j (ldo >= n + k + 5 doubles apart, from out_off): c (n) | a (k) | S | misfit | passes of the state solve | passes
 * of the parameter solve | status.  status: 1 the state solve failed on its data (NaN / Inf in p_ij or G_j, or G_j without full
 * column rank: c, a, S, misfit are NaN), 2 the parameter solve did (NaN / Inf in R_j, or B_ij without full column rank: a and S
 * are NaN), 4 the state solve stopped at max_iter, 8 the parameter solve did; bits add.  Bad data is no error of the call: it is
 * reported per system.  label_host: K int32.
 * Three launches whatever K and kc are (the Gram matrices G_j^T G_j; one workgroup per system for 1 - 3, with both iterations
 * inside the launch and B_ij and its Gram matrix in LDS; the selection), one host synchronisation.  No input buffer is modified;
 * no floating-point atomics, one fixed order in every sum, no system reads what another writes: the same bits on a repeated call
 * and for every split of the rows.
 * rom_local_select_layout (host only; the single place of the limits and of the LDS carve-up): 1 <= n <= 64, 1 <= k <= 16,
 * n <= r <= 96, k <= rank <= rank_max(n, k, r), the largest rank whose B fits the workgroup's 64 KB of LDS beside the factor
 * (638 at n = 32, k = 9; 1195 at n = 64, k = 4); ROM_ERR_INVALID outside.  rom_local_select adds 1 <= kc <= 256, K <= 2^23 and K kc <= 2^30; K = 0 is a
 * no-op.  out8: LDS bytes of the fit kernel, doubles of an OUT row (n + k + 5), rank_max, the limit of kc, and in doubles the
 * LDS offsets of the factor, of B and of B^T B; the number of launches.
 * info8_host (8 doubles or NULL): systems K kc, kernel launches, host synchronisations, bytes of workspace, passes executed (both
 * solves), factorisations executed (both summed on the device in integers), flops of steps 2 and of B^T B, systems of
 * status != 0. */
int rom_local_select_layout(int n, int k, int rank, int r, int64_t* out8);
int rom_local_select(rom_ctx* ctx, int kc, int n, int k, int rank, int r, rom_buf* RT, rom_buf* GR, rom_buf* P, size_t p_off,
                     int64_t ldp, int K, const double* c_lo_host, const double* c_hi_host, const double* a_lo_host,
                     const double* a_hi_host, int max_iter, rom_buf* OUT, size_t out_off, int64_t ldo, int32_t* label_host,
                     double* info8_host);

/* ---- D-optimal sensor selection for parameter estimation (greedy Bayesian experimental design) ----
 * Which m of ncand candidate points make point measurements determine theta = log a best, on average over a library of M
 * parameters: expected information gain under the linearised Gaussian model.  romhighcontrast_amd/inverse.py::sensor_dopt_host is
 * the same algorithm on the host.  With c(theta) = A(theta)^-1 bhat, A = sum_q e^theta_q Ahat_q, X_j = -dc/dtheta at entry j
 * (n x k, column q = e^theta_q A^-1 Ahat_q c), e_x (n) the basis at candidate x (row x of E, from an element offset with a row
 * stride), independent noise N(0, sigma^2) per sensor and the prior covariance T0 T0^T, the posterior precision of a sensor set S
 * at entry j is F_j(S) = Gamma_0 + sigma^-2 sum_S g g^T, g = X_j^T e_x, and the criterion
 *     Phi(S) = 1 / (2 M) sum_j log det(Gamma_0^-1 F_j(S)),
 * monotone submodular in S, so the greedy reaches (1 - 1/e) of the optimum.
 * STATE holds one block per entry (rom_sensor_dopt_layout): Z_j^T (kp rows of n_pad doubles, Z_j = X_j T_j / sigma) | T_j (kp x kp
 * row-major, T_j T_j^T = F_j^-1) | status | s of the last update; kp = k rounded up to 1, 2, 4, 8 or 16, n_pad = n rounded up to a
 * multiple of 4, the padding zero.
 * rom_sensor_dopt_init: STATE for the empty sensor set, Z_j = X_j T0 / sigma and T_j = T0 (T0_host: k x k row-major, any factor of
 * the prior covariance; a zero column is a parameter that is known), from the rows theta_j of THETA (M rows of k, from t_off with
 * stride ldt).  One workgroup per entry assembles A(theta_j), factors it (L D L^T) and solves for c and the k columns of X_j.  An
 * entry whose A has a pivot that is not positive (status 1) or whose theta is not finite (status 2) gets Z_j = 0: it contributes
 * exactly 0 to every score, and the call succeeds.  info_host (8 doubles or NULL): such entries, launches, host synchronisations,
 * bytes of workspace, 0 ...
 * rom_sensor_dopt_scores: SCORE[sc_off + x] = sum_j log1p(|Z_j^T e_x|^2), the gain in 2 M Phi of adding candidate x -- one
 * scoring pass without an update, and the information map one plots.  The product E [Z_1 .. Z_M] (ncand x M kp) runs on
 * v_mfma_f64_16x16x4_f64 and is never written: 128 candidates are an LDS-resident table, the rows of Z^T stream through in slabs
 * of 32, the epilogue (square, sum over an entry's kp columns, log1p, add in ascending j) stays in registers.  The library is cut
 * into chunks of 2048 / kp entries, whatever the candidates are, and the chunks' partial sums are added in chunk order by a second
 * kernel: a candidate's score has the same bits whichever other candidates are in the call, and on every call.
 * rom_sensor_dopt: m greedy steps, each the scoring pass, the pick -- the first maximum among the candidates not yet picked whose
 * score is finite; a NaN or infinite score (NaN / Inf in a row of E) is never picked -- and the rank-one update of every entry,
 *     u = Z_j^T e_x*, s = |u|^2, rho = sqrt(1 + s), beta = 1 / (rho (rho + 1)), Z_j -= beta (Z_j u) u^T, T_j -= beta (T_j u) u^T,
 * the symmetric square root of the Sherman-Morrison downdate.  Three launches per step (four where the library has more than one
 * chunk), enqueued without host involvement, one host synchronisation at the end.  Stop reasons: 0 m picks made; 1 the gain was
 * <= rel_tol x the first gain of this call (with rel_tol = 0: no information left to gain); 2 no candidate left.  STATE is updated
 * in place, so a second call continues the design: taken_host (ntaken candidate indices, or NULL with 0) lists the picks of the
 * earlier calls, which are then not picked again -- a design split over calls has the bits of the unsplit one (rel_tol = 0).
 * picks_out (m int32, -1 behind the picks made), gain_out (m doubles, 0 behind them): gain = the score of the pick; the information
 * Phi after pick t is the sum of the gains up to t over 2 (M - skipped entries).
 * info_host (8 doubles or NULL): picks made, stop reason, entries of status != 0, candidates whose first score was not finite, launches,
 * host synchronisations, bytes of workspace, flops executed by the scoring passes.
 * 1 <= n <= 64, 1 <= k <= 16, 1 <= M <= 2^24, 1 <= ncand <= 2^22, 1 <= m <= min(1024, ncand), sigma > 0, 0 <= rel_tol < 1, the
 * partial sums (chunks x ncand doubles) within the workspace limit: ROM_ERR_INVALID outside, naming the limit.  No operand but
 * STATE and the outputs is modified; fp64 only, no floating-point atomics: the same bits on a repeated call.
 * rom_sensor_dopt_layout (host only) out8: kp, n_pad, doubles per entry, entries per chunk, LDS bytes of the scoring kernel, the
 * offsets of T_j and of the status in an entry's block, candidates per table. */
int rom_sensor_dopt_layout(int n, int k, int64_t* out8);
int rom_sensor_dopt_init(rom_ctx* ctx, int n, int k, rom_buf* Ahat, rom_buf* bhat, rom_buf* THETA, size_t t_off, int64_t ldt, int64_t M,
                         const double* T0_host, double sigma, rom_buf* STATE, size_t s_off, double* info_host);
int rom_sensor_dopt_scores(rom_ctx* ctx, int n, int k, rom_buf* STATE, size_t s_off, int64_t M, rom_buf* E, size_t e_off, int64_t lde,
                           int64_t ncand, rom_buf* SCORE, size_t sc_off);
int rom_sensor_dopt(rom_ctx* ctx, int n, int k, rom_buf* STATE, size_t s_off, int64_t M, rom_buf* E, size_t e_off, int64_t lde,
                    int64_t ncand, int m, double rel_tol, const int32_t* taken_host, int ntaken, int32_t* picks_out, double* gain_out,
                    double* info_host);

/* ---- multi-GPU: RCCL all-gather of the snapshot block --------------------- */
/* id_out: 128 bytes (ncclUniqueId).  librccl is dlopen()ed on first use. */
int rom_comm_unique_id(char* id_out, size_t cap);
int rom_comm_init(rom_ctx* ctx, const char* id, size_t id_len, int rank, int nranks);
int rom_comm_destroy(rom_ctx* ctx);
/* recv[(r*count) ...] = send of rank r; count doubles per rank */
int rom_comm_allgather(rom_ctx* ctx, rom_buf* send, size_t send_off, rom_buf* recv, size_t recv_off,
                       size_t count);
/* same collective on the context's communication stream, ordered after the work enqueued so far on the
 * compute stream but not blocking it (the next sweep step overlaps the exchange); rom_comm_wait makes the
 * compute stream (and the host if host_sync != 0) wait for the outstanding collectives */
int rom_comm_allgather_async(rom_ctx* ctx, rom_buf* send, size_t send_off, rom_buf* recv, size_t recv_off,
                             size_t count, int slot /* 0|1: double-buffer slot of the send buffer */);
/* The exchange of one step of a sharded sweep in ONE call: pack the interface vectors Y[y_row0 .. +M) of the own shard
 * into their compact form (into `send`, M x rom_fem_compact_stride() doubles of scratch) and all-gather them into
 * recv[recv_off ...] (nranks x M x compact stride) -- both on the communication stream, after everything enqueued so
 * far on the compute stream, which is not blocked.  Slots as in rom_comm_allgather_async. */
int rom_comm_allgather_packed_async(rom_fem* fem, rom_buf* Y, int64_t y_row0, int M, rom_buf* send, rom_buf* recv,
                                    size_t recv_off, int slot);
int rom_comm_wait(rom_ctx* ctx, int host_sync);
/* compute stream waits for the collective last issued with `slot` (before its send buffer is rewritten) */
int rom_comm_wait_slot(rom_ctx* ctx, int slot);
/* in-place max / sum all-reduce of n host doubles staged through the device (control plane:
 * barrier + max-over-ranks timing of bench.py) */
int rom_comm_allreduce_host(rom_ctx* ctx, double* vals, int n, int op /*0=sum,1=max*/);

#ifdef __cplusplus
}
#endif
#endif /* ROMHC_H */
