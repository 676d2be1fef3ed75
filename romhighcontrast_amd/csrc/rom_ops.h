// Internal launchers of rom_ops.hip shared with rom_basis.hip and rom_small_dense.hip: raw device pointers, work only
// ENQUEUED on the context's compute stream (no host synchronisation), results left on the device.
#pragma once
#include "romhc_internal.h"

struct StencilGeom {
  int nr, nc, N, ncb, kblk;
  long long dim;
};
StencilGeom rom_make_geom(int nrb, int ncb, int N);

// C[m,n] = alpha * A[m,k] B[k,n] + beta C.  A split-K product keeps its partials in the context's scratch, or in
// `part_ws` (rom_gemm_nn_partial_doubles(m, n, k, lda, ldb) doubles) when one is given.  prof_name: the profile name
// of the product (default "gemm_nn")
int rom_launch_gemm_nn(rom_ctx* ctx, int64_t m, int64_t n, int64_t k, double alpha, const double* A, int64_t lda,
                       const double* B, int64_t ldb, double beta, double* C, int64_t ldc, double* part_ws = nullptr,
                       const char* prof_name = nullptr);
size_t rom_gemm_nn_partial_doubles(int64_t m, int64_t n, int64_t k, int64_t lda, int64_t ldb);
// C[m,m] = A A^T (lower tiles on MFMA + mirror); prof_name: the profile name of the product (default "gram")
int rom_launch_gram(rom_ctx* ctx, int64_t m, int64_t k, const double* A, int64_t lda, double* C, int64_t ldc,
                    const char* prof_name = nullptr);
// Y[k,:] = A(coef) X[k,:]; d_coef: kblk block coefficients ON THE DEVICE, or null for the unit operator A_1
int rom_launch_stencil_apply(rom_fem* f, const double* d_coef, const double* X, int K, double* Y);
// the same on the interior mesh rows [row_lo, row_hi] only (Y is not written outside the slabs that cover them)
int rom_launch_stencil_apply_band(rom_fem* f, const double* d_coef, const double* X, int K, double* Y, int row_lo, int row_hi);
// Y[b, :] = A_b x for all kblk blocks in one launch (d_onehot: kblk x kblk identity on the device)
int rom_launch_stencil_apply_blocks(rom_fem* f, const double* d_onehot, const double* x, double* Y);
// d_out[k] = ||U_k - V_k||_{H10} (V may be null); squared norms if !take_sqrt.  Same kernels, same bits as rom_h10norm.
int rom_launch_h10norm(rom_fem* f, const double* U, const double* V, int K, double* d_out, bool take_sqrt);
// d_out[k] = ||U_k||_2 (or its square)
int rom_launch_l2norm(rom_ctx* ctx, const double* U, int K, int64_t dim, double* d_out, bool take_sqrt);
// d_out[k] = U_k . z  (rows of length dim against one vector)
int rom_launch_rowdot(rom_ctx* ctx, const double* U, int K, int64_t dim, const double* z, double* d_out);
// batched reduced solves, Ahat (kb, ldA, ldA) of which the leading n x n blocks are used; no status read-back
// (a non-positive pivot sets bit 0 of ctx->d_status, which the caller clears before and reads after)
int rom_launch_reduced_solve(rom_ctx* ctx, int n, int ldA, int kb, int M, const double* Ahat, const double* w,
                             const double* rhs, int rhs_per_system, double* c_out);
// X[row, :] *= fac[row] with the factors on the device
int rom_launch_rows_scale(rom_ctx* ctx, double* X, int rows, int64_t dim, const double* d_fac);
int rom_launch_center_rows(rom_ctx* ctx, double* X, int M, int64_t dim, double* d_mean);
int rom_launch_subtract_row(rom_ctx* ctx, double* X, int M, int64_t dim, const double* d_row);
int rom_launch_rows_sign_flip(rom_ctx* ctx, double* X, int rows, int64_t dim);
// evaluate_solutions' P1 gather (rom_ops.hip): out[k * npts + p] = U_k at point p; grid ((npts + 255) / 256, K) x 256
__global__ void k_eval_points(int nr, int nc, long long dim, const double* __restrict__ U, int K, int npts,
                              const int* __restrict__ ix, const int* __restrict__ iy,
                              const double* __restrict__ tx, const double* __restrict__ ty,
                              double* __restrict__ out);
// the sine tables of rom_riesz_h10, built once per FE space into f->d_riesz: S_r (nr x nr), S_c (nc x nc), lam_r, lam_c
int rom_riesz_tables(rom_fem* f);
// where they lie in f->d_riesz (valid after rom_riesz_tables)
struct SineTables { const double *Sr, *Sc, *lam_r, *lam_c; };
SineTables rom_sine_tables(const rom_fem* f);
// the 2-D sine transform of K dense rows (rom_spectral.hip): OUT[k] = Lambda^(post/2) o (S_r (Lambda^(pre/2) o X[k]) S_c) on raw
// device rows, OUT != X; its flop count (both factors)
int rom_launch_sine_transform(rom_fem* f, const double* X, int K, int pre, int post, double* OUT);
double rom_sine_transform_flops(rom_fem* f, int K);

// P1 weights of a point on the interior dofs (rom_riesz.hip, rom_sensors.hip): the locating convention of k_eval_points (rom_ops.hip), vertex (y, x) of
// the grid with its Dirichlet ring -> dof (y-1, x-1); weights on boundary vertices drop out (y = -1: none)
struct PointWeights {
  int y[3], x[3];
  double w[3];
};
__device__ inline PointWeights point_weights(int nr, int nc, int x0, int y0, double qx, double qy) {
  PointWeights pw;
  if (qx + qy < 1) {
    pw.w[0] = 1 - qx - qy; pw.y[0] = y0;     pw.x[0] = x0;
    pw.w[1] = qx;          pw.y[1] = y0;     pw.x[1] = x0 + 1;
    pw.w[2] = qy;          pw.y[2] = y0 + 1; pw.x[2] = x0;
  } else {
    pw.w[0] = qx + qy - 1; pw.y[0] = y0 + 1; pw.x[0] = x0 + 1;
    pw.w[1] = 1 - qx;      pw.y[1] = y0 + 1; pw.x[1] = x0;
    pw.w[2] = 1 - qy;      pw.y[2] = y0;     pw.x[2] = x0 + 1;
  }
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    if (pw.y[t] >= 1 && pw.y[t] <= nr && pw.x[t] >= 1 && pw.x[t] <= nc) {
      pw.y[t] -= 1;
      pw.x[t] -= 1;
    } else {
      pw.y[t] = -1;
    }
  }
  return pw;
}
