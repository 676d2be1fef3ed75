// H^1_0 Riesz representers of P1 point evaluations (rom_riesz_h10, include/romhc.h).
//
// The reference's generate_riesz(x, "h10") (src/lib/SolutionsManagers.py:70-86) was left unimplemented; its intent is
// omega_i = A_1^{-1} r_i with r_i the evaluation vector of point i.  A_1 (A_preassembled4h1_norm) is the 5-point
// Laplacian on the nr x nc interior grid (diagonal 4, neighbours -1, uniform up to the boundary), which the 2-D sine
// transform diagonalises exactly:
//   S_n[j,p] = sqrt(2/(n+1)) sin(pi (j+1)(p+1)/(n+1))     (0-based; symmetric and orthogonal)
//   Lambda[j,k] = lam_r[j] + lam_c[k],  lam_n[j] = 4 sin^2(pi (j+1) / (2(n+1)))
//   omega = S_r (Rhat / Lambda) S_c,  Rhat = S_r R S_c      (R = r as an nr x nc array)
// and G[i,l] = r_i^T A_1^{-1} r_l = sum Rhat_i Rhat_l / Lambda.  The call
//   1. builds S_r, S_c, lam_r, lam_c once per FE space (kr_sine; the sine argument is reduced in integers, so the
//      tables keep their digits at n = 1023, and lam comes in the sin^2 form: 4 - 2 cos - 2 cos cancels on the lowest
//      mode);
//   2. forms Rhat_i from the at most three P1 weights of each point (kr_spectral): Rhat/sqrt(Lambda) as rows for the
//      Gram product, Rhat/Lambda as What[j][i][k] for the back transform;
//   3. G = one rom_launch_gram on the Rhat/sqrt(Lambda) rows (mirrored upper triangle: symmetric to the bit);
//   4. Z = S_r What ([p][i][k], one NN product over all points), Z S_c on the nr*npts rows of length nc ([p][i][q]), and
//      a permute into the caller's rows [i][p][q] (kr_permute).
#include <algorithm>
#include <cmath>

#include "rom_ops.h"

#include "rom_basis_int.h"

namespace {

// rows of the general NN product per launch: its grid has one workgroup row per 64 output rows (grid.y <= 65535)
constexpr int64_t RZ_MAX_ROWS = int64_t(65535) * 64;

// S (n x n) and lam (n) of one grid direction
__global__ void kr_sine(double* __restrict__ S, double* __restrict__ lam, int n) {
  const long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  const long long n1 = n + 1;
  const double scale = sqrt(2.0 / double(n1));
  if (idx < (long long)n * n) {
    const long long j = idx / n, p = idx % n;
    // sin(pi t / (n+1)) with t = (j+1)(p+1) mod 2(n+1), folded into [0, (n+1)/2] in integers
    long long t = ((j + 1) * (p + 1)) % (2 * n1);
    double sgn = 1.0;
    if (t > n1) {
      t -= n1;
      sgn = -1.0;
    }
    if (2 * t > n1) t = n1 - t;
    S[idx] = sgn * scale * sinpi(double(t) / double(n1));
  }
  if (idx < n) {
    const double s = sinpi(double(idx + 1) / double(2 * n1));
    lam[idx] = 4.0 * s * s;
  }
}

// Rhat_i[j,k] = sum_t w_t S_r[j, y_t] S_c[x_t, k].  Gs[i][j*nc + k] = Rhat / sqrt(Lambda); What[j][i][k] = Rhat / Lambda
// (What may be null).  Thread: one (j, k); grid.y strides over the points.
__global__ __launch_bounds__(256) void kr_spectral(int nr, int nc, int npts, const int* __restrict__ ix,
                                                   const int* __restrict__ iy, const double* __restrict__ tx,
                                                   const double* __restrict__ ty, const double* __restrict__ Sr,
                                                   const double* __restrict__ Sc, const double* __restrict__ lam_r,
                                                   const double* __restrict__ lam_c, double* __restrict__ Gs,
                                                   double* __restrict__ What) {
  const long long dim = (long long)nr * nc;
  const long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (idx >= dim) return;
  const int j = int(idx / nc), k = int(idx % nc);
  const double lam = lam_r[j] + lam_c[k];
  const double inv_sqrt = 1.0 / sqrt(lam), inv = 1.0 / lam;
  for (int i = blockIdx.y; i < npts; i += gridDim.y) {
    const PointWeights pw = point_weights(nr, nc, ix[i], iy[i], tx[i], ty[i]);
    double v = 0.0;
#pragma unroll
    for (int t = 0; t < 3; ++t)
      if (pw.y[t] >= 0) v += pw.w[t] * Sr[(long long)j * nr + pw.y[t]] * Sc[(long long)pw.x[t] * nc + k];
    Gs[(long long)i * dim + idx] = v * inv_sqrt;
    if (What) What[((long long)j * npts + i) * nc + k] = v * inv;
  }
}

// OMEGA[i][p*nc + q] = O[p][i][q]
__global__ __launch_bounds__(256) void kr_permute(int nr, int nc, int npts, const double* __restrict__ O,
                                                  double* __restrict__ OMEGA) {
  const long long dim = (long long)nr * nc, total = dim * npts;
  for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const long long i = idx / dim, r = idx % dim, p = r / nc, q = r % nc;
    OMEGA[idx] = O[(p * npts + i) * nc + q];
  }
}

}  // namespace

SineTables rom_sine_tables(const rom_fem* f) {
  const double* Sr = f->d_riesz;
  const double* Sc = Sr + size_t(f->nr) * f->nr;
  const double* lr = Sc + size_t(f->nc) * f->nc;
  return {Sr, Sc, lr, lr + f->nr};
}

int rom_riesz_tables(rom_fem* f) {
  if (f->d_riesz) return ROM_OK;
  rom_ctx* ctx = f->ctx;
  const size_t n = size_t(f->nr) * f->nr + size_t(f->nc) * f->nc + f->nr + f->nc;
  ROM_HIP(hipMalloc(&f->d_riesz, n * sizeof(double)));
  const SineTables st = rom_sine_tables(f);  // (this call owns the block: the one place that writes through the pointers)
  {
    ROM_PROF(ctx, "riesz_sine", 4.0 * double(n), 8.0 * double(n));
    kr_sine<<<blocks_for(size_t(f->nr) * f->nr), 256, 0, ctx->stream>>>(const_cast<double*>(st.Sr), const_cast<double*>(st.lam_r), f->nr);
    ROM_HIP(hipGetLastError());
    kr_sine<<<blocks_for(size_t(f->nc) * f->nc), 256, 0, ctx->stream>>>(const_cast<double*>(st.Sc), const_cast<double*>(st.lam_c), f->nc);
    ROM_HIP(hipGetLastError());
  }
  return ROM_OK;
}

extern "C" int rom_riesz_h10(rom_fem* f, int npts, const int* ix_host, const int* iy_host, const double* tx_host,
                             const double* ty_host, rom_buf* OMEGA, int64_t row0, double* gram_host) {
  ROM_CHECK(f && (npts == 0 || (ix_host && iy_host && tx_host && ty_host)), "rom_riesz_h10: null argument");
  ROM_CHECK(npts >= 0 && row0 >= 0, "rom_riesz_h10: negative size");
  const int nr = f->nr, nc = f->nc;
  const int64_t dim = f->dim;
  ROM_CHECK(!OMEGA || size_t(row0 + npts) * dim <= OMEGA->n, "rom_riesz_h10: rows out of range");
  for (int p = 0; p < npts; ++p)
    ROM_CHECK(ix_host[p] >= 0 && ix_host[p] <= nc && iy_host[p] >= 0 && iy_host[p] <= nr,
              "rom_riesz_h10: point %d outside the domain", p);
  if (npts == 0 || (!OMEGA && !gram_host)) return ROM_OK;
  rom_ctx* ctx = f->ctx;
  ROM_TRY(rom_riesz_tables(f));
  const SineTables st = rom_sine_tables(f);
  DevPoints pts;
  ROM_TRY(pts.upload(ctx, npts, ix_host, iy_host, tx_host, ty_host));
  Tmp Gs, What, Gd;
  const size_t block = size_t(npts) * dim;
  ROM_TRY(Gs.get(ctx, block));
  if (OMEGA) ROM_TRY(What.get(ctx, block));
  {
    const dim3 grid(unsigned((dim + 255) / 256), unsigned(std::min(npts, 65535)));
    ROM_PROF(ctx, "riesz_spectral", 8.0 * double(block), 8.0 * (OMEGA ? 2.0 : 1.0) * double(block));
    kr_spectral<<<grid, 256, 0, ctx->stream>>>(nr, nc, npts, pts.ix, pts.iy, pts.tx, pts.ty, st.Sr, st.Sc, st.lam_r, st.lam_c, Gs,
                                               OMEGA ? What.p() : nullptr);
    ROM_HIP(hipGetLastError());
  }
  if (gram_host) {
    ROM_TRY(Gd.get(ctx, size_t(npts) * npts));
    ROM_TRY(rom_launch_gram(ctx, npts, dim, Gs, dim, Gd, npts, "riesz_gram"));
    ROM_HIP(hipMemcpyAsync(gram_host, Gd.p(), size_t(npts) * npts * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  }
  if (OMEGA) {
    // Z = S_r What: [p][i][k] into the Gs block (the Gram product has read it: same stream)
    double* Z = Gs.p();
    const int64_t wide = int64_t(npts) * nc;
    ROM_TRY(rom_launch_gemm_nn(ctx, nr, wide, nr, 1.0, st.Sr, nr, What, wide, 0.0, Z, wide, nullptr, "riesz_transform_r"));
    // Z S_c on the nr*npts rows of length nc: [p][i][q] into the What block
    const int64_t rows = int64_t(nr) * npts;
    for (int64_t r0 = 0; r0 < rows; r0 += RZ_MAX_ROWS) {
      const int64_t take = std::min(RZ_MAX_ROWS, rows - r0);
      ROM_TRY(rom_launch_gemm_nn(ctx, take, nc, nc, 1.0, Z + r0 * nc, nc, st.Sc, nc, 0.0, What.p() + r0 * nc, nc, nullptr,
                                 "riesz_transform_c"));
    }
    {
      ROM_PROF(ctx, "riesz_permute", 0.0, 16.0 * double(block));
      const unsigned grid = unsigned(std::min<size_t>((block + 255) / 256, size_t(16) * 1024));
      kr_permute<<<grid, 256, 0, ctx->stream>>>(nr, nc, npts, What, OMEGA->p + row0 * dim);
      ROM_HIP(hipGetLastError());
    }
  }
  ROM_HIP(hipStreamSynchronize(ctx->stream));  // the one host synchronisation: G is on the host, the points are free
  return ROM_OK;
}
