// Greedy sensor selection for PBDW state estimation (rom_riesz_norms_h10, rom_sensor_greedy; include/romhc.h).
//
// PBDW (rom_riesz_h10, lib/ReducedBasis.py) is as good as the inf-sup constant beta(V_n, W_m) between the reduced space
// and the span W_m of the sensors' H^1_0 Riesz representers omega_x = A_1^-1 r_x.  The greedy of Binev, Cohen, Mula and
// Nichols (SIAM/ASA JUQ 2018) picks, from a dictionary of candidate points, the point whose representer best captures
// the part of V_n the sensors do not see yet.  Everything it needs is
//   * nu_x = ||omega_x||^2 = r_x^T A_1^-1 r_x for every candidate: the diagonal of rom_riesz_h10's G, here from four
//     VERTEX-PAIR GREEN TABLES built once per FE space.  With the sine tables of rom_riesz.hip (S symmetric),
//       A_1^-1[(y,x),(y+dy,x+dx)] = sum_j sum_k S_r[j,y] S_r[j,y+dy] S_c[k,x] S_c[k,x+dx] / (lam_r[j] + lam_c[k]),
//     and the at most three P1 vertices of a point are equal or differ by (dy, dx) in {(0,1), (1,0), (1,-1)} on the
//     SW-NE split; the (1,-1) entry at (y, x) is the (1,1) table at (y, x-1) (the sine products are symmetric in their
//     pair), so T_{dy,dx}, (dy, dx) in {0,1}^2, suffice.  T = P_r^dy Q_dx, Q_dx = Linv P_c^dx, with Linv[j,k] =
//     1 / (lam_r[j] + lam_c[k]), P_r^dy[y,j] = S_r[j,y] S_r[j,y+dy], P_c^dx[k,x] = S_c[k,x] S_c[k,x+dx]: six NN products.
//     T_00 is a sum of positive terms, and every entry of A_1^-1 is positive (A_1 is an M-matrix) as are the P1 weights,
//     so nu_x adds at most nine positive terms: no cancellation anywhere;
//   * the basis values at the candidates (a gather) and, per step, the values of the picked representer at all
//     candidates (the Green row: one explicit representer -- the spectral kernel of rom_riesz.hip for one point read by
//     index from device memory, its two transform products, a gather);
//   * one fused pass over the candidates per step (ks_step) that extends the sensor basis psi by one row, removes the
//     new direction from the residuals of the basis and forms the next criterion with per-workgroup argmax partials.
// The small quantities between the passes (the Cholesky row of the sensors' Gram matrix, the row of A, A^T A and its
// smallest eigenvector in the worst-case mode) stay on the device; the call waits for the stream once, at its end.
#include <algorithm>
#include <cmath>
#include <vector>

#include "rom_ops.h"

#include "rom_basis_int.h"

namespace {

constexpr int SG_TPB = 256;        // candidates per workgroup of the per-step pass (one lane each)
constexpr int SG_SELECT = 1024;    // threads of the single-workgroup argmax over the partials
constexpr int SG_MAX_N = 128, SG_MAX_N_WORST = SE_LDS_MAX, SG_MAX_M = 1024;

// ---- the vertex-pair Green tables -----------------------------------------------------------------------------------
// Linv (nr x nc), P_r^0, P_r^1 (nr x nr, ld nr; the last row of P_r^1 is 0), P_c^0, P_c^1 (nc x nc, ld nc; the last
// column of P_c^1 is 0), in one grid-stride launch
__global__ void ks_pair_factors(int nr, int nc, const double* __restrict__ Sr, const double* __restrict__ Sc,
                                const double* __restrict__ lam_r, const double* __restrict__ lam_c, double* __restrict__ Linv,
                                double* __restrict__ Pr0, double* __restrict__ Pr1, double* __restrict__ Pc0,
                                double* __restrict__ Pc1) {
  const long long a = (long long)nr * nc, b = (long long)nr * nr, c = (long long)nc * nc, total = a + b + c;
  for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
    if (idx < a) {
      const int j = int(idx / nc), k = int(idx % nc);
      Linv[idx] = 1.0 / (lam_r[j] + lam_c[k]);
    } else if (idx < a + b) {  // P_r[y, j] = S_r[j, y] S_r[j, y + d]
      const long long e = idx - a;
      const int y = int(e / nr), j = int(e % nr);
      const double s = Sr[(long long)j * nr + y];
      Pr0[e] = s * s;
      Pr1[e] = y + 1 < nr ? s * Sr[(long long)j * nr + y + 1] : 0.0;
    } else {  // P_c[k, x] = S_c[k, x] S_c[k, x + d]
      const long long e = idx - a - b;
      const int k = int(e / nc), x = int(e % nc);
      const double s = Sc[(long long)k * nc + x];
      Pc0[e] = s * s;
      Pc1[e] = x + 1 < nc ? s * Sc[(long long)k * nc + x + 1] : 0.0;
    }
  }
}

int green_tables(rom_fem* f) {
  if (f->d_green) return ROM_OK;
  ROM_TRY(rom_riesz_tables(f));
  rom_ctx* ctx = f->ctx;
  const int nr = f->nr, nc = f->nc;
  const int64_t dim = f->dim;
  const SineTables st = rom_sine_tables(f);
  double* T = nullptr;
  ROM_HIP(hipMalloc(&T, 4 * size_t(dim) * sizeof(double)));
  // (the entries past the last row / column of T_01, T_10, T_11 are never read; they are zeroed so that no table holds
  // uninitialised memory)
  ROM_HIP(hipMemsetAsync(T, 0, 4 * size_t(dim) * sizeof(double), ctx->stream));
  Tmp Linv, Pr, Pc, Q;
  ROM_TRY(Linv.get(ctx, dim));
  ROM_TRY(Pr.get(ctx, 2 * size_t(nr) * nr));
  ROM_TRY(Pc.get(ctx, 2 * size_t(nc) * nc));
  ROM_TRY(Q.get(ctx, 2 * size_t(dim)));
  double* Pr0 = Pr.p();
  double* Pr1 = Pr0 + size_t(nr) * nr;
  double* Pc0 = Pc.p();
  double* Pc1 = Pc0 + size_t(nc) * nc;
  {
    const double cnt = double(dim) + double(nr) * nr + double(nc) * nc;
    ROM_PROF(ctx, "sensor_pair_factors", cnt, 8.0 * (double(dim) + 2.0 * nr * nr + 2.0 * nc * nc));
    ks_pair_factors<<<unsigned(std::min<double>((cnt + 255) / 256, 4096.0)), 256, 0, ctx->stream>>>(nr, nc, st.Sr, st.Sc, st.lam_r, st.lam_c, Linv,
                                                                                                   Pr0, Pr1, Pc0, Pc1);
    ROM_HIP(hipGetLastError());
  }
  for (int dx = 0; dx < 2; ++dx)  // Q_dx = Linv P_c^dx: nr x (nc - dx), ld nc
    ROM_TRY(rom_launch_gemm_nn(ctx, nr, nc - dx, nc, 1.0, Linv, nc, dx ? Pc1 : Pc0, nc, 0.0, Q.p() + dx * size_t(dim), nc,
                               nullptr, "sensor_tables_q"));
  for (int dy = 0; dy < 2; ++dy)  // T_{dy,dx} = P_r^dy Q_dx: (nr - dy) x (nc - dx), ld nc
    for (int dx = 0; dx < 2; ++dx)
      ROM_TRY(rom_launch_gemm_nn(ctx, nr - dy, nc - dx, nr, 1.0, dy ? Pr1 : Pr0, nr, Q.p() + dx * size_t(dim), nc, 0.0,
                                 T + (2 * dy + dx) * size_t(dim), nc, nullptr, "sensor_tables_t"));
  f->d_green = T;  // (the temporaries go back to the context's cache; later work on this stream runs after the products)
  return ROM_OK;
}

// A_1^-1 between two vertices of one triangle of the SW-NE split (dofs (ya, xa), (yb, xb))
__device__ inline double green_pair(const double* __restrict__ T, int nc, long long dim, int ya, int xa, int yb, int xb) {
  int dy = yb - ya, dx = xb - xa;
  if (dy < 0 || (dy == 0 && dx < 0)) {
    dy = -dy;
    dx = -dx;
    ya = yb;
    xa = xb;
  }
  if (dx < 0) xa -= 1;  // (1, -1) at (y, x) = (1, 1) at (y, x - 1)
  return T[(2 * dy + (dx != 0)) * dim + (long long)ya * nc + xa];
}

// nu = r^T A_1^-1 r of the point (x0, y0, qx, qy): the at most nine weighted table entries, in a fixed order
__device__ inline double point_norm2(const double* __restrict__ T, int nr, int nc, int x0, int y0, double qx, double qy) {
  const long long dim = (long long)nr * nc;
  const PointWeights pw = point_weights(nr, nc, x0, y0, qx, qy);
  double s = 0.0;
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    if (pw.y[t] < 0) continue;
    s += pw.w[t] * pw.w[t] * T[(long long)pw.y[t] * nc + pw.x[t]];
#pragma unroll
    for (int u = t + 1; u < 3; ++u)
      if (pw.y[u] >= 0) s += 2.0 * pw.w[t] * pw.w[u] * green_pair(T, nc, dim, pw.y[t], pw.x[t], pw.y[u], pw.x[u]);
  }
  return s;
}

__global__ __launch_bounds__(256) void ks_norms(int nr, int nc, int npts, const int* __restrict__ ix, const int* __restrict__ iy,
                                                const double* __restrict__ tx, const double* __restrict__ ty,
                                                const double* __restrict__ T, double* __restrict__ out) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p < npts) out[p] = point_norm2(T, nr, nc, ix[p], iy[p], tx[p], ty[p]);
}

// ---- the greedy -----------------------------------------------------------------------------------------------------
// state (ints): [0] stopped, [1] stop reason, [2] picks made; scal (doubles): [0] best criterion of step 1

// dead count -> info; A^T A of no sensor: 0, with 2 on the diagonal of a dead direction (every eigenvalue of A^T A is at
// most 1 -- A holds coefficients of orthonormal rows in an orthonormal basis -- so the smallest eigenvector stays in the
// live directions and is exactly 0 on the dead ones: the two blocks never couple)
__global__ void ks_init(int n, const int* __restrict__ dead, double* __restrict__ AtA, double* __restrict__ info) {
  for (int idx = threadIdx.x; idx < n * n; idx += blockDim.x) {
    const int i = idx / n, l = idx % n;
    if (AtA) AtA[idx] = (i == l && dead[i]) ? 2.0 : 0.0;
  }
  if (threadIdx.x == 0) {
    int s = 0;
    for (int i = 0; i < n; ++i) s += dead[i];
    info[0] = double(s);
  }
}

// What = Rhat / Lambda of the point picks[k] (kr_spectral of rom_riesz.hip for one point, its index read on the device)
__global__ __launch_bounds__(256) void ks_spectral_pick(int nr, int nc, const int* __restrict__ picks, int k,
                                                        const int* __restrict__ ix, const int* __restrict__ iy,
                                                        const double* __restrict__ tx, const double* __restrict__ ty,
                                                        const double* __restrict__ Sr, const double* __restrict__ Sc,
                                                        const double* __restrict__ lam_r, const double* __restrict__ lam_c,
                                                        const int* __restrict__ state, double* __restrict__ What) {
  if (state[0]) return;
  const long long dim = (long long)nr * nc;
  const long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (idx >= dim) return;
  const int j = int(idx / nc), c = int(idx % nc);
  const int p = picks[k];
  const PointWeights pw = point_weights(nr, nc, ix[p], iy[p], tx[p], ty[p]);
  double v = 0.0;
#pragma unroll
  for (int t = 0; t < 3; ++t)
    if (pw.y[t] >= 0) v += pw.w[t] * Sr[(long long)j * nr + pw.y[t]] * Sc[(long long)pw.x[t] * nc + c];
  What[idx] = v / (lam_r[j] + lam_c[c]);
}

// The per-step pass, one lane per candidate x (k < 0: no update, the criterion of the first step only):
//   Phi[k,x] = (g(x) - sum_{j<k} L[k,j] Phi[j,x]) / L[k,k]          (psi_k at the candidates)
//   Res[i,x] -= A[k,i] Phi[k,x]                                       (w_i - P_{W_k+1} w_i at the candidates)
//   c(x) = sum_i Res[i,x]^2 / nu_x (MODE 0), (sum_i alpha_i Res[i,x])^2 / nu_x (MODE 1); 0 where nu_x = 0
// and the first maximum of c over the workgroup's candidates into pval / pidx[blockIdx.x].  L, A and alpha are the same
// for every lane (scalar loads).  Bytes: 8 ncand (k + 2 n + 3) -- Phi rows read, one written, Res read and written, g, nu.
template <int MODE>
__global__ __launch_bounds__(SG_TPB) void ks_step(int ncand, int n, int k, const double* __restrict__ g,
                                                  const double* __restrict__ Lrow, const double* __restrict__ lkk,
                                                  const double* __restrict__ A, double* __restrict__ Phi, double* __restrict__ Res,
                                                  const double* __restrict__ nu, const double* __restrict__ alpha,
                                                  const int* __restrict__ state, double* __restrict__ pval, int* __restrict__ pidx) {
  __shared__ double bv[SG_TPB];
  __shared__ int bi[SG_TPB];
  if (state[0]) return;
  const int x = blockIdx.x * SG_TPB + threadIdx.x;
  double c = -1.0;
  if (x < ncand) {
    double phi = 0.0;
    if (k >= 0) {
      double s = g[x];
      const double* ph = Phi + x;
      int j = 0;
      for (; j + 4 <= k; j += 4) {
        const double p0 = ph[(long long)j * ncand], p1 = ph[(long long)(j + 1) * ncand];
        const double p2 = ph[(long long)(j + 2) * ncand], p3 = ph[(long long)(j + 3) * ncand];
        s -= Lrow[j] * p0;
        s -= Lrow[j + 1] * p1;
        s -= Lrow[j + 2] * p2;
        s -= Lrow[j + 3] * p3;
      }
      for (; j < k; ++j) s -= Lrow[j] * ph[(long long)j * ncand];
      phi = s / lkk[k];
      Phi[(long long)k * ncand + x] = phi;
    }
    const double* Ak = A + (long long)(k >= 0 ? k : 0) * n;
    double s = 0.0;
    for (int i = 0; i < n; ++i) {
      double r = Res[(long long)i * ncand + x];
      if (k >= 0) {
        r -= Ak[i] * phi;
        Res[(long long)i * ncand + x] = r;
      }
      if (MODE == 0) s += r * r;
      else s += alpha[i] * r;
    }
    const double v = nu[x];
    c = v > 0.0 ? (MODE == 0 ? s : s * s) / v : 0.0;
  }
  bv[threadIdx.x] = c;
  bi[threadIdx.x] = x;
  __syncthreads();
  for (int h = SG_TPB / 2; h > 0; h >>= 1) {
    if (int(threadIdx.x) < h) {
      const double o = bv[threadIdx.x + h];
      const int oi = bi[threadIdx.x + h];
      if (o > bv[threadIdx.x] || (o == bv[threadIdx.x] && oi < bi[threadIdx.x])) {
        bv[threadIdx.x] = o;
        bi[threadIdx.x] = oi;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    pval[blockIdx.x] = bv[0];
    pidx[blockIdx.x] = bi[0];
  }
}

// Step k's pick: the first maximum over the partials (each thread walks its blocks in ascending order, then a tree that
// prefers the lower index on ties: the np.argmax pick, the same bits on every run), the stop rules, and in MODE 1 the
// direction alpha that chose it (the last eigenvector row of T) into alpha_out[k].  A step after a stop writes -1 / 0.
__global__ __launch_bounds__(SG_SELECT) void ks_select(int nblk, int k, int n, double rel_tol, const double* __restrict__ pval,
                                                       const int* __restrict__ pidx, const double* __restrict__ T,
                                                       int* __restrict__ state, double* __restrict__ scal, int* __restrict__ picks,
                                                       double* __restrict__ crit, double* __restrict__ alpha_out) {
  __shared__ double bv[SG_SELECT];
  __shared__ int bi[SG_SELECT];
  __shared__ int take;
  if (state[0]) {
    if (threadIdx.x == 0) {
      picks[k] = -1;
      crit[k] = 0.0;
    }
    return;
  }
  double best = -1.0;
  int at = 0x7fffffff;
  for (int b = threadIdx.x; b < nblk; b += SG_SELECT) {
    const double v = pval[b];
    if (v > best) {
      best = v;
      at = pidx[b];
    }
  }
  bv[threadIdx.x] = best;
  bi[threadIdx.x] = at;
  __syncthreads();
  for (int h = SG_SELECT / 2; h > 0; h >>= 1) {
    if (int(threadIdx.x) < h) {
      const double o = bv[threadIdx.x + h];
      const int oi = bi[threadIdx.x + h];
      if (o > bv[threadIdx.x] || (o == bv[threadIdx.x] && oi < bi[threadIdx.x])) {
        bv[threadIdx.x] = o;
        bi[threadIdx.x] = oi;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double c = bv[0];
    if (k == 0) scal[0] = c;
    int reason = -1;
    if (!(c > 0.0)) reason = 2;
    else if (k > 0 && c <= rel_tol * scal[0]) reason = 1;
    if (reason >= 0) {
      state[0] = 1;
      state[1] = reason;
      picks[k] = -1;
      crit[k] = 0.0;
    } else {
      picks[k] = bi[0];
      crit[k] = c;
      state[2] += 1;
    }
    take = reason < 0;
  }
  __syncthreads();
  if (alpha_out && take)
    for (int i = threadIdx.x; i < n; i += SG_SELECT) alpha_out[(long long)k * n + i] = T[(long long)(n - 1) * n + i];
}

// The Cholesky row of the sensors' Gram matrix and the row of A for pick p = picks[k]:
//   L[k,j] = Phi[j,p] (j < k),  L[k,k]^2 = nu_p - sum_j L[k,j]^2,  A[k,i] = Res[i,p] / L[k,k],
// then A^T A += A[k]^T A[k] (MODE 1) and nu_p = 0 (the pick is never taken again, whatever roundoff its residual keeps).
// L[k,k]^2 = ||omega_p - P_{W_k} omega_p||^2 and Res[i,p] = <omega_p - P_{W_k} omega_p, w_i>, so by Bessel's inequality
// (orthonormal w_i, unit alpha) L[k,k]^2 / nu_p >= c(p) = c_max in both modes: while the stop rule keeps c_max above
// rel_tol times the first step's criterion, the subtraction keeps that fraction of nu_p and does not cancel.  A pivot
// that is not positive all the same (rel_tol = 0 and a criterion at roundoff) ends the run as "no candidate left".
__global__ __launch_bounds__(256) void ks_prep(int ncand, int n, int k, int* __restrict__ picks, const double* __restrict__ Phi, const double* __restrict__ Res,
                                               double* __restrict__ nu, double* __restrict__ Lrow, double* __restrict__ lkk,
                                               double* __restrict__ A, double* __restrict__ AtA, int* __restrict__ state,
                                               double* __restrict__ crit, double* __restrict__ alpha_out) {
  __shared__ double red[256];
  __shared__ double arow[SG_MAX_N];
  __shared__ double l_sh;
  __shared__ int ok;
  if (state[0]) return;
  const int t = threadIdx.x;
  const int p = picks[k];
  double s = 0.0;
  for (int j = t; j < k; j += 256) {
    const double v = Phi[(long long)j * ncand + p];
    Lrow[j] = v;
    s += v * v;
  }
  red[t] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) red[t] += red[t + h];
    __syncthreads();
  }
  if (t == 0) {
    const double d2 = nu[p] - red[0];
    ok = d2 > 0.0;
    l_sh = sqrt(d2);
    if (ok) {
      lkk[k] = l_sh;
      nu[p] = 0.0;
    } else {
      state[0] = 1;
      state[1] = 2;
      state[2] -= 1;
      picks[k] = -1;
      crit[k] = 0.0;
    }
  }
  __syncthreads();
  if (!ok) {
    if (alpha_out)
      for (int i = t; i < n; i += 256) alpha_out[(long long)k * n + i] = 0.0;
    return;
  }
  for (int i = t; i < n; i += 256) {
    const double a = Res[(long long)i * ncand + p] / l_sh;
    arow[i] = a;
    A[(long long)k * n + i] = a;
  }
  __syncthreads();
  if (AtA)
    for (int idx = t; idx < n * n; idx += 256) AtA[idx] += arow[idx / n] * arow[idx % n];
}

__global__ void ks_info(const int* __restrict__ state, double* __restrict__ info) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    info[1] = double(state[2]);
    info[2] = state[0] ? double(state[1]) : 0.0;
  }
}

}  // namespace

extern "C" int rom_riesz_norms_h10(rom_fem* f, int npts, const int* ix_host, const int* iy_host, const double* tx_host,
                                   const double* ty_host, double* out_host) {
  ROM_CHECK(f && (npts == 0 || (ix_host && iy_host && tx_host && ty_host && out_host)), "rom_riesz_norms_h10: null argument");
  ROM_CHECK(npts >= 0, "rom_riesz_norms_h10: negative size");
  for (int p = 0; p < npts; ++p)
    ROM_CHECK(ix_host[p] >= 0 && ix_host[p] <= f->nc && iy_host[p] >= 0 && iy_host[p] <= f->nr,
              "rom_riesz_norms_h10: point %d outside the domain", p);
  if (npts == 0) return ROM_OK;
  rom_ctx* ctx = f->ctx;
  ROM_TRY(green_tables(f));
  DevPoints pts;
  ROM_TRY(pts.upload(ctx, npts, ix_host, iy_host, tx_host, ty_host));
  Tmp out;
  ROM_TRY(out.get(ctx, npts));
  {
    ROM_PROF(ctx, "sensor_norms", 30.0 * npts, 8.0 * 12.0 * npts);
    ks_norms<<<blocks_for(npts), 256, 0, ctx->stream>>>(f->nr, f->nc, npts, pts.ix, pts.iy, pts.tx, pts.ty, f->d_green, out);
    ROM_HIP(hipGetLastError());
  }
  return download(ctx, out, out_host, npts);  // the one host synchronisation
}

extern "C" int rom_sensor_greedy(rom_fem* f, rom_buf* C, int64_t c_row0, int n, int ncand, const int* ix_host, const int* iy_host,
                                 const double* tx_host, const double* ty_host, int m, int mode, double rel_tol, int64_t* picks_out,
                                 double* crit_out, double* A_out, double* alpha_out, double* info_host) {
  ROM_CHECK(f && C && ix_host && iy_host && tx_host && ty_host && picks_out && crit_out && A_out, "rom_sensor_greedy: null argument");
  ROM_CHECK(mode == 0 || mode == 1, "rom_sensor_greedy: mode must be 0 (collective) or 1 (worst case)");
  ROM_CHECK(n >= 1 && n <= (mode ? SG_MAX_N_WORST : SG_MAX_N),
            "rom_sensor_greedy: n = %d basis rows; 1 <= n <= %d (collective) or %d (worst case)", n, SG_MAX_N, SG_MAX_N_WORST);
  ROM_CHECK(m >= 1 && m <= SG_MAX_M, "rom_sensor_greedy: m = %d sensors; 1 <= m <= %d", m, SG_MAX_M);
  ROM_CHECK(ncand >= 1, "rom_sensor_greedy: no candidate points");
  ROM_CHECK(rel_tol >= 0.0, "rom_sensor_greedy: rel_tol must be >= 0");
  ROM_CHECK(c_row0 >= 0 && size_t(c_row0 + n) * f->dim <= C->n, "rom_sensor_greedy: rows out of range");
  for (int p = 0; p < ncand; ++p)
    ROM_CHECK(ix_host[p] >= 0 && ix_host[p] <= f->nc && iy_host[p] >= 0 && iy_host[p] <= f->nr,
              "rom_sensor_greedy: point %d outside the domain", p);
  rom_ctx* ctx = f->ctx;
  const int nr = f->nr, nc = f->nc;
  const int64_t dim = f->dim;
  const bool worst = mode == 1;
  ROM_TRY(green_tables(f));
  const SineTables st = rom_sine_tables(f);
  DevPoints pts;
  ROM_TRY(pts.upload(ctx, ncand, ix_host, iy_host, tx_host, ty_host));

  // 1. W: CGS2 in the A_1 inner product with the dead-row rule
  Tmp W, AW, norm0, t1, nrm1, nrm2, dead;
  ROM_TRY(W.get(ctx, size_t(n) * dim));
  ROM_TRY(AW.get(ctx, size_t(n) * dim));
  ROM_TRY(norm0.get(ctx, n));
  ROM_TRY(t1.get(ctx, n));
  ROM_TRY(nrm1.get(ctx, n));
  ROM_TRY(nrm2.get(ctx, n));
  ROM_TRY(dead.get(ctx, n));  // n ints in a block of n doubles
  int* d_dead = reinterpret_cast<int*>(dead.p());
  ROM_HIP(hipMemsetAsync(dead.p(), 0, size_t(n) * sizeof(double), ctx->stream));
  const double* c = C->p + c_row0 * dim;
  {
    ROM_PROF(ctx, "sensor_basis", 12.0 * n * n * double(dim), 48.0 * n * double(dim));
    ROM_TRY(rom_launch_h10norm(f, c, nullptr, n, norm0, false));
    ROM_HIP(hipMemcpyAsync(W.p(), c, size_t(n) * dim * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    for (int i = 0; i < n; ++i) ROM_TRY(romb_a1_append(f, W, AW, i, norm0, t1, t1, nrm1.p() + i, nrm2.p() + i, d_dead));
  }

  // 2. the candidates: nu (masked as they are picked), the basis values (Res at k = 0)
  Tmp nu, Res, Phi, g, What, Z, Om, Lrow, lkk, Ad, alpha, AtA, lam, T, crit, pick, part, state, scal, info;
  const int nblk = int(blocks_for(ncand, SG_TPB));
  ROM_TRY(nu.get(ctx, ncand));
  ROM_TRY(Res.get(ctx, size_t(n) * ncand));
  ROM_TRY(Phi.get(ctx, size_t(m) * ncand));
  ROM_TRY(g.get(ctx, ncand));
  ROM_TRY(What.get(ctx, dim));
  ROM_TRY(Z.get(ctx, dim));
  ROM_TRY(Om.get(ctx, dim));
  ROM_TRY(Lrow.get(ctx, m));
  ROM_TRY(lkk.get(ctx, m));
  ROM_TRY(Ad.get(ctx, size_t(m) * n));
  ROM_TRY(crit.get(ctx, m));
  ROM_TRY(pick.get(ctx, m));                   // m ints
  ROM_TRY(part.get(ctx, 2 * size_t(nblk)));    // values, then indices as ints
  ROM_TRY(state.get(ctx, 2));                  // 4 ints
  ROM_TRY(scal.get(ctx, 1));
  ROM_TRY(info.get(ctx, 4));
  if (worst) {
    ROM_TRY(alpha.get(ctx, size_t(m) * n));
    ROM_TRY(AtA.get(ctx, size_t(n) * n));
    ROM_TRY(lam.get(ctx, n));
    ROM_TRY(T.get(ctx, size_t(n) * n));
    ROM_HIP(hipMemsetAsync(alpha.p(), 0, size_t(m) * n * sizeof(double), ctx->stream));
  }
  int* d_state = reinterpret_cast<int*>(state.p());
  int* d_pick = reinterpret_cast<int*>(pick.p());
  double* pval = part.p();
  int* pidx = reinterpret_cast<int*>(part.p() + nblk);
  ROM_HIP(hipMemsetAsync(state.p(), 0, 2 * sizeof(double), ctx->stream));
  ROM_HIP(hipMemsetAsync(Ad.p(), 0, size_t(m) * n * sizeof(double), ctx->stream));
  ROM_HIP(hipMemsetAsync(info.p(), 0, 4 * sizeof(double), ctx->stream));
  ks_init<<<1, 256, 0, ctx->stream>>>(n, d_dead, worst ? AtA.p() : nullptr, info);
  ROM_HIP(hipGetLastError());
  {
    ROM_PROF(ctx, "sensor_norms", 30.0 * ncand, 8.0 * 12.0 * ncand);
    ks_norms<<<blocks_for(ncand), 256, 0, ctx->stream>>>(nr, nc, ncand, pts.ix, pts.iy, pts.tx, pts.ty, f->d_green, nu);
    ROM_HIP(hipGetLastError());
  }
  {
    ROM_PROF(ctx, "sensor_eval_basis", 8.0 * n * double(ncand), 8.0 * n * (4.0 * ncand));
    k_eval_points<<<dim3(blocks_for(ncand), n), 256, 0, ctx->stream>>>(nr, nc, dim, W, n, ncand, pts.ix, pts.iy, pts.tx, pts.ty,
                                                                      Res);
    ROM_HIP(hipGetLastError());
  }

  // 3. the steps
  auto step_pass = [&](int k) -> int {
    const double* al = worst ? T.p() + size_t(n - 1) * n : nullptr;
    const double rows = double(k > 0 ? k : 0) + (k >= 0 ? 2.0 : 0.0) + (k >= 0 ? 2.0 : 1.0) * n + 1.0;
    ROM_PROF(ctx, "sensor_step", double(ncand) * (2.0 * std::max(k, 0) + 4.0 * n), 8.0 * double(ncand) * rows);
    if (worst)
      ks_step<1><<<nblk, SG_TPB, 0, ctx->stream>>>(ncand, n, k, g, Lrow, lkk, Ad, Phi, Res, nu, al, d_state, pval, pidx);
    else
      ks_step<0><<<nblk, SG_TPB, 0, ctx->stream>>>(ncand, n, k, g, Lrow, lkk, Ad, Phi, Res, nu, al, d_state, pval, pidx);
    ROM_HIP(hipGetLastError());
    return ROM_OK;
  };
  if (worst) ROM_TRY(romb_small_eig(ctx, n, AtA, n, lam, T, n, SE_EIG, 0.0, true));
  ROM_TRY(step_pass(-1));
  for (int k = 0; k < m; ++k) {
    {
      ROM_PROF(ctx, "sensor_select", double(nblk), 12.0 * nblk);
      ks_select<<<1, SG_SELECT, 0, ctx->stream>>>(nblk, k, n, rel_tol, pval, pidx, worst ? T.p() : nullptr, d_state, scal, d_pick,
                                                  crit, worst ? alpha.p() : nullptr);
      ROM_HIP(hipGetLastError());
    }
    {
      ROM_PROF(ctx, "sensor_prep", 2.0 * (k + n * n), 8.0 * (k + 2.0 * n + n * n));
      ks_prep<<<1, 256, 0, ctx->stream>>>(ncand, n, k, d_pick, Phi, Res, nu, Lrow, lkk, Ad, worst ? AtA.p() : nullptr, d_state,
                                          crit, worst ? alpha.p() : nullptr);
      ROM_HIP(hipGetLastError());
    }
    if (k == m - 1) break;
    // the Green row g = omega_{p_k} at the candidates: one representer (spectral kernel, S_r What, (S_r What) S_c), a gather
    {
      ROM_PROF(ctx, "sensor_spectral", 8.0 * double(dim), 8.0 * double(dim));
      ks_spectral_pick<<<blocks_for(dim), 256, 0, ctx->stream>>>(nr, nc, d_pick, k, pts.ix, pts.iy, pts.tx, pts.ty, st.Sr, st.Sc, st.lam_r,
                                                                 st.lam_c, d_state, What);
      ROM_HIP(hipGetLastError());
    }
    ROM_TRY(rom_launch_gemm_nn(ctx, nr, nc, nr, 1.0, st.Sr, nr, What, nc, 0.0, Z, nc, nullptr, "sensor_green_r"));
    ROM_TRY(rom_launch_gemm_nn(ctx, nr, nc, nc, 1.0, Z, nc, st.Sc, nc, 0.0, Om, nc, nullptr, "sensor_green_c"));
    {
      ROM_PROF(ctx, "sensor_green_eval", 8.0 * ncand, 32.0 * ncand);
      k_eval_points<<<dim3(blocks_for(ncand), 1), 256, 0, ctx->stream>>>(nr, nc, dim, Om, 1, ncand, pts.ix, pts.iy, pts.tx, pts.ty,
                                                                        g);
      ROM_HIP(hipGetLastError());
    }
    if (worst) ROM_TRY(romb_small_eig(ctx, n, AtA, n, lam, T, n, SE_EIG, 0.0, true));
    ROM_TRY(step_pass(k));
  }

  // 4. results: the one host synchronisation
  ks_info<<<1, 1, 0, ctx->stream>>>(d_state, info);
  ROM_HIP(hipGetLastError());
  std::vector<int> picks_h(m);
  double info_h[4];
  ROM_HIP(hipMemcpyAsync(picks_h.data(), d_pick, size_t(m) * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  ROM_HIP(hipMemcpyAsync(crit_out, crit.p(), size_t(m) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ROM_HIP(hipMemcpyAsync(A_out, Ad.p(), size_t(m) * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (worst && alpha_out)
    ROM_HIP(hipMemcpyAsync(alpha_out, alpha.p(), size_t(m) * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ROM_HIP(hipMemcpyAsync(info_h, info.p(), 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ROM_HIP(hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < m; ++k) picks_out[k] = picks_h[k];
  if (info_host) {
    info_host[0] = info_h[0];
    info_host[1] = info_h[1];
    info_host[2] = info_h[2];
    info_host[3] = 1.0;
  }
  return ROM_OK;
}
