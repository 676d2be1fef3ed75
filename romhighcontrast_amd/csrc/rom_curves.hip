// Error curves of a GIVEN basis for every dimension in one call (rom_error_curves, include/romhc.h).
//
// The statistics loop of the reference's experiment() (src/experiments/HighContrast.py:176-214) measures, for every
// n = 1 .. vn_max_dim, the H^1_0 error of the projection onto span C[0..n) and of the Galerkin ROM on that span.  Both
// depend on the span only, so the call
//   1. builds an A_1-orthonormal W with span W[0..n) = span C[0..n) for every n: CGS2 in the A_1 inner product
//      (romb_a1_append); a row whose residual after the first round is at roundoff of its norm (a1_dead) becomes 0 and
//      adds no direction.  C = T W, T lower;
//   2. takes the projection coefficients P = U (A_1 W)^T with one MFMA product (P_n u_m = sum_{j<n} p_mj w_j);
//   3. forms, in ONE pass over U, every residual u_m - P_n u_m explicitly and its edge-form H^1_0 norm for all n
//      (kc_curve: the per-edge differences of the basis rows, DW, precomputed; lanes run over snapshots, each lane
//      carries the running residual of one edge through the basis and adds its square to the accumulator of every n);
//   4. with parameters a: for every m, the reduced matrix A(a_m) = sum_b a_mb W A_b W^T, factored ONCE by Cholesky; the
//      leading n x n block of the factor is the factor of the leading block, so one forward substitution serves all n
//      and each n costs one back substitution (kc_galerkin_nested: O(N^3) per parameter).  The Galerkin solution differs
//      from the projection inside span W[0..n) only:  ||u - g_n||^2 = ||u - P_n u||^2 + sum_{j<n} (c_j^(n) - p_mj)^2.
#include <algorithm>
#include <cmath>
#include <vector>

#include "rom_ops.h"

#include "rom_basis_int.h"

namespace {

// ---- small kernels ------------------------------------------------------------------------------------------------
// row i of T (N x N, lower): C_i = sum_{j<i} (t1_j + s1 t2_j) w_j + s1 s2 w_i with s1 = sqrt(nrm1), s2 = sqrt(nrm2)
__global__ void kc_trow(double* __restrict__ T, int N, int i, const double* __restrict__ t1, const double* __restrict__ t2,
                        const double* __restrict__ nrm1, const double* __restrict__ nrm2, const int* __restrict__ dead) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= N) return;
  const double s1 = sqrt(*nrm1);
  double v = 0.0;
  if (j < i) v = t1[j] + (dead[i] ? 0.0 : s1 * t2[j]);
  else if (j == i) v = dead[i] ? 0.0 : (i == 0 ? s1 : s1 * sqrt(*nrm2));
  T[size_t(i) * N + j] = v;
}

__global__ void kc_count_dead(const int* __restrict__ dead, int N, double* __restrict__ out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    int s = 0;
    for (int i = 0; i < N; ++i) s += dead[i];
    out[0] = double(s);
  }
}

__global__ void kc_status(const int* __restrict__ status, double* __restrict__ out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) out[0] = double(*status);
}

// a dead direction: unit diagonal in every block form (its row and column are exactly 0: w = 0), as kb_grow_ahat does
__global__ void kc_fix_dead(double* __restrict__ Ahat, int k, int N, const int* __restrict__ dead) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= k * N) return;
  const int b = idx / N, i = idx % N;
  if (dead[i]) Ahat[(size_t(b) * N + i) * N + i] = 1.0;
}

// ---- edges of the H^1_0 form --------------------------------------------------------------------------------------
// ||x||_A^2 = sum over edges e of (x(i_e) - x(i2_e))^2 (x(-1) = 0), the edge form of k_h10_partial / kb_greedy_pass:
// e < 2 dim: point pt = e / 2, even: east neighbour (none in the last column), odd: north neighbour (none in row 0);
// then nr west boundary terms (column 0) and nc south boundary terms (last row), without a neighbour
__device__ inline void edge_of(const StencilGeom& g, long long e, long long& i, long long& i2) {
  if (e < 2 * g.dim) {
    i = e >> 1;
    if ((e & 1) == 0) i2 = (i % g.nc) + 1 < g.nc ? i + 1 : -1;
    else i2 = i >= g.nc ? i - g.nc : -1;
  } else {
    const long long b = e - 2 * g.dim;
    i = b < g.nr ? b * g.nc : (long long)(g.nr - 1) * g.nc + (b - g.nr);
    i2 = -1;
  }
}

__host__ __device__ inline long long n_edges(const StencilGeom& g) { return 2 * g.dim + g.nr + g.nc; }

// DW[e * NP + j] = w_j(i_e) - w_j(i2_e) for j < N, 0 for N <= j < NP; one thread per edge writes its row
__global__ __launch_bounds__(256) void kc_edge_diffs(StencilGeom g, const double* __restrict__ W, int N, int NP,
                                                     double* __restrict__ DW) {
  const long long E = n_edges(g);
  for (long long e = blockIdx.x * 256ll + threadIdx.x; e < E; e += (long long)gridDim.x * 256) {
    long long i, i2;
    edge_of(g, e, i, i2);
    double* out = DW + e * NP;
    for (int j = 0; j < N; ++j) {
      const double* w = W + (long long)j * g.dim;
      out[j] = i2 >= 0 ? w[i] - w[i2] : w[i];
    }
    for (int j = N; j < NP; ++j) out[j] = 0.0;
  }
}

// ---- the one-pass residual curve ----------------------------------------------------------------------------------
// Lane = snapshot m (CV_SNAP per workgroup), workgroup = a contiguous range of edges.  Per edge the lane forms the
// residual difference x = (u_m - sum_{j<j0} p_mj w_j)(i) - (...)(i2) -- carried through the earlier chunks of the basis,
// then through this chunk one vector at a time -- and adds x^2 to acc[q], the squared error of n = j0 + q.  The edge
// index is uniform across the wave: the loads of DW are scalar (broadcast), the lanes' own loads are u_m(i), u_m(i2)
// (cache-line resident across consecutive edges) and, for a later chunk, the coefficients of the earlier ones.
// partial[(tile * (NC + 1) + q) * M + m].  NC <= 32: p and acc stay in registers.
constexpr int CV_SNAP = 256;
template <int NC>
__global__ __launch_bounds__(CV_SNAP) void kc_curve(StencilGeom g, const double* __restrict__ U, const double* __restrict__ DW,
                                                    int NP, const double* __restrict__ PT, int M, int N, int j0,
                                                    long long e_per_tile, double* __restrict__ partial) {
  const int m = blockIdx.x * CV_SNAP + threadIdx.x;
  const int mm = min(m, M - 1);
  const long long E = n_edges(g);
  const long long e_lo = blockIdx.y * e_per_tile, e_hi = min(E, e_lo + e_per_tile);
  const double* u = U + (long long)mm * g.dim;
  double p[NC], acc[NC + 1];
#pragma unroll
  for (int q = 0; q < NC; ++q) p[q] = j0 + q < N ? PT[(long long)(j0 + q) * M + mm] : 0.0;
#pragma unroll
  for (int q = 0; q <= NC; ++q) acc[q] = 0.0;
  for (long long e = e_lo; e < e_hi; ++e) {
    long long i, i2;
    edge_of(g, e, i, i2);
    const double* dw = DW + e * NP;
    double x = i2 >= 0 ? u[i] - u[i2] : u[i];
    for (int j = 0; j < j0; ++j) x -= PT[(long long)j * M + mm] * dw[j];
    acc[0] += x * x;
#pragma unroll
    for (int q = 0; q < NC; ++q) {
      x -= p[q] * dw[j0 + q];
      acc[q + 1] += x * x;
    }
  }
  if (m < M) {
#pragma unroll
    for (int q = 0; q <= NC; ++q) partial[((long long)blockIdx.y * (NC + 1) + q) * M + m] = acc[q];
  }
}

// ERR2[n * M + m] = sum over tiles (in order) of the partials, n = j0 + q for q in [q_lo, q_hi]
__global__ void kc_curve_finish(const double* __restrict__ partial, int ntiles, int NC, int M, int j0, int q_lo, int q_hi,
                                double* __restrict__ ERR2) {
  const long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  const int nq = q_hi - q_lo + 1;
  if (idx >= (long long)nq * M) return;
  const int q = q_lo + int(idx / M), m = int(idx % M);
  double s = 0.0;
  for (int t = 0; t < ntiles; ++t) s += partial[((long long)t * (NC + 1) + q) * M + m];
  ERR2[(long long)(j0 + q) * M + m] = s;
}

// ---- the nested Galerkin systems ----------------------------------------------------------------------------------
// One workgroup per parameter (grid-stride over m).  A (N x N, lower part used) = sum_b a_mb Ahat_b, factored in place
// (right-looking Cholesky, a barrier per column); y = L^{-1} bhat; thread t then takes n = t + 1 (stride blockDim):
// back substitution L_n^T c = y[0..n) in its own column of Z (Z[j * N + t]) and gap_n = sum_{j<n} (c_j - p_mj)^2.
// LDS: A and Z in shared memory (N <= GAL_LDS_MAX); else in a global slice per workgroup.  A non-positive pivot sets
// bit 0 of the status word (as the reduced solves do) and the system's gaps become NaN.
constexpr int GAL_LDS_MAX = 64, GAL_THREADS = 256;
template <bool LDS>
__global__ __launch_bounds__(GAL_THREADS) void kc_galerkin_nested(int N, int k, int M, const double* __restrict__ Ahat,
                                                                  const double* __restrict__ bhat, const double* __restrict__ a,
                                                                  const double* __restrict__ PT, double* __restrict__ ws,
                                                                  double* __restrict__ GAP, int* __restrict__ status) {
  __shared__ double sh[LDS ? 2 * GAL_LDS_MAX * GAL_LDS_MAX + GAL_LDS_MAX : 1];
  __shared__ int bad;
  double* A = LDS ? sh : ws + size_t(blockIdx.x) * (2 * size_t(N) * N + N);
  double* Z = A + size_t(N) * N;
  double* y = Z + size_t(N) * N;
  const int t = threadIdx.x;
  for (int m = blockIdx.x; m < M; m += gridDim.x) {
    for (int idx = t; idx < N * N; idx += GAL_THREADS) {
      double s = 0.0;
      for (int b = 0; b < k; ++b) s += a[size_t(m) * k + b] * Ahat[size_t(b) * N * N + idx];
      A[idx] = s;
    }
    for (int i = t; i < N; i += GAL_THREADS) y[i] = bhat[i];
    if (t == 0) bad = 0;
    __syncthreads();
    for (int c = 0; c < N; ++c) {  // column c: pivot, scale, rank-1 update of the trailing lower triangle
      const double d = A[c * N + c];
      if (!(d > 0.0)) {
        if (t == 0) bad = 1;
      }
      const double l = sqrt(d);
      __syncthreads();
      for (int r = c + 1 + t; r < N; r += GAL_THREADS) A[r * N + c] /= l;
      __syncthreads();
      if (t == 0) A[c * N + c] = l;
      const int len = N - c - 1;
      for (int idx = t; idx < len * len; idx += GAL_THREADS) {
        const int r = c + 1 + idx / len, s = c + 1 + idx % len;
        if (s <= r) A[r * N + s] -= A[r * N + c] * A[s * N + c];
      }
      __syncthreads();
    }
    for (int c = 0; c < N; ++c) {  // forward substitution, shared by every n
      if (t == 0) y[c] /= A[c * N + c];
      __syncthreads();
      for (int r = c + 1 + t; r < N; r += GAL_THREADS) y[r] -= A[r * N + c] * y[c];
      __syncthreads();
    }
    for (int tn = t; tn < N; tn += GAL_THREADS) {
      const int n = tn + 1;
      for (int j = 0; j < n; ++j) Z[j * N + tn] = y[j];
      double gap = 0.0;
      for (int j = n - 1; j >= 0; --j) {  // column-oriented back substitution: c_j, then remove it from the rows above
        const double cj = Z[j * N + tn] / A[j * N + j];
        for (int i = 0; i < j; ++i) Z[i * N + tn] -= A[j * N + i] * cj;
        const double dlt = cj - PT[size_t(j) * M + m];
        gap += dlt * dlt;
      }
      GAP[size_t(n) * M + m] = bad ? NAN : gap;
    }
    if (t == 0) {
      GAP[m] = 0.0;
      if (bad) atomicOr(status, 1);
    }
    __syncthreads();
  }
}

// ERR[(0 * (N+1) + n) * M + m] = sqrt(ERR2), ERR[(1 * (N+1) + n) * M + m] = sqrt(ERR2 + GAP) when GAP is given
__global__ void kc_curve_out(const double* __restrict__ ERR2, const double* __restrict__ GAP, size_t cnt, double* __restrict__ ERR) {
  const size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x;
  if (i >= cnt) return;
  const double e2 = fmax(ERR2[i], 0.0);
  ERR[i] = sqrt(e2);
  if (GAP) ERR[cnt + i] = sqrt(e2 + GAP[i]);
}

template <int NC>
void launch_curve(dim3 grid, hipStream_t st, const StencilGeom& g, const double* U, const double* DW, int NP, const double* PT,
                  int M, int N, int j0, long long ept, double* part) {
  kc_curve<NC><<<grid, CV_SNAP, 0, st>>>(g, U, DW, NP, PT, M, N, j0, ept, part);
}

}  // namespace

extern "C" int rom_error_curves(rom_fem* f, rom_buf* U, int64_t u_row0, int M, rom_buf* C, int64_t c_row0, int N, rom_buf* a,
                                rom_buf* ERR, rom_buf* P, rom_buf* T, double* info_host) {
  ROM_CHECK(f && U && ERR && (C || N == 0) && (P || N == 0 || M == 0) && (T || N == 0), "rom_error_curves: null argument");
  ROM_CHECK(M >= 0 && N >= 0 && u_row0 >= 0 && c_row0 >= 0, "rom_error_curves: negative size or offset");
  ROM_CHECK(M <= (1 << 24) && N <= 2048, "rom_error_curves: at most 2048 basis rows and 2^24 snapshots");
  const int64_t dim = f->dim;
  const int k = f->nrb * f->ncb;
  const int curves = a ? 2 : 1;
  ROM_CHECK(size_t(u_row0 + M) * dim <= U->n && (N == 0 || size_t(c_row0 + N) * dim <= C->n), "rom_error_curves: rows out of range");
  ROM_CHECK(size_t(curves) * (N + 1) * M <= ERR->n && (N == 0 || M == 0 || size_t(M) * N <= P->n) && (N == 0 || size_t(N) * N <= T->n) &&
                (!a || size_t(M) * k <= a->n),
            "rom_error_curves: output or parameter buffer too small");
  rom_ctx* ctx = f->ctx;
  const StencilGeom g = rom_make_geom(f->nrb, f->ncb, f->N);
  const double* u = U->p + u_row0 * dim;
  const double* c = N ? C->p + c_row0 * dim : nullptr;
  const int Nb = std::max(N, 1);
  Tmp W, AW, norm0, t1, t2, nrm1, nrm2, dead, PT, ERR2, GAP, info;
  ROM_TRY(W.get(ctx, size_t(Nb) * dim));
  ROM_TRY(AW.get(ctx, size_t(Nb) * dim));
  ROM_TRY(norm0.get(ctx, Nb));
  ROM_TRY(t1.get(ctx, size_t(Nb) * Nb));
  ROM_TRY(t2.get(ctx, size_t(Nb) * Nb));
  ROM_TRY(nrm1.get(ctx, Nb));
  ROM_TRY(nrm2.get(ctx, Nb));
  ROM_TRY(dead.get(ctx, Nb));  // N ints in a block of N doubles
  ROM_TRY(info.get(ctx, 2));
  int* d_dead = reinterpret_cast<int*>(dead.p());
  ROM_HIP(hipMemsetAsync(ctx->d_status, 0, sizeof(int), ctx->stream));
  ROM_HIP(hipMemsetAsync(dead.p(), 0, size_t(Nb) * sizeof(double), ctx->stream));
  // 1. CGS2 in the A_1 inner product
  if (N) {
    ROM_PROF(ctx, "curves_basis", 12.0 * N * N * double(dim), 48.0 * N * double(dim));
    ROM_TRY(rom_launch_h10norm(f, c, nullptr, N, norm0, false));  // ||C_i||_A^2
    ROM_HIP(hipMemcpyAsync(W.p(), c, size_t(N) * dim * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    for (int i = 0; i < N; ++i) {  // (row i of the N x N blocks t1, t2: kc_trow reads them)
      ROM_TRY(romb_a1_append(f, W, AW, i, norm0, t1.p() + size_t(i) * Nb, t2.p() + size_t(i) * Nb, nrm1.p() + i, nrm2.p() + i, d_dead));
      kc_trow<<<blocks_for(N), 256, 0, ctx->stream>>>(T->p, N, i, t1.p() + size_t(i) * Nb, t2.p() + size_t(i) * Nb,
                                                       nrm1.p() + i, nrm2.p() + i, d_dead);
      ROM_HIP(hipGetLastError());
    }
  }
  kc_count_dead<<<1, 1, 0, ctx->stream>>>(d_dead, N, info.p());
  ROM_HIP(hipGetLastError());
  int gal_route = -1, chunks = 0, ntiles = 0;
  if (M > 0) {
    // 2. projection coefficients, PT[j * M + m] = <u_m, w_j>_A
    ROM_TRY(ERR2.get(ctx, size_t(N + 1) * M));
    ROM_TRY(PT.get(ctx, size_t(Nb) * M));
    if (N) {
      ROM_TRY(rom_launch_gemm_nt(ctx, N, M, dim, 1.0, AW, dim, u, dim, 0.0, PT, M, "gemm_nt"));
      ROM_TRY(romb_transpose(ctx, P->p, N, PT, M, N, M));
    }
    // 3. the residual curves: one pass over U per chunk of 32 basis vectors
    {
      const long long E = n_edges(g);
      const int NP = N <= 8 ? 8 : N <= 16 ? 16 : ((N + 31) / 32) * 32;
      Tmp DW, part;
      ROM_TRY(DW.get(ctx, size_t(E) * NP));
      {
        ROM_PROF(ctx, "curves_edge_diffs", 2.0 * double(E) * N, 8.0 * double(E) * (2.0 * N + NP));
        kc_edge_diffs<<<unsigned(std::min<long long>((E + 255) / 256, 4096)), 256, 0, ctx->stream>>>(g, W, N, NP, DW);
        ROM_HIP(hipGetLastError());
      }
      const int mgroups = (M + CV_SNAP - 1) / CV_SNAP;
      ntiles = int(std::max<long long>(1, std::min<long long>((2 * ctx->n_cu + mgroups - 1) / mgroups, (E + 255) / 256)));
      const long long ept = (E + ntiles - 1) / ntiles;
      ntiles = int((E + ept - 1) / ept);
      const int NCmax = NP <= 8 ? 8 : NP <= 16 ? 16 : 32;
      ROM_TRY(part.get(ctx, size_t(ntiles) * (NCmax + 1) * M));
      const dim3 grid(mgroups, ntiles);
      int j0 = 0;
      do {
        const int rest = N - j0;
        const int NC = rest <= 8 ? 8 : rest <= 16 ? 16 : 32;
        const int used = std::min(rest, NC);
        {
          ROM_PROF(ctx, NC == 8 ? "curves_pass_nc8" : NC == 16 ? "curves_pass_nc16" : "curves_pass_nc32",
                   4.0 * double(M) * E * (NC + j0 / 2.0), 8.0 * double(M) * dim);
          if (NC == 8) launch_curve<8>(grid, ctx->stream, g, u, DW, NP, PT, M, N, j0, ept, part);
          else if (NC == 16) launch_curve<16>(grid, ctx->stream, g, u, DW, NP, PT, M, N, j0, ept, part);
          else launch_curve<32>(grid, ctx->stream, g, u, DW, NP, PT, M, N, j0, ept, part);
          ROM_HIP(hipGetLastError());
        }
        const int q_lo = j0 == 0 ? 0 : 1;
        kc_curve_finish<<<blocks_for(size_t(used - q_lo + 1) * M), 256, 0, ctx->stream>>>(part, ntiles, NC, M, j0, q_lo, used, ERR2);
        ROM_HIP(hipGetLastError());
        ++chunks;
        j0 += used;
      } while (j0 < N);
    }
    // 4. the nested Galerkin systems
    if (a) {
      ROM_TRY(GAP.get(ctx, size_t(N + 1) * M));
      if (N == 0) {
        ROM_HIP(hipMemsetAsync(GAP.p(), 0, size_t(M) * sizeof(double), ctx->stream));
      } else {
        Tmp Ahat, bhat, ws;
        ROM_TRY(Ahat.get(ctx, size_t(k) * N * N));
        ROM_TRY(bhat.get(ctx, N));
        ROM_TRY(romb_reduced_tensor(f, W, N, AW, Ahat, bhat));  // Ahat_b = W A_b W^T, W B_total (AW is free: PT holds the coefficients)
        kc_fix_dead<<<blocks_for(size_t(k) * N), 256, 0, ctx->stream>>>(Ahat, k, N, d_dead);
        ROM_HIP(hipGetLastError());
        if (N <= GAL_LDS_MAX) {
          gal_route = 0;
          ROM_PROF(ctx, "curves_galerkin_lds", double(M) * (2.0 * k * N * N + N * N * N), 8.0 * double(M) * (k + 2.0 * N));
          kc_galerkin_nested<true><<<unsigned(std::min(M, 65535)), GAL_THREADS, 0, ctx->stream>>>(N, k, M, Ahat, bhat, a->p, PT,
                                                                                                 nullptr, GAP, ctx->d_status);
        } else {
          // global route: A, Z and y of a workgroup in its own slice of at most 2^25 doubles in all
          gal_route = 1;
          const size_t per = 2 * size_t(N) * N + N;
          const int nwg = int(std::max<size_t>(1, std::min<size_t>({size_t(M), size_t(4 * ctx->n_cu), (size_t(1) << 25) / per})));
          ROM_TRY(ws.get(ctx, per * nwg));
          ROM_PROF(ctx, "curves_galerkin_global", double(M) * (2.0 * k * N * N + N * N * N), 8.0 * double(M) * (k + 2.0 * N));
          kc_galerkin_nested<false><<<unsigned(nwg), GAL_THREADS, 0, ctx->stream>>>(N, k, M, Ahat, bhat, a->p, PT, ws, GAP,
                                                                                   ctx->d_status);
        }
        ROM_HIP(hipGetLastError());
      }
    }
    kc_curve_out<<<blocks_for(size_t(N + 1) * M), 256, 0, ctx->stream>>>(ERR2, a ? GAP.p() : nullptr, size_t(N + 1) * M, ERR->p);
    ROM_HIP(hipGetLastError());
  }
  // the one host synchronisation: dead count and status word
  kc_status<<<1, 1, 0, ctx->stream>>>(ctx->d_status, info.p() + 1);
  ROM_HIP(hipGetLastError());
  double host[2] = {0.0, 0.0};
  ROM_TRY(download(ctx, info, host, 2));
  if (info_host) {
    info_host[0] = host[0];
    info_host[1] = double(gal_route);
    info_host[2] = double(chunks);
    info_host[3] = double(ntiles);
  }
  if (host[1] != 0.0) {
    ROM_HIP(hipMemsetAsync(ctx->d_status, 0, sizeof(int), ctx->stream));
    rom_set_error("rom_error_curves: reduced matrix not positive definite");
    return ROM_ERR_NOT_SPD;
  }
  return ROM_OK;
}
