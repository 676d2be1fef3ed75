// The batched 2-D sine transform of dense snapshot rows, and the POD in the H^1_0 inner product built on it
// (rom_sine_transform, rom_pod_h10; include/romhc.h).
//
// A_1 (A_preassembled4h1_norm, src/lib/SolutionsManagers.py:49) = S Lambda S with S = S_r (x) S_c symmetric and orthogonal and
// Lambda[j,k] = lam_r[j] + lam_c[k] (rom_riesz.hip, header comment; the tables are rom_riesz_tables').  With a snapshot row as
// an nr x nc array X_i and W_i = sqrt(Lambda) o (S_r X_i S_c),
//     <x_i, x_l>_{H^1_0} = <w_i, w_l>_2 ,
// so the H^1_0-POD of the block X -- the n-dimensional space that minimises sum_m ||u_m - P_n u_m||^2_{H^1_0}, where the PCA fit
// of ReducedBasisPCA.build (src/lib/ReducedBasis.py:189-200) minimises the Euclidean sum -- is the Euclidean POD of W = Z Sigma
// Q^T mapped back: singular values Sigma, modes v_i = S_r (Lambda^-1/2 o q_i) S_c, A_1-orthonormal.  Centring commutes with the
// (linear) transform: rom_pod_ex centres W and X is never written.  Nothing is squared on the way (the method of snapshots on
// G = U A_1 U^T stops at sqrt(eps) sigma_1): the transform is orthogonal up to the diagonal scaling, so rom_pod_ex keeps its range.
//
// The transform  OUT_i = Lambda^(post/2) o ( S_r (Lambda^(pre/2) o X_i) S_c )  is two MFMA products per chunk of rows:
//   right factor  T S_c : ONE rom_launch_gemm_nn over the K * nr rows of length nc (chunks of 65535 * 64 rows);
//   left factor   S_r T_i per snapshot: k_sine_left, a strided-batched NN product on the rom_mma.h tile engine.  It contracts the
//     MIDDLE index of the (K, nr, nc) array in place of the [j][i][k] re-layout + permute pass of rom_riesz_h10 (two more passes
//     over the block): A operand = S_r (shared by all snapshots, K-contiguous, odd leading dimension: k-major staging map),
//     B operand = snapshot i at stride dim (lane -> column: 512 contiguous bytes per wave-instruction), snapshot index in
//     grid.z, so the launch count does not grow with K (one launch per 65535 snapshots).  Fused: Lambda^(pre/2) on the B operand
//     as it is staged, Lambda^(post/2) on the accumulators as they are stored.
// pre == 0: right factor first, the left factor's epilogue scales.  pre != 0: left factor first (its staging scales), then the
// right factor, then -- only when post != 0 as well -- one elementwise pass.  No floating-point atomics anywhere; k_sine_left sums
// in one fixed order, and the right factor takes whatever route rom_launch_gemm_nn picks for its shape (the general kernel, the
// thin one, or split-K with its deterministic reduction): the same bits on every call with the same arguments and workspace
// limit.  The workspace T is K x dim doubles, or as many whole rows as rom_set_workspace_limit allows (at least one): the
// transform then runs in row chunks, and a chunk of very few rows of a wide grid (K nr <= ~384 with nc >= 256) can put the
// right factor on another route than the whole block takes -- equal to rounding, not to the bit.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "rom_mma.h"
#include "rom_ops.h"

#include "rom_basis_int.h"

namespace {

constexpr int64_t SP_MAX_ROWS = int64_t(65535) * 64;  // rows of the general NN product per launch (grid.y <= 65535)
constexpr int SP_MAX_BATCH = 65535;                    // snapshots per launch of k_sine_left (grid.z)

// lam^(e/2), e in {-2, -1, 0, 1, 2}
__device__ inline double lam_pow(double lam, int e) {
  switch (e) {
    case 2: return lam;
    case 1: return sqrt(lam);
    case -1: return 1.0 / sqrt(lam);
    case -2: return 1.0 / lam;
    default: return 1.0;
  }
}

// OUT_i[p, q] = Lambda^(post/2)[p, q] * sum_j S_r[p, j] * Lambda^(pre/2)[j, q] * X_i[j, q],  i = blockIdx.z.
// grid (ceil(nc / 64), ceil(nr / 64), snapshots) x 256.  Tails in p, q and j are staged as zeros and never stored.
__global__ __launch_bounds__(256) void k_sine_left(int nr, int nc, const double* __restrict__ Sr,
                                                   const double* __restrict__ lam_r, const double* __restrict__ lam_c,
                                                   const double* __restrict__ X, double* __restrict__ OUT, int pre, int post) {
  __shared__ __align__(16) double stage[STAGE_TOTAL];
  const WavePos wp;
  const int t = threadIdx.x;
  const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
  const long long dim = (long long)nr * nc;
  const double* __restrict__ Xi = X + blockIdx.z * dim;
  double* __restrict__ Oi = OUT + blockIdx.z * dim;
  // A staging (rows of S_r, only 8-byte aligned): lane -> k, rows (t >> 4) + 16 x
  const int ak = kmajor_k();
  // B staging: lane -> column, k rows (t >> 6) + 4 x
  const int bc = t & 63, bk0 = t >> 6;
  const int col = c0 + bc;
  const bool col_ok = col < nc;
  const double lc_stage = (pre != 0 && col_ok) ? lam_c[col] : 0.0;
  auto load = [&](int ch, double va[4], double vb[4]) {
    const int k0 = ch * BK;
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      const int r = r0 + kmajor_row(x), k = k0 + ak;
      va[x] = (r < nr && k < nr) ? Sr[(long long)r * nr + k] : 0.0;
    }
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      const int k = k0 + bk0 + 4 * x;
      double v = 0.0;
      if (k < nr && col_ok) {
        v = Xi[(long long)k * nc + col];
        if (pre != 0) v *= lam_pow(lam_r[k] + lc_stage, pre);
      }
      vb[x] = v;
    }
  };
  Acc acc;
  acc_zero(acc);
  const int nch = (nr + BK - 1) / BK;
  double va[4], vb[4];
  load(0, va, vb);
  for (int ch = 0; ch < nch; ++ch) {
    double* sA = stage + (ch & 1) * STAGE_DOUBLES;
    double* sB = stage + 2 * STAGE_DOUBLES + (ch & 1) * STAGE_DOUBLES;
    stage_store_kmajor(sA, va);
#pragma unroll
    for (int x = 0; x < 4; ++x) sB[bc * LDK + bk0 + 4 * x] = vb[x];
    __syncthreads();
    if (ch + 1 < nch) load(ch + 1, va, vb);
    mma_chunk(sA, sB, acc, wp);
    // (the buffer written next iteration is the other one; that iteration's barrier orders its readers, as in gemm_loop2)
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = c0 + acc_col(wp, j);
    if (c >= nc) continue;
    const double lc = post != 0 ? lam_c[c] : 0.0;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int r = r0 + acc_row(wp, i, g);
        if (r >= nr) continue;
        double v = acc.c[i][j][g];
        if (post != 0) v *= lam_pow(lam_r[r] + lc, post);
        Oi[(long long)r * nc + c] = v;
      }
  }
}

// X_i o= Lambda^(e/2) for `rows` rows (the one combination the fused scalings do not cover: pre != 0 and post != 0)
__global__ __launch_bounds__(256) void k_lambda_scale(int nr, int nc, long long rows, const double* __restrict__ lam_r,
                                                      const double* __restrict__ lam_c, double* __restrict__ X, int e) {
  const long long dim = (long long)nr * nc, total = dim * rows;
  for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
    const long long r = idx % dim;
    X[idx] *= lam_pow(lam_r[r / nc] + lam_c[r % nc], e);
  }
}

int launch_left(rom_fem* f, const double* X, int K, int pre, int post, double* OUT) {
  rom_ctx* ctx = f->ctx;
  const int nr = f->nr, nc = f->nc;
  const SineTables st = rom_sine_tables(f);
  for (int i0 = 0; i0 < K; i0 += SP_MAX_BATCH) {
    const int take = std::min(SP_MAX_BATCH, K - i0);
    const dim3 grid(unsigned((nc + 63) / 64), unsigned((nr + 63) / 64), unsigned(take));
    ROM_PROF(ctx, "sine_transform_r", 2.0 * take * double(nr) * nr * nc, 16.0 * take * double(f->dim));
    k_sine_left<<<grid, 256, 0, ctx->stream>>>(nr, nc, st.Sr, st.lam_r, st.lam_c, X + size_t(i0) * f->dim, OUT + size_t(i0) * f->dim, pre, post);
    ROM_HIP(hipGetLastError());
  }
  return ROM_OK;
}

int launch_right(rom_fem* f, const double* X, int K, double* OUT) {
  rom_ctx* ctx = f->ctx;
  const int nr = f->nr, nc = f->nc;
  const double* Sc = rom_sine_tables(f).Sc;
  const int64_t rows = int64_t(K) * nr;
  for (int64_t q0 = 0; q0 < rows; q0 += SP_MAX_ROWS) {
    const int64_t take = std::min(SP_MAX_ROWS, rows - q0);
    ROM_TRY(rom_launch_gemm_nn(ctx, take, nc, nc, 1.0, X + q0 * nc, nc, Sc, nc, 0.0, OUT + q0 * nc, nc, nullptr, "sine_transform_c"));
  }
  return ROM_OK;
}

}  // namespace

// OUT[k] = Lambda^(post/2) o (S_r (Lambda^(pre/2) o X[k]) S_c), k < K, on raw device rows (OUT != X; enqueued only).
int rom_launch_sine_transform(rom_fem* f, const double* X, int K, int pre, int post, double* OUT) {
  if (K <= 0) return ROM_OK;
  rom_ctx* ctx = f->ctx;
  ROM_TRY(rom_riesz_tables(f));
  const int64_t dim = f->dim;
  const int chunk = int(std::max<size_t>(1, std::min<size_t>(size_t(K), ctx->ws_limit / (size_t(dim) * sizeof(double)))));
  Tmp T;
  ROM_TRY(T.get(ctx, size_t(chunk) * dim));
  for (int k0 = 0; k0 < K; k0 += chunk) {
    const int take = std::min(chunk, K - k0);
    const double* x = X + size_t(k0) * dim;
    double* out = OUT + size_t(k0) * dim;
    if (pre == 0) {
      ROM_TRY(launch_right(f, x, take, T));
      ROM_TRY(launch_left(f, T, take, 0, post, out));
    } else {
      ROM_TRY(launch_left(f, x, take, pre, 0, T));
      ROM_TRY(launch_right(f, T, take, out));
      if (post != 0) {
        const SineTables st = rom_sine_tables(f);
        const size_t total = size_t(take) * dim;
        ROM_PROF(ctx, "sine_transform_scale", 4.0 * double(total), 16.0 * double(total));
        k_lambda_scale<<<unsigned(std::min<size_t>((total + 255) / 256, size_t(16) * 1024)), 256, 0, ctx->stream>>>(
            f->nr, f->nc, take, st.lam_r, st.lam_c, out, post);
        ROM_HIP(hipGetLastError());
      }
    }
  }
  return ROM_OK;
}

double rom_sine_transform_flops(rom_fem* f, int K) {
  return 2.0 * K * (double(f->nr) * f->nr * f->nc + double(f->nr) * f->nc * f->nc);
}

extern "C" int rom_sine_transform(rom_fem* f, rom_buf* X, int64_t x_row0, int K, int pre, int post, rom_buf* OUT, int64_t out_row0) {
  ROM_CHECK(f && X && OUT, "rom_sine_transform: null argument");
  ROM_CHECK(K >= 0 && x_row0 >= 0 && out_row0 >= 0, "rom_sine_transform: negative size");
  ROM_CHECK(pre >= -2 && pre <= 2 && post >= -2 && post <= 2, "rom_sine_transform: pre and post must be in -2 .. 2");
  const int64_t dim = f->dim;
  ROM_CHECK(size_t(x_row0 + K) * dim <= X->n && size_t(out_row0 + K) * dim <= OUT->n, "rom_sine_transform: rows out of range");
  if (K == 0) return ROM_OK;
  const double* x = X->p + x_row0 * dim;
  double* out = OUT->p + out_row0 * dim;
  ROM_CHECK(out + size_t(K) * dim <= x || x + size_t(K) * dim <= out, "rom_sine_transform: OUT overlaps X");
  ROM_TRY(rom_launch_sine_transform(f, x, K, pre, post, out));
  ROM_HIP(hipStreamSynchronize(f->ctx->stream));  // (the workspace goes back to the allocator)
  return ROM_OK;
}

// rom_pod_ex in the H^1_0 inner product: W = X in energy coordinates (M x dim temporary), its Euclidean POD, the modes back.
extern "C" int rom_pod_h10(rom_fem* f, rom_buf* Xb, int64_t x_row0, int M, int n, int center, double rel_floor, rom_buf* Vb,
                           int64_t v_row0, double* sigma_host, double* info_host) {
  ROM_CHECK(f && Xb && Vb && (sigma_host || n == 0), "rom_pod_h10: null argument");
  ROM_CHECK(M >= 1 && n >= 0 && x_row0 >= 0 && v_row0 >= 0, "rom_pod_h10: bad sizes");
  const int64_t dim = f->dim;
  ROM_CHECK(n <= std::min<int64_t>(M, dim), "rom_pod_h10: %d modes requested from a %d x %lld block", n, M, (long long)dim);
  ROM_CHECK(size_t(x_row0 + M) * dim <= Xb->n && size_t(v_row0 + n) * dim <= Vb->n, "rom_pod_h10: buffers too small");
  rom_ctx* ctx = f->ctx;
  Tmp W, Q;
  ROM_TRY(W.get(ctx, size_t(M) * dim));
  ROM_TRY(Q.get(ctx, size_t(std::max(n, 1)) * dim));
  ROM_TRY(rom_launch_sine_transform(f, Xb->p + x_row0 * dim, M, 0, 1, W));
  double info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  ROM_TRY(rom_pod_ex(ctx, W.b, 0, M, dim, n, center, rel_floor, Q.b, 0, sigma_host, info));
  if (n > 0) {
    // orthonormal rows (completed ones included) -> A_1-orthonormal rows; the sign rule on the rows that are returned
    double* V = Vb->p + v_row0 * dim;
    ROM_TRY(rom_launch_sine_transform(f, Q, n, -1, 0, V));
    ROM_TRY(rom_launch_rows_sign_flip(ctx, V, n, dim));
  }
  ROM_HIP(hipStreamSynchronize(ctx->stream));
  if (info_host) {
    info[4] += rom_sine_transform_flops(f, M + n);
    memcpy(info_host, info, sizeof(info));
  }
  return ROM_OK;
}
