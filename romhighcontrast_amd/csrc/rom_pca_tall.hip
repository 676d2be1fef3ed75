// rom_pca_tall: full PCA of a TALL snapshot block (M >> dim, dim <= 1024) -- PCA(n).fit + .transform of the reference's
// second experiment (src/experiments/NonLinearROM.py:34-41: 25,000 x 81).
//
// Method: block one-sided Jacobi whose sweeps are Gram matrices of the ROTATED DATA.
//   V = I;  repeat:  Y = Xc V^T,  G = Y^T Y,  d_i = sqrt(g_ii);
//                    converged when |g_ij| <= 64 eps max(d) max(d_i, d_j) for all i != j;
//                    G = Q diag(lam) Q^T by Jacobi with the relative stopping rule (romb_small_eig, gram_like);
//                    V <- Q^T V, rows re-orthonormalised (one Newton-Schulz step: the defect is O(dim eps)).
// After the first rotation G is graded (its diagonal spans sigma_1^2 ... (eps sigma_1)^2) and a Jacobi that stops on
// |a_pq| <= tol sqrt(a_pp a_qq) delivers its small eigenvalues to high relative accuracy: no sqrt(eps) floor as in the
// one-pass covariance route.  G always comes from the data (never as V C V^T): that is what carries the accuracy.
//
// Kernels: k_pca_tall_fused (dim <= 96: the slab engine of rom_slab.h, rotation and Y^T Y in one pass over the block, scores
// written from the same slab), k_syrk_tn (any dim: G = Y^T Y of a row-major block, the TN product the NT / NN engines of
// rom_mma.h do not have), both with per-chunk partial sums that kb_partials_reduce adds in a fixed order (no floating-point
// atomics: the same bits on every call).
#include <cmath>
#include <cstring>
#include <numeric>

#include "rom_basis_int.h"
#include "rom_slab.h"

namespace {

constexpr int PT_FUSED_MAX = 96;   // largest dim of the fused kernel (V + two slabs in 160 KB of LDS)
constexpr int PT_XREG = SLAB_ROWS * PT_FUSED_MAX / SLAB_THREADS;   // doubles of a slab per thread
constexpr int PT_PASS_CAP = 6;
constexpr double PT_EPS = 1.1102230246251565e-16;   // 2^-53
constexpr double PT_C = 64.0;
constexpr double PT_NOISE_FLOOR = 1e-13;

// ---- column means with fixed-order partials -------------------------------------------------------------------------
// part[chunk][j] = sum of column j over the rows of the chunk; 256 threads = (256 / cw) row lanes x cw columns
__global__ __launch_bounds__(256) void k_colsum_partial(const double* __restrict__ X, int M, int dim, int rows_per_chunk, int cw,
                                                        double* __restrict__ part) {
  __shared__ double red[256];
  const int t = threadIdx.x, c0 = t % cw, ry = t / cw, nry = 256 / cw;
  const long long r_begin = (long long)blockIdx.x * rows_per_chunk;
  const long long r_end = min((long long)M, r_begin + rows_per_chunk);
  for (int cb = 0; cb < dim; cb += cw) {
    const int c = cb + c0;
    double s = 0.0;
    if (c < dim)
      for (long long r = r_begin + ry; r < r_end; r += nry) s += X[r * dim + c];
    red[t] = s;
    __syncthreads();
    if (ry == 0 && c < dim) {
      for (int q = 1; q < nry; ++q) s += red[q * cw + c0];
      part[size_t(blockIdx.x) * dim + c] = s;
    }
    __syncthreads();
  }
}

__global__ void k_subtract_mean(double* __restrict__ X, size_t count, int dim, const double* __restrict__ mean) {
  for (size_t e = blockIdx.x * size_t(blockDim.x) + threadIdx.x; e < count; e += size_t(gridDim.x) * blockDim.x)
    X[e] -= mean[e % size_t(dim)];
}

// ---- fused pass, dim <= 96 ------------------------------------------------------------------------------------------
// Workgroup `b` owns slabs_per_chunk slabs of 32 rows.  Per slab: Xs <- rows of X (prefetched in registers under the
// previous slab's MFMAs), Ys = Xs Vs^T (NT), acc += Ys^T Ys (TN: the lower 16x16 tiles, at most three per wave).  With S the
// slab of scores goes to S[(row, col < n_s)] as it is formed.  P[b] (dpad x dpad, lower tiles) receives the partial.
__global__ __launch_bounds__(SLAB_THREADS) void k_pca_tall_fused(const double* __restrict__ X, int M, int dim, int dpad,
                                                                const double* __restrict__ V, int slabs_per_chunk,
                                                                double* __restrict__ P, double* __restrict__ S, int n_s) {
  extern __shared__ double pt_lds[];
  const int LX = slab_ld_nt(dpad), LY = slab_ld_tn(dpad);
  double* Vs = pt_lds;                 // dpad x LX
  double* Xs = Vs + dpad * LX;         // 32 x LX
  double* Ys = Xs + SLAB_ROWS * LX;    // 32 x LY
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int i = lane & 15, k = lane >> 4;
  const int nct = dpad >> 4;

  for (int e = t; e < dpad * LX; e += SLAB_THREADS) {
    const int j = e / LX, c = e - j * LX;
    Vs[e] = (j < dim && c < dim) ? V[size_t(j) * dim + c] : 0.0;
  }
  for (int e = t; e < SLAB_ROWS * LX; e += SLAB_THREADS) Xs[e] = 0.0;   // (the padding columns stay zero: the slabs only write c < dim)

  // this thread's entries of a slab: e = t + 512 q of the 32 * dim contiguous doubles
  const int slab_doubles = SLAB_ROWS * dim;
  int xoff[PT_XREG];
#pragma unroll
  for (int q = 0; q < PT_XREG; ++q) {
    const int e = t + SLAB_THREADS * q;
    const int r = e / dim;
    xoff[q] = e < slab_doubles ? r * LX + (e - r * dim) : -1;
  }
  const size_t total = size_t(M) * dim;
  long long slab0, slab1;
  slab_chunk_range(M, slabs_per_chunk, &slab0, &slab1);
  double xr[PT_XREG];
  auto load_slab = [&](long long s) {
    const size_t base = size_t(s) * slab_doubles;
#pragma unroll
    for (int q = 0; q < PT_XREG; ++q) {
      const size_t g = base + t + SLAB_THREADS * q;
      xr[q] = (xoff[q] >= 0 && g < total) ? X[g] : 0.0;
    }
  };

  const int rt = w & 1, ct0 = w >> 1;
  int gti[3], gtj[3];   // Gram: lower tiles w + 8 q
  d4_t acc[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    lower_tile(w + 8 * q, &gti[q], &gtj[q]);
    if (gti[q] >= nct) gti[q] = -1;
    acc[q] = d4_t{0.0, 0.0, 0.0, 0.0};
  }

  if (slab0 < slab1) load_slab(slab0);
  __syncthreads();
  for (long long s = slab0; s < slab1; ++s) {
#pragma unroll
    for (int q = 0; q < PT_XREG; ++q)
      if (xoff[q] >= 0) Xs[xoff[q]] = xr[q];
    __syncthreads();
    if (s + 1 < slab1) load_slab(s + 1);
    {
      d4_t y[2];
      slab_nt(Xs, LX, Vs, LX, dpad, nct, y);   // Ys = Xs Vs^T
      const long long grow0 = s * SLAB_ROWS + rt * 16 + k;
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const int ct = ct0 + 4 * jj;
        if (ct < nct) {
          const int col = ct * 16 + i;
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            Ys[(rt * 16 + k + 4 * g) * LY + col] = y[jj][g];
            if (S && col < n_s && grow0 + 4 * g < M) S[size_t(grow0 + 4 * g) * n_s + col] = y[jj][g];
          }
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 3; ++q)
      if (gti[q] >= 0) slab_tn_acc(Ys, LY, gti[q] * 16, gtj[q] * 16, acc[q]);
    // (the next iteration writes Xs, last read before the barrier above, and then passes a barrier before Ys is rewritten)
  }
  double* Pb = P + size_t(blockIdx.x) * dpad * dpad;
#pragma unroll
  for (int q = 0; q < 3; ++q)
    if (gti[q] >= 0) slab_tn_store(Pb, dpad, gti[q] * 16, gtj[q] * 16, acc[q]);
}

// ---- G = Y^T Y of a row-major block (TN) ----------------------------------------------------------------------------
// grid (lower 64 x 64 blocks, row chunks) x 256 threads; a wave owns a 32 x 32 quadrant as 2 x 2 MFMA tiles.  The TN
// layout is the MFMA's own: the A operand of lane (i = l & 15, k = l >> 4) is Y[r0 + k][c0 + i] -- 16 consecutive doubles
// of a row.  Slabs of 32 rows x 64 columns per operand in LDS (stride 80: consecutive rows half the banks apart), the next
// slab prefetched in registers.  P[chunk] (dpad x dpad, dpad = dim rounded up to 64): the lower quadrants of the block.
constexpr int ST_ROWS = 32, ST_LD = 80;
__global__ __launch_bounds__(256) void k_syrk_tn(const double* __restrict__ Y, int M, int dim, long long ld, int rows_per_chunk,
                                                 int dpad, double* __restrict__ P) {
  __shared__ double As[ST_ROWS * ST_LD];
  __shared__ double Bs[ST_ROWS * ST_LD];
  int bi, bj;
  lower_tile(int(blockIdx.x), &bi, &bj);
  const bool diag = bi == bj;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wr = w >> 1, wc = w & 1;
  const int i = lane & 15, k = lane >> 4;
  const int col = t & 63, rq = t >> 6;
  const int ca = bi * 64 + col, cb = bj * 64 + col;
  const long long r_begin = (long long)blockIdx.y * rows_per_chunk;
  const long long r_end = min((long long)M, r_begin + rows_per_chunk);
  double va[8], vb[8];
  auto load = [&](long long r0) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const long long r = r0 + rq + 4 * q;
      const bool in = r < r_end;
      va[q] = (in && ca < dim) ? Y[r * ld + ca] : 0.0;
      vb[q] = (in && cb < dim && !diag) ? Y[r * ld + cb] : 0.0;
    }
  };
  Acc acc;
  acc_zero(acc);
  const bool active = !(diag && wr < wc);
  const double* sB = diag ? As : Bs;
  if (r_begin < r_end) load(r_begin);
  for (long long r0 = r_begin; r0 < r_end; r0 += ST_ROWS) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      As[(rq + 4 * q) * ST_LD + col] = va[q];
      if (!diag) Bs[(rq + 4 * q) * ST_LD + col] = vb[q];
    }
    __syncthreads();
    if (r0 + ST_ROWS < r_end) load(r0 + ST_ROWS);
    if (active) {
      const double* pa = As + k * ST_LD + wr * 32 + i;
      const double* pb = sB + k * ST_LD + wc * 32 + i;
#pragma unroll
      for (int r = 0; r < ST_ROWS; r += 4) {
        const double a0 = pa[r * ST_LD], a1 = pa[r * ST_LD + 16];
        const double b0 = pb[r * ST_LD], b1 = pb[r * ST_LD + 16];
        acc.c[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc.c[0][0], 0, 0, 0);
        acc.c[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc.c[0][1], 0, 0, 0);
        acc.c[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc.c[1][0], 0, 0, 0);
        acc.c[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc.c[1][1], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  if (!active) return;
  double* Pb = P + size_t(blockIdx.y) * dpad * dpad;
#pragma unroll
  for (int ii = 0; ii < 2; ++ii)
#pragma unroll
    for (int jj = 0; jj < 2; ++jj)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        Pb[size_t(bi * 64 + wr * 32 + ii * 16 + k + 4 * g) * dpad + bj * 64 + wc * 32 + jj * 16 + i] = acc.c[ii][jj][g];
}

// stat[0] = max over i != j of |g_ij| / (64 eps max(d) max(d_i, d_j)), stat[1] = max(d), stat[2] = entries of G that are
// not finite, stat[3] = 0; stat[4 + i] = d_i = sqrt(g_ii).  One workgroup.
__global__ __launch_bounds__(1024) void k_pca_tall_check(const double* __restrict__ G, int dim, double* __restrict__ stat) {
  __shared__ double red[16];
  __shared__ double bad_s[16];
  __shared__ double dmax_s;
  const int t = threadIdx.x;
  double dm = 0.0;
  for (int j = t; j < dim; j += 1024) {
    const double g = G[size_t(j) * dim + j];
    const double d = g > 0.0 ? sqrt(g) : 0.0;
    stat[4 + j] = d;
    dm = fmax(dm, d);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) dm = fmax(dm, __shfl_xor(dm, o, 64));
  if ((t & 63) == 0) red[t >> 6] = dm;
  __syncthreads();
  if (t == 0) {
    double m = 0.0;
    for (int q = 0; q < 16; ++q) m = fmax(m, red[q]);
    dmax_s = m;
  }
  __syncthreads();
  const double scale = PT_C * PT_EPS * dmax_s;
  double worst = 0.0, bad = 0.0;
  for (int idx = t; idx < dim * dim; idx += 1024) {
    const int r = idx / dim, c = idx - r * dim;
    const double g = fabs(G[idx]);
    if (!(g <= 1.7976931348623157e308)) bad += 1.0;
    else if (r != c) worst = fmax(worst, g / fmax(scale * fmax(stat[4 + r], stat[4 + c]), 1e-300));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    worst = fmax(worst, __shfl_xor(worst, o, 64));
    bad += __shfl_xor(bad, o, 64);   // (a count: exact in any order)
  }
  __syncthreads();
  if ((t & 63) == 0) {
    red[t >> 6] = worst;
    bad_s[t >> 6] = bad;
  }
  __syncthreads();
  if (t == 0) {
    double m = 0.0, b = 0.0;
    for (int q = 0; q < 16; ++q) {
      m = fmax(m, red[q]);
      b += bad_s[q];
    }
    stat[0] = m;
    stat[1] = dmax_s;
    stat[2] = b;
    stat[3] = 0.0;
  }
}

// T = 1.5 I - 0.5 E: one Newton-Schulz step of (V V^T)^(-1/2) for E = V V^T = I + O(dim eps)
__global__ void k_newton_schulz_matrix(const double* __restrict__ E, int n, double* __restrict__ T) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * n) return;
  const int r = idx / n, c = idx - r * n;
  T[idx] = (r == c ? 1.5 : 0.0) - 0.5 * E[idx];
}

// Vn[i, :] = Vc[perm[i], :]: a pure copy, the rows keep their bits
__global__ void k_permute_rows(const double* __restrict__ Vc, const int* __restrict__ perm, int n, double* __restrict__ Vn) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * n) return;
  const int r = idx / n, c = idx - r * n;
  Vn[idx] = Vc[size_t(perm[r]) * n + c];
}

// S[r, i] <- S[r, perm[i]] for every row r, in place (n <= 1024 columns: a row is read whole by its workgroup, then written)
__global__ __launch_bounds__(256) void k_permute_cols(double* __restrict__ S, int M, int n, const int* __restrict__ perm) {
  for (long long r = blockIdx.x; r < M; r += gridDim.x) {
    double* row = S + size_t(r) * n;
    double v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = threadIdx.x + 256 * q;
      v[q] = i < n ? row[perm[i]] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = threadIdx.x + 256 * q;
      if (i < n) row[i] = v[q];
    }
    __syncthreads();
  }
}

struct TallPlan {
  bool fused;
  int dpad, chunks, per_chunk;   // per_chunk: slabs (fused) or rows (unfused) of a chunk
  int nblk;                      // unfused: lower 64 x 64 blocks
};

TallPlan make_plan(const rom_ctx* ctx, int M, int dim) {
  TallPlan p;
  p.fused = dim <= PT_FUSED_MAX;
  if (p.fused) {
    const SlabPlan sp = rom_slab_plan(ctx, M, dim);
    p.dpad = sp.pad;
    p.nblk = 1;
    p.per_chunk = int(sp.per_chunk);
    p.chunks = sp.chunks;
  } else {
    const int n_cu = ctx->n_cu > 0 ? ctx->n_cu : 256;
    const int nslabs = (M + ST_ROWS - 1) / ST_ROWS;
    p.dpad = (dim + 63) / 64 * 64;
    const int nb = p.dpad / 64;
    p.nblk = nb * (nb + 1) / 2;
    int want = std::max(1, (4 * n_cu + p.nblk - 1) / p.nblk);   // four workgroups (40 KB of LDS each) per CU
    want = std::min(want, nslabs);
    const int slabs = (nslabs + want - 1) / want;
    p.per_chunk = slabs * ST_ROWS;
    p.chunks = (nslabs + slabs - 1) / slabs;
  }
  return p;
}

}  // namespace

extern "C" int rom_pca_tall(rom_ctx* ctx, rom_buf* X, int64_t x_row0, int M, int dim, int n, int center, rom_buf* V,
                            int64_t v_row0, rom_buf* S, int64_t s_row0, rom_buf* mean, double* sigma_host, double* info_host) {
  ROM_CHECK(ctx && X && (V || n == 0) && (sigma_host || n == 0), "rom_pca_tall: null argument");
  ROM_CHECK(M >= 1 && dim >= 1 && n >= 0 && x_row0 >= 0 && v_row0 >= 0 && s_row0 >= 0, "rom_pca_tall: bad sizes");
  ROM_CHECK(dim <= SE_MAX, "rom_pca_tall: dim = %d, at most %d columns (a tall block: M >> dim)", dim, SE_MAX);
  ROM_CHECK(n <= dim, "rom_pca_tall: n = %d components of a space of dim = %d", n, dim);
  ROM_CHECK(size_t(x_row0 + M) * size_t(dim) <= X->n, "rom_pca_tall: X holds %zu doubles, rows [%lld, %lld) x %d need more",
            X->n, (long long)x_row0, (long long)(x_row0 + M), dim);
  ROM_CHECK(n == 0 || size_t(v_row0 + n) * size_t(dim) <= V->n, "rom_pca_tall: V too small for %d rows of %d at row %lld", n, dim,
            (long long)v_row0);
  ROM_CHECK(!S || size_t(s_row0 + M) * size_t(n) <= S->n, "rom_pca_tall: S too small for %d rows of %d at row %lld", M, n,
            (long long)s_row0);
  ROM_CHECK(!mean || size_t(dim) <= mean->n, "rom_pca_tall: mean holds %zu doubles, dim = %d", mean ? mean->n : size_t(0), dim);
  // (the rotation product of the unfused form walks the rows in a grid dimension of 64-row tiles, at most 65535 of them)
  ROM_CHECK(dim <= PT_FUSED_MAX || M <= 65535 * 64, "rom_pca_tall: M = %d rows with dim = %d > %d, at most %d rows in that form", M, dim,
            PT_FUSED_MAX, 65535 * 64);
  ROM_HIP(hipSetDevice(ctx->device));
  double* x = X->p + x_row0 * dim;
  double* s_out = (S && n > 0) ? S->p + s_row0 * n : nullptr;
  const size_t dd = size_t(dim) * dim;
  const TallPlan plan = make_plan(ctx, M, dim);
  double executed = 0.0;
  int syncs = 0;
  const unsigned long long helper_syncs0 = ctx->host_syncs;

  // column means (fixed-order partials), subtracted in place
  Tmp mean_tmp, mean_part;   // (the partial sums live to the end of the call: nothing waits for the means)
  if (center || mean) {
    double* d_mean = mean ? mean->p : nullptr;
    if (!d_mean) {
      ROM_TRY(mean_tmp.get(ctx, dim));
      d_mean = mean_tmp;
    }
    if (center) {
      const int cw = dim <= 32 ? 32 : dim <= 64 ? 64 : dim <= 128 ? 128 : 256;
      const int chunks = int(std::min<int64_t>(1024, (int64_t(M) + 63) / 64));
      const int per = (M + chunks - 1) / chunks;
      ROM_TRY(mean_part.get(ctx, size_t(chunks) * dim));
      double* part = mean_part;
      {
        ROM_PROF(ctx, "pca_tall_center", 2.0 * M * dim, 24.0 * M * dim);
        k_colsum_partial<<<chunks, 256, 0, ctx->stream>>>(x, M, dim, per, cw, part);
        kb_partials_colsum<<<(dim + 255) / 256, 256, 0, ctx->stream>>>(part, chunks, dim, double(M), d_mean);
        k_subtract_mean<<<unsigned(std::min<size_t>((size_t(M) * dim + 255) / 256, 8192)), 256, 0, ctx->stream>>>(x, size_t(M) * dim, dim,
                                                                                                             d_mean);
      }
      ROM_HIP(hipGetLastError());
      executed += 2.0 * M * dim;
    } else {
      ROM_HIP(hipMemsetAsync(d_mean, 0, size_t(dim) * sizeof(double), ctx->stream));
    }
  }

  Tmp Va, Vb, G, T, lam, stat, P, Ytmp;
  ROM_TRY(Va.get(ctx, dd));
  ROM_TRY(Vb.get(ctx, dd));
  ROM_TRY(G.get(ctx, dd));
  ROM_TRY(T.get(ctx, dd));
  ROM_TRY(lam.get(ctx, dim));
  ROM_TRY(stat.get(ctx, size_t(dim) + 4));
  ROM_TRY(P.get(ctx, size_t(plan.chunks) * plan.dpad * plan.dpad));
  double* y_buf = nullptr;   // unfused: the rotated block
  if (!plan.fused) {
    if (s_out && n == dim) y_buf = s_out;
    else {
      ROM_TRY(Ytmp.get(ctx, size_t(M) * dim));
      y_buf = Ytmp;
    }
  }
  double *Vc = Va, *Vn = Vb;
  const unsigned gdd = unsigned((dd + 255) / 256);
  ROM_TRY(romb_onehot(ctx, int(dim), Vc));

  size_t fused_lds = 0;
  if (plan.fused) {
    fused_lds = (size_t(plan.dpad + SLAB_ROWS) * slab_ld_nt(plan.dpad) + size_t(SLAB_ROWS) * slab_ld_tn(plan.dpad)) * sizeof(double);
    if (fused_lds > 64 * 1024)
      ROM_TRY(rom_lds_optin(ctx->lds_optin_pca_tall, reinterpret_cast<const void*>(k_pca_tall_fused), 160 * 1024));
  }

  // one pass over the block: G = (Xc Vc^T)^T (Xc Vc^T), the scores into S when `write_s`
  auto pass = [&](bool rotate, bool write_s) -> int {
    if (plan.fused) {
      char nm[48];
      rom_prof_name(nm, sizeof nm, "pca_tall_fused", "_d%d", dim);
      const double fl = 3.0 * M * double(plan.dpad) * plan.dpad;
      ROM_PROF(ctx, nm, fl, 8.0 * M * dim + (write_s ? 8.0 * M * n : 0.0));
      k_pca_tall_fused<<<plan.chunks, SLAB_THREADS, fused_lds, ctx->stream>>>(x, M, dim, plan.dpad, Vc, plan.per_chunk, P,
                                                                            write_s ? s_out : nullptr, n);
      executed += fl;
    } else {
      const double* src = x;
      if (rotate) {
        char nm[48];
        rom_prof_name(nm, sizeof nm, "pca_tall_rotate", "_d%d", dim);
        ROM_TRY(rom_launch_gemm_nt(ctx, M, dim, dim, 1.0, x, dim, Vc, dim, 0.0, y_buf, dim, nm));
        executed += 2.0 * M * double(dim) * dim;
        src = y_buf;
      }
      char nm[48];
      rom_prof_name(nm, sizeof nm, "syrk_tn", "_d%d", dim);
      const double fl = double(M) * plan.dpad * (plan.dpad + 64.0);
      ROM_PROF(ctx, nm, fl, 8.0 * M * dim);
      k_syrk_tn<<<dim3(plan.nblk, plan.chunks), 256, 0, ctx->stream>>>(src, M, dim, dim, plan.per_chunk, plan.dpad, P);
      executed += fl;
    }
    ROM_HIP(hipGetLastError());
    {
      ROM_PROF(ctx, "syrk_tn_reduce", double(plan.chunks) * dd, 8.0 * plan.chunks * dd);
      kb_partials_reduce<<<gdd, 256, 0, ctx->stream>>>(P, plan.chunks, plan.dpad, plan.dpad, dim, 0, G, nullptr, 0, 0);
      k_pca_tall_check<<<1, 1024, 0, ctx->stream>>>(G, dim, stat);
    }
    ROM_HIP(hipGetLastError());
    return ROM_OK;
  };
  // Vc <- Tm Vc, rows re-orthonormalised by one Newton-Schulz step, signs of svd_flip(u_based_decision=False)
  auto rotate_basis = [&](const double* Tm) -> int {
    ROM_TRY(rom_launch_gemm_nn(ctx, dim, dim, dim, 1.0, Tm, dim, Vc, dim, 0.0, Vn, dim));
    std::swap(Vc, Vn);
    ROM_TRY(rom_launch_gram(ctx, dim, dim, Vc, dim, G, dim));
    k_newton_schulz_matrix<<<gdd, 256, 0, ctx->stream>>>(G, dim, T);
    ROM_HIP(hipGetLastError());
    ROM_TRY(rom_launch_gemm_nn(ctx, dim, dim, dim, 1.0, T, dim, Vc, dim, 0.0, Vn, dim));
    std::swap(Vc, Vn);
    executed += 7.0 * double(dim) * dim * dim;
    return rom_launch_rows_sign_flip(ctx, Vc, dim, dim);
  };

  std::vector<double> h(size_t(dim) + 4, 0.0);
  std::vector<int> perm(dim);
  int passes = 0, decomps = 0, stop = 1;
  double worst = 0.0;
  bool scores_current = false;
  for (int p = 1; p <= PT_PASS_CAP; ++p) {
    // (the scores of a pass are final only if that pass turns out to be the last one: every pass from the second on writes
    // them -- the first, with V = I, would write the block itself)
    const bool write_s = s_out != nullptr && p >= 2;
    ROM_TRY(pass(p > 1, write_s));
    passes += 1;
    ROM_TRY(download(ctx, stat, h.data(), size_t(dim) + 4));
    syncs += 1;
    const double dmax = h[1];
    if (h[2] != 0.0) {
      // NaN / Inf in the Gram matrix: entries of the block that are not finite (scikit-learn's PCA raises on those), or
      // entries whose squares leave the range of fp64
      Tmp st;
      ROM_TRY(st.get(ctx, 2));
      unsigned long long* d_st = reinterpret_cast<unsigned long long*>(st.p());
      ROM_HIP(hipMemsetAsync(d_st, 0, 2 * sizeof(unsigned long long), ctx->stream));
      kp_block_amax<<<1024, 256, 0, ctx->stream>>>(x, size_t(M) * dim, d_st);
      ROM_HIP(hipGetLastError());
      unsigned long long h_st[2] = {0, 0};
      ROM_HIP(hipMemcpyAsync(h_st, d_st, sizeof(h_st), hipMemcpyDeviceToHost, ctx->stream));
      ROM_HIP(hipStreamSynchronize(ctx->stream));
      double amax;
      memcpy(&amax, &h_st[0], sizeof(double));
      ROM_CHECK(h_st[1] == 0, "rom_pca_tall: the block contains %llu NaN / Inf entries", h_st[1]);
      ROM_CHECK(false, "rom_pca_tall: entries of magnitude %.3g -- their squares leave the range of fp64; rescale the block", amax);
    }
    // (the small eigenproblem compares squares of entries of the Gram matrix, sigma^4)
    ROM_CHECK(dmax == 0.0 || (dmax < 1e70 && dmax > 1e-70),
              "rom_pca_tall: singular values of magnitude %.3g -- their fourth powers leave the range of fp64; rescale the block", dmax);
    worst = h[0];
    const double* d = h.data() + 4;
    const bool converged = worst <= 1.0;
    // the measured norms in descending order?  Modes at noise level (and the members of a cluster) come out in any order.
    std::iota(perm.begin(), perm.end(), 0);
    std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return d[a] > d[b]; });
    bool sorted = true;
    for (int i = 0; i < n; ++i) sorted = sorted && (perm[i] == i || d[perm[i]] == d[i]);   // (of what is returned)
    scores_current = write_s || s_out == nullptr;
    if (converged && scores_current && (sorted || n == dim)) {
      if (!sorted) {
        // a full request: the rows of V, the columns of the scores and the norms are permuted -- copies, nothing is recomputed
        int* d_perm = reinterpret_cast<int*>(lam.p());   // (dim ints in the dim doubles of `lam`)
        ROM_HIP(hipMemcpyAsync(d_perm, perm.data(), size_t(dim) * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        k_permute_rows<<<gdd, 256, 0, ctx->stream>>>(Vc, d_perm, dim, Vn);
        if (s_out) k_permute_cols<<<unsigned(std::min(M, 8192)), 256, 0, ctx->stream>>>(s_out, M, dim, d_perm);
        ROM_HIP(hipGetLastError());
        ROM_HIP(hipStreamSynchronize(ctx->stream));   // (perm is host memory)
        syncs += 1;
        std::swap(Vc, Vn);
        std::vector<double> ds(dim);
        for (int i = 0; i < dim; ++i) ds[i] = d[perm[i]];
        std::copy(ds.begin(), ds.end(), h.begin() + 4);
      }
      stop = 0;
      break;
    }
    if (p == PT_PASS_CAP) break;
    if (!converged) {
      ROM_TRY(romb_small_eig(ctx, dim, G, dim, lam, T, dim, SE_EIG, 0.0, true, true));
      decomps += 1;
      executed += 30.0 * double(dim) * dim * dim;
      ROM_TRY(rotate_basis(T));
    } else {
      // diagonal already, but the scores are not written yet (a first pass) or the request is a part of the modes and the
      // measured norms are out of order: the rows of V are PERMUTED (`perm` above), nothing else -- they keep their bits,
      // so the next pass measures the same norms again, to the bit, in descending order
      int* d_perm = reinterpret_cast<int*>(lam.p());   // (dim ints in the dim doubles of `lam`, free between decompositions)
      ROM_HIP(hipMemcpyAsync(d_perm, perm.data(), size_t(dim) * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
      k_permute_rows<<<gdd, 256, 0, ctx->stream>>>(Vc, d_perm, dim, Vn);
      ROM_HIP(hipGetLastError());
      ROM_HIP(hipStreamSynchronize(ctx->stream));   // (perm is host memory that the next pass rewrites)
      syncs += 1;
      std::swap(Vc, Vn);
    }
  }

  const double* d = h.data() + 4;
  int resolved = 0;
  for (int i = 0; i < n; ++i) {
    sigma_host[i] = d[i];
    if (d[i] > PT_NOISE_FLOOR * h[1]) resolved += 1;
  }
  if (n > 0) ROM_HIP(hipMemcpyAsync(V->p + v_row0 * dim, Vc, size_t(n) * dim * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  if (!plan.fused && s_out && y_buf != s_out) {
    // the leading n columns of the rotated block (a first pass that was the only one never rotated: the loop above does
    // not end there when scores are asked for)
    ROM_HIP(hipMemcpy2DAsync(s_out, size_t(n) * sizeof(double), y_buf, size_t(dim) * sizeof(double), size_t(n) * sizeof(double), M,
                             hipMemcpyDeviceToDevice, ctx->stream));
  }
  ROM_HIP(hipStreamSynchronize(ctx->stream));   // (the temporaries go back to the allocator)
  syncs += 1;
  if (info_host) {
    info_host[0] = resolved;
    info_host[1] = passes;
    info_host[2] = decomps;
    info_host[3] = executed;
    info_host[4] = worst;
    info_host[5] = stop;
    info_host[6] = double(syncs) + double(ctx->host_syncs - helper_syncs0);
    info_host[7] = 0.0;
  }
  return ROM_OK;
}
