// rom_poly_fit / rom_poly_predict: least-squares polynomial maps between columns of a tall device block -- the third stage of
// the reference's second experiment (src/experiments/NonLinearROM.py:54-70,131-139: PolynomialFeatures(d) + LinearRegression
// from the leading PCA coordinates of a solution to its higher ones).
//
// Feature space: the P = C(m + d, d) products prod_j L_{alpha_j}(t_j), |alpha| <= d, of Legendre polynomials (three-term
// recurrence) of t_j = (x_j - c_j) / h_j, c_j / h_j the mid-range / half-range of input column j over the training rows; the
// exponent rows alpha in the order of PolynomialFeatures(d).powers_.  The same SPACE as scikit-learn's monomials, but a basis
// whose columns are O(1) whatever the scales of the inputs are.
//
// Method (that of rom_pca_tall: Gram matrices always come from the DATA): CholeskyQR in passes over the block,
//   pass k:  Psi = Phi T_k^T by slabs of 32 rows,  G_k = Psi^T Psi,  B_k = Psi^T Y;
//   pass 1:  T_1 = I.  G_1 is column-normalised (D G_1 D, D = diag(g_ii)^-1/2) and the pivoted Cholesky factorisation of that
//            gives the rank-revealing whitening transform T^ (romb_pivchol_whiten: romb_small_eig's mode 3); T_2 = T^ D;
//   pass 2+: G_k = I + delta on the leading rank x rank block.  W = T_k^T G_k^-1 B_k carries the remaining non-orthogonality
//            exactly; the solve costs a factor cond(G_k) <= (1 + |delta|_2) / (1 - |delta|_2) on eps.  Another pass (with T
//            <- whitening of G_k times T) only while P |delta|_max > PL_DELTA_OK; at most PL_PASS_CAP passes.
// Kernels: k_poly_pass (features generated in LDS from an exponent table; NT product with T and TN product Psi^T [Psi | Y] by the
// slab engine of rom_slab.h, one partial per workgroup that kb_partials_reduce adds in chunk order), k_poly_predict (the same
// slab times W^T, written as it is formed, with optional Yref - prediction and per-column sums of squares).  No floating-point
// atomics: the same bits on every call.
#include <cmath>
#include <cstring>

#include "rom_basis_int.h"
#include "rom_block.h"
#include "rom_poly_host.h"   // PL_MAX, PL_MMAX, PL_DMAX, PL_NOFAC and the host arithmetic of the fit
#include "rom_slab.h"

namespace {

constexpr int PL_QG = 96;        // target columns of one launch
constexpr int PL_QMAX = 1024;
constexpr int PL_YREG = SLAB_ROWS * PL_QG / SLAB_THREADS;   // target values of a slab per thread
constexpr int PL_TILES = 8;      // 16 x 16 tiles of Psi^T [Psi | Y] per wave: 21 lower Gram tiles + 36 of B <= 64
constexpr int PL_PASS_CAP = 4;
constexpr double PL_EPS = 1.1102230246251565e-16;   // 2^-53
// A pass is accepted when P |delta|_max <= 1/3: |delta|_2 <= P |delta|_max, so cond(G) <= (1 + 1/3) / (1 - 1/3) = 2 -- the
// solve G^-1 B loses at most one bit against an exactly orthonormal Psi, and a further pass could not gain more than that.
constexpr double PL_DELTA_OK = 1.0 / 3.0;

// device block of a map: c (16) | h (16) | bad count (1, then padding to 40) | factor table (PL_MAX x PL_DMAX bytes) | W (q x P)
constexpr size_t PL_OFF_BAD = 32, PL_OFF_TAB = 40, PL_OFF_W = PL_OFF_TAB + PL_MAX * PL_DMAX / sizeof(double);

// LDS row stride of the Legendre table: odd (a lane per row)
__host__ __device__ inline int pl_ld_leg(int m, int d) { return (m * d) | 1; }

// ---- mid-range and half-range of the input columns (fixed-order partials) -------------------------------------------------
// part[chunk][0 | 1 | 2][j] = min, max, number of non-finite entries of column j over the rows of the chunk; 256 threads =
// 16 row lanes x 16 columns
__global__ __launch_bounds__(256) void k_poly_minmax_partial(const double* __restrict__ X, long long ldx, int m, long long M,
                                                             long long rows_per_chunk, double* __restrict__ part) {
  __shared__ double smin[256], smax[256], sbad[256];
  const int t = threadIdx.x, j = t & 15, ry = t >> 4;
  const long long r_begin = (long long)blockIdx.x * rows_per_chunk;
  const long long r_end = min(M, r_begin + rows_per_chunk);
  double mn = 1.7976931348623157e308, mx = -1.7976931348623157e308, bad = 0.0;
  if (j < m)
    for (long long r = r_begin + ry; r < r_end; r += 16) {
      const double v = X[r * ldx + j];
      if (fabs(v) <= 1.7976931348623157e308) {
        mn = fmin(mn, v);
        mx = fmax(mx, v);
      } else {
        bad += 1.0;
      }
    }
  smin[t] = mn;
  smax[t] = mx;
  sbad[t] = bad;
  __syncthreads();
  if (ry == 0) {
    for (int q = 1; q < 16; ++q) {
      mn = fmin(mn, smin[q * 16 + j]);
      mx = fmax(mx, smax[q * 16 + j]);
      bad += sbad[q * 16 + j];   // (a count: exact in any order)
    }
    double* p = part + size_t(blockIdx.x) * 48;
    p[j] = mn;
    p[16 + j] = mx;
    p[32 + j] = bad;
  }
}

// ch[j] = c_j, ch[16 + j] = h_j, ch[32] = non-finite entries of all columns
__global__ __launch_bounds__(64) void k_poly_minmax_finish(const double* __restrict__ part, int chunks, int m, double* __restrict__ ch) {
  __shared__ double sbad[16];
  const int j = threadIdx.x;
  if (j < 16) {
    double mn = 1.7976931348623157e308, mx = -1.7976931348623157e308, bad = 0.0;
    for (int q = 0; q < chunks; ++q) {
      mn = fmin(mn, part[size_t(q) * 48 + j]);
      mx = fmax(mx, part[size_t(q) * 48 + 16 + j]);
      bad += part[size_t(q) * 48 + 32 + j];
    }
    const bool some = j < m && mn <= mx;
    ch[j] = some ? 0.5 * mn + 0.5 * mx : 0.0;
    ch[16 + j] = some ? 0.5 * mx - 0.5 * mn : 0.0;
    sbad[j] = j < m ? bad : 0.0;
  }
  __syncthreads();
  if (j == 0) {
    double b = 0.0;
    for (int q = 0; q < 16; ++q) b += sbad[q];
    ch[PL_OFF_BAD] = b;
  }
}

// ---- the feature slab ---------------------------------------------------------------------------------------------------
// Leg[r][j d + k - 1] = L_k(t_rj), k = 1 .. d, by thread (r = t >> 4, j = t & 15): (k + 1) L_{k+1} = (2k + 1) t L_k - k L_{k-1}.
// A constant column (h = 0) has t = 0.
__device__ inline void pl_legendre_rows(double* __restrict__ Leg, int LL, int m, int d, double x, double c, double h) {
  const int t = threadIdx.x, j = t & 15, r = t >> 4;
  if (j >= m) return;
  const double tt = h > 0.0 ? (x - c) / h : 0.0;
  double* out = Leg + r * LL + j * d;
  double p0 = 1.0, p1 = tt;
  out[0] = p1;
  for (int k = 1; k < d; ++k) {
    const double p2 = (double(2 * k + 1) * tt * p1 - double(k) * p0) / double(k + 1);
    out[k] = p2;
    p0 = p1;
    p1 = p2;
  }
}

// dst[r][p] = prod over the factors of term p of Leg[r][factor], p < P (zero for the rows at and beyond `rows_valid`): thread
// -> row t & 31, terms (t >> 5) + 16 u.  tab: PL_DMAX factor indices (j d + alpha_j - 1, PL_NOFAC = none) per term, in LDS.
__device__ inline void pl_features(double* __restrict__ dst, int ld, const double* __restrict__ Leg, int LL,
                                   const unsigned char* __restrict__ tab, int P, int d, long long rows_valid) {
  const int t = threadIdx.x, r = t & 31;
  const double* lr = Leg + r * LL;
  const bool valid = r < rows_valid;
  for (int p = t >> 5; p < P; p += 16) {
    const unsigned char* f = tab + p * PL_DMAX;
    double v = 1.0;
    for (int q = 0; q < d; ++q) {
      const int fi = f[q];
      if (fi == PL_NOFAC) break;
      v *= lr[fi];
    }
    dst[r * ld + p] = valid ? v : 0.0;
  }
}

// ---- one pass of the fit --------------------------------------------------------------------------------------------------
// Workgroup b owns slabs_per_chunk slabs of 32 rows.  Per slab: the Legendre values of the m inputs (prefetched in registers
// under the previous slab's MFMAs, as the targets), the 32 x P feature slab, Psi = Phi T^T (NT product; T == NULL: Psi = Phi,
// the features go straight to the TN slab), acc += Psi^T [Psi | Y] (TN product: the lower Gram tiles when `gram`, and the
// ppad x qpad tiles of B; at most PL_TILES per wave).  Part[b] (ppad x (ppad + qpad)) receives the partial.
__global__ __launch_bounds__(SLAB_THREADS) void k_poly_pass(const double* __restrict__ X, long long ldx, int m, int d,
                                                           const double* __restrict__ ch, const unsigned char* __restrict__ tab_g,
                                                           int P, int ppad, const double* __restrict__ T,
                                                           const double* __restrict__ Y, long long ldy, int qg, int qpad, long long M,
                                                           long long slabs_per_chunk, int gram, double* __restrict__ Part) {
  extern __shared__ double pl_lds[];
  __shared__ unsigned char tab[PL_MAX * PL_DMAX];
  const int LX = slab_ld_nt(ppad), LY = slab_ld_tn(ppad + qpad), LL = pl_ld_leg(m, d);
  double* Ts = pl_lds;                 // ppad x LX
  double* Fs = Ts + ppad * LX;         // 32 x LX: the features (NT operand)
  double* Ys = Fs + SLAB_ROWS * LX;    // 32 x LY: [Psi | Y] (TN operand)
  double* Leg = Ys + SLAB_ROWS * LY;   // 32 x LL
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int i = lane & 15, k = lane >> 4;
  const int nct = ppad >> 4, nqt = qpad >> 4;
  const bool identity = T == nullptr;

  for (int e = t; e < PL_MAX * PL_DMAX; e += SLAB_THREADS) tab[e] = tab_g[e];
  for (int e = t; e < ppad * LX; e += SLAB_THREADS) {
    const int j = e / LX, c = e - j * LX;
    Ts[e] = (!identity && j < P && c < P) ? T[size_t(j) * P + c] : 0.0;
  }
  for (int e = t; e < SLAB_ROWS * LX; e += SLAB_THREADS) Fs[e] = 0.0;   // (the padding columns stay zero: the slabs write p < P)
  for (int e = t; e < SLAB_ROWS * LY; e += SLAB_THREADS) Ys[e] = 0.0;

  // this thread's input value of a slab: row t >> 4, column t & 15; its targets: e = t + 512 u of the 32 x qg values
  const int xj = t & 15, xrow = t >> 4;
  const double xc = xj < m ? ch[xj] : 0.0, xh = xj < m ? ch[16 + xj] : 0.0;
  int yrow[PL_YREG], ycol[PL_YREG];
#pragma unroll
  for (int u = 0; u < PL_YREG; ++u) {
    const int e = t + SLAB_THREADS * u;
    const int r = e / qg;
    yrow[u] = e < SLAB_ROWS * qg ? r : -1;
    ycol[u] = e - r * qg;
  }
  long long slab0, slab1;
  slab_chunk_range(M, slabs_per_chunk, &slab0, &slab1);
  double xr = 0.0, yr[PL_YREG];
  auto load_slab = [&](long long s) {
    const long long row0 = s * SLAB_ROWS;
    xr = (xj < m && row0 + xrow < M) ? X[(row0 + xrow) * ldx + xj] : 0.0;
#pragma unroll
    for (int u = 0; u < PL_YREG; ++u)
      yr[u] = (yrow[u] >= 0 && row0 + yrow[u] < M) ? Y[(row0 + yrow[u]) * ldy + ycol[u]] : 0.0;
  };

  const int rt = w & 1, ct0 = w >> 1;
  // TN tiles of this wave: w + 8 u of the list [lower Gram tiles | B tiles], as column offsets (ca, cb) into the TN slab
  const int ngram = gram ? nct * (nct + 1) / 2 : 0, ntile = ngram + nct * nqt;
  int tca[PL_TILES], tcb[PL_TILES];
  d4_t acc[PL_TILES];
#pragma unroll
  for (int u = 0; u < PL_TILES; ++u) {
    const int tt = w + 8 * u;
    tca[u] = -1;
    tcb[u] = 0;
    if (tt < ngram) {
      int ti, tj;
      lower_tile(tt, &ti, &tj);
      tca[u] = ti * 16;
      tcb[u] = tj * 16;
    } else if (tt < ntile) {
      const int tb = tt - ngram, bi = tb / nqt;
      tca[u] = bi * 16;
      tcb[u] = ppad + (tb - bi * nqt) * 16;
    }
    acc[u] = d4_t{0.0, 0.0, 0.0, 0.0};
  }

  if (slab0 < slab1) load_slab(slab0);
  __syncthreads();
  for (long long s = slab0; s < slab1; ++s) {
    pl_legendre_rows(Leg, LL, m, d, xr, xc, xh);
    __syncthreads();   // (every wave is past the TN product of the previous slab: the TN slab is free)
    pl_features(identity ? Ys : Fs, identity ? LY : LX, Leg, LL, tab, P, d, M - s * SLAB_ROWS);
#pragma unroll
    for (int u = 0; u < PL_YREG; ++u)
      if (yrow[u] >= 0) Ys[yrow[u] * LY + ppad + ycol[u]] = yr[u];
    if (s + 1 < slab1) load_slab(s + 1);
    __syncthreads();
    if (!identity) {
      d4_t y[2];
      slab_nt(Fs, LX, Ts, LX, ppad, nct, y);   // Psi = Phi T^T
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const int ct = ct0 + 4 * jj;
        if (ct < nct) {
#pragma unroll
          for (int g = 0; g < 4; ++g) Ys[(rt * 16 + k + 4 * g) * LY + ct * 16 + i] = y[jj][g];
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < PL_TILES; ++u)
      if (tca[u] >= 0) slab_tn_acc(Ys, LY, tca[u], tcb[u], acc[u]);   // acc += Psi^T [Psi | Y]
  }
  const int ldp = ppad + qpad;
  double* Pb = Part + size_t(blockIdx.x) * ppad * ldp;
#pragma unroll
  for (int u = 0; u < PL_TILES; ++u)
    if (tca[u] >= 0) slab_tn_store(Pb, ldp, tca[u], tcb[u], acc[u]);
}

// Gh = D G D with D = diag(g_ii)^-1/2 (0 for a column that is zero), Dv = the diagonal of D
__global__ void k_poly_normalise(const double* __restrict__ G, int P, double* __restrict__ Gh, double* __restrict__ Dv) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= P * P) return;
  const int r = idx / P, c = idx - r * P;
  const double gr = G[size_t(r) * P + r], gc = G[size_t(c) * P + c];
  const double dr = gr > 0.0 ? 1.0 / sqrt(gr) : 0.0, dc = gc > 0.0 ? 1.0 / sqrt(gc) : 0.0;
  Gh[idx] = r == c ? (gr > 0.0 ? 1.0 : 0.0) : G[idx] * dr * dc;
  if (c == 0) Dv[r] = dr;
}

// ---- prediction ---------------------------------------------------------------------------------------------------------
// grid (row chunks, target groups of <= 96 columns).  Per slab: the feature slab as in k_poly_pass, times W_g^T (NT), written
// as it is formed: OUT <- the prediction, or Yref - prediction.  SS[chunk][c] (with SS != NULL) = the chunk's sum of squares
// of what OUT receives in column c: per lane over its rows and slabs, then over the four k lanes and the two row tiles, always
// in the same order.
__global__ __launch_bounds__(SLAB_THREADS) void k_poly_predict(const double* __restrict__ X, long long ldx, int m, int d,
                                                              const double* __restrict__ ch, const unsigned char* __restrict__ tab_g,
                                                              int P, int ppad, const double* __restrict__ W, int q, long long M,
                                                              long long slabs_per_chunk, double* __restrict__ OUT, long long ldo,
                                                              const double* __restrict__ Yref, long long ldr, double* __restrict__ SS) {
  extern __shared__ double pl_lds[];
  __shared__ unsigned char tab[PL_MAX * PL_DMAX];
  __shared__ double red[2 * PL_QG];
  const int c0 = blockIdx.y * PL_QG, qg = min(PL_QG, q - c0), qpad = (qg + 15) / 16 * 16;
  const int LX = slab_ld_nt(ppad), LL = pl_ld_leg(m, d);
  double* Ws = pl_lds;                 // qpad x LX
  double* Fs = Ws + qpad * LX;         // 32 x LX
  double* Leg = Fs + SLAB_ROWS * LX;   // 32 x LL
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int i = lane & 15, k = lane >> 4;
  const int nqt = qpad >> 4;

  for (int e = t; e < PL_MAX * PL_DMAX; e += SLAB_THREADS) tab[e] = tab_g[e];
  for (int e = t; e < qpad * LX; e += SLAB_THREADS) {
    const int j = e / LX, c = e - j * LX;
    Ws[e] = (j < qg && c < P) ? W[size_t(c0 + j) * P + c] : 0.0;
  }
  for (int e = t; e < SLAB_ROWS * LX; e += SLAB_THREADS) Fs[e] = 0.0;
  const int xj = t & 15, xrow = t >> 4;
  const double xc = xj < m ? ch[xj] : 0.0, xh = xj < m ? ch[16 + xj] : 0.0;
  long long slab0, slab1;
  slab_chunk_range(M, slabs_per_chunk, &slab0, &slab1);
  auto load_x = [&](long long s) {
    const long long row = s * SLAB_ROWS + xrow;
    return (xj < m && row < M) ? X[row * ldx + xj] : 0.0;
  };
  const int rt = w & 1, ct0 = w >> 1;
  double ss[2] = {0.0, 0.0};
  double xr = slab0 < slab1 ? load_x(slab0) : 0.0;
  __syncthreads();
  for (long long s = slab0; s < slab1; ++s) {
    pl_legendre_rows(Leg, LL, m, d, xr, xc, xh);
    __syncthreads();
    pl_features(Fs, LX, Leg, LL, tab, P, d, M - s * SLAB_ROWS);
    if (s + 1 < slab1) xr = load_x(s + 1);
    __syncthreads();
    d4_t y[2];
    slab_nt(Fs, LX, Ws, LX, ppad, nqt, y);   // the slab times W_g^T
    const long long grow0 = s * SLAB_ROWS + rt * 16 + k;
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int col = (ct0 + 4 * jj) * 16 + i;
      if (col < qg) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const long long row = grow0 + 4 * g;
          if (row < M) {
            const double v = Yref ? Yref[row * ldr + c0 + col] - y[jj][g] : y[jj][g];
            if (OUT) OUT[row * ldo + c0 + col] = v;
            ss[jj] += v * v;
          }
        }
      }
    }
    // (the next slab writes Leg, last read before the barrier above, and passes a barrier before it writes Fs)
  }
  if (!SS) return;
#pragma unroll
  for (int jj = 0; jj < 2; ++jj) {
    ss[jj] += __shfl_xor(ss[jj], 16, 64);
    ss[jj] += __shfl_xor(ss[jj], 32, 64);
    const int col = (ct0 + 4 * jj) * 16 + i;
    if (k == 0 && col < PL_QG) red[rt * PL_QG + col] = ss[jj];
  }
  __syncthreads();
  if (t < qg) SS[size_t(blockIdx.x) * q + c0 + t] = red[t] + red[PL_QG + t];
}

// ---- host side ------------------------------------------------------------------------------------------------------------
// (the terms, the factor table and the dense steps between the passes: rom_poly_host.h)
size_t pass_lds(int ppad, int qpad, int m, int d) {
  return (size_t(ppad + SLAB_ROWS) * slab_ld_nt(ppad) + size_t(SLAB_ROWS) * slab_ld_tn(ppad + qpad) + size_t(SLAB_ROWS) * pl_ld_leg(m, d)) *
         sizeof(double);
}
size_t predict_lds(int ppad, int qpad, int m, int d) {
  return (size_t(qpad + SLAB_ROWS) * slab_ld_nt(ppad) + size_t(SLAB_ROWS) * pl_ld_leg(m, d)) * sizeof(double);
}

}  // namespace

struct rom_poly {
  rom_ctx* ctx = nullptr;
  int m = 0, d = 0, P = 0, q = 0, rank = 0, passes = 0;
  int64_t M_train = 0;
  unsigned long long syncs = 0;
  rom_buf* dev = nullptr;   // c | h | bad | factor table | W
  std::vector<double> dropped;
};

extern "C" int rom_poly_terms(int m, int d, int* P_out, int* powers_out) {
  ROM_CHECK(m >= 1 && m <= PL_MMAX, "rom_poly_terms: m = %d inputs, between 1 and %d", m, PL_MMAX);
  ROM_CHECK(d >= 1 && d <= PL_DMAX, "rom_poly_terms: degree d = %d, between 1 and %d", d, PL_DMAX);
  const long long P = poly_count(m, d);
  ROM_CHECK(P <= PL_MAX, "rom_poly_terms: P = C(%d + %d, %d) = %lld terms, at most %d", m, d, d, P, PL_MAX);
  if (P_out) *P_out = int(P);
  if (powers_out) {
    std::vector<int> powers;
    poly_powers(m, d, powers);
    std::copy(powers.begin(), powers.end(), powers_out);
  }
  return ROM_OK;
}

extern "C" int rom_poly_destroy(rom_poly* h) {
  if (!h) return ROM_OK;
  if (h->dev) rom_buf_free(h->dev);
  delete h;
  return ROM_OK;
}

namespace {

// One fit between its steps: setup, first_pass, pass_loop, finish.  h is the handle under construction (m, d, P, q, M_train set).
struct PolyFit {
  rom_ctx* ctx;
  rom_poly* h;
  const double *x, *y;   // the blocks at their offsets
  int64_t ldx, ldy;
  double rc;
  int m, d, P, q;
  int64_t M;
  SlabPlan plan;
  size_t pp;             // P^2
  unsigned long long helper_syncs0;
  std::vector<unsigned char> tab;
  Tmp mm_part, Gh, lam, Td, That, GB, Part;   // lam: lam | D; GB: G | B, one download per pass
  std::vector<double> hT, hGB, hsmall, hW, tnew;
  std::vector<long double> L, z;
  int syncs = 0, passes = 0, rank = 0, stop = 0;
  double executed = 0.0, delta = 0.0, piv_ratio = 0.0;
  bool solved = false;

  PolyFit(rom_poly* h_, const double* x_, int64_t ldx_, const double* y_, int64_t ldy_, double rc_)
      : ctx(h_->ctx), h(h_), x(x_), y(y_), ldx(ldx_), ldy(ldy_), rc(rc_), m(h_->m), d(h_->d), P(h_->P), q(h_->q), M(h_->M_train),
        plan(rom_slab_plan(ctx, M, P)), pp(size_t(P) * P), helper_syncs0(ctx->host_syncs) {}

  double* dev() const { return h->dev->p; }
  double* d_G() const { return GB; }
  double* d_B() const { return GB.p() + pp; }

  // the handle's device block with the factor table, c and h of the input columns, the scratch of the passes
  int setup() {
    ROM_TRY(rom_buf_alloc(ctx, PL_OFF_W + size_t(q) * P, &h->dev));
    std::vector<int> powers;
    poly_powers(m, d, powers);
    tab = poly_factor_table(powers, m, d, P);
    ROM_HIP(hipMemcpyAsync(dev() + PL_OFF_TAB, tab.data(), tab.size(), hipMemcpyHostToDevice, ctx->stream));
    {
      const int chunks = int(std::min<int64_t>(1024, (M + 63) / 64));
      const long long per = (M + chunks - 1) / chunks;
      ROM_TRY(mm_part.get(ctx, size_t(chunks) * 48));
      ROM_PROF(ctx, "poly_minmax", 2.0 * M * m, 8.0 * M * m);
      k_poly_minmax_partial<<<chunks, 256, 0, ctx->stream>>>(x, ldx, m, M, per, mm_part);
      k_poly_minmax_finish<<<1, 64, 0, ctx->stream>>>(mm_part, chunks, m, dev());
      ROM_HIP(hipGetLastError());
    }
    ROM_TRY(GB.get(ctx, pp + size_t(P) * q));
    ROM_TRY(Gh.get(ctx, pp));
    ROM_TRY(lam.get(ctx, 2 * size_t(P)));
    ROM_TRY(Td.get(ctx, pp));
    ROM_TRY(That.get(ctx, pp));
    ROM_TRY(Part.get(ctx, size_t(plan.chunks) * plan.pad * (plan.pad + PL_QG)));
    if (pass_lds(plan.pad, PL_QG, m, d) > 64 * 1024)
      ROM_TRY(rom_lds_optin(ctx->lds_optin_poly_pass, reinterpret_cast<const void*>(k_poly_pass), 159 * 1024));
    hT.assign(pp, 0.0);
    hGB.resize(pp + size_t(P) * q);
    hsmall.resize(2 * size_t(P) + pp);
    hW.assign(size_t(q) * P, 0.0);
    tnew.resize(pp);
    z.resize(P);
    return ROM_OK;
  }

  // one pass: every target group through the kernel (the Gram tiles with the first), G and B reduced in chunk order
  int pass(const double* T) {
    const int ppad = plan.pad, ngroups = (q + PL_QG - 1) / PL_QG;
    const unsigned char* d_tab = reinterpret_cast<const unsigned char*>(dev() + PL_OFF_TAB);
    for (int g = 0; g < ngroups; ++g) {
      const int c0 = g * PL_QG, qg = std::min(PL_QG, q - c0), qpad = (qg + 15) / 16 * 16;
      const int ntile = (g == 0 ? (ppad / 16) * (ppad / 16 + 1) / 2 : 0) + (ppad / 16) * (qpad / 16);
      const double fl = double(M) * ((T ? 2.0 * ppad * ppad : 0.0) + 512.0 * ntile);
      {
        char nm[48];
        rom_prof_name(nm, sizeof nm, "poly_pass", "_P%d_q%d", P, qg);
        ROM_PROF(ctx, nm, fl, 8.0 * M * (m + qg));
        k_poly_pass<<<plan.chunks, SLAB_THREADS, pass_lds(ppad, qpad, m, d), ctx->stream>>>(x, ldx, m, d, dev(), d_tab, P, ppad, T, y + c0, ldy,
                                                                                       qg, qpad, M, plan.per_chunk, g == 0, Part);
      }
      ROM_HIP(hipGetLastError());
      executed += fl;
      {
        ROM_PROF(ctx, "poly_reduce", double(plan.chunks) * (pp + P * qg), 8.0 * plan.chunks * (pp + P * qg));
        kb_partials_reduce<<<blocks_for((g == 0 ? pp : 0) + size_t(P) * qg), 256, 0, ctx->stream>>>(Part, plan.chunks, ppad, ppad + qpad, P,
                                                                                                    qg, g == 0 ? d_G() : nullptr, d_B(), q, c0);
      }
      ROM_HIP(hipGetLastError());
    }
    return ROM_OK;
  }

  // pass 1: T = I, the column-normalised Gram matrix and its rank-revealing whitening transform
  int first_pass() {
    ROM_TRY(pass(nullptr));
    passes = 1;
    k_poly_normalise<<<blocks_for(pp), 256, 0, ctx->stream>>>(d_G(), P, Gh, lam.p() + P);
    ROM_HIP(hipGetLastError());
    ROM_TRY(romb_pivchol_whiten(ctx, P, Gh, P, lam, That, P, rc * rc));
    executed += double(P) * P * P;
    double bad = 0.0;
    ROM_HIP(hipMemcpyAsync(&bad, dev() + PL_OFF_BAD, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ROM_HIP(hipMemcpyAsync(hsmall.data(), lam.p(), 2 * size_t(P) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ROM_TRY(download(ctx, That, hsmall.data() + 2 * P, pp));
    syncs += 1;
    ROM_CHECK(bad == 0.0, "rom_poly_fit: the inputs contain %.0f NaN / Inf entries", bad);
    const double* hl = hsmall.data();
    rank = poly_first_transform(P, hl, hl + P, hl + 2 * P, hT.data(), &piv_ratio, h->dropped.data());
    ROM_CHECK(rank >= 1, "rom_poly_fit: no term of the feature space has a finite positive norm (NaN / Inf in the features?)");
    return ROM_OK;
  }

  // pass p >= 2 with the current T: G (I + delta on the leading rank x rank block) and B on the host, |delta|_max
  int gram_of_pass(int p) {
    ROM_HIP(hipMemcpyAsync(Td, hT.data(), pp * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ROM_TRY(pass(Td));
    passes = p;
    ROM_TRY(download(ctx, GB, hGB.data(), hGB.size()));
    syncs += 1;
    bool finite = true;
    for (double v : hGB) finite = finite && std::fabs(v) <= 1.7976931348623157e308;
    ROM_CHECK(finite, "rom_poly_fit: the targets contain NaN / Inf entries (or products with them leave the range of fp64)");
    delta = 0.0;
    for (int i = 0; i < rank; ++i)
      for (int c = 0; c < rank; ++c) delta = std::max(delta, std::fabs(hGB[size_t(i) * P + c] - (i == c ? 1.0 : 0.0)));
    return ROM_OK;
  }

  // T <- (whitening transform of G_p) T; a pivot at the noise level of G_p = I + delta lowers the rank
  int rewhiten(int p) {
    ROM_TRY(romb_pivchol_whiten(ctx, P, d_G(), P, lam, That, P, double(P) * PL_EPS));
    executed += double(P) * P * P;
    ROM_HIP(hipMemcpyAsync(hsmall.data(), lam.p(), size_t(P) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ROM_TRY(download(ctx, That, hsmall.data() + 2 * P, pp));
    syncs += 1;
    const double* hl = hsmall.data();
    int r2 = 0;
    for (int i = 0; i < P; ++i) r2 += hl[i] > 0.0 ? 1 : 0;
    ROM_CHECK(r2 >= 1, "rom_poly_fit: the Gram matrix of pass %d has no positive pivot", p);
    poly_update_t(P, rank, r2, hl + 2 * P, hT.data(), tnew.data());
    hT.swap(tnew);
    rank = r2;
    return ROM_OK;
  }

  // passes 2 .. PL_PASS_CAP: a pass is accepted and solved (W = T^T G^-1 B), or T is re-whitened for another
  int pass_loop() {
    for (int p = 2; p <= PL_PASS_CAP; ++p) {
      ROM_TRY(gram_of_pass(p));
      const bool pd = host_cholesky(L, hGB.data(), P, rank);
      const bool good = pd && double(P) * delta <= PL_DELTA_OK;
      if (good || (pd && p == PL_PASS_CAP)) {
        poly_solve_w(P, q, rank, L, hGB.data() + pp, hT.data(), z.data(), hW.data());
        executed += 2.0 * q * (double(rank) * rank + double(rank) * P) + double(rank) * rank * rank / 3.0;
        solved = true;
        stop = good ? (rank < P ? 1 : 0) : 2;
        break;
      }
      ROM_CHECK(p < PL_PASS_CAP, "rom_poly_fit: the Gram matrix of pass %d is not positive definite (|delta|_max = %.3g): pass budget reached",
                p, delta);
      ROM_TRY(rewhiten(p));
    }
    ROM_CHECK(solved, "rom_poly_fit: no pass was accepted");
    return ROM_OK;
  }

  // W to the handle, the handle's figures and info_host
  int finish(double* info_host) {
    ROM_HIP(hipMemcpyAsync(dev() + PL_OFF_W, hW.data(), hW.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ROM_HIP(hipStreamSynchronize(ctx->stream));   // (hW is host memory; the temporaries go back to the allocator)
    syncs += 1;
    h->rank = rank;
    h->passes = passes;
    h->syncs = (unsigned long long)syncs + (ctx->host_syncs - helper_syncs0);
    if (info_host) {
      info_host[0] = P;
      info_host[1] = rank;
      info_host[2] = passes;
      info_host[3] = delta;
      info_host[4] = piv_ratio;
      info_host[5] = executed;
      info_host[6] = double(h->syncs);
      info_host[7] = stop;
    }
    return ROM_OK;
  }
};

}  // namespace

extern "C" int rom_poly_fit(rom_ctx* ctx, rom_buf* X, size_t x_off, int64_t ldx, int m, rom_buf* Y, size_t y_off, int64_t ldy, int q,
                            int64_t M, int d, double rcond, rom_poly** out, double* info_host) {
  const char* who = "rom_poly_fit";
  ROM_CHECK(ctx && X && Y && out, "rom_poly_fit: null argument (context, X, Y or the handle's address)");
  ROM_CHECK(m >= 1 && m <= PL_MMAX, "rom_poly_fit: m = %d inputs, between 1 and %d", m, PL_MMAX);
  ROM_CHECK(d >= 1 && d <= PL_DMAX, "rom_poly_fit: degree d = %d, between 1 and %d", d, PL_DMAX);
  const long long Pl = poly_count(m, d);
  ROM_CHECK(Pl <= PL_MAX, "rom_poly_fit: P = C(%d + %d, %d) = %lld terms, at most %d", m, d, d, Pl, PL_MAX);
  ROM_CHECK(q >= 1 && q <= PL_QMAX, "rom_poly_fit: q = %d target columns, between 1 and %d", q, PL_QMAX);
  ROM_TRY(rom_check_rows(who, M));
  ROM_TRY(rom_check_block(who, {"X", "ldx", "m"}, X->n, x_off, ldx, m, M));
  ROM_TRY(rom_check_block(who, {"Y", "ldy", "q"}, Y->n, y_off, ldy, q, M));
  ROM_HIP(hipSetDevice(ctx->device));
  const int P = int(Pl);
  // A Cholesky factorisation of a Gram matrix sees the SQUARE of the condition number: a squared pivot of the column-
  // normalised G_1 at or below about P eps of the largest is rounding noise of the P-term sums behind it, so the default
  // drops a term there: rcond^2 = P eps, rcond = sqrt(P eps) (1e-7 at P = 96).
  const double rc = rcond > 0.0 ? rcond : std::sqrt(double(P) * PL_EPS);

  rom_poly* h = new rom_poly;
  HandleGuard<rom_poly, rom_poly_destroy> guard{h};
  h->ctx = ctx, h->m = m, h->d = d, h->P = P, h->q = q, h->M_train = M;
  h->dropped.assign(P, 0.0);
  PolyFit fit(h, X->p + x_off, ldx, Y->p + y_off, ldy, rc);
  ROM_TRY(fit.setup());
  ROM_TRY(fit.first_pass());
  ROM_TRY(fit.pass_loop());
  ROM_TRY(fit.finish(info_host));
  *out = guard.release();
  return ROM_OK;
}

extern "C" int rom_poly_predict(rom_poly* h, rom_buf* X, size_t x_off, int64_t ldx, int64_t M, rom_buf* OUT, size_t o_off, int64_t ldo,
                                rom_buf* Yref, size_t r_off, int64_t ldr, double* sumsq_host) {
  ROM_CHECK(h && X, "rom_poly_predict: null argument (handle or X)");
  ROM_CHECK(OUT || sumsq_host, "rom_poly_predict: OUT == NULL requires sumsq_host");
  rom_ctx* ctx = h->ctx;
  const int m = h->m, d = h->d, P = h->P, q = h->q;
  ROM_TRY(rom_check_predict_blocks("rom_poly_predict", M, X, x_off, ldx, m, q, OUT, o_off, ldo, Yref, r_off, ldr));
  ROM_HIP(hipSetDevice(ctx->device));
  const SlabPlan plan = rom_slab_plan(ctx, M, P);
  const int ppad = plan.pad, ngroups = (q + PL_QG - 1) / PL_QG;
  const int qpad_max = (std::min(q, PL_QG) + 15) / 16 * 16;
  const size_t lds = predict_lds(ppad, qpad_max, m, d);
  if (lds > 64 * 1024) ROM_TRY(rom_lds_optin(ctx->lds_optin_poly_predict, reinterpret_cast<const void*>(k_poly_predict), 112 * 1024));
  SumsqTail tail;
  if (sumsq_host) ROM_TRY(tail.get(ctx, plan.chunks, q));
  const double* dev = h->dev->p;
  {
    char nm[48];
    rom_prof_name(nm, sizeof nm, "poly_predict", "_P%d_q%d", P, q);
    ROM_PROF(ctx, nm, 2.0 * M * ppad * double(ngroups > 1 ? ngroups * PL_QG : qpad_max), 8.0 * M * (m + q * (Yref ? 2.0 : 1.0)));
    k_poly_predict<<<dim3(plan.chunks, ngroups), SLAB_THREADS, lds, ctx->stream>>>(
        X->p + x_off, ldx, m, d, dev, reinterpret_cast<const unsigned char*>(dev + PL_OFF_TAB), P, ppad, dev + PL_OFF_W, q, M, plan.per_chunk,
        OUT ? OUT->p + o_off : nullptr, ldo, Yref ? Yref->p + r_off : nullptr, ldr, tail.partials());
  }
  ROM_HIP(hipGetLastError());
  ROM_TRY(tail.finish(ctx, plan.chunks, q, sumsq_host));
  h->syncs += 1;
  return ROM_OK;
}

extern "C" int rom_poly_query(rom_poly* h, int64_t* out8) {
  ROM_CHECK(h && out8, "rom_poly_query: null argument");
  out8[0] = h->m;
  out8[1] = h->d;
  out8[2] = h->P;
  out8[3] = h->q;
  out8[4] = h->rank;
  out8[5] = h->M_train;
  out8[6] = h->passes;
  out8[7] = int64_t(h->syncs);
  return ROM_OK;
}

extern "C" int rom_poly_download(rom_poly* h, int what, double* host, size_t count) {
  ROM_CHECK(h && host, "rom_poly_download: null argument");
  ROM_CHECK(what >= 0 && what <= 3, "rom_poly_download: what = %d, one of 0 (c), 1 (h), 2 (W), 3 (dropped flags)", what);
  const size_t need = what <= 1 ? size_t(h->m) : what == 2 ? size_t(h->q) * h->P : size_t(h->P);
  ROM_CHECK(count == need, "rom_poly_download: part %d holds %zu doubles, count = %zu", what, need, count);
  if (what == 3) {
    std::copy(h->dropped.begin(), h->dropped.end(), host);
    return ROM_OK;
  }
  ROM_HIP(hipSetDevice(h->ctx->device));
  const double* src = h->dev->p + (what == 0 ? 0 : what == 1 ? 16 : PL_OFF_W);
  h->syncs += 1;
  return download(h->ctx, src, host, need);
}
