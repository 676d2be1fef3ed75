// rom_sensor_dopt: greedy Bayesian D-optimal sensor selection for the PARAMETER problem -- which m of ncand candidate points make
// the data determine theta = log a best, on average over a library of M parameters, under the linearised Gaussian model (expected
// information gain).  romhighcontrast_amd/inverse.py::sensor_dopt_host is the specification.
//
// The model: c(theta) = A(theta)^-1 bhat, A = sum_q e^theta_q Ahat_q; X_j = -dc/dtheta at library entry j (n x k, column q =
// e^theta_q A^-1 Ahat_q c: inverse.py:59-60); a candidate x is its row e_x (n) of the basis at x, its Jacobian row at entry j is
// g = X_j^T e_x.  Noise N(0, sigma^2) per sensor, prior covariance T0 T0^T: the posterior precision of a sensor set S is
// F_j(S) = Gamma_0 + sigma^-2 sum_S g g^T and the criterion Phi(S) = 1 / (2 M) sum_j log det(Gamma_0^-1 F_j(S)).
//
// STATE holds per entry the block [Z_j^T | T_j | status, s] (OedLayout): T_j T_j^T = F_j^-1 (k x k), Z_j = X_j T_j / sigma (n x k,
// stored by columns: row q of Z_j^T is n_pad doubles), k padded to kp in {1, 2, 4, 8, 16} and n to a multiple of 4 with zeros.
//   k_dopt_sens    one workgroup per entry: A(theta_j) assembled, factored and solved with lm_factor / lm_solve for c and the k
//                  columns of X_j; Z_j = X_j T0 / sigma, T_j = T0.  An entry whose A has a pivot that is not positive (status 1) or
//                  whose theta is not finite (status 2) gets Z_j = 0: it adds exactly 0 to every score.
//   k_dopt_score   score(x) = sum_j log1p(|Z_j^T e_x|^2), the gain of x.  The product E (ncand x n) [Z_1 .. Z_M] runs on
//                  v_mfma_f64_16x16x4_f64 and is never written: up to 128 candidates are the LDS-resident table, the rows (j, q) of
//                  Z^T stream through in slabs of 32 (the layout, strides and operand maps of rom_slab.h).  A wave owns 16
//                  candidates and both row tiles of a slab, so a candidate's running sum lives in registers and grows in
//                  ascending j.  The rows of a tile are staged in an order that puts the kp values of an entry into one lane's
//                  registers (kp <= 4) or into lanes 16 (and 32) apart (kp = 8, 16): the sum over an entry costs no LDS trip.
//                  The library is cut into chunks of OED_CHUNK_ROWS rows of Z^T -- a function of kp alone, never of the candidates
//                  -- and k_dopt_reduce adds the chunks' partial sums in chunk order: a candidate's score has the same bits
//                  whichever other candidates are in the call.
//   k_dopt_pick    the first maximum among the candidates not yet picked whose score is finite; the stop rules; one workgroup.
//   k_dopt_update  one wave per entry: u = Z_j^T e_x*, s = |u|^2, rho = sqrt(1 + s), beta = 1 / (rho (rho + 1)),
//                  Z_j -= beta (Z_j u) u^T, T_j -= beta (T_j u) u^T -- the symmetric square root of the Sherman-Morrison downdate,
//                  (I - beta u u^T)^2 = I - u u^T / (1 + s): no factorisation, no difference of near-equal numbers.
// The m steps are enqueued without host involvement (a device flag turns the launches after a stop into no-ops); one host
// synchronisation at the end.  fp64 only, no floating-point atomics: the same bits on a repeated call.
#include <cmath>
#include <cstring>

#include "rom_basis_int.h"
#include "rom_block.h"
#include "rom_lm_small.h"
#include "rom_slab.h"

namespace {

constexpr int OED_NMAX = 64, OED_KMAX = 16, OED_PICKS_MAX = 1024;
constexpr int OED_TAB = 128;            // candidates of one LDS table: 16 per wave
constexpr int OED_CHUNK_ROWS = 2048;    // rows of Z^T of one chunk: 64 slabs
constexpr long long OED_M_MAX = 1LL << 24, OED_NCAND_MAX = 1LL << 22;   // chunks in grid.x, candidate tables in grid.y (<= 65535)
enum { OED_STOP = 0, OED_REASON = 1, OED_MADE = 2, OED_NANS = 3, OED_SKIPPED = 4, OED_CTL = 8 };   // the control words

// the block of one library entry in STATE, in doubles (host and device): rom_sensor_dopt_layout
struct OedLayout {
  int kp, npad, tmat, tail, ent;
  __host__ __device__ OedLayout(int n, int k) {
    kp = 1;
    while (kp < k) kp *= 2;
    npad = (n + 3) / 4 * 4;
    tmat = kp * npad, tail = tmat + kp * kp, ent = tail + 2;   // Z^T (kp x npad) | T (kp x kp) | status | s of the last update
  }
};
size_t oed_score_lds(int npad) { return size_t(OED_TAB + 2 * SLAB_ROWS) * slab_ld_nt(npad) * sizeof(double); }

struct OedPrior {
  double T0[OED_KMAX * OED_KMAX];   // k x k, row-major
};

// ---- the sensitivities ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LMS_THREADS) void k_dopt_sens(int n, int k, const double* __restrict__ Ahat, const double* __restrict__ bhat,
                                                           const double* __restrict__ THETA, long long ldt, double inv_sigma,
                                                           const OedPrior prior, double* __restrict__ STATE, int* __restrict__ ctl) {
  __shared__ double As[OED_NMAX * (OED_NMAX + 1)], invd[OED_NMAX], cs[OED_NMAX], Xs[OED_KMAX * OED_NMAX], ea[OED_KMAX];
  __shared__ double T0s[OED_KMAX * OED_KMAX], flag[2];
  const OedLayout o(n, k);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, ldn = n | 1;
  const long long j = blockIdx.x;
  double* ent = STATE + size_t(j) * o.ent;
  if (tid < 64) {
    bool bad = false;
    if (lane < k) {
      const double th = THETA[j * ldt + lane];
      bad = !(fabs(th) <= 1.7976931348623157e308);
      ea[lane] = exp(th);
    }
    const unsigned long long any = __ballot(bad);
    if (lane == 0) flag[1] = any ? 1.0 : 0.0;
  }
  for (int e = tid; e < k * k; e += LMS_THREADS) T0s[e] = prior.T0[e];
  __syncthreads();
  for (int idx = tid; idx < n * n; idx += LMS_THREADS) {   // py:54
    const int row = idx / n, col = idx - row * n;
    double s = 0.0;
    for (int q = 0; q < k; ++q) s = fma(ea[q], Ahat[size_t(q) * n * n + idx], s);
    As[row * ldn + col] = s;
  }
  __syncthreads();
  const bool spd = lm_factor(As, ldn, n, invd, flag);
  const bool finite = flag[1] == 0.0;
  if (!spd || !finite) {   // (every thread takes this branch or none: both flags are LDS values behind a barrier)
    for (int e = tid; e < o.tmat; e += LMS_THREADS) ent[e] = 0.0;
    for (int e = tid; e < o.kp * o.kp; e += LMS_THREADS) {
      const int a = e / o.kp, b = e - a * o.kp;
      ent[o.tmat + e] = (a < k && b < k) ? T0s[a * k + b] : 0.0;
    }
    if (tid == 0) {
      ent[o.tail] = finite ? 1.0 : 2.0;
      ent[o.tail + 1] = 0.0;
      atomicAdd(ctl + OED_SKIPPED, 1);
    }
    return;
  }
  if (tid < 64) {   // py:55
    double b[1] = {lane < n ? bhat[lane] : 0.0};
    lm_solve<1>(As, ldn, n, invd, b, lane);
    if (lane < n) cs[lane] = b[0];
  }
  __syncthreads();
  for (int idx = tid; idx < n * k; idx += LMS_THREADS) {   // py:59: column q of V = e^theta_q Ahat_q c
    const int q = idx / n, i = idx - q * n;
    const double* arow = Ahat + (size_t(q) * n + i) * n;
    double s = 0.0;
    for (int c = 0; c < n; ++c) s = fma(arow[c], cs[c], s);
    Xs[q * OED_NMAX + i] = ea[q] * s;
  }
  __syncthreads();
  if (4 * w < k) {   // py:60: X = A^-1 V, wave w the columns 4 w .. 4 w + 3
    double b[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) b[u] = (4 * w + u < k && lane < n) ? Xs[(4 * w + u) * OED_NMAX + lane] : 0.0;
    lm_solve<4>(As, ldn, n, invd, b, lane);
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (4 * w + u < k && lane < n) Xs[(4 * w + u) * OED_NMAX + lane] = b[u];
  }
  __syncthreads();
  for (int e = tid; e < o.tmat; e += LMS_THREADS) {   // Z = X T0 / sigma, by columns
    const int p = e / o.npad, i = e - p * o.npad;
    double v = 0.0;
    if (p < k && i < n) {
      for (int q = 0; q < k; ++q) v = fma(Xs[q * OED_NMAX + i], T0s[q * k + p], v);
      v *= inv_sigma;
    }
    ent[e] = v;
  }
  for (int e = tid; e < o.kp * o.kp; e += LMS_THREADS) {
    const int a = e / o.kp, b = e - a * o.kp;
    ent[o.tmat + e] = (a < k && b < k) ? T0s[a * k + b] : 0.0;
  }
  if (tid == 0) ent[o.tail] = 0.0, ent[o.tail + 1] = 0.0;
}

// ---- the scores -----------------------------------------------------------------------------------------------------------------
// Where row rp = (entry e, column q) = (rp / KP, rp % KP) of the 16 consecutive rows of a tile is staged: result register g of lane
// (i, k4) is tile row k4 + 4 g, so with KP <= 4 lane k4 holds the entries k4 (4 / KP) .. in its registers, q fastest, and with
// KP = 8, 16 an entry's q = 4 c + g sits in register g of lane k4 = e KP / 4 + c.
template <int KP>
__device__ __forceinline__ int oed_tile_pos(int rp) {
  const int e = rp / KP, q = rp % KP;
  if constexpr (KP <= 4) {
    constexpr int EPL = 4 / KP;
    return e / EPL + 4 * ((e % EPL) * KP + q);
  } else {
    return e * (KP / 4) + (q >> 2) + 4 * (q & 3);
  }
}
#ifdef ROMHC_OED_PLAIN_SUM   // (A/B build libromhc_oed_plain.so of tools/gpu_sensor_dopt.py: what the log1p of the epilogue costs)
#define OED_LOG1P(s) (s)
#else
#define OED_LOG1P(s) log1p(s)
#endif
// run += log1p(|Z_j^T e_x|^2) over the 16 / KP entries of one tile in ascending j; afterwards the four lanes of a candidate hold the
// same sum
template <int KP>
__device__ __forceinline__ void oed_tile_sum(const d4_t& y, double& run, int i) {
  if constexpr (KP <= 4) {
    constexpr int EPL = 4 / KP;
    double l[EPL];
#pragma unroll
    for (int a = 0; a < EPL; ++a) {
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < KP; ++q) s = fma(y[a * KP + q], y[a * KP + q], s);
      l[a] = OED_LOG1P(s);
    }
#pragma unroll
    for (int e = 0; e < 16 / KP; ++e) run += __shfl(l[e % EPL], i + 16 * (e / EPL), 64);
  } else {
    double s = 0.0;
#pragma unroll
    for (int g = 0; g < 4; ++g) s = fma(y[g], y[g], s);
    s += __shfl_xor(s, 16, 64);
    if (KP == 16) s += __shfl_xor(s, 32, 64);
    const double l = OED_LOG1P(s);
#pragma unroll
    for (int e = 0; e < 16 / KP; ++e) run += __shfl(l, i + 16 * e * (KP / 4), 64);
  }
}

// grid (chunks, candidate tables).  Workgroup (x, y): the candidates [y OED_TAB, ..) as the table, the rows [x OED_CHUNK_ROWS, ..) of
// Z^T as slabs; OUT[x ncand + candidate] = the chunk's sum.  A row past M KP is zero and adds log1p(0) = 0.
template <int KP>
__global__ __launch_bounds__(SLAB_THREADS) void k_dopt_score(const double* __restrict__ STATE, long long M, int n, int npad, int ent,
                                                            const double* __restrict__ E, long long lde, int ncand,
                                                            double* __restrict__ OUT, const int* __restrict__ ctl) {
  if (ctl && ctl[OED_STOP]) return;
  extern __shared__ double oed_lds[];
  const int LX = slab_ld_nt(npad);
  double* Bs = oed_lds;               // OED_TAB x LX
  double* As = Bs + OED_TAB * LX;     // 2 x 32 x LX
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, i = lane & 15, k4 = lane >> 4;
  const int q0 = blockIdx.y * OED_TAB, nqv = min(OED_TAB, ncand - q0), nct = (nqv + 15) >> 4;
  for (int e = t; e < OED_TAB * LX; e += SLAB_THREADS) {
    const int j = e / LX, c = e - j * LX;
    Bs[e] = (j < nqv && c < n) ? E[(long long)(q0 + j) * lde + c] : 0.0;
  }
  // staging map of a slab: row t >> 4 of the slab, columns (t & 15) + 16 u
  const int srow = t >> 4, scl = t & 15;
  const int spos = (srow & 16) + oed_tile_pos<KP>(srow & 15);
  const long long nrows = M * KP, nslabs = (nrows + SLAB_ROWS - 1) / SLAB_ROWS;
  const long long slab0 = (long long)blockIdx.x * (OED_CHUNK_ROWS / SLAB_ROWS), slab1 = min(nslabs, slab0 + OED_CHUNK_ROWS / SLAB_ROWS);
  double zv[4];
  auto load_slab = [&](long long s) {
    const long long row = s * SLAB_ROWS + srow;
    const double* src = STATE + size_t(row / KP) * ent + int(row % KP) * npad;
#pragma unroll
    for (int u = 0; u < 4; ++u) zv[u] = (row < nrows && scl + 16 * u < npad) ? src[scl + 16 * u] : 0.0;
  };
  double run = 0.0;
  load_slab(slab0);
  for (long long s = slab0; s < slab1; ++s) {
    double* Ab = As + (int(s - slab0) & 1) * SLAB_ROWS * LX;
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (scl + 16 * u < npad) Ab[spos * LX + scl + 16 * u] = zv[u];
    if (s + 1 < slab1) load_slab(s + 1);
    __syncthreads();   // slab s is staged (and the table); every wave is past the product of slab s - 1, in the other buffer
    if (w < nct) {
      d4_t y0 = {0.0, 0.0, 0.0, 0.0}, y1 = {0.0, 0.0, 0.0, 0.0};
      const double* pa = Ab + i * LX + k4;
      const double* pb = Bs + (w * 16 + i) * LX + k4;
      for (int kk = 0; kk < npad; kk += 4) {
        const double b = pb[kk];
        y0 = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[kk], b, y0, 0, 0, 0);
        y1 = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[16 * LX + kk], b, y1, 0, 0, 0);
      }
      oed_tile_sum<KP>(y0, run, i);
      oed_tile_sum<KP>(y1, run, i);
    }
  }
  if (w < nct && k4 == 0 && w * 16 + i < nqv) OUT[size_t(blockIdx.x) * ncand + q0 + w * 16 + i] = run;
}

// SCORE[x] = the chunks' sums in chunk order
__global__ void k_dopt_reduce(const double* __restrict__ PART, int chunks, int ncand, double* __restrict__ SCORE, const int* __restrict__ ctl) {
  if (ctl && ctl[OED_STOP]) return;
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= ncand) return;
  double s = PART[x];
  for (int c = 1; c < chunks; ++c) s += PART[size_t(c) * ncand + x];
  SCORE[x] = s;
}

// ---- the pick -------------------------------------------------------------------------------------------------------------------
// one workgroup: the first maximum of the finite scores of the candidates not yet taken, and the stop rules
__global__ __launch_bounds__(1024) void k_dopt_pick(const double* __restrict__ SCORE, int ncand, int step, double rel_tol,
                                                    int* __restrict__ taken, int* __restrict__ picks, double* __restrict__ gains,
                                                    double* __restrict__ first_gain, int* __restrict__ ctl) {
  __shared__ double sv[1024];
  __shared__ int si[1024], sn[1024];
  if (ctl[OED_STOP]) return;
  const int tid = threadIdx.x;
  double bv = 0.0;
  int bi = -1, nans = 0;
  for (int x = tid; x < ncand; x += 1024) {
    const double v = SCORE[x];
    const bool number = fabs(v) <= 1.7976931348623157e308;   // (neither NaN nor Inf)
    nans += !number;
    if (number && !taken[x] && (bi < 0 || v > bv)) bv = v, bi = x;
  }
  sv[tid] = bv, si[tid] = bi, sn[tid] = nans;
  __syncthreads();
  for (int h = 512; h >= 1; h >>= 1) {
    if (tid < h) {
      const double ov = sv[tid + h];
      const int oi = si[tid + h], mi = si[tid];
      if (oi >= 0 && (mi < 0 || ov > sv[tid] || (ov == sv[tid] && oi < mi))) sv[tid] = ov, si[tid] = oi;
      sn[tid] += sn[tid + h];
    }
    __syncthreads();
  }
  if (tid != 0) return;
  if (step == 0) ctl[OED_NANS] = sn[0];
  bv = sv[0], bi = si[0];
  if (bi < 0) {
    ctl[OED_STOP] = 1, ctl[OED_REASON] = 2;
    return;
  }
  if (step == 0) *first_gain = bv;
  if (bv <= rel_tol * *first_gain) {
    ctl[OED_STOP] = 1, ctl[OED_REASON] = 1;
    return;
  }
  picks[step] = bi;
  gains[step] = bv;
  taken[bi] = 1;
  ctl[OED_MADE] = step + 1;
}

// ---- the update -----------------------------------------------------------------------------------------------------------------
// a wave per entry, four entries per workgroup; lane = row i of Z_j (and row a of T_j)
__global__ __launch_bounds__(256) void k_dopt_update(double* __restrict__ STATE, long long M, int n, int k, const double* __restrict__ E,
                                                     long long lde, const int* __restrict__ picks, int step, int* __restrict__ ctl) {
  const OedLayout o(n, k);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long j = (long long)blockIdx.x * 4 + w;
  if (j >= M) return;
  double* ent = STATE + size_t(j) * o.ent;
  if (step == 0 && lane == 0 && ent[o.tail] != 0.0) atomicAdd(ctl + OED_SKIPPED, 1);
  if (ctl[OED_STOP]) return;
  const double e = lane < n ? E[(long long)picks[step] * lde + lane] : 0.0;
  double uq = 0.0, s = 0.0;   // u_q lives in lane q
  for (int q = 0; q < k; ++q) {
    const double z = lane < n ? ent[q * o.npad + lane] : 0.0;
    const double u = wave_sum(z * e);
    s = fma(u, u, s);
    uq = lane == q ? u : uq;
  }
  const double rho = sqrt(1.0 + s), beta = 1.0 / (rho * (rho + 1.0));
  double zu = 0.0, tu = 0.0;
  for (int q = 0; q < k; ++q) {
    const double u = __shfl(uq, q, 64);
    zu = fma(lane < n ? ent[q * o.npad + lane] : 0.0, u, zu);
    tu = fma(lane < k ? ent[o.tmat + lane * o.kp + q] : 0.0, u, tu);
  }
  zu *= beta, tu *= beta;
  for (int q = 0; q < k; ++q) {
    const double u = __shfl(uq, q, 64);
    if (lane < n) ent[q * o.npad + lane] = fma(-zu, u, ent[q * o.npad + lane]);
    if (lane < k) ent[o.tmat + lane * o.kp + q] = fma(-tu, u, ent[o.tmat + lane * o.kp + q]);
  }
  if (lane == 0) ent[o.tail + 1] = s;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
int oed_check_sizes(const char* who, int n, int k) {
  ROM_CHECK(n >= 1 && n <= OED_NMAX, "%s: n = %d reduced unknowns, between 1 and %d", who, n, OED_NMAX);
  ROM_CHECK(k >= 1 && k <= OED_KMAX, "%s: k = %d parameters, between 1 and %d", who, k, OED_KMAX);
  return ROM_OK;
}
int oed_check_library(const char* who, const OedLayout& o, rom_buf* STATE, size_t s_off, int64_t M) {
  ROM_CHECK(M >= 1 && M <= OED_M_MAX, "%s: M = %lld library entries, between 1 and %lld", who, (long long)M, OED_M_MAX);
  return rom_check_block(who, {"STATE", "the entry block", "the entry block"}, STATE->n, s_off, o.ent, o.ent, M);
}
int oed_check_candidates(const char* who, int n, rom_buf* E, size_t e_off, int64_t lde, int64_t ncand) {
  ROM_CHECK(ncand >= 1 && ncand <= OED_NCAND_MAX, "%s: ncand = %lld candidates, between 1 and %lld", who, (long long)ncand, OED_NCAND_MAX);
  return rom_check_block(who, {"E", "lde", "n"}, E->n, e_off, lde, n, ncand);
}

struct ScorePass {
  int kp, npad, ent, chunks, ncand;
  long long M;
  size_t lds;
  double flops;
};
int oed_plan_score(rom_ctx* ctx, const char* who, int n, const OedLayout& o, long long M, int ncand, ScorePass* sp) {
  const long long nslabs = (M * o.kp + SLAB_ROWS - 1) / SLAB_ROWS;
  sp->kp = o.kp, sp->npad = o.npad, sp->ent = o.ent, sp->M = M, sp->ncand = ncand;
  sp->chunks = int((M * o.kp + OED_CHUNK_ROWS - 1) / OED_CHUNK_ROWS);
  sp->lds = oed_score_lds(o.npad);
  sp->flops = 2.0 * double(nslabs) * SLAB_ROWS * o.npad * 16.0 * ((ncand + 15) / 16);
  const int idx = o.kp == 1 ? 0 : o.kp == 2 ? 1 : o.kp == 4 ? 2 : o.kp == 8 ? 3 : 4;
  const void* kern[5] = {reinterpret_cast<const void*>(k_dopt_score<1>), reinterpret_cast<const void*>(k_dopt_score<2>),
                         reinterpret_cast<const void*>(k_dopt_score<4>), reinterpret_cast<const void*>(k_dopt_score<8>),
                         reinterpret_cast<const void*>(k_dopt_score<16>)};
  if (sp->lds > 64 * 1024) ROM_TRY(rom_lds_optin(ctx->lds_optin_dopt_score[idx], kern[idx], 160 * 1024));
  if (sp->chunks > 1)
    ROM_CHECK(size_t(sp->chunks) * ncand * sizeof(double) <= ctx->ws_limit, "%s: %d chunks x %d candidates of partial sums exceed the workspace limit",
              who, sp->chunks, ncand);
  return ROM_OK;
}
// one pass: the scores of all candidates -> SCORE (PART: chunks x ncand doubles when chunks > 1).  Returns the launches made.
int oed_launch_score(rom_ctx* ctx, const ScorePass& sp, int n, const double* state, const double* e, long long lde, double* PART,
                     double* SCORE, const int* ctl) {
  const dim3 grid(sp.chunks, (sp.ncand + OED_TAB - 1) / OED_TAB);
  double* out = sp.chunks > 1 ? PART : SCORE;
  {
    char nm[48];
    rom_prof_name(nm, sizeof nm, "dopt_score", "_n%d_kp%d", n, sp.kp);
    ROM_PROF(ctx, nm, sp.flops, 8.0 * (double(sp.M) * sp.ent * grid.y + double(sp.ncand) * (n + sp.chunks)));
#define OED_SCORE(KP) k_dopt_score<KP><<<grid, SLAB_THREADS, sp.lds, ctx->stream>>>(state, sp.M, n, sp.npad, sp.ent, e, lde, sp.ncand, out, ctl)
    switch (sp.kp) {
      case 1: OED_SCORE(1); break;
      case 2: OED_SCORE(2); break;
      case 4: OED_SCORE(4); break;
      case 8: OED_SCORE(8); break;
      default: OED_SCORE(16); break;
    }
#undef OED_SCORE
  }
  if (sp.chunks > 1) {
    ROM_PROF(ctx, "dopt_reduce", double(sp.chunks) * sp.ncand, 8.0 * double(sp.chunks + 1) * sp.ncand);
    k_dopt_reduce<<<blocks_for(sp.ncand), 256, 0, ctx->stream>>>(PART, sp.chunks, sp.ncand, SCORE, ctl);
  }
  return sp.chunks > 1 ? 2 : 1;
}

}  // namespace

extern "C" int rom_sensor_dopt_layout(int n, int k, int64_t* out8) {
  ROM_CHECK(out8, "rom_sensor_dopt_layout: null argument");
  ROM_TRY(oed_check_sizes("rom_sensor_dopt_layout", n, k));
  const OedLayout o(n, k);
  const int64_t v[8] = {o.kp, o.npad, o.ent, OED_CHUNK_ROWS / o.kp, int64_t(oed_score_lds(o.npad)), o.tmat, o.tail, OED_TAB};
  std::memcpy(out8, v, sizeof v);
  return ROM_OK;
}

extern "C" int rom_sensor_dopt_init(rom_ctx* ctx, int n, int k, rom_buf* Ahat, rom_buf* bhat, rom_buf* THETA, size_t t_off, int64_t ldt,
                                    int64_t M, const double* T0_host, double sigma, rom_buf* STATE, size_t s_off, double* info_host) {
  ROM_CHECK(ctx && Ahat && bhat && THETA && T0_host && STATE, "rom_sensor_dopt_init: null argument");
  ROM_TRY(oed_check_sizes("rom_sensor_dopt_init", n, k));
  ROM_CHECK(sigma > 0.0 && sigma <= 1.7976931348623157e308, "rom_sensor_dopt_init: sigma = %g, the noise level must be positive and finite", sigma);
  const OedLayout o(n, k);
  ROM_TRY(oed_check_library("rom_sensor_dopt_init", o, STATE, s_off, M));
  ROM_TRY(rom_check_block("rom_sensor_dopt_init", {"THETA", "ldt", "k"}, THETA->n, t_off, ldt, k, M));
  ROM_CHECK(Ahat->n >= size_t(k) * n * n && bhat->n >= size_t(n), "rom_sensor_dopt_init: Ahat or bhat holds fewer than k n n = %zu, n = %d doubles",
            size_t(k) * n * n, n);
  OedPrior prior;
  std::memset(&prior, 0, sizeof prior);
  for (int e = 0; e < k * k; ++e) {
    ROM_CHECK(std::isfinite(T0_host[e]), "rom_sensor_dopt_init: T0 (the factor of the prior covariance) holds NaN / Inf");
    prior.T0[e] = T0_host[e];
  }
  if (info_host) std::fill(info_host, info_host + 8, 0.0);
  ROM_HIP(hipSetDevice(ctx->device));
  Tmp ws;
  ROM_TRY(ws.get(ctx, OED_CTL / 2));
  int* ctl = reinterpret_cast<int*>(ws.p());
  ROM_HIP(hipMemsetAsync(ctl, 0, OED_CTL * sizeof(int), ctx->stream));
  {
    char nm[48];
    rom_prof_name(nm, sizeof nm, "dopt_sens", "_n%d_k%d", n, k);
    ROM_PROF(ctx, nm, double(M) * (double(n) * n * n / 3.0 + 2.0 * double(k + 1) * n * n + 2.0 * double(k) * n * n), 8.0 * double(M) * o.ent);
    k_dopt_sens<<<unsigned(M), LMS_THREADS, 0, ctx->stream>>>(n, k, Ahat->p, bhat->p, THETA->p + t_off, ldt, 1.0 / sigma, prior,
                                                             STATE->p + s_off, ctl);
  }
  ROM_HIP(hipGetLastError());
  int hctl[OED_CTL] = {};
  ROM_HIP(hipMemcpyAsync(hctl, ctl, sizeof hctl, hipMemcpyDeviceToHost, ctx->stream));
  ROM_HIP(hipStreamSynchronize(ctx->stream));
  if (info_host) {
    info_host[0] = hctl[OED_SKIPPED];
    info_host[1] = 1;   // launches
    info_host[2] = 1;   // host synchronisations
    info_host[3] = double(OED_CTL) * sizeof(int);
  }
  return ROM_OK;
}

extern "C" int rom_sensor_dopt_scores(rom_ctx* ctx, int n, int k, rom_buf* STATE, size_t s_off, int64_t M, rom_buf* E, size_t e_off,
                                      int64_t lde, int64_t ncand, rom_buf* SCORE, size_t sc_off) {
  ROM_CHECK(ctx && STATE && E && SCORE, "rom_sensor_dopt_scores: null argument");
  ROM_TRY(oed_check_sizes("rom_sensor_dopt_scores", n, k));
  const OedLayout o(n, k);
  ROM_TRY(oed_check_library("rom_sensor_dopt_scores", o, STATE, s_off, M));
  ROM_TRY(oed_check_candidates("rom_sensor_dopt_scores", n, E, e_off, lde, ncand));
  ROM_TRY(rom_check_block("rom_sensor_dopt_scores", {"SCORE", "ncand", "ncand"}, SCORE->n, sc_off, ncand, int(ncand), 1));
  ROM_HIP(hipSetDevice(ctx->device));
  ScorePass sp;
  ROM_TRY(oed_plan_score(ctx, "rom_sensor_dopt_scores", n, o, M, int(ncand), &sp));
  Tmp part;
  if (sp.chunks > 1) ROM_TRY(part.get(ctx, size_t(sp.chunks) * ncand));
  oed_launch_score(ctx, sp, n, STATE->p + s_off, E->p + e_off, lde, sp.chunks > 1 ? part.p() : nullptr, SCORE->p + sc_off, nullptr);
  ROM_HIP(hipGetLastError());
  ROM_HIP(hipStreamSynchronize(ctx->stream));
  return ROM_OK;
}

extern "C" int rom_sensor_dopt(rom_ctx* ctx, int n, int k, rom_buf* STATE, size_t s_off, int64_t M, rom_buf* E, size_t e_off, int64_t lde,
                               int64_t ncand, int m, double rel_tol, const int32_t* taken_host, int ntaken, int32_t* picks_out,
                               double* gain_out, double* info_host) {
  ROM_CHECK(ctx && STATE && E && picks_out && gain_out, "rom_sensor_dopt: null argument");
  ROM_TRY(oed_check_sizes("rom_sensor_dopt", n, k));
  const OedLayout o(n, k);
  ROM_CHECK(m >= 1 && m <= OED_PICKS_MAX && m <= ncand, "rom_sensor_dopt: m = %d picks, between 1 and min(%d, ncand = %lld)", m, OED_PICKS_MAX,
            (long long)ncand);
  ROM_TRY(oed_check_library("rom_sensor_dopt", o, STATE, s_off, M));
  ROM_TRY(oed_check_candidates("rom_sensor_dopt", n, E, e_off, lde, ncand));
  ROM_CHECK(rel_tol >= 0.0 && rel_tol < 1.0, "rom_sensor_dopt: rel_tol = %g, at least 0 and below 1", rel_tol);
  ROM_CHECK(ntaken >= 0 && (ntaken == 0 || taken_host), "rom_sensor_dopt: ntaken = %d candidates taken before, without their list", ntaken);
  for (int e = 0; e < ntaken; ++e)
    ROM_CHECK(taken_host[e] >= 0 && taken_host[e] < ncand, "rom_sensor_dopt: taken[%d] = %d is no candidate (ncand = %lld)", e, taken_host[e],
              (long long)ncand);
  if (info_host) std::fill(info_host, info_host + 8, 0.0);
  std::fill(picks_out, picks_out + m, -1);
  std::fill(gain_out, gain_out + m, 0.0);
  ROM_HIP(hipSetDevice(ctx->device));
  ScorePass sp;
  ROM_TRY(oed_plan_score(ctx, "rom_sensor_dopt", n, o, M, int(ncand), &sp));

  // workspace: scores | partial sums | gains | the first gain | taken (ints) | picks (ints) | control words (ints)
  const size_t nc = size_t(ncand), n_part = sp.chunks > 1 ? size_t(sp.chunks) * nc : 0, n_taken = (nc + 1) / 2, n_picks = (size_t(m) + 1) / 2;
  const size_t ws_doubles = nc + n_part + m + 1 + n_taken + n_picks + OED_CTL / 2;
  Tmp ws;
  ROM_TRY(ws.get(ctx, ws_doubles));
  double* score = ws.p();
  double* part = score + nc;
  double* gains = part + n_part;
  double* first_gain = gains + m;
  int* taken = reinterpret_cast<int*>(first_gain + 1);
  int* picks = reinterpret_cast<int*>(first_gain + 1 + n_taken);
  int* ctl = reinterpret_cast<int*>(first_gain + 1 + n_taken + n_picks);
  ROM_HIP(hipMemsetAsync(gains, 0, (ws_doubles - nc - n_part) * sizeof(double), ctx->stream));
  std::vector<int> one(ntaken, 1);   // (alive until the synchronisation below)
  for (int e = 0; e < ntaken; ++e)
    ROM_HIP(hipMemcpyAsync(taken + taken_host[e], one.data() + e, sizeof(int), hipMemcpyHostToDevice, ctx->stream));

  double* state = STATE->p + s_off;
  const double* e = E->p + e_off;
  int launches = 0;
  for (int step = 0; step < m; ++step) {
    launches += oed_launch_score(ctx, sp, n, state, e, lde, part, score, ctl);
    {
      ROM_PROF(ctx, "dopt_pick", 0.0, 12.0 * double(ncand));
      k_dopt_pick<<<1, 1024, 0, ctx->stream>>>(score, int(ncand), step, rel_tol, taken, picks, gains, first_gain, ctl);
    }
    {
      ROM_PROF(ctx, "dopt_update", 6.0 * double(M) * k * (n + k), 16.0 * double(M) * o.ent);
      k_dopt_update<<<unsigned((M + 3) / 4), 256, 0, ctx->stream>>>(state, M, n, k, e, lde, picks, step, ctl);
    }
    launches += 2;
  }
  ROM_HIP(hipGetLastError());
  int hctl[OED_CTL] = {};
  std::vector<int> hpicks(m);
  ROM_HIP(hipMemcpyAsync(hctl, ctl, sizeof hctl, hipMemcpyDeviceToHost, ctx->stream));
  ROM_HIP(hipMemcpyAsync(hpicks.data(), picks, size_t(m) * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  ROM_HIP(hipMemcpyAsync(gain_out, gains, size_t(m) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ROM_HIP(hipStreamSynchronize(ctx->stream));
  const int made = hctl[OED_MADE];
  for (int s = 0; s < m; ++s) {
    picks_out[s] = s < made ? hpicks[s] : -1;
    if (s >= made) gain_out[s] = 0.0;
  }
  if (info_host) {
    info_host[0] = made;
    info_host[1] = hctl[OED_REASON];
    info_host[2] = hctl[OED_SKIPPED];
    info_host[3] = hctl[OED_NANS];
    info_host[4] = launches;
    info_host[5] = 1;   // host synchronisations
    info_host[6] = double(ws_doubles) * sizeof(double);
    info_host[7] = sp.flops * (made + (made < m ? 1 : 0));   // executed by the score passes that ran
  }
  return ROM_OK;
}
