// rom_nearest: for K query rows P, the t rows of a tall library Q (M rows, r <= 128 columns) at the smallest Euclidean distance --
// the search of the library-based parameter estimation (romhighcontrast_amd/inverse.py): which of the M reduced states that
// rom_resid_eval left on the device explain K measurement vectors best.
//
// The ANSWER is defined by one device function, nn_dist2: d2 = sum_c (p_c - q_c)^2 from the original operands, differences
// first, one fma chain in column order.  The t rows returned are the smallest under the total order (d2, row index) -- what an
// exhaustive scan with that function returns (k_nn_exhaust + k_nn_merge: mode 1, and the fallback of mode 0).
//
// Mode 0 finds the same rows without forming the K x M scores:
//   k_nn_screen   s_jk = |q~_j|^2 - 2 p~_k . q~_j on operands shifted by the library's column means, by the slab engine of
//                 rom_slab.h: up to 128 queries are the LDS-resident B table, library slabs of 32 rows stream through as A.  Only
//                 the minimum of every slab (group, G = 32 rows) and query leaves the kernel: a K x ceil(M / 32) table.
//   k_nn_select   one workgroup per query: the T' = t + 4 groups of smallest minima, their rows rescored with nn_dist2, the top
//                 t of those, and the certificate
//                     d2_(t) (1 + (r + 2) eps) + delta_k  <  (smallest minimum of the groups not rescored) + |p~_k|^2.
//                 delta_k = 4 (r + 4) (eps (|p~_k|^2 + max_j |q~_j|^2) + 2^-1022), eps = 2^-52, bounds every error between the
//                 right-hand side and the exact squared distance of a row not rescored: with u = eps / 2 and S = |p~|^2 + |q~|^2,
//                     the r-term fma dot product of the MFMA, in any order, times 2:     r u 2 |p~| |q~|  <=  r u S
//                     |q~_j|^2 and |p~_k|^2, r-term fma chains:                                               r u S
//                     the fma that forms s and the addition of |p~_k|^2:                                      4 u S
//                     one rounding of each centred entry, |(p~ - q~) - (p - q)| <= u (|p~| + |q~|):           4 u S
//                 in all (2 r + 8) u S = (r + 4) eps S -- a quarter of delta_k, whose second term covers operations that underflow.
//                 A row that was not rescored then has an exact distance above d2_(t) (1 + (r + 2) eps), so nn_dist2 (relative error
//                 below (r + 2) u) puts it strictly behind the t rows found.  The certificate decides which path computes a query's
//                 answer, never the answer: a query that fails it (NaN and overflow in the screen fail it) goes to the exhaustive kernel.
// No floating-point atomics anywhere: partial results are combined in a fixed order, a repeated call returns the same bits.
#include <cmath>
#include <cstring>

#include "rom_basis_int.h"
#include "rom_block.h"
#include "rom_dist.h"
#include "rom_slab.h"

namespace {

constexpr int NN_TMAX = 8;              // (NN_RMAX, NN_EPS, NN_INF, nn_dist2, nn_less and the column statistics: rom_dist.h)
constexpr int NN_EXTRA = 4;          // T' = t + NN_EXTRA groups are rescored
constexpr int NN_SLOTS = 16;         // slabs whose minima wait in LDS: one query's minima leave as a 128-byte line
constexpr int NN_LDM = NN_SLOTS + 1;
constexpr int NN_QB = 16;            // queries of one workgroup of the exhaustive kernel (four per wave)
constexpr int NN_TILE = 64;          // library rows of one tile of the exhaustive kernel (a lane each)
constexpr int NN_STAT = 130;         // mean (128) | non-finite entries of Q | of P
constexpr long long NN_NOROW = 0x7fffffffffffffffLL;

// ---- a sorted list of t (distance, row) pairs held by the lanes s < t of a wave ----------------------------------------------
// insert the wave-uniform candidate (cd, cj): the entries below it are a prefix of the list, the rest moves up one lane
__device__ __forceinline__ void topt_insert(double& ed, long long& ej, double cd, long long cj, int t, int lane) {
  const bool below = lane < t && nn_less(ed, ej, cd, cj);
  const int pos = __popcll(__ballot(below));
  const double ud = __shfl_up(ed, 1, 64);
  const long long uj = __shfl_up(ej, 1, 64);
  if (pos >= t) return;
  if (lane == pos) {
    ed = cd;
    ej = cj;
  } else if (lane > pos && lane < t) {
    ed = ud;
    ej = uj;
  }
}
// every lane offers its own (d, j); the ones that beat the list's last entry are inserted in lane order.  The last entry is read
// again after every insertion: a lane it has overtaken meanwhile costs no insertion.
__device__ __forceinline__ void topt_offer(double& ed, long long& ej, double d, long long j, bool valid, int t, int lane) {
  unsigned long long open = ~0ull;   // lanes not yet looked at
  for (;;) {
    const double td = __shfl(ed, t - 1, 64);
    const long long tj = __shfl(ej, t - 1, 64);
    const unsigned long long mask = __ballot(valid && nn_less(d, j, td, tj)) & open;
    if (!mask) break;
    const int l = __ffsll((long long)mask) - 1;
    open = l == 63 ? 0ull : ~0ull << (l + 1);
    const double cd = __shfl(d, l, 64);
    const long long cj = __shfl(j, l, 64);
    topt_insert(ed, ej, cd, cj, t, lane);
  }
}

// pn[k] = |p~_k|^2, p~ = fl(p - mean): the entries the screen's B table holds
__global__ void k_nn_pnorm(const double* __restrict__ P, long long ldp, int K, int r, const double* __restrict__ mean, double* __restrict__ pn) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  double s = 0.0;
  for (int c = 0; c < r; ++c) {
    const double v = P[(long long)k * ldp + c] - mean[c];
    s = fma(v, v, s);
  }
  pn[k] = s;
}

// ---- the screen -------------------------------------------------------------------------------------------------------------
// grid (slab chunks, query tables).  Workgroup (x, y): queries [y nq_tab, (y + 1) nq_tab) of the launch's kq as the B table, the
// slabs [x per_chunk, (x + 1) per_chunk) of the library as A (per_chunk is a multiple of NN_SLOTS).  tab[k][g] (row stride ngs) =
// min over the rows j of slab g of |q~_j|^2 - 2 p~_k . q~_j; a NaN score counts as -inf (the group is rescored or the query is
// not certified), a row past M as +inf.  qmax_part[x] = max of |q~_j|^2 over the chunk's rows (written by y == 0).
__global__ __launch_bounds__(SLAB_THREADS) void k_nn_screen(const double* __restrict__ Q, long long ldq, long long M,
                                                           const double* __restrict__ P, long long ldp, int kq, int r, int rpad,
                                                           int nq_tab, const double* __restrict__ mean, long long per_chunk,
                                                           double* __restrict__ tab, long long ngs, double* __restrict__ qmax_part) {
  extern __shared__ double nn_lds[];
  const int LX = slab_ld_nt(rpad);
  double* Bs = nn_lds;                         // nq_tab x LX
  double* As = Bs + nq_tab * LX;               // 2 x 32 x LX
  double* nqs = As + 2 * SLAB_ROWS * LX;       // 2 x 32: |q~|^2 of the slab's rows
  double* mb = nqs + 2 * SLAB_ROWS;            // 2 row tiles x nq_tab x NN_LDM
  double* qred = mb + 2 * nq_tab * NN_LDM;     // 32
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, i = lane & 15, k4 = lane >> 4;
  const int rt = w & 1, ct0 = w >> 1;
  const int q0 = blockIdx.y * nq_tab, nqv = min(nq_tab, kq - q0), nct = (nqv + 15) >> 4;

  for (int e = t; e < nq_tab * LX; e += SLAB_THREADS) {
    const int j = e / LX, c = e - j * LX;
    Bs[e] = (j < nqv && c < r) ? P[(long long)(q0 + j) * ldp + c] - mean[c] : 0.0;
  }
  // staging map of a slab: row t >> 4, columns (t & 15) + 16 u
  const int srow = t >> 4, scl = t & 15;
  double mu[8], qv[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) mu[u] = scl + 16 * u < r ? mean[scl + 16 * u] : 0.0;
  long long slab0, slab1;
  slab_chunk_range(M, per_chunk, &slab0, &slab1);
  auto load_slab = [&](long long s) {
    const long long row = s * SLAB_ROWS + srow;
#pragma unroll
    for (int u = 0; u < 8; ++u) qv[u] = (row < M && scl + 16 * u < r) ? Q[row * ldq + scl + 16 * u] - mu[u] : 0.0;
  };
  double qmax = 0.0;
  if (slab0 < slab1) load_slab(slab0);
  for (long long s = slab0; s < slab1; ++s) {
    const int buf = int(s - slab0) & 1, slot = int(s - slab0) & (NN_SLOTS - 1);
    double* Ab = As + buf * SLAB_ROWS * LX;
    {
      double nq = 0.0;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (scl + 16 * u < rpad) Ab[srow * LX + scl + 16 * u] = qv[u];
        nq = fma(qv[u], qv[u], nq);
      }
      nq += __shfl_xor(nq, 1, 64);
      nq += __shfl_xor(nq, 2, 64);
      nq += __shfl_xor(nq, 4, 64);
      nq += __shfl_xor(nq, 8, 64);
      if (scl == 0) {
        nqs[buf * SLAB_ROWS + srow] = nq;
        if (s * SLAB_ROWS + srow < M) qmax = nq > qmax || nq != nq ? nq : qmax;   // (NaN stays: the certificate then fails)
      }
    }
    if (s + 1 < slab1) load_slab(s + 1);
    __syncthreads();   // slab s is staged; every wave is past the product of slab s - 1 (the other buffer) and the last flush
    d4_t y[2];
    slab_nt(Ab, LX, Bs, LX, rpad, nct, y);
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int ct = ct0 + 4 * jj;
      if (ct < nct) {
        double m = NN_INF;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int rl = rt * 16 + k4 + 4 * g;
          double sc = fma(-2.0, y[jj][g], nqs[buf * SLAB_ROWS + rl]);
          sc = sc != sc ? -NN_INF : sc;
          sc = s * SLAB_ROWS + rl < M ? sc : NN_INF;
          m = sc < m ? sc : m;
        }
        double o = __shfl_xor(m, 16, 64);
        m = o < m ? o : m;
        o = __shfl_xor(m, 32, 64);
        m = o < m ? o : m;
        if (k4 == 0) mb[(rt * nq_tab + ct * 16 + i) * NN_LDM + slot] = m;
      }
    }
    if (slot == NN_SLOTS - 1 || s + 1 == slab1) {
      __syncthreads();
      const long long g0 = s - slot;
      for (int e = t; e < nq_tab * NN_SLOTS; e += SLAB_THREADS) {
        const int j = e >> 4, sl = e & (NN_SLOTS - 1);
        if (j < nqv && sl <= slot) {
          const double a = mb[j * NN_LDM + sl], b = mb[(nq_tab + j) * NN_LDM + sl];
          tab[(long long)(q0 + j) * ngs + g0 + sl] = b < a ? b : a;
        }
      }
      // (the next slab's minima are written after the next barrier)
    }
  }
  if (blockIdx.y != 0) return;
  if (scl == 0) qred[srow] = qmax;
  __syncthreads();
  if (t == 0) {
    double m = qred[0];
    for (int q = 1; q < SLAB_ROWS; ++q) m = qred[q] > m || qred[q] != qred[q] ? qred[q] : m;
    qmax_part[blockIdx.x] = m;
  }
}

// ---- select, rescore, certify: one workgroup per query ----------------------------------------------------------------------
// the lists of the four waves (up to 16 sorted entries each, in mv / mi) merged into one list of n, held by every wave
__device__ __forceinline__ void topt_merge4(double& ed, long long& ej, const double* mv, const long long* mi, int n, int lane) {
  const double v = mv[lane];
  const long long j = mi[lane];
  ed = NN_INF;
  ej = NN_NOROW;
  topt_offer(ed, ej, v, j, (lane & 15) < n && j != NN_NOROW, n, lane);
}

__global__ __launch_bounds__(256) void k_nn_select(const double* __restrict__ Q, long long ldq, long long M, const double* __restrict__ P,
                                                   long long ldp, int k0, int r, int t, int Tp, const double* __restrict__ tab,
                                                   long long ngs, long long ng, const double* __restrict__ pn,
                                                   const double* __restrict__ qmax_part, int qchunks, double* __restrict__ res_d,
                                                   long long* __restrict__ res_j, double* __restrict__ cert) {
  __shared__ double prow[NN_RMAX], mv[64];
  __shared__ long long mi[64], sel[16];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, k = k0 + blockIdx.x;
  const double* trow = tab + (long long)blockIdx.x * ngs;
  for (int c = tid; c < r; c += 256) prow[c] = P[(long long)k * ldp + c];

  // one pass over the query's minima: the Tp + 1 <= 13 smallest (minimum, group) -- the groups to rescore and the best one left
  const int T1 = Tp + 1;
  double ed = NN_INF;
  long long ej = NN_NOROW;
  for (long long g0 = (long long)w * 64; g0 < ng; g0 += 1024) {
    double v[4];   // (four loads in flight: the offers between them are cross-lane operations the loads would wait behind)
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = g0 + 256 * u + lane < ng ? trow[g0 + 256 * u + lane] : NN_INF;
#pragma unroll
    for (int u = 0; u < 4; ++u) topt_offer(ed, ej, v[u], g0 + 256 * u + lane, g0 + 256 * u + lane < ng, T1, lane);
  }
  if (lane < 16) {
    mv[w * 16 + lane] = ed;
    mi[w * 16 + lane] = lane < T1 ? ej : NN_NOROW;
  }
  __syncthreads();
  topt_merge4(ed, ej, mv, mi, T1, lane);
  const int found = __popcll(__ballot(lane < T1 && ej != NN_NOROW)), nsel = min(found, Tp);
  const bool all_rescored = found <= Tp;   // (then found == ng: every group is rescored)
  const double rest = all_rescored ? NN_INF : __shfl(ed, Tp, 64);
  if (w == 0 && lane < nsel) sel[lane] = ej;
  __syncthreads();

  // rescore the rows of those groups with nn_dist2; top t per wave, then of the four waves
  const int ncand = nsel * SLAB_ROWS;
  ed = NN_INF;
  ej = NN_NOROW;
  for (int e0 = w * 64; e0 < ncand; e0 += 256) {
    const int e = e0 + lane;
    const long long j = e < ncand ? sel[e >> 5] * SLAB_ROWS + (e & 31) : NN_NOROW;
    double d[1] = {NN_INF};
    if (j < M) nn_dist2<1>(prow, 0, Q + j * ldq, r, d);
    topt_offer(ed, ej, d[0], j, j < M, t, lane);
  }
  if (lane < 16) {
    mv[w * 16 + lane] = ed;
    mi[w * 16 + lane] = lane < t ? ej : NN_NOROW;
  }
  __syncthreads();
  if (w != 0) return;
  topt_merge4(ed, ej, mv, mi, t, lane);
  if (lane < t) {
    res_d[(long long)k * t + lane] = ed;
    res_j[(long long)k * t + lane] = ej;
  }
  const double dt = __shfl(ed, t - 1, 64);
  const bool complete = __shfl(ej, t - 1, 64) != NN_NOROW;   // (t <= M rows were among the candidates)
  if (lane == 0) {
    double qmax = 0.0;
    for (int q = 0; q < qchunks; ++q) qmax = qmax_part[q] > qmax || qmax_part[q] != qmax_part[q] ? qmax_part[q] : qmax;
    // (the second term covers operations that underflow: (r + 8) of them, 2^-1075 each)
    const double delta = 4.0 * double(r + 4) * (NN_EPS * (pn[k] + qmax) + 2.2250738585072014e-308);
    const double lhs = dt * (1.0 + double(r + 2) * NN_EPS) + delta;
    cert[k] = (complete && (all_rescored || lhs < rest + pn[k])) ? 1.0 : 0.0;
  }
}

// ---- the exhaustive scan ----------------------------------------------------------------------------------------------------
// grid (row chunks, blocks of NN_QB listed queries from block qb0 on), 256 threads.  Library tiles of 64 rows go through LDS (a
// lane per row, odd stride); wave w scores its four queries against the tile with nn_dist2 and offers the results to its running top-t lists.
// part[(query slot, chunk)][t] receives the chunk's list.
__global__ __launch_bounds__(256) void k_nn_exhaust(const double* __restrict__ Q, long long ldq, long long M, const double* __restrict__ P,
                                                    long long ldp, const int* __restrict__ list, int nlist, int qb0, int r, int t,
                                                    long long rows_per_chunk, double* __restrict__ part_d, long long* __restrict__ part_j) {
  extern __shared__ double nn_lds[];
  const int LQ = r | 1;
  double* Ps = nn_lds;            // NN_QB x r
  double* Qs = Ps + NN_QB * r;    // NN_TILE x LQ
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int qb = (qb0 + int(blockIdx.y)) * NN_QB;
  for (int e = tid; e < NN_QB * r; e += 256) {
    const int n = e / r, c = e - n * r;
    Ps[e] = P[(long long)list[min(qb + n, nlist - 1)] * ldp + c];
  }
  double ed[4];
  long long ej[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    ed[n] = NN_INF;
    ej[n] = NN_NOROW;
  }
  const long long r0 = (long long)blockIdx.x * rows_per_chunk, r1 = min(M, r0 + rows_per_chunk);
  for (long long row0 = r0; row0 < r1; row0 += NN_TILE) {
    __syncthreads();
    for (int e = tid; e < NN_TILE * r; e += 256) {
      const int rr = e / r, c = e - rr * r;
      Qs[rr * LQ + c] = row0 + rr < r1 ? Q[(row0 + rr) * ldq + c] : 0.0;
    }
    __syncthreads();
    double d[4];
    nn_dist2<4>(Ps + w * 4 * r, r, Qs + lane * LQ, r, d);
#pragma unroll
    for (int n = 0; n < 4; ++n) topt_offer(ed[n], ej[n], d[n], row0 + lane, row0 + lane < r1, t, lane);
  }
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int qi = qb + w * 4 + n;
    if (qi < nlist && lane < t) {
      const size_t at = (size_t(qi) * gridDim.x + blockIdx.x) * t + lane;
      part_d[at] = ed[n];
      part_j[at] = ej[n];
    }
  }
}
// one wave per listed query: the top t of its chunks' lists
__global__ __launch_bounds__(64) void k_nn_merge(const double* __restrict__ part_d, const long long* __restrict__ part_j, int chunks,
                                                 const int* __restrict__ list, int t, double* __restrict__ res_d,
                                                 long long* __restrict__ res_j) {
  const int lane = threadIdx.x, qi = blockIdx.x, n = chunks * t;
  double ed = NN_INF;
  long long ej = NN_NOROW;
  for (int base = 0; base < n; base += 64) {
    const int e = base + lane;
    const bool valid = e < n;
    const double d = valid ? part_d[size_t(qi) * n + e] : NN_INF;
    const long long j = valid ? part_j[size_t(qi) * n + e] : NN_NOROW;
    topt_offer(ed, ej, d, j, valid && j != NN_NOROW, t, lane);
  }
  if (lane < t) {
    res_d[(long long)list[qi] * t + lane] = ed;
    res_j[(long long)list[qi] * t + lane] = ej;
  }
}

size_t screen_lds(int rpad, int nq_tab) {
  return (size_t(nq_tab + 2 * SLAB_ROWS) * slab_ld_nt(rpad) + 2 * SLAB_ROWS + 2 * size_t(nq_tab) * NN_LDM + SLAB_ROWS) * sizeof(double);
}
size_t exhaust_lds(int r) { return (size_t(NN_QB) * r + size_t(NN_TILE) * (r | 1)) * sizeof(double); }

}  // namespace

extern "C" int rom_nearest(rom_ctx* ctx, rom_buf* Q, size_t q_off, int64_t ldq, int64_t M, rom_buf* P, size_t p_off, int64_t ldp, int K,
                           int r, int t, int mode, int64_t* idx_host, double* dist2_host, double* info_host) {
  ROM_CHECK(ctx && Q, "rom_nearest: null argument (context or Q)");
  ROM_CHECK(r >= 1 && r <= NN_RMAX, "rom_nearest: r = %d columns, between 1 and %d", r, NN_RMAX);
  ROM_CHECK(t >= 1 && t <= NN_TMAX, "rom_nearest: t = %d neighbours, between 1 and %d", t, NN_TMAX);
  ROM_CHECK(M >= t && M <= (int64_t(1) << 40), "rom_nearest: M = %lld library rows, at least t = %d", (long long)M, t);
  ROM_CHECK(K >= 0, "rom_nearest: K = %d queries", K);
  ROM_CHECK(mode == 0 || mode == 1, "rom_nearest: mode = %d, 0 (screened search) or 1 (exhaustive scan)", mode);
  ROM_TRY(rom_check_block("rom_nearest", {"Q", "ldq", "r"}, Q->n, q_off, ldq, r, M));
  if (info_host) std::fill(info_host, info_host + 8, 0.0);
  if (K == 0) return ROM_OK;
  ROM_CHECK(P && idx_host && dist2_host, "rom_nearest: null argument (P, idx_host or dist2_host)");
  ROM_TRY(rom_check_block("rom_nearest", {"P", "ldp", "r"}, P->n, p_off, ldp, r, K));
  ROM_HIP(hipSetDevice(ctx->device));
  const double* q = Q->p + q_off;
  const double* p = P->p + p_off;
  int launches = 0, syncs = 0;
  double executed = 0.0;
  size_t ws_doubles = 0;
  auto take = [&](Tmp& tmp, size_t n) -> int {
    ws_doubles += n;
    return tmp.get(ctx, n);
  };

  // column means of the library; NaN / Inf in either operand
  Tmp stat, spart, res;
  ROM_TRY(take(stat, NN_STAT));
  int rp = 1;
  while (rp < r) rp *= 2;
  {
    const int qc = int(std::min<int64_t>(512, (M + 63) / 64)), pc = int(std::min<int64_t>(512, (int64_t(K) + 63) / 64));
    ROM_TRY(take(spart, size_t(std::max(qc, pc)) * (NN_RMAX + 1)));
    ROM_PROF(ctx, "nn_stats", 2.0 * double(M + K) * r, 8.0 * double(M + K) * r);
    k_nn_stats_partial<<<qc, 256, 0, ctx->stream>>>(q, ldq, M, r, rp, (M + qc - 1) / qc, spart);
    k_nn_stats_finish<<<1, 1024, 0, ctx->stream>>>(spart, qc, r, M, 1, NN_RMAX, stat);
    k_nn_stats_partial<<<pc, 256, 0, ctx->stream>>>(p, ldp, K, r, rp, (int64_t(K) + pc - 1) / pc, spart);
    k_nn_stats_finish<<<1, 1024, 0, ctx->stream>>>(spart, pc, r, K, 0, NN_RMAX + 1, stat);
    ROM_HIP(hipGetLastError());
    launches += 4;
  }
  // results: dist2 (K t) | rows (K t, as 64-bit integers) | certified flags (K)
  const size_t kt = size_t(K) * t;
  ROM_TRY(take(res, 2 * kt + K));
  double* res_d = res;
  long long* res_j = reinterpret_cast<long long*>(res.p() + kt);
  double* cert = res.p() + 2 * kt;
  ROM_HIP(hipMemsetAsync(cert, 0, size_t(K) * sizeof(double), ctx->stream));
  std::vector<double> hres(2 * kt + K), hstat(2);
  std::vector<int> list;
  const int Tp = t + NN_EXTRA;
  int certified = 0;

  Tmp tab, pn, qmax_part, dlist, part;
  const int rpad = (r + 3) / 4 * 4, nq_tab = rpad <= 64 ? 128 : 64;
  const long long nslabs = (M + SLAB_ROWS - 1) / SLAB_ROWS, ngs = (nslabs + NN_SLOTS - 1) / NN_SLOTS * NN_SLOTS;
  // the queries of one pass: as many tables as the workspace limit allows (none: every query goes to the exhaustive scan)
  const long long k_fit = (long long)(ctx->ws_limit / (size_t(ngs) * sizeof(double))) / nq_tab * nq_tab;
  const bool screened = mode == 0 && k_fit >= nq_tab;
  if (screened) {
    // (and at most 65535 tables per pass: they are the workgroups of grid.y)
    const int kc = int(std::min<long long>({k_fit, (K + nq_tab - 1) / nq_tab * nq_tab, 65535LL * nq_tab}));
    const SlabPlan sp = rom_slab_plan(ctx, M, r);
    const long long per = (sp.per_chunk + NN_SLOTS - 1) / NN_SLOTS * NN_SLOTS;
    const int chunks = int((nslabs + per - 1) / per);
    ROM_TRY(take(tab, size_t(kc) * ngs));
    ROM_TRY(take(pn, K));
    ROM_TRY(take(qmax_part, chunks));
    const size_t lds = screen_lds(rpad, nq_tab);
    if (lds > 64 * 1024) ROM_TRY(rom_lds_optin(ctx->lds_optin_nn_screen, reinterpret_cast<const void*>(k_nn_screen), 160 * 1024));
    k_nn_pnorm<<<blocks_for(K), 256, 0, ctx->stream>>>(p, ldp, K, r, stat, pn);
    ROM_HIP(hipGetLastError());
    launches += 1;
    for (int k0 = 0; k0 < K; k0 += kc) {
      const int kq = std::min(kc, K - k0), ntab = (kq + nq_tab - 1) / nq_tab;
      {
        const double fl = 2.0 * double(nslabs) * SLAB_ROWS * rpad * 16.0 * ((kq + 15) / 16);
        char nm[48];
        rom_prof_name(nm, sizeof nm, "nn_screen", "_r%d_K%d", r, kq);
        ROM_PROF(ctx, nm, fl, 8.0 * (double(M) * r * ntab + double(kq) * ngs));
        k_nn_screen<<<dim3(chunks, ntab), SLAB_THREADS, lds, ctx->stream>>>(q, ldq, M, p + size_t(k0) * ldp, ldp, kq, r, rpad, nq_tab, stat,
                                                                          per, tab, ngs, qmax_part);
        executed += fl;
      }
      ROM_HIP(hipGetLastError());
      {
        const double cand = double(std::min<long long>(Tp, nslabs)) * SLAB_ROWS;
        ROM_PROF(ctx, "nn_select", 3.0 * kq * cand * r, 8.0 * kq * (double(Tp + 1) * nslabs + cand * r));
        k_nn_select<<<kq, 256, 0, ctx->stream>>>(q, ldq, M, p, ldp, k0, r, t, Tp, tab, ngs, nslabs, pn, qmax_part, chunks, res_d, res_j, cert);
        executed += 3.0 * kq * cand * r;
      }
      ROM_HIP(hipGetLastError());
      launches += 2;
    }
    // the answers of the certified queries, and which queries the certificate leaves
    ROM_HIP(hipMemcpyAsync(hstat.data(), stat.p() + NN_RMAX, 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ROM_TRY(download(ctx, res, hres.data(), 2 * kt + K));
    syncs += 1;
    ROM_CHECK(hstat[0] == 0.0 && hstat[1] == 0.0, "rom_nearest: NaN / Inf in the operands (%.0f entries of Q, %.0f of P)", hstat[0], hstat[1]);
    for (int k = 0; k < K; ++k) {
      if (hres[2 * kt + k] != 0.0) certified += 1;
      else list.push_back(k);
    }
  } else {
    list.resize(K);
    for (int k = 0; k < K; ++k) list[k] = k;
  }
  const int nlist = int(list.size());
  if (nlist > 0) {
    const int nqb = (nlist + NN_QB - 1) / NN_QB;
    const int rc = int(std::max<int64_t>(1, std::min<int64_t>({256, (M + NN_TILE - 1) / NN_TILE, int64_t((2048 + nqb - 1) / nqb)})));
    const long long rows_per = ((M + rc - 1) / rc + NN_TILE - 1) / NN_TILE * NN_TILE;
    const int chunks = int((M + rows_per - 1) / rows_per);
    ROM_TRY(take(dlist, (size_t(nlist) + 1) / 2));
    ROM_TRY(take(part, 2 * size_t(nlist) * chunks * t));
    int* d_list = reinterpret_cast<int*>(dlist.p());
    double* part_d = part;
    long long* part_j = reinterpret_cast<long long*>(part.p() + size_t(nlist) * chunks * t);
    ROM_HIP(hipMemcpyAsync(d_list, list.data(), size_t(nlist) * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    const size_t lds = exhaust_lds(r);
    if (lds > 64 * 1024) ROM_TRY(rom_lds_optin(ctx->lds_optin_nn_exhaust, reinterpret_cast<const void*>(k_nn_exhaust), 96 * 1024));
    {
      ROM_PROF(ctx, "nn_exhaust", 3.0 * double(nqb) * NN_QB * double(M) * r, 8.0 * double(nqb) * double(M) * r);
      for (int b0 = 0; b0 < nqb; b0 += 65535) {  // grid.y holds at most 65535 query blocks per launch
        k_nn_exhaust<<<dim3(chunks, std::min(65535, nqb - b0)), 256, lds, ctx->stream>>>(q, ldq, M, p, ldp, d_list, nlist, b0, r, t, rows_per,
                                                                                        part_d, part_j);
        launches += 1;
      }
    }
    ROM_HIP(hipGetLastError());
    {
      ROM_PROF(ctx, "nn_merge", 0.0, 16.0 * double(nlist) * chunks * t);
      k_nn_merge<<<nlist, 64, 0, ctx->stream>>>(part_d, part_j, chunks, d_list, t, res_d, res_j);
    }
    ROM_HIP(hipGetLastError());
    launches += 1;
    executed += 3.0 * double(nlist) * double(M) * r;
  }
  if (!screened) ROM_HIP(hipMemcpyAsync(hstat.data(), stat.p() + NN_RMAX, 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (nlist > 0) {
    ROM_TRY(download(ctx, res, hres.data(), 2 * kt));   // (also the end of every kernel that reads `list`)
    syncs += 1;
  }
  ROM_CHECK(hstat[0] == 0.0 && hstat[1] == 0.0, "rom_nearest: NaN / Inf in the operands (%.0f entries of Q, %.0f of P)", hstat[0], hstat[1]);
  std::copy(hres.begin(), hres.begin() + kt, dist2_host);
  std::memcpy(idx_host, hres.data() + kt, kt * sizeof(int64_t));
  if (info_host) {
    info_host[0] = SLAB_ROWS;
    info_host[1] = screened ? Tp : 0;
    info_host[2] = certified;
    info_host[3] = nlist;
    info_host[4] = launches;
    info_host[5] = syncs;
    info_host[6] = double(ws_doubles) * sizeof(double);
    info_host[7] = executed;
  }
  return ROM_OK;
}
