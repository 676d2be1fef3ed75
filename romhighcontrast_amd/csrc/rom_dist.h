// The squared Euclidean distance that rom_nearest and rom_kmeans define their answers by, and the column statistics both take
// of a tall block before they screen it (internal; device code, included by rom_nearest.hip and rom_kmeans.hip).
#pragma once
#include "romhc_internal.h"

namespace {

constexpr int NN_RMAX = 128;                        // most columns of a row
constexpr double NN_EPS = 2.220446049250313e-16;   // 2^-52
constexpr double NN_INF = __builtin_huge_val();

// ---- THE distance: out[n] += sum_c (p_n[c] - q[c])^2, n < N query rows ldp apart, columns in order ----------------------------
template <int N>
__device__ __forceinline__ void nn_dist2(const double* __restrict__ p, int ldp, const double* __restrict__ q, int r, double (&out)[N]) {
#pragma unroll
  for (int n = 0; n < N; ++n) out[n] = 0.0;
  for (int c = 0; c < r; ++c) {
    const double qc = q[c];
#pragma unroll
    for (int n = 0; n < N; ++n) {
      const double d = p[n * ldp + c] - qc;
      out[n] = fma(d, d, out[n]);
    }
  }
}

// The same chain with the differences d_c = p_c - q_c already formed and spread over the sixteen lanes of a row's group: lane
// (l & 15) holds d[u] = d_(l & 15) + 16 u.  Every lane of the group returns the value nn_dist2 returns, bit for bit (column order,
// one fma per column, from 0.0).  All 64 lanes of the wave call it.
__device__ __forceinline__ double nn_dist2_lanes16(const double (&d)[8], int r) {
  const int base = int(threadIdx.x) & 48;
  double out = 0.0;
#pragma unroll
  for (int u = 0; u < 8; ++u)
    if (16 * u < r) {
#pragma unroll
      for (int l = 0; l < 16; ++l)
        if (16 * u + l < r) {
          const double dc = __shfl(d[u], base + l, 64);
          out = fma(dc, dc, out);
        }
    }
  return out;
}

__device__ __forceinline__ bool nn_less(double d, long long j, double d2, long long j2) { return d < d2 || (d == d2 && j < j2); }

// ---- column sums and the count of non-finite entries, fixed-order partials ---------------------------------------------------
// part[chunk][c] = sum of column c over the chunk's rows, part[chunk][128] = its entries that are NaN or Inf.  256 threads =
// (256 / rp) row lanes x rp columns, rp the power of two >= r.
__global__ __launch_bounds__(256) void k_nn_stats_partial(const double* __restrict__ X, long long ld, long long rows, int r, int rp,
                                                          long long rows_per_chunk, double* __restrict__ part) {
  __shared__ double ssum[256], sbad[256];
  const int t = threadIdx.x, c = t & (rp - 1), nl = 256 / rp, ry = t / rp;
  const long long r0 = (long long)blockIdx.x * rows_per_chunk, r1 = min(rows, r0 + rows_per_chunk);
  double s = 0.0, bad = 0.0;
  if (c < r)
    for (long long j = r0 + ry; j < r1; j += nl) {
      const double v = X[j * ld + c];
      s += v;
      bad += fabs(v) <= 1.7976931348623157e308 ? 0.0 : 1.0;
    }
  ssum[t] = s;
  sbad[t] = bad;
  __syncthreads();
  double* out = part + size_t(blockIdx.x) * (NN_RMAX + 1);
  if (t < rp && t < r) {
    for (int q = 1; q < nl; ++q) s += ssum[q * rp + t];
    out[t] = s;
  }
  if (t == 0) {
    double b = 0.0;
    for (int q = 0; q < 256; ++q) b += sbad[q];   // (a count: exact in any order)
    out[NN_RMAX] = b;
  }
}
// stat[c] = column mean (mean != 0), stat[bad_at] = the count.  1024 threads = 8 sub-sums x 128 columns: sub-sum s adds the
// chunks s, s + 8, ... in order, then the eight are added in order (a single chain over all chunks is latency-bound)
__global__ __launch_bounds__(1024) void k_nn_stats_finish(const double* __restrict__ part, int chunks, int r, long long rows, int mean,
                                                          int bad_at, double* __restrict__ stat) {
  __shared__ double sub[8][NN_RMAX + 1];
  const int c = threadIdx.x & 127, sl = threadIdx.x >> 7;
  {
    double s = 0.0, b = 0.0;
    for (int q = sl; q < chunks; q += 8) {
      if (c < r) s += part[size_t(q) * (NN_RMAX + 1) + c];
      if (c == 0) b += part[size_t(q) * (NN_RMAX + 1) + NN_RMAX];
    }
    sub[sl][c] = s;
    if (c == 0) sub[sl][NN_RMAX] = b;
  }
  __syncthreads();
  if (sl != 0) return;
  if (mean && c < r) {
    double s = sub[0][c];
    for (int q = 1; q < 8; ++q) s += sub[q][c];
    stat[c] = s / double(rows);
  }
  if (c == 0) {
    double b = 0.0;
    for (int q = 0; q < 8; ++q) b += sub[q][NN_RMAX];
    stat[bad_at] = b;
  }
}

}  // namespace
