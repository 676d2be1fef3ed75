// The small dense pieces of the batched Levenberg-Marquardt kernels (rom_lm.hip: rom_lm_polish, rom_sense.hip: rom_poly_sense),
// for one workgroup of 256 threads (4 waves) per system: wave reductions, the L D L^T factorisation and solve of a matrix of
// order <= 64 in LDS, the one-sided Jacobi for the smallest singular value of a tall matrix held by columns in LDS, and the
// kernel that keeps the best start of every query.  (internal)
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr int LMS_THREADS = 256;   // the workgroup the routines below assume
constexpr int LMS_SWEEPS = 30;     // bound of the Jacobi sweeps (<= 16 columns converge in under 10)
enum { LMS_FN = 0, LMS_MOVED = 1, LMS_MAXNEW = 2, LMS_OKH = 3, LMS_OKA = 4 };   // the slots of `scal` (5 .. 7: the system's own)

__device__ __forceinline__ double wave_sum(double v) {   // (the butterfly leaves the same bits in every lane)
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ double wave_max_nan(double v) {   // NaN wins, as in numpy's max
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const double o = __shfl_xor(v, m, 64);
    v = (o > v || o != o) ? o : v;
  }
  return v;
}
__device__ __forceinline__ double group16_sum(double v) {
  v += __shfl_xor(v, 8, 64);
  v += __shfl_xor(v, 4, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 1, 64);
  return v;
}

// L D L^T in place on the lower triangle, all 256 threads: afterwards M[r][c] = l_rc d_c (c < r), M[j][j] = d_j, invd[j] = 1 / d_j.
// Wave w takes the rows j + 1 + w, + 4, ..; a lane takes column j + 1 + lane (n <= 64).  *flag = 1.0 iff every pivot is > 0.
__device__ bool lm_factor(double* M, int ld, int n, double* invd, double* flag) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int j = 0; j < n - 1; ++j) {
    const double inv = 1.0 / M[j * ld + j];
    const int c = j + 1 + lane;
    if (c < n) {
      const double lc = M[c * ld + j] * inv;
      for (int r = j + 1 + w; r < n; r += 4)
        if (c <= r) M[r * ld + c] -= M[r * ld + j] * lc;
    }
    __syncthreads();   // column j + 1 is final; step j wrote nothing that it read (it reads column j, writes columns > j)
  }
  if (tid < 64) {
    bool good = true;
    if (lane < n) {
      const double d = M[lane * ld + lane];
      good = d > 0.0;
      invd[lane] = 1.0 / d;
    }
    const unsigned long long bad = __ballot(!good);
    if (lane == 0) *flag = bad ? 0.0 : 1.0;
  }
  __syncthreads();
  return *flag != 0.0;
}

// x = (L D L^T)^-1 b for NR right-hand sides held by one wave, lane = row
template <int NR>
__device__ __forceinline__ void lm_solve(const double* M, int ld, int n, const double* invd, double (&b)[NR], int lane) {
  for (int j = 0; j < n - 1; ++j) {
    const double l = (lane > j && lane < n) ? M[lane * ld + j] * invd[j] : 0.0;
#pragma unroll
    for (int u = 0; u < NR; ++u) b[u] = fma(-l, __shfl(b[u], j, 64), b[u]);
  }
  const double di = lane < n ? invd[lane] : 0.0;
#pragma unroll
  for (int u = 0; u < NR; ++u) b[u] *= di;
  for (int j = n - 1; j > 0; --j) {
    const double l = lane < j ? M[j * ld + lane] * invd[lane] : 0.0;
#pragma unroll
    for (int u = 0; u < NR; ++u) b[u] = fma(-l, __shfl(b[u], j, 64), b[u]);
  }
}

// The smallest singular value of the r x k matrix whose column q lies at Js + q ldr (Js is overwritten): one-sided (Hestenes)
// Jacobi on its k columns by one wave, a lane holding the rows lane, lane + 64, .. (r <= 64 RPL).  Every lane holds the same
// alpha, beta, gamma (wave_sum), so the wave's control flow is uniform.  k = 0: +infinity.
template <int RPL>
__device__ double lm_sigma_min_wave(double* Js, int ldr, int k, int r, int lane) {
  for (int sweep = 0; sweep < LMS_SWEEPS; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < k - 1; ++p)
      for (int q = p + 1; q < k; ++q) {
        double x[RPL], y[RPL];
#pragma unroll
        for (int u = 0; u < RPL; ++u) {
          const int i = lane + 64 * u;
          x[u] = i < r ? Js[p * ldr + i] : 0.0;
          y[u] = i < r ? Js[q * ldr + i] : 0.0;
        }
        double xx = x[0] * x[0], yy = y[0] * y[0], xy = x[0] * y[0];
#pragma unroll
        for (int u = 1; u < RPL; ++u) xx += x[u] * x[u], yy += y[u] * y[u], xy += x[u] * y[u];
        const double alpha = wave_sum(xx), beta = wave_sum(yy), gamma = wave_sum(xy);
        if (!(alpha > 0.0 && beta > 0.0) || !(fabs(gamma) > 2.220446049250313e-16 * sqrt(alpha) * sqrt(beta))) continue;
        rotated = true;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double tn = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double cs = 1.0 / sqrt(1.0 + tn * tn), sn = cs * tn;
#pragma unroll
        for (int u = 0; u < RPL; ++u) {
          const int i = lane + 64 * u;
          if (i < r) {
            Js[p * ldr + i] = cs * x[u] - sn * y[u];
            Js[q * ldr + i] = sn * x[u] + cs * y[u];
          }
        }
      }
    if (!rotated) break;
  }
  double smin = __builtin_huge_val();
  for (int q = 0; q < k; ++q) {
    double xx = 0.0;
#pragma unroll
    for (int u = 0; u < RPL; ++u) {
      const int i = lane + 64 * u;
      const double x = i < r ? Js[q * ldr + i] : 0.0;
      xx = u == 0 ? x * x : xx + x * x;
    }
    const double s = sqrt(wave_sum(xx));
    smin = (s < smin || s != s) ? s : smin;
  }
  return smin;
}

// Per query the start of smallest misfit (the lowest index among equals, the first NaN if there is one: numpy.argmin); one wave
// per query copies that system's row of W (ldw doubles, the misfit at column mcol) and appends the start
__global__ __launch_bounds__(64) void k_lm_select(const double* __restrict__ W, int ldw, int t, int mcol, double* __restrict__ OUT, long long ldo) {
  const long long q = blockIdx.x;
  const int lane = threadIdx.x;
  int best = 0;
  double bm = W[size_t(q * t) * ldw + mcol];
  for (int s = 1; s < t; ++s) {
    const double v = W[size_t(q * t + s) * ldw + mcol];
    if (bm == bm && (v < bm || v != v)) {
      bm = v;
      best = s;
    }
  }
  const double* row = W + size_t(q * t + best) * ldw;
  double* o = OUT + q * ldo;
  for (int e = lane; e < ldw; e += 64) o[e] = row[e];
  if (lane == 0) o[ldw] = double(best);
}

}  // namespace
