// One system of box-constrained least squares  min over lo <= c <= hi of ||p - G c||^2  for one workgroup of 256 threads: the
// Stark-Parker active-set iteration of romhighcontrast_amd/inverse.py::bvls_host (cited below as `py:` with the names of that
// function), shared by rom_bvls.hip (G and G^T G in global memory, one G for every system) and rom_local_select.hip (the same
// for its first solve; the second one has its own matrix and Gram matrix per system, in LDS).  The matrix, its Gram matrix and
// the status word are reached through pointers, the box comes per lane; everything else is the caller's LDS.  (internal)
//
// n <= 64 is one lane per column, so every decision of a pass (feasibility, the step to the first bound, the multiplier to
// free, the bars) is taken by wave 0 with ballots and wave reductions, written to LDS, and read from there by all 256 threads:
// control flow is uniform within a workgroup.  Every loop is bounded by max_iter, n or r.  One fixed order in every sum.
//
// A pass (py:_bvls_solve): the Gram block of the free columns -- packed to the front in ascending order by a ballot, which gives
// the factor the host gets from the identity rows it puts in the place of the bound ones, without their elimination steps -- is
// factored in LDS (L D L^T, lm_factor of rom_lm_small.h, all four waves) and solved by wave 0 (lm_solve); one refinement step
// follows with the residual formed on the columns of G themselves, so the error of c is that of a least-squares solve, not of
// the bare normal equations.
#pragma once
#include "rom_lm_small.h"

namespace {

constexpr int BV_NMAX = 64, BV_RMAX = 96, BV_LD = BV_NMAX + 1;

__device__ __forceinline__ bool bv_finite(double v) { return fabs(v) < __builtin_huge_val(); }

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmin(v, __shfl_xor(v, m, 64));
  return v;
}

// gram = G^T G (n x n) of the matrix blockIdx.y (r x n each, one after the other; so are the Gram matrices and the status
// words): block j, thread k, ascending rows; every block also looks at every entry of G
__global__ __launch_bounds__(BV_NMAX) void k_bvls_gram(const double* __restrict__ G, int n, int r, double* __restrict__ gram, int* status) {
  const int j = blockIdx.x, k = threadIdx.x;
  if (k >= n) return;
  G += size_t(blockIdx.y) * r * n, gram += size_t(blockIdx.y) * n * n, status += blockIdx.y;
  bool bad = false;
  double s = 0.0;
  for (int i = 0; i < r; ++i) {
    const double gk = G[size_t(i) * n + k];
    bad |= !bv_finite(gk);
    s = fma(G[size_t(i) * n + j], gk, s);
  }
  gram[j * n + k] = s;
  if (bad) atomicOr(status, 1);
}

struct BvSys {
  int n, r;
  const double *G, *gram;   // r x n and n x n, row-major, global or LDS
  int* status;              // bit 1 is set when a pivot of the free Gram block is not positive
  // LDS: H BV_LD n; invd, c, z, v, gn n each; part 256; ps, rs r each (ps holds p); flag 2
  double *H, *invd, *c, *z, *v, *gn, *part, *ps, *rs, *flag;
  int *st, *barred, *idx, *ctl;   // n each and ctl 3: the pass was infeasible; nothing left to free; free columns
  int nf = 0;
  unsigned long long factorisations = 0;

  // rs = p - G v  (r rows, 16 lanes per row: columns q, q + 16, .. by fma, then the butterfly)
  __device__ void residual() {
    const int tid = threadIdx.x, q = tid & 15;
    for (int row = tid >> 4; row < (r + 15) / 16 * 16; row += 16) {
      double s = 0.0;
      if (row < r)
        for (int j = q; j < n; j += 16) s = fma(G[size_t(row) * n + j], v[j], s);
      s = group16_sum(s);
      if (row < r && q == 0) rs[row] = ps[row] - s;
    }
    __syncthreads();
  }

  // v = G^T rs  (lane = column; wave w takes the rows w, w + 4, .. by fma; the four partial sums are added in wave order)
  __device__ void gradient() {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    double s = 0.0;
    if (lane < n)
      for (int i = w; i < r; i += 4) s = fma(G[size_t(i) * n + lane], rs[i], s);
    part[tid] = s;
    __syncthreads();
    if (tid < n) v[tid] = ((part[tid] + part[64 + tid]) + part[128 + tid]) + part[192 + tid];
    __syncthreads();
  }

  // wave 0: x = (L D L^T)^-1 (v on the free columns); lane = position among the free columns
  __device__ double solve(int lane) const {
    double b[1] = {lane < nf ? v[idx[lane]] : 0.0};
    lm_solve<1>(H, BV_LD, nf, invd, b, lane);
    return b[0];
  }

  // py:_bvls_solve with rhs = p - G (c on the bound columns): z = the solution on the free columns, c on the bound ones
  __device__ void least_squares() {
    const int tid = threadIdx.x;
    if (tid < 64) {
      const bool is_free = tid < n && st[tid] == 0;
      const unsigned long long free_mask = __ballot(is_free);
      if (is_free) idx[__popcll(free_mask & ((1ull << tid) - 1ull))] = tid;
      if (tid == 0) ctl[2] = __popcll(free_mask);
    }
    if (tid < n) v[tid] = st[tid] == 0 ? 0.0 : c[tid];
    __syncthreads();
    nf = ctl[2];
    for (int x = tid; x < nf * nf; x += LMS_THREADS) {
      const int i = x / nf, k = x - i * nf;
      if (k <= i) H[i * BV_LD + k] = gram[idx[i] * n + idx[k]];
    }
    __syncthreads();
    if (!lm_factor(H, BV_LD, nf, invd, flag) && tid == 0) atomicOr(status, 2);
    factorisations += 1;
    residual();
    gradient();
    if (tid < 64) {
      const double x = solve(tid);
      if (tid < nf) z[idx[tid]] = x;
      if (tid < n && st[tid] != 0) z[tid] = c[tid];
    }
    __syncthreads();
    if (tid < n) v[tid] = z[tid];
    __syncthreads();
    residual();
    gradient();
    if (tid < 64) {
      const double x = solve(tid);
      if (tid < nf) z[idx[tid]] += x;
    }
    __syncthreads();
  }

  // The whole iteration from p in ps: c and st afterwards (lo, hi: the bounds of column `lane`, whatever beyond n).  Returns
  // the passes made; *conv: the Karush-Kuhn-Tucker conditions were reached.
  __device__ int run(double lo, double hi, int max_iter, bool* conv_out) {
    const int tid = threadIdx.x, lane = tid & 63;
    const bool in = tid < n;   // (of wave 0: this lane has a column)
    if (in) {
      gn[tid] = sqrt(gram[tid * n + tid]);
      st[tid] = 0, barred[tid] = 0, c[tid] = 0.0;
    }
    __syncthreads();
    least_squares();   // py:`start`
    if (in) {
      const double x = z[tid];
      c[tid] = fmin(fmax(x, lo), hi);
      st[tid] = (lo == hi || x <= lo) ? -1 : (x >= hi ? 1 : 0);
    }
    __syncthreads();

    int passes = 0, freed = -1, side = 0;   // (freed, side: wave 0's)
    bool conv = false;
    for (int it = 0; it < max_iter && !conv; ++it) {
      passes += 1;
      least_squares();
      if (tid < 64) {
#pragma clang fp contract(off)   // (the step c + alpha (z - c) as the host forms it)
        const int s_old = in ? st[lane] : 0;
        const bool F = in && s_old == 0;
        const double zj = in ? z[lane] : 0.0, cj = in ? c[lane] : 0.0;
        const bool below = F && zj < lo, above = F && zj > hi;
        const bool infeasible = __ballot(below || above) != 0ull;
        if (infeasible) {   // py:`infeasible`: to the first bound on the segment; what hits it is bound
          const double ratio = below ? (cj - lo) / (cj - zj) : (above ? (hi - cj) / (zj - cj) : __builtin_huge_val());
          const double alpha = wave_min(ratio);
          double cn = cj;
          int s = s_old;
          if (F) {
            cn = fmin(fmax(cj + alpha * (zj - cj), lo), hi);
            if (ratio == alpha) cn = below ? lo : hi;
            s = cn == lo ? -1 : (cn == hi ? 1 : 0);
          }
          const unsigned long long changed = __ballot(s != s_old);
          const int fs = __shfl(s, freed >= 0 ? freed : 0, 64);
          const bool same = freed >= 0 && ((changed >> freed) & 1ull) && fs == side;
          const unsigned long long others = same ? changed & ~(1ull << freed) : changed;
          if (in) {
            if (others) barred[lane] = 0;
            if (same && lane == freed) barred[lane] = 1;
            c[lane] = cn, st[lane] = s;
          }
          freed = -1;
        } else if (in) {   // py:`~infeasible`: the solution is taken (a free variable exactly on a bound: bound)
          c[lane] = zj, v[lane] = zj;
          if (F) st[lane] = zj == lo ? -1 : (zj == hi ? 1 : 0);
        }
        if (lane == 0) ctl[0] = infeasible ? 1 : 0;
      }
      __syncthreads();
      if (ctl[0] == 0) {
        residual();
        gradient();   // v = G^T (p - G c) = -g
        if (tid < 64) {
          if (freed >= 0 && in) barred[lane] = 0;   // the variable freed in the last pass has stayed free
          const int s = in ? st[lane] : 0;
          double viol = 0.0;
          if (in && s != 0 && lo != hi && !barred[lane]) {
            const double x = (s < 0 ? v[lane] : -v[lane]) / gn[lane];
            viol = x > 0.0 ? x : 0.0;
          }
          const double worst = wave_max_nan(viol);
          const unsigned long long at = __ballot(viol == worst && worst > 0.0);
          freed = -1;
          if (at) {   // the lowest index among equals
            freed = __ffsll((long long)at) - 1;
            side = __shfl(s, freed, 64);
            if (lane == freed) st[lane] = 0;
          }
          if (lane == 0) ctl[1] = at ? 0 : 1;
        }
        __syncthreads();
        conv = ctl[1] != 0;
      }
    }
    *conv_out = conv;
    return passes;
  }

  // ||p - G c||^2 in every lane of wave 0 (the other waves: 0)
  __device__ double misfit2() {
    const int tid = threadIdx.x;
    if (tid < n) v[tid] = c[tid];
    __syncthreads();
    residual();
    double f = 0.0;
    if (tid < 64) {
      for (int i = tid; i < r; i += 64) f = fma(rs[i], rs[i], f);
      f = wave_sum(f);
    }
    return f;
  }
};

}  // namespace
