// rom_bvls: box-constrained least squares  min over lo <= c <= hi of ||p - G_r c||^2  for K right-hand sides p and one shared
// G_r (r x n, full column rank) -- a port, decision for decision, of romhighcontrast_amd/inverse.py::bvls_host (cited below as
// `py:` with the names of that function): Stark-Parker BVLS from the clipped unconstrained solution, with the anti-cycling rule.
//
// One workgroup of 256 threads per system, the whole active-set iteration in one launch; n <= 64 is one lane per column, so every
// decision of a pass (feasibility, the step to the first bound, the multiplier to free, the bars) is taken by wave 0 with
// ballots and wave reductions, written to LDS, and read from there by all 256 threads: control flow is uniform within a
// workgroup, free between workgroups.  Every loop is bounded by max_iter, n or r; nothing waits on another workgroup.  No
// floating-point atomics and one fixed order in every sum: a repeated call returns the same bits.
//
// A pass (py:_bvls_solve): the Gram block of the free columns -- packed to the front in ascending order by a ballot, which gives
// the factor the host gets from the identity rows it puts in the place of the bound ones, without their elimination steps -- is
// factored in LDS (L D L^T, lm_factor of rom_lm_small.h, all four waves) and solved by wave 0 (lm_solve); one refinement step
// follows with the residual formed on the columns of G_r themselves, so the error of c is that of a least-squares solve, not of
// the bare normal equations.
// G^T G is formed once per call by k_bvls_gram (shared by every system).  G_r (at most 48 KB) and G^T G (32 KB) are read through
// L2: with G_r in LDS beside the 33 KB factor a CU would hold one workgroup; here the LDS is 40.2 KB and four fit.
#include <cmath>

#include "rom_basis_int.h"
#include "rom_block.h"
#include "rom_lm_small.h"

namespace {

constexpr int BV_NMAX = 64, BV_RMAX = 96, BV_LD = BV_NMAX + 1;

struct BvBox {
  double lo[BV_NMAX], hi[BV_NMAX];
};

struct BvArgs {
  int n, r, max_iter;
  const double *G, *gram, *Pq, *aux;
  long long ldp, ldo;
  double *OUT, *BOUND;
  unsigned long long* counters;   // passes, factorisations
  int* status;                    // bit 0: NaN / Inf in an operand; bit 1: a pivot of the free Gram block is not positive
};

__device__ __forceinline__ bool bv_finite(double v) { return fabs(v) < __builtin_huge_val(); }

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmin(v, __shfl_xor(v, m, 64));
  return v;
}

// gram = G^T G (n x n): block j, thread k, ascending rows; every block also looks at every entry of G
__global__ __launch_bounds__(BV_NMAX) void k_bvls_gram(const double* __restrict__ G, int n, int r, double* __restrict__ gram, int* status) {
  const int j = blockIdx.x, k = threadIdx.x;
  if (k >= n) return;
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
  const BvArgs& a;
  double *H, *invd, *c, *z, *v, *gn, *part, *ps, *rs, *flag;
  int *st, *idx, *nfree;   // the state; the free columns in ascending order and their number
  int nf = 0;
  unsigned long long factorisations = 0;

  // rs = p - G v  (r rows, 16 lanes per row: columns q, q + 16, .. by fma, then the butterfly)
  __device__ void residual() {
    const int tid = threadIdx.x, q = tid & 15, n = a.n, r = a.r;
    for (int row = tid >> 4; row < (r + 15) / 16 * 16; row += 16) {
      double s = 0.0;
      if (row < r)
        for (int j = q; j < n; j += 16) s = fma(a.G[size_t(row) * n + j], v[j], s);
      s = group16_sum(s);
      if (row < r && q == 0) rs[row] = ps[row] - s;
    }
    __syncthreads();
  }

  // v = G^T rs  (lane = column; wave w takes the rows w, w + 4, .. by fma; the four partial sums are added in wave order)
  __device__ void gradient() {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n = a.n, r = a.r;
    double s = 0.0;
    if (lane < n)
      for (int i = w; i < r; i += 4) s = fma(a.G[size_t(i) * n + lane], rs[i], s);
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
    const int tid = threadIdx.x, n = a.n;
    if (tid < 64) {
      const bool is_free = tid < n && st[tid] == 0;
      const unsigned long long free_mask = __ballot(is_free);
      if (is_free) idx[__popcll(free_mask & ((1ull << tid) - 1ull))] = tid;
      if (tid == 0) *nfree = __popcll(free_mask);
    }
    if (tid < n) v[tid] = st[tid] == 0 ? 0.0 : c[tid];
    __syncthreads();
    nf = *nfree;
    for (int x = tid; x < nf * nf; x += LMS_THREADS) {
      const int i = x / nf, k = x - i * nf;
      if (k <= i) H[i * BV_LD + k] = a.gram[idx[i] * n + idx[k]];
    }
    __syncthreads();
    if (!lm_factor(H, BV_LD, nf, invd, flag) && tid == 0) atomicOr(a.status, 2);
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
};

__global__ __launch_bounds__(LMS_THREADS) void k_bvls(const BvArgs a, const BvBox box) {
  __shared__ double H[BV_NMAX * BV_LD];
  __shared__ double invd[BV_NMAX], c[BV_NMAX], z[BV_NMAX], v[BV_NMAX], gn[BV_NMAX], part[LMS_THREADS], ps[BV_RMAX], rs[BV_RMAX], flag[2];
  __shared__ int st[BV_NMAX], barred[BV_NMAX], idx[BV_NMAX], ctl[3];   // ctl: the pass was infeasible; nothing left to free; free columns
  const int tid = threadIdx.x, lane = tid & 63, n = a.n, r = a.r;
  const long long sys = blockIdx.x;
  BvSys S = {a, H, invd, c, z, v, gn, part, ps, rs, flag, st, idx, ctl + 2};
  const bool in = tid < n;   // (of wave 0: this lane has a column)
  const double lo = box.lo[lane], hi = box.hi[lane];

  if (tid < r) {
    const double p = a.Pq[sys * a.ldp + tid];
    if (!bv_finite(p)) atomicOr(a.status, 1);
    ps[tid] = p;
  }
  if (in) {
    gn[tid] = sqrt(a.gram[tid * n + tid]);
    st[tid] = 0, barred[tid] = 0, c[tid] = 0.0;
  }
  __syncthreads();
  S.least_squares();   // py:`start`
  if (in) {
    const double x = z[tid];
    c[tid] = fmin(fmax(x, lo), hi);
    st[tid] = (lo == hi || x <= lo) ? -1 : (x >= hi ? 1 : 0);
  }
  __syncthreads();

  int passes = 0, freed = -1, side = 0;   // (freed, side: wave 0's)
  bool conv = false;
  for (int it = 0; it < a.max_iter && !conv; ++it) {
    passes += 1;
    S.least_squares();
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
      S.residual();
      S.gradient();   // v = G^T (p - G c) = -g
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

  if (in) v[tid] = c[tid];
  __syncthreads();
  S.residual();
  if (tid < 64) {
    double f = 0.0;
    for (int i = lane; i < r; i += 64) f = fma(rs[i], rs[i], f);
    f = wave_sum(f);
    const unsigned long long nb = __ballot(in && st[lane] != 0);
    double* out = a.OUT + sys * a.ldo;
    if (in) {
      out[lane] = c[lane];
      if (a.BOUND) a.BOUND[sys * n + lane] = double(st[lane]);
    }
    if (lane == 0) {
      out[n] = sqrt(f + (a.aux ? a.aux[2 * sys] : 0.0));
      out[n + 1] = double(__popcll(nb));
      out[n + 2] = conv ? 1.0 : 0.0;
      out[n + 3] = double(passes);
      atomicAdd(a.counters, (unsigned long long)passes);
      atomicAdd(a.counters + 1, S.factorisations);
    }
  }
}

}  // namespace

extern "C" int rom_bvls(rom_ctx* ctx, int n, int r, rom_buf* Gr, rom_buf* P, size_t p_off, int64_t ldp, int K, const double* lo_host,
                        const double* hi_host, rom_buf* AUX, int max_iter, rom_buf* OUT, size_t out_off, int64_t ldo, rom_buf* BOUND,
                        double* info8_host) {
  ROM_CHECK(ctx && Gr && lo_host && hi_host, "rom_bvls: null argument (context, Gr, lo or hi)");
  ROM_CHECK(n >= 1 && n <= BV_NMAX, "rom_bvls: n = %d unknowns, between 1 and %d", n, BV_NMAX);
  ROM_CHECK(r >= n && r <= BV_RMAX, "rom_bvls: r = %d rows, between n = %d and %d", r, n, BV_RMAX);
  ROM_CHECK(Gr->n >= size_t(r) * n, "rom_bvls: Gr holds %zu doubles, r n = %zu needed", Gr->n, size_t(r) * n);
  ROM_CHECK(K >= 0 && K <= (1 << 30), "rom_bvls: K = %d right-hand sides (at most 2^30)", K);
  ROM_CHECK(max_iter >= 0, "rom_bvls: max_iter = %d", max_iter);
  ROM_CHECK(ldo >= int64_t(n) + 4, "rom_bvls: ldo = %lld < n + 4 = %d", (long long)ldo, n + 4);
  BvBox box;
  for (int j = 0; j < BV_NMAX; ++j) {
    box.lo[j] = j < n ? lo_host[j] : 0.0;
    box.hi[j] = j < n ? hi_host[j] : 0.0;
    // (a NaN fails the comparison; lo = +inf or hi = -inf leaves no finite point)
    ROM_CHECK(box.lo[j] <= box.hi[j] && box.lo[j] < __builtin_huge_val() && box.hi[j] > -__builtin_huge_val(),
              "rom_bvls: the box needs lo <= hi without NaN, coordinate %d has [%g, %g]", j, box.lo[j], box.hi[j]);
  }
  if (info8_host) std::fill(info8_host, info8_host + 8, 0.0);
  if (K == 0) return ROM_OK;
  ROM_CHECK(P && OUT, "rom_bvls: null argument (P or OUT)");
  ROM_TRY(rom_check_block("rom_bvls", {"P", "ldp", "r"}, P->n, p_off, ldp, r, K));
  ROM_CHECK(!AUX || AUX->n >= 2 * size_t(K), "rom_bvls: AUX holds %zu doubles, 2 K = %zu needed", AUX ? AUX->n : 0, 2 * size_t(K));
  ROM_TRY(rom_check_block("rom_bvls", {"OUT", "ldo", "n + 4"}, OUT->n, out_off, ldo, n + 4, K));   // (ldo >= n + 4: checked above)
  ROM_CHECK(!BOUND || BOUND->n >= size_t(K) * n, "rom_bvls: BOUND holds %zu doubles, K n = %zu needed", BOUND ? BOUND->n : 0, size_t(K) * n);
  ROM_HIP(hipSetDevice(ctx->device));

  Tmp ws;
  const size_t ws_doubles = size_t(n) * n + 2;
  ROM_TRY(ws.get(ctx, ws_doubles));
  unsigned long long* counters = reinterpret_cast<unsigned long long*>(ws.p() + size_t(n) * n);
  ROM_HIP(hipMemsetAsync(counters, 0, 2 * sizeof(unsigned long long), ctx->stream));
  ROM_HIP(hipMemsetAsync(ctx->d_status, 0, sizeof(int), ctx->stream));
  {
    ROM_PROF(ctx, "bvls_gram", 2.0 * r * n * n, 8.0 * r * n);
    k_bvls_gram<<<n, BV_NMAX, 0, ctx->stream>>>(Gr->p, n, r, ws.p(), ctx->d_status);
  }
  ROM_HIP(hipGetLastError());
  {
    BvArgs a;
    a.n = n, a.r = r, a.max_iter = max_iter;
    a.G = Gr->p, a.gram = ws.p(), a.Pq = P->p + p_off, a.aux = AUX ? AUX->p : nullptr, a.ldp = ldp, a.ldo = ldo;
    a.OUT = OUT->p + out_off, a.BOUND = BOUND ? BOUND->p : nullptr, a.counters = counters, a.status = ctx->d_status;
    char nm[48];
    rom_prof_name(nm, sizeof nm, "bvls", "_n%d_r%d", n, r);
    ROM_PROF(ctx, nm, 0.0, 0.0);
    k_bvls<<<K, LMS_THREADS, 0, ctx->stream>>>(a, box);
  }
  ROM_HIP(hipGetLastError());
  unsigned long long hc[2] = {0, 0};
  int status = 0;
  ROM_HIP(hipMemcpyAsync(hc, counters, sizeof hc, hipMemcpyDeviceToHost, ctx->stream));
  ROM_HIP(hipMemcpyAsync(&status, ctx->d_status, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  ROM_HIP(hipStreamSynchronize(ctx->stream));
  if (info8_host) {
    info8_host[0] = 2;   // launches
    info8_host[1] = 1;   // host synchronisations
    info8_host[2] = double(ws_doubles) * sizeof(double);
    info8_host[3] = K;
    info8_host[4] = double(hc[0]);
    info8_host[5] = double(hc[1]);
  }
  if (status) {
    // (reported once: the word is cleared, or the next call on this context -- whatever it is -- would report this failure again)
    ROM_HIP(hipMemsetAsync(ctx->d_status, 0, sizeof(int), ctx->stream));
    rom_set_error("rom_bvls: %s", (status & 1) ? "NaN / Inf in Gr or P" : "Gr has no full column rank (a pivot of G^T G is not positive)");
    return ROM_ERR_INVALID;
  }
  return ROM_OK;
}
