// rom_lm_polish: the Levenberg-Marquardt polish of the library-based parameter estimation on the device -- a port, line for
// line, of romhighcontrast_amd/inverse.py::polish_parameters (cited below as `py:NN`, the line numbers of that file) to reduced
// sensor coordinates: with the compact SVD diag(w) E^T = U S V^T of rank r, p = U^T (w y) and G_r = S V^T (r x n),
//     ||w (y - E^T c)||^2 = ||p - G_r c||^2 + perp2,   perp2 = ||(I - U U^T)(w y)||^2,   J = U J_r,  J_r = G_r X,
// so the device works on r <= n rows instead of m and J_r has the singular values of J.
//
// One SYSTEM is one pair (query, start); k_lm_polish runs one workgroup of 256 threads per system and the whole iteration inside
// the launch.  In LDS: A (n x n, row stride n | 1: an odd stride of doubles keeps a column read by 32 lanes on 32 different bank
// pairs), the right-hand sides / solutions X ((k + 1) x n), J_r (k columns of r), J^T J and the damped k x k system, and the
// vectors.  Ahat (k n^2 doubles) and G_r are read through L2.  At the limits (n = 64, k = 16, r = 64) that is 58.6 KB: inside
// the default 64 KB of dynamic LDS, no opt-in.
// The iteration itself is lm_drive (rom_lm_drive.h, with the contract on control flow); LmSys below is its model.
//
// A(theta) is factored as L D L^T without pivoting (the elimination order of k_reduced_solve, rom_ops.hip); the solves keep a
// right-hand side in the registers of one wave, lane = row.  The factor in LDS is that of the CURRENT theta whenever an iteration
// starts (an iteration that goes on ended with an accepted trial, whose factor is the last one made), so the Jacobian costs no
// factorisation; only the final Jacobian of a system whose last trial was rejected factors again.
// sigma_min of the final J_r: one-sided (Hestenes) Jacobi on its k columns -- not the eigenvalues of J^T J, which lose every
// singular value below sqrt(eps) sigma_max.
#include <cmath>
#include <cstring>
#include <type_traits>

#include "rom_lm_drive.h"
#include "rom_lm_eval.h"

namespace {

constexpr int LM_NMAX = 64, LM_KMAX = 16, LM_RMAX = 64, LM_TMAX = 8;
constexpr int LM_THREADS = LMS_THREADS;
constexpr double LM_NAN = __builtin_nan("");

struct LmBox {
  double lo[LM_KMAX], hi[LM_KMAX];
};

struct LmArgs {
  int n, k, r, t, max_iter;
  const double* Ahat;    // k n n
  const double* bhat;    // n
  const double* Gr;      // r n
  const double* P;       // query rows, ldp apart
  long long ldp;
  const double* theta0;  // K t k
  const double* aux;     // K x 2 (perp2, scale) or null
  double misfit_tol;
  double* W;             // per system: theta (k) | c (n) | misfit | sigma_min | converged | iterations
  int ldw;
  unsigned long long* counters;   // LM iterations, factorisations
  int* status;
};

// the LDS map, in doubles (host and device)
struct LmLds {
  int ldn, ldr, ldk;
  int As, Xs, Js, JtJ, Hs, invd, cs, cn, rho, rhon, ps, th, thn, ea, g, hinv, scal, total;
  __host__ __device__ LmLds(int n, int k, int r) {
    ldn = n | 1, ldr = r | 1, ldk = k | 1;
    int at = 0;
    auto take = [&](int cnt) {
      const int o = at;
      at += cnt;
      return o;
    };
    As = take(n * ldn), Xs = take((k + 1) * ldn), Js = take(k * ldr), JtJ = take(k * ldk), Hs = take(k * ldk);
    invd = take(n), cs = take(n), cn = take(n), rho = take(r), rhon = take(r), ps = take(r);
    th = take(k), thn = take(k), ea = take(k), g = take(k), hinv = take(k);
    scal = take(8);   // the slots LMS_* of rom_lm_drive.h
    total = at;
  }
};

struct LmSys {
  const LmArgs& a;
  const LmLds& m;
  const LmBox& box;
  double* sm;
  unsigned long long factorisations = 0;
  bool factor_current = true;   // the factor in As is that of the current theta (see the head of the file)
  __device__ LmSys(const LmArgs& a_, const LmLds& m_, const LmBox& box_, double* sm_) : a(a_), m(m_), box(box_), sm(sm_) {}
  __device__ int cols() const { return a.k; }
  __device__ unsigned long long work() const { return factorisations; }

  // py:51-58 without the Jacobian: c(theta) -> cn, rho = p - G_r c -> rhon, |rho|^2 -> scal[LMS_FN]; theta from sm[thx ..).
  // Returns whether every pivot of A(theta) was positive (otherwise cn, rhon and fn mean nothing).
  __device__ bool eval(int thx) {
    factorisations += 1;
    return lm_eval(sm, m, a.n, a.k, a.r, a.Ahat, a.bhat, a.Gr, thx);   // (rom_lm_eval.h, shared with k_mcmc)
  }

  // py:59-61 and py:97-98 at the current theta (th), its c (cs), its rho and ITS FACTOR in As: X = A^-1 [e^theta_q Ahat_q c]_q,
  // J_r = G_r X -> Js (column q at Js + q ldr), J^T J -> JtJ, g = J^T rho
  __device__ void jacobian() {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n = a.n, k = a.k, r = a.r, l16 = tid & 15;
    double* As = sm + m.As;
    double* Xs = sm + m.Xs;
    double* Js = sm + m.Js;
    if (tid < k) sm[m.ea + tid] = exp(sm[m.th + tid]);   // (a rejected trial has overwritten ea)
    __syncthreads();
    const int rows = k * n;
    for (int row0 = 0; row0 < rows; row0 += 16) {   // py:59: 16 lanes per row (q, i) of Ahat
      const int row = row0 + (tid >> 4);
      double s = 0.0;
      if (row < rows)
        for (int j = l16; j < n; j += 16) s = fma(a.Ahat[size_t(row) * n + j], sm[m.cs + j], s);
      s = group16_sum(s);
      if (row < rows && l16 == 0) {
        const int q = row / n, i = row - q * n;
        Xs[(1 + q) * m.ldn + i] = sm[m.ea + q] * s;
      }
    }
    __syncthreads();
    // py:60: wave w solves the columns w, w + 4, ..
    auto solve_cols = [&](auto tag) {
      constexpr int NR = decltype(tag)::value;
      double b[NR];
#pragma unroll
      for (int u = 0; u < NR; ++u) {
        const int q = w + 4 * u;
        b[u] = (q < k && lane < n) ? Xs[(1 + q) * m.ldn + lane] : 0.0;
      }
      lm_solve<NR>(As, m.ldn, n, sm + m.invd, b, lane);
#pragma unroll
      for (int u = 0; u < NR; ++u) {
        const int q = w + 4 * u;
        if (q < k && lane < n) Xs[(1 + q) * m.ldn + lane] = b[u];
      }
    };
    if (k <= 4) solve_cols(std::integral_constant<int, 1>{});
    else if (k <= 8) solve_cols(std::integral_constant<int, 2>{});
    else solve_cols(std::integral_constant<int, 4>{});
    __syncthreads();
    for (int i0 = 0; i0 < r; i0 += 16) {   // py:61
      const int i = i0 + (tid >> 4);
      double gv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) gv[u] = (i < r && l16 + 16 * u < n) ? a.Gr[size_t(i) * n + l16 + 16 * u] : 0.0;
      for (int q = 0; q < k; ++q) {
        double s = 0.0;
#pragma unroll
        for (int u = 0; u < 4; ++u) s = fma(gv[u], l16 + 16 * u < n ? Xs[(1 + q) * m.ldn + l16 + 16 * u] : 0.0, s);
        s = group16_sum(s);
        if (i < r && l16 == 0) Js[q * m.ldr + i] = s;
      }
    }
    __syncthreads();
    for (int e = tid; e < k * k; e += LM_THREADS) {   // py:97
      const int q = e / k, p = e - q * k;
      double s = 0.0;
      for (int i = 0; i < r; ++i) s = fma(Js[q * m.ldr + i], Js[p * m.ldr + i], s);
      sm[m.JtJ + q * m.ldk + p] = s;
    }
    if (tid < k) {   // py:98
      double s = 0.0;
      for (int i = 0; i < r; ++i) s = fma(Js[tid * m.ldr + i], sm[m.rho + i], s);
      sm[m.g + tid] = s;
    }
    __syncthreads();
  }

  // py:107-109: the clipped trial theta (lane = parameter) from the step b
  __device__ void step(double b, int lane) {
    double moved = 0.0, mx = 0.0;
    if (lane < a.k) {
      const double old = sm[m.th + lane], v = old - b;
      const double nw = v < box.lo[lane] ? box.lo[lane] : (v > box.hi[lane] ? box.hi[lane] : v);
      sm[m.thn + lane] = nw;
      moved = fabs(nw - old);
      mx = fabs(nw);
    }
    moved = wave_max_nan(moved);
    mx = wave_max_nan(mx);
    if (lane == 0) {
      sm[m.scal + LMS_MOVED] = moved;
      sm[m.scal + LMS_MAXNEW] = mx;
    }
  }
  __device__ bool trial() {   // (its factor replaces that of the current theta)
    factor_current = false;
    return eval(m.thn);
  }
  __device__ void keep() {   // py:114-115
    const int tid = threadIdx.x;
    if (tid < a.k) sm[m.th + tid] = sm[m.thn + tid];
    if (tid < a.n) sm[m.cs + tid] = sm[m.cn + tid];
    if (tid < a.r) sm[m.rho + tid] = sm[m.rhon + tid];
    factor_current = true;
  }
  // c, rho and f are the accepted ones; a factor left by a rejected trial is remade
  __device__ void refresh() {
    if (factor_current) return;
    const bool ok = eval(m.th);   // (the same operations as when this theta was accepted: the same bits)
    if (!ok && threadIdx.x == 0) atomicOr(a.status, 1);
  }
  __device__ int head(double* out) const {   // theta | c
    const int tid = threadIdx.x;
    if (tid < a.k) out[tid] = sm[m.th + tid];
    if (tid < a.n) out[a.k + tid] = sm[m.cs + tid];
    return a.k + a.n;
  }
  // the smallest singular value of J_r (Js is overwritten): one-sided Jacobi on its k columns, wave 0, lane = row
  __device__ double sigma_min(int lane) { return lm_sigma_min_wave<1>(sm + m.Js, m.ldr, a.k, a.r, lane); }
};

__global__ __launch_bounds__(LM_THREADS) void k_lm_polish(const LmArgs a, const LmBox box) {
  extern __shared__ __align__(16) double lm_lds[];
  double* sm = lm_lds;
  const LmLds m(a.n, a.k, a.r);
  const int tid = threadIdx.x, n = a.n, k = a.k, r = a.r;
  const long long sys = blockIdx.x, query = sys / a.t;
  LmSys S(a, m, box, sm);
  double* out = a.W + size_t(sys) * a.ldw;

  // py:81-84: the query's row, the clipped start, the scale
  if (tid < r) sm[m.ps + tid] = a.P[query * a.ldp + tid];
  if (tid < k) {
    const double v = a.theta0[size_t(sys) * k + tid];
    sm[m.th + tid] = v < box.lo[tid] ? box.lo[tid] : (v > box.hi[tid] ? box.hi[tid] : v);
  }
  __syncthreads();
  double perp2;
  const double scale = lm_scale(a.aux, query, sm + m.ps, r, perp2);

  // py:85-86
  if (!S.eval(m.th)) {   // a start whose A(theta) is not positive definite: the call fails
    if (tid == 0) atomicOr(a.status, 1);
    for (int e = tid; e < a.ldw; e += LM_THREADS) out[e] = LM_NAN;
    return;
  }
  if (tid < n) sm[m.cs + tid] = sm[m.cn + tid];
  if (tid < r) sm[m.rho + tid] = sm[m.rhon + tid];
  lm_drive(S, perp2, scale, out);   // py:87-132
}

// py:130-133: per query the start of smallest misfit: k_lm_select (rom_lm_small.h)

}  // namespace

extern "C" int rom_lm_polish(rom_ctx* ctx, int n, int k, int r, rom_buf* Ahat, rom_buf* bhat, rom_buf* Gr, rom_buf* P, size_t p_off,
                             int64_t ldp, int K, int t, rom_buf* THETA0, const double* lo_host, const double* hi_host, rom_buf* AUX,
                             int max_iter, double misfit_tol, rom_buf* OUT, size_t out_off, int64_t ldo, double* info8_host) {
  ROM_CHECK(ctx && Ahat && bhat && Gr && lo_host && hi_host, "rom_lm_polish: null argument (context, Ahat, bhat, Gr, lo or hi)");
  ROM_CHECK(n >= 1 && n <= LM_NMAX, "rom_lm_polish: n = %d reduced unknowns, between 1 and %d", n, LM_NMAX);
  ROM_CHECK(k >= 1 && k <= LM_KMAX, "rom_lm_polish: k = %d parameters, between 1 and %d", k, LM_KMAX);
  ROM_CHECK(r >= 1 && r <= LM_RMAX, "rom_lm_polish: r = %d sensor coordinates, between 1 and %d", r, LM_RMAX);
  ROM_CHECK(Ahat->n >= size_t(k) * n * n && bhat->n >= size_t(n) && Gr->n >= size_t(r) * n,
            "rom_lm_polish: Ahat, bhat or Gr holds fewer than k n n = %zu, n = %d, r n = %zu doubles", size_t(k) * n * n, n, size_t(r) * n);
  const LmLds map(n, k, r);
  const size_t lds = size_t(map.total) * sizeof(double);
  ROM_CHECK(lds <= 64 * 1024, "rom_lm_polish: %zu bytes of LDS", lds);   // (58.6 KB at the limits)

  LmBox box;
  for (int q = 0; q < LM_KMAX; ++q) {
    box.lo[q] = q < k ? lo_host[q] : 0.0;
    box.hi[q] = q < k ? hi_host[q] : 0.0;
  }
  const LmCall call = {"rom_lm_polish", r, K, t, LM_TMAX, max_iter, k, k + n, "THETA0", "k", "k + n", P, THETA0, AUX, OUT, p_off, out_off,
                       ldp, ldo, info8_host, "lm_select", "A(theta) not positive definite at a start", ROM_ERR_NOT_SPD};
  return lm_launch(ctx, call, [&](double* W, int ldw, unsigned long long* counters) {
    LmArgs a;
    a.n = n, a.k = k, a.r = r, a.t = t, a.max_iter = max_iter;
    a.Ahat = Ahat->p, a.bhat = bhat->p, a.Gr = Gr->p, a.P = P->p + p_off, a.ldp = ldp;
    a.theta0 = THETA0->p, a.aux = AUX ? AUX->p : nullptr, a.misfit_tol = misfit_tol;
    a.W = W, a.ldw = ldw, a.counters = counters, a.status = ctx->d_status;
    char nm[48];
    rom_prof_name(nm, sizeof nm, "lm_polish", "_n%d_k%d_r%d", n, k, r);
    ROM_PROF(ctx, nm, 0.0, 0.0);
    k_lm_polish<<<K * t, LM_THREADS, lds, ctx->stream>>>(a, box);
  });
}
