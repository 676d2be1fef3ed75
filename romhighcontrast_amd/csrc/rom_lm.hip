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
// Every control decision is taken by all threads from the same LDS values: control flow is uniform within a workgroup (every
// __syncthreads is reached by all 256 threads) and free between workgroups.  Every loop is bounded by max_iter, LM_TRIALS, n, k,
// r or LMS_SWEEPS; nothing waits on another workgroup.  No floating-point atomics: a repeated call returns the same bits.
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

#include "rom_basis_int.h"
#include "rom_lm_small.h"

namespace {

constexpr int LM_NMAX = 64, LM_KMAX = 16, LM_RMAX = 64, LM_TMAX = 8;
constexpr int LM_TRIALS = 8;     // py:101
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
    scal = take(8);   // fn | moved | max |new| | flag of the A factor | flag of the H factor
    total = at;
  }
};
enum { S_FN = 0, S_MOVED = 1, S_MAXNEW = 2, S_OKA = 3, S_OKH = 4 };

struct LmSys {
  const LmArgs& a;
  const LmLds& m;
  double* sm;
  unsigned long long factorisations = 0;
  __device__ LmSys(const LmArgs& a_, const LmLds& m_, double* sm_) : a(a_), m(m_), sm(sm_) {}

  // py:51-58 without the Jacobian: c(theta) -> cn, rho = p - G_r c -> rhon, |rho|^2 -> scal[S_FN]; theta from sm[thx ..).
  // Returns whether every pivot of A(theta) was positive (otherwise cn, rhon and fn mean nothing).
  __device__ bool eval(int thx) {
    const int tid = threadIdx.x, lane = tid & 63, n = a.n, k = a.k, r = a.r, l16 = tid & 15;
    double* As = sm + m.As;
    if (tid < k) sm[m.ea + tid] = exp(sm[thx + tid]);   // py:53
    __syncthreads();
    for (int idx = tid; idx < n * n; idx += LM_THREADS) {   // py:54
      const int row = idx / n, col = idx - row * n;
      double s = 0.0;
      for (int q = 0; q < k; ++q) s = fma(sm[m.ea + q], a.Ahat[size_t(q) * n * n + idx], s);
      As[row * m.ldn + col] = s;
    }
    __syncthreads();
    const bool ok = lm_factor(As, m.ldn, n, sm + m.invd, sm + m.scal + S_OKA);
    factorisations += 1;
    if (tid < 64) {   // py:55
      double b[1] = {lane < n ? a.bhat[lane] : 0.0};
      lm_solve<1>(As, m.ldn, n, sm + m.invd, b, lane);
      if (lane < n) sm[m.cn + lane] = b[0];
    }
    __syncthreads();
    for (int i0 = 0; i0 < r; i0 += 16) {   // py:56: 16 lanes per row of G_r
      const int i = i0 + (tid >> 4);
      double s = 0.0;
      if (i < r)
        for (int j = l16; j < n; j += 16) s = fma(a.Gr[size_t(i) * n + j], sm[m.cn + j], s);
      s = group16_sum(s);
      if (i < r && l16 == 0) sm[m.rhon + i] = sm[m.ps + i] - s;
    }
    __syncthreads();
    if (tid < 64) {
      const double v = lane < r ? sm[m.rhon + lane] : 0.0;
      const double f = wave_sum(v * v);
      if (lane == 0) sm[m.scal + S_FN] = f;
    }
    __syncthreads();
    return ok;
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

  // the smallest singular value of J_r (Js is overwritten): one-sided Jacobi on its k columns, wave 0, lane = row
  __device__ double sigma_min_wave0(int lane) { return lm_sigma_min_wave<1>(sm + m.Js, m.ldr, a.k, a.r, lane); }
};

__global__ __launch_bounds__(LM_THREADS) void k_lm_polish(const LmArgs a, const LmBox box) {
  extern __shared__ __align__(16) double lm_lds[];
  double* sm = lm_lds;
  const LmLds m(a.n, a.k, a.r);
  const int tid = threadIdx.x, lane = tid & 63, n = a.n, k = a.k, r = a.r;
  const long long sys = blockIdx.x, query = sys / a.t;
  LmSys S(a, m, sm);
  double* out = a.W + size_t(sys) * a.ldw;

  // py:81-84: the query's row, the clipped start, the scale
  if (tid < r) sm[m.ps + tid] = a.P[query * a.ldp + tid];
  if (tid < k) {
    const double v = a.theta0[size_t(sys) * k + tid];
    sm[m.th + tid] = v < box.lo[tid] ? box.lo[tid] : (v > box.hi[tid] ? box.hi[tid] : v);
  }
  __syncthreads();
  double perp2 = 0.0, scale;
  if (a.aux) {
    perp2 = a.aux[2 * query];
    scale = a.aux[2 * query + 1];
  } else {
    scale = 0.0;
    for (int i = 0; i < r; ++i) scale = fmax(scale, fabs(sm[m.ps + i]));
  }
  scale = fmax(scale, 2.2250738585072014e-308);

  // py:85-86
  if (!S.eval(m.th)) {   // a start whose A(theta) is not positive definite: the call fails
    if (tid == 0) atomicOr(a.status, 1);
    for (int e = tid; e < a.ldw; e += LM_THREADS) out[e] = LM_NAN;
    return;
  }
  if (tid < n) sm[m.cs + tid] = sm[m.cn + tid];
  if (tid < r) sm[m.rho + tid] = sm[m.rhon + tid];
  double f = sm[m.scal + S_FN], lam = 1e-3;   // py:87
  bool active = a.max_iter > 0, stationary = false, factor_current = true;
  int iterations = 0;
  __syncthreads();

  for (int it = 0; it < a.max_iter && active; ++it) {   // py:91
    iterations += 1;                                    // py:95
    S.jacobian();                                       // py:96-98 (factor_current holds here, see the head of the file)
    double dmax = 0.0;                                  // py:99, py:105
    for (int q = 0; q < k; ++q) {
      const double d = sm[m.JtJ + q * m.ldk + q];
      dmax = (d > dmax || d != d) ? d : dmax;
    }
    bool todo = true;
    for (int trial = 0; trial < LM_TRIALS && todo; ++trial) {   // py:101
      if (tid < k * k) {                                        // py:105-106
        const int q = tid / k, p = tid - q * k;
        double h = sm[m.JtJ + q * m.ldk + p];
        if (p == q) h += lam * (h + 1e-300) + 1e-30 * dmax;
        sm[m.Hs + q * m.ldk + p] = h;
      }
      __syncthreads();
      const bool ok_h = lm_factor(sm + m.Hs, m.ldk, k, sm + m.hinv, sm + m.scal + S_OKH);
      if (!ok_h) {   // a damped system that is not positive definite has no step: a rejected trial
        lam *= 4.0;
        continue;
      }
      if (tid < 64) {   // py:107-109
        double b[1] = {lane < k ? sm[m.g + lane] : 0.0};
        lm_solve<1>(sm + m.Hs, m.ldk, k, sm + m.hinv, b, lane);
        double moved = 0.0, mx = 0.0;
        if (lane < k) {
          const double old = sm[m.th + lane], v = old - b[0];
          const double nw = v < box.lo[lane] ? box.lo[lane] : (v > box.hi[lane] ? box.hi[lane] : v);
          sm[m.thn + lane] = nw;
          moved = fabs(nw - old);
          mx = fabs(nw);
        }
        moved = wave_max_nan(moved);
        mx = wave_max_nan(mx);
        if (lane == 0) {
          sm[m.scal + S_MOVED] = moved;
          sm[m.scal + S_MAXNEW] = mx;
        }
      }
      __syncthreads();
      const bool ok_a = S.eval(m.thn);   // py:110-111; a non-positive pivot counts as a rejected trial
      factor_current = false;
      const double fn = sm[m.scal + S_FN], moved = sm[m.scal + S_MOVED], mx = sm[m.scal + S_MAXNEW];
      const bool ok = ok_a && fn < f;                        // py:112
      const bool still = moved <= 1e-13 * (1.0 + mx);        // py:113
      __syncthreads();   // (everyone has read the scalars and ok before the vectors move)
      if (ok) {                                              // py:114-116
        if (tid < k) sm[m.th + tid] = sm[m.thn + tid];
        if (tid < n) sm[m.cs + tid] = sm[m.cn + tid];
        if (tid < r) sm[m.rho + tid] = sm[m.rhon + tid];
        f = fn;
        lam = fmax(lam / 3.0, 1e-12);
        factor_current = true;
      } else {
        lam *= 4.0;                                          // py:117
      }
      const bool tiny = ok && moved <= 1e-10 * (1.0 + mx);   // py:119
      // py:120: the host's f holds the whole misfit; here perp2 is the part outside the range of U
      const bool done = still || tiny || sqrt(f + perp2) <= 1e-14 * scale;
      if (done) {                                            // py:121-122
        stationary = true;
        active = false;
      }
      if (ok || done) todo = false;                          // py:123
      __syncthreads();
    }
    if (todo) {   // py:124-126
      stationary = true;
      active = false;
    }
  }

  // py:127-129: the Jacobian at the final theta.  c, rho and f are the accepted ones; a factor left by a rejected trial is remade
  if (!factor_current) {
    const bool ok = S.eval(m.th);   // (the same operations as when this theta was accepted: the same bits)
    if (!ok && tid == 0) atomicOr(a.status, 1);
  }
  S.jacobian();
  const double misfit = sqrt(f + perp2);
  if (tid < k) out[tid] = sm[m.th + tid];
  if (tid < n) out[k + tid] = sm[m.cs + tid];
  if (tid < 64) {
    const double smin = S.sigma_min_wave0(lane);
    if (lane == 0) {
      const bool conv = (stationary || misfit <= 1e-14 * scale) && misfit <= a.misfit_tol * scale;   // py:132
      out[k + n] = misfit;
      out[k + n + 1] = smin;
      out[k + n + 2] = conv ? 1.0 : 0.0;
      out[k + n + 3] = double(iterations);
      atomicAdd(a.counters, (unsigned long long)iterations);
      atomicAdd(a.counters + 1, S.factorisations);
    }
  }
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
  ROM_CHECK(t >= 1 && t <= LM_TMAX, "rom_lm_polish: t = %d starts per query, between 1 and %d", t, LM_TMAX);
  ROM_CHECK(K >= 0 && int64_t(K) * t <= (int64_t(1) << 30), "rom_lm_polish: K = %d queries (K t at most 2^30)", K);
  ROM_CHECK(max_iter >= 0, "rom_lm_polish: max_iter = %d", max_iter);
  ROM_CHECK(ldo >= int64_t(k) + n + 5, "rom_lm_polish: ldo = %lld < k + n + 5 = %d", (long long)ldo, k + n + 5);
  ROM_CHECK(Ahat->n >= size_t(k) * n * n && bhat->n >= size_t(n) && Gr->n >= size_t(r) * n,
            "rom_lm_polish: Ahat, bhat or Gr holds fewer than k n n = %zu, n = %d, r n = %zu doubles", size_t(k) * n * n, n, size_t(r) * n);
  if (info8_host) std::fill(info8_host, info8_host + 8, 0.0);
  if (K == 0) return ROM_OK;
  ROM_CHECK(P && THETA0 && OUT, "rom_lm_polish: null argument (P, THETA0 or OUT)");
  ROM_CHECK(ldp >= r, "rom_lm_polish: ldp = %lld < r = %d", (long long)ldp, r);
  ROM_CHECK(p_off + size_t(K - 1) * size_t(ldp) + size_t(r) <= P->n,
            "rom_lm_polish: P holds %zu doubles, %d rows of %d at offset %zu with stride %lld need more", P->n, K, r, p_off, (long long)ldp);
  ROM_CHECK(THETA0->n >= size_t(K) * t * k, "rom_lm_polish: THETA0 holds %zu doubles, K t k = %zu needed", THETA0->n, size_t(K) * t * k);
  ROM_CHECK(!AUX || AUX->n >= 2 * size_t(K), "rom_lm_polish: AUX holds %zu doubles, 2 K = %zu needed", AUX ? AUX->n : 0, 2 * size_t(K));
  ROM_CHECK(out_off + size_t(K - 1) * size_t(ldo) + size_t(k + n + 5) <= OUT->n,
            "rom_lm_polish: OUT holds %zu doubles, %d rows of %d at offset %zu with stride %lld need more", OUT->n, K, k + n + 5, out_off,
            (long long)ldo);
  const LmLds map(n, k, r);
  const size_t lds = size_t(map.total) * sizeof(double);
  ROM_CHECK(lds <= 64 * 1024, "rom_lm_polish: %zu bytes of LDS", lds);   // (58.6 KB at the limits)
  ROM_HIP(hipSetDevice(ctx->device));

  LmBox box;
  for (int q = 0; q < LM_KMAX; ++q) {
    box.lo[q] = q < k ? lo_host[q] : 0.0;
    box.hi[q] = q < k ? hi_host[q] : 0.0;
  }
  const int B = K * t, ldw = k + n + 4;
  Tmp ws;
  const size_t ws_doubles = size_t(B) * ldw + 2;
  ROM_TRY(ws.get(ctx, ws_doubles));
  unsigned long long* counters = reinterpret_cast<unsigned long long*>(ws.p() + size_t(B) * ldw);
  ROM_HIP(hipMemsetAsync(counters, 0, 2 * sizeof(unsigned long long), ctx->stream));
  ROM_HIP(hipMemsetAsync(ctx->d_status, 0, sizeof(int), ctx->stream));
  LmArgs a;
  a.n = n, a.k = k, a.r = r, a.t = t, a.max_iter = max_iter;
  a.Ahat = Ahat->p, a.bhat = bhat->p, a.Gr = Gr->p, a.P = P->p + p_off, a.ldp = ldp;
  a.theta0 = THETA0->p, a.aux = AUX ? AUX->p : nullptr, a.misfit_tol = misfit_tol;
  a.W = ws.p(), a.ldw = ldw, a.counters = counters, a.status = ctx->d_status;
  {
    char nm[48];
    rom_prof_name(nm, sizeof nm, "lm_polish", "_n%d_k%d_r%d", n, k, r);
    ROM_PROF(ctx, nm, 0.0, 0.0);
    k_lm_polish<<<B, LM_THREADS, lds, ctx->stream>>>(a, box);
  }
  ROM_HIP(hipGetLastError());
  {
    ROM_PROF(ctx, "lm_select", 0.0, 8.0 * double(B) * ldw);
    k_lm_select<<<K, 64, 0, ctx->stream>>>(ws.p(), ldw, t, k + n, OUT->p + out_off, ldo);
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
    info8_host[3] = B;
    info8_host[4] = double(hc[0]);
    info8_host[5] = double(hc[1]);
  }
  if (status) {
    rom_set_error("rom_lm_polish: A(theta) not positive definite at a start");
    return ROM_ERR_NOT_SPD;
  }
  return ROM_OK;
}
