// rom_mcmc: batched posterior sampling of the parameters of the reduced model -- a port, step for step, of
// romhighcontrast_amd/inverse.py::mcmc_host (cited below as `spec N`, the numbered steps of that function's docstring) in the reduced
// sensor coordinates of rom_lm_polish: theta = log a in the box [lo, hi]^k with a uniform prior, the potential
// Phi(theta) = ||p - G_r c(theta)||^2, the log-posterior -invvar Phi / 2 inside the box.
//
// One CHAIN is one pair (query, chain index); k_mcmc runs one workgroup of 256 threads per chain and the loop over the steps inside
// the launch: adaptive random-walk Metropolis (Robbins-Monro on the log of the proposal scale during burn-in, frozen afterwards),
// one evaluation of the model per proposal inside the box (lm_eval of rom_lm_eval.h, the evaluation of k_lm_polish), the draws from
// Philox4x32-10 keyed by (seed; step, chain id, purpose) (rom_philox.h), Welford moments of theta and the running mean of c.
// In LDS: A (n x n, row stride n | 1), the vectors of the evaluation, the k draws, the query's proposal factor L, the mean, M2 and
// the mean of c: 42 KB at the limits (n = 64, k = 16, r = 64), inside the default 64 KB of dynamic LDS, no opt-in.
//
// Control flow follows the contract at the head of rom_lm_drive.h: every decision is taken by all threads from the same LDS values
// (the scalars of a chain -- Phi, the scale, the counters -- are held by every thread, computed from the same operands); every loop is
// bounded by `steps` or the sizes of the system.  No floating-point atomics: the same bits on a repeated call.  The whole state of a
// chain is its row of STATE, so a call split at any step -- by rom_mcmc itself, which launches at most MC_LAUNCH_STEPS steps at a
// time, or by the caller through step0 -- returns the bits of the unsplit call: a launch that resumes evaluates the model at the
// row's theta once more, which are the operations that accepted it.
#include <cmath>
#include <cstring>

#include "rom_basis_int.h"
#include "rom_block.h"
#include "rom_lm_eval.h"
#include "rom_philox.h"

namespace {

constexpr int MC_NMAX = 64, MC_KMAX = 16, MC_RMAX = 64, MC_TMAX = 8;
constexpr int MC_THREADS = LMS_THREADS;
constexpr int MC_LAUNCH_STEPS = 1024;   // steps per launch: no launch runs for seconds
constexpr double MC_NAN = __builtin_nan("");
enum { MCS_OUTSIDE = 5, MCS_LOGU = 6 };   // the chain's own slots of `scal` beside LMS_FN and LMS_OKA

struct McBox {
  double lo[MC_KMAX], hi[MC_KMAX];
};

// the state row of a chain, in doubles (host and device): rom_mcmc_layout
struct McRow {
  int theta, phi, ls, mean, M2, meanc, kept, accepted, outside, notspd, phimin, thmin, total;
  __host__ __device__ McRow(int n, int k) {
    theta = 0, phi = k, ls = k + 1, mean = k + 2, M2 = mean + k, meanc = M2 + k * k;
    kept = meanc + n, accepted = kept + 1, outside = kept + 2, notspd = kept + 3, phimin = kept + 4, thmin = kept + 5;
    total = thmin + k;
  }
};

struct McArgs {
  int n, k, r, t;
  const double* Ahat;     // k n n
  const double* bhat;     // n
  const double* Gr;       // r n
  const double* P;        // query rows, ldp apart
  long long ldp;
  const double* invvar;   // K
  const double* Lprop;    // K k k
  unsigned long long seed;
  long long chain0, step0;
  int steps, burn, thin;
  double* STATE;
  long long lds;
  double* SAMPLES;        // [chain][slot][k] or null
  long long slots;
  unsigned long long* counters;   // steps taken, evaluations
  int* status;
};

// the LDS map, in doubles (host and device)
struct McLds {
  int ldn;
  int As, invd, cs, cn, rhon, ps, th, thn, ea, xi, L, mean, M2, meanc, dl, dn, thmin, scal, total;
  __host__ __device__ McLds(int n, int k, int r) {
    ldn = n | 1;
    int at = 0;
    auto take = [&](int cnt) {
      const int o = at;
      at += cnt;
      return o;
    };
    As = take(n * ldn), invd = take(n), cs = take(n), cn = take(n), rhon = take(r), ps = take(r);
    th = take(k), thn = take(k), ea = take(k), xi = take(2 * ((k + 1) / 2)), L = take(k * k);
    mean = take(k), M2 = take(k * k), meanc = take(n), dl = take(k), dn = take(k), thmin = take(k);
    scal = take(8);
    total = at;
  }
};

__global__ __launch_bounds__(MC_THREADS) void k_mcmc(const McArgs a, const McBox box) {
  extern __shared__ __align__(16) double mc_lds[];
  double* sm = mc_lds;
  const McLds m(a.n, a.k, a.r);
  const McRow o(a.n, a.k);
  const int tid = threadIdx.x, lane = tid & 63, n = a.n, k = a.k, r = a.r, kh = (k + 1) >> 1;
  const long long sys = blockIdx.x, query = sys / a.t;
  const unsigned long long chain = (unsigned long long)(a.chain0 + sys);
  const bool fresh = a.step0 == 0;
  double* row = a.STATE + size_t(sys) * a.lds;

  // the query's row and proposal factor; the start clipped to the box, or the row an earlier launch left
  if (tid < r) sm[m.ps + tid] = a.P[query * a.ldp + tid];
  if (tid < k) {
    const double v = row[o.theta + tid];
    sm[m.th + tid] = !fresh ? v : (v < box.lo[tid] ? box.lo[tid] : (v > box.hi[tid] ? box.hi[tid] : v));
    sm[m.mean + tid] = fresh ? 0.0 : row[o.mean + tid];
    sm[m.thmin + tid] = fresh ? 0.0 : row[o.thmin + tid];
  }
  if (tid < n) sm[m.meanc + tid] = fresh ? 0.0 : row[o.meanc + tid];
  for (int e = tid; e < k * k; e += MC_THREADS) {
    sm[m.L + e] = a.Lprop[size_t(query) * k * k + e];
    sm[m.M2 + e] = fresh ? 0.0 : row[o.M2 + e];
  }
  __syncthreads();
  if (!fresh && sm[m.th] != sm[m.th]) return;   // a row that an earlier launch filled with NaN stays (the status is raised once)

  unsigned long long evals = 1;
  const bool ok0 = lm_eval(sm, m, n, k, r, a.Ahat, a.bhat, a.Gr, m.th);
  double phi = sm[m.scal + LMS_FN];
  if (!ok0 || phi != phi) {
    // A(theta_0) is not positive definite: the call fails; NaN in the query: the chain has no posterior.  Either way a NaN row.
    if (!ok0 && tid == 0) atomicOr(a.status, 1);
    for (int e = tid; e < o.total; e += MC_THREADS) row[e] = MC_NAN;
    return;
  }
  if (tid < n) sm[m.cs + tid] = sm[m.cn + tid];
  if (fresh && tid < k) sm[m.thmin + tid] = sm[m.th + tid];
  double ls = fresh ? 0.0 : row[o.ls], kept = fresh ? 0.0 : row[o.kept], accepted = fresh ? 0.0 : row[o.accepted];
  double outside = fresh ? 0.0 : row[o.outside], notspd = fresh ? 0.0 : row[o.notspd], phimin = fresh ? phi : row[o.phimin];
  double s = exp(ls);
  const double invvar = a.invvar[query];
  __syncthreads();

  for (int it = 0; it < a.steps; ++it) {
    const long long i = a.step0 + it;
    // spec 1: the draws
    if (tid < kh) {
      double z0, z1;
      rom_mcmc_normal_pair(a.seed, chain, uint32_t(i), uint32_t(tid), z0, z1);
      sm[m.xi + 2 * tid] = z0;
      sm[m.xi + 2 * tid + 1] = z1;
    } else if (tid == kh) {
      sm[m.scal + MCS_LOGU] = log(rom_mcmc_accept_uniform(a.seed, chain, uint32_t(i)));
    }
    __syncthreads();
    // spec 2, 3: the proposal (lane = coordinate), and whether it left the box
    if (tid < 64) {
      bool out = false;
      if (lane < k) {
        double v = 0.0;
        for (int p = 0; p <= lane; ++p) v = fma(sm[m.L + lane * k + p], sm[m.xi + p], v);
        const double old = sm[m.th + lane];
        const double nw = box.lo[lane] == box.hi[lane] ? old : old + s * v;
        sm[m.thn + lane] = nw;
        out = !(nw >= box.lo[lane] && nw <= box.hi[lane]);
      }
      const unsigned long long any = __ballot(out);
      if (lane == 0) sm[m.scal + MCS_OUTSIDE] = any ? 1.0 : 0.0;
    }
    __syncthreads();
    // spec 3, 4: the decision
    double alpha = 0.0, phin = phi;
    bool accept = false;
    if (sm[m.scal + MCS_OUTSIDE] != 0.0) {
      outside += 1.0;
    } else {
      evals += 1;
      if (!lm_eval(sm, m, n, k, r, a.Ahat, a.bhat, a.Gr, m.thn)) {
        notspd += 1.0;
      } else {
        phin = sm[m.scal + LMS_FN];
        const double l = -0.5 * invvar * (phin - phi);
        if (l == l) {
          accept = sm[m.scal + MCS_LOGU] < l;
          alpha = fmin(1.0, exp(fmin(l, 0.0)));
        }
      }
    }
    if (accept) {
      if (tid < k) sm[m.th + tid] = sm[m.thn + tid];
      if (tid < n) sm[m.cs + tid] = sm[m.cn + tid];
      phi = phin;
    }
    __syncthreads();   // (everyone has read the scalars of this step; the state has moved)
    if (i < a.burn) {   // spec 5
      ls += pow(double(i + 1), -0.6) * (alpha - 0.234);
      s = exp(ls);
    } else {            // spec 6
      kept += 1.0;
      if (accept) accepted += 1.0;
      if (tid < k) {
        const double x = sm[m.th + tid], d = x - sm[m.mean + tid], mu = sm[m.mean + tid] + d / kept;
        sm[m.mean + tid] = mu;
        sm[m.dl + tid] = d;
        sm[m.dn + tid] = x - mu;
        if (phi < phimin) sm[m.thmin + tid] = x;
        const long long j = i - a.burn;
        if (a.SAMPLES && j % a.thin == a.thin - 1 && j / a.thin < a.slots)
          a.SAMPLES[(size_t(sys) * size_t(a.slots) + size_t(j / a.thin)) * k + tid] = x;
      } else if (tid >= 64 && tid - 64 < n) {
        const int j = tid - 64;
        sm[m.meanc + j] += (sm[m.cs + j] - sm[m.meanc + j]) / kept;
      }
      if (phi < phimin) phimin = phi;
      __syncthreads();
      for (int e = tid; e < k * k; e += MC_THREADS) {
        const int q = e / k, p = e - q * k;
        sm[m.M2 + e] = fma(sm[m.dl + q], sm[m.dn + p], sm[m.M2 + e]);
      }
    }
  }
  __syncthreads();

  // the row
  if (tid < k) {
    row[o.theta + tid] = sm[m.th + tid];
    row[o.mean + tid] = sm[m.mean + tid];
    row[o.thmin + tid] = sm[m.thmin + tid];
  }
  if (tid < n) row[o.meanc + tid] = sm[m.meanc + tid];
  for (int e = tid; e < k * k; e += MC_THREADS) row[o.M2 + e] = sm[m.M2 + e];
  if (tid == 0) {
    row[o.phi] = phi;
    row[o.ls] = ls;
    row[o.kept] = kept;
    row[o.accepted] = accepted;
    row[o.outside] = outside;
    row[o.notspd] = notspd;
    row[o.phimin] = phimin;
    atomicAdd(a.counters, (unsigned long long)a.steps);
    atomicAdd(a.counters + 1, evals);
  }
}

}  // namespace

extern "C" int rom_mcmc_layout(int n, int k, int64_t* out8) {
  ROM_CHECK(out8, "rom_mcmc_layout: null argument");
  ROM_CHECK(n >= 1 && n <= MC_NMAX && k >= 1 && k <= MC_KMAX, "rom_mcmc_layout: n = %d, k = %d, 1 <= n <= %d and 1 <= k <= %d", n, k,
            MC_NMAX, MC_KMAX);
  const McRow o(n, k);
  const int64_t v[8] = {o.total, o.phi, o.ls, o.mean, o.M2, o.meanc, o.kept, o.phimin};
  std::memcpy(out8, v, sizeof v);
  return ROM_OK;
}

extern "C" int rom_mcmc(rom_ctx* ctx, int n, int k, int r, rom_buf* Ahat, rom_buf* bhat, rom_buf* Gr, rom_buf* P, size_t p_off, int64_t ldp,
                        int K, int t, rom_buf* INVVAR, rom_buf* LPROP, const double* lo_host, const double* hi_host, int64_t seed,
                        int64_t chain0, int64_t step0, int steps, int burn, int thin, rom_buf* STATE, size_t s_off, int64_t lds,
                        rom_buf* SAMPLES, size_t smp_off, int64_t slots, double* info8_host) {
  ROM_CHECK(ctx && Ahat && bhat && Gr && lo_host && hi_host, "rom_mcmc: null argument (context, Ahat, bhat, Gr, lo or hi)");
  ROM_CHECK(n >= 1 && n <= MC_NMAX, "rom_mcmc: n = %d reduced unknowns, between 1 and %d", n, MC_NMAX);
  ROM_CHECK(k >= 1 && k <= MC_KMAX, "rom_mcmc: k = %d parameters, between 1 and %d", k, MC_KMAX);
  ROM_CHECK(r >= 1 && r <= MC_RMAX, "rom_mcmc: r = %d sensor coordinates, between 1 and %d", r, MC_RMAX);
  ROM_CHECK(t >= 1 && t <= MC_TMAX, "rom_mcmc: t = %d chains per query, between 1 and %d", t, MC_TMAX);
  ROM_CHECK(K >= 0 && int64_t(K) * t <= (int64_t(1) << 30), "rom_mcmc: K = %d queries (K t at most 2^30)", K);
  ROM_CHECK(steps >= 0 && burn >= 0 && thin >= 1, "rom_mcmc: steps = %d, burn = %d, thin = %d (steps >= 0, burn >= 0, thin >= 1)", steps, burn,
            thin);
  ROM_CHECK(step0 >= 0 && step0 <= (int64_t(1) << 31) - steps, "rom_mcmc: step0 = %lld (0 <= step0, step0 + steps at most 2^31)",
            (long long)step0);
  ROM_CHECK(chain0 >= 0, "rom_mcmc: chain0 = %lld", (long long)chain0);
  ROM_CHECK(Ahat->n >= size_t(k) * n * n && bhat->n >= size_t(n) && Gr->n >= size_t(r) * n,
            "rom_mcmc: Ahat, bhat or Gr holds fewer than k n n = %zu, n = %d, r n = %zu doubles", size_t(k) * n * n, n, size_t(r) * n);
  const McLds map(n, k, r);
  const McRow o(n, k);
  const size_t lds_bytes = size_t(map.total) * sizeof(double);
  ROM_CHECK(lds_bytes <= 64 * 1024, "rom_mcmc: %zu bytes of LDS", lds_bytes);   // (42 KB at the limits)
  ROM_CHECK(lds >= int64_t(o.total), "rom_mcmc: lds = %lld < the state row = %d", (long long)lds, o.total);
  if (info8_host) std::fill(info8_host, info8_host + 8, 0.0);
  if (K == 0) return ROM_OK;
  const int B = K * t;
  ROM_CHECK(P && INVVAR && LPROP && STATE, "rom_mcmc: null argument (P, INVVAR, LPROP or STATE)");
  ROM_TRY(rom_check_block("rom_mcmc", {"P", "ldp", "r"}, P->n, p_off, ldp, r, K));
  ROM_CHECK(INVVAR->n >= size_t(K) && LPROP->n >= size_t(K) * k * k, "rom_mcmc: INVVAR or LPROP holds fewer than K = %d, K k k = %zu doubles",
            K, size_t(K) * k * k);
  ROM_TRY(rom_check_block("rom_mcmc", {"STATE", "lds", "its row"}, STATE->n, s_off, lds, o.total, B));
  if (SAMPLES) {
    ROM_CHECK(slots >= 0 && slots <= (int64_t(1) << 26), "rom_mcmc: slots = %lld, between 0 and 2^26", (long long)slots);
    if (slots > 0) ROM_TRY(rom_check_block("rom_mcmc", {"SAMPLES", "slots k", "slots k"}, SAMPLES->n, smp_off, slots * k, int(slots * k), B));
  }
  ROM_HIP(hipSetDevice(ctx->device));

  McBox box;
  for (int q = 0; q < MC_KMAX; ++q) {
    box.lo[q] = q < k ? lo_host[q] : 0.0;
    box.hi[q] = q < k ? hi_host[q] : 0.0;
  }
  Tmp ws;
  ROM_TRY(ws.get(ctx, 2));
  unsigned long long* counters = reinterpret_cast<unsigned long long*>(ws.p());
  ROM_HIP(hipMemsetAsync(counters, 0, 2 * sizeof(unsigned long long), ctx->stream));
  ROM_HIP(hipMemsetAsync(ctx->d_status, 0, sizeof(int), ctx->stream));
  McArgs a;
  a.n = n, a.k = k, a.r = r, a.t = t;
  a.Ahat = Ahat->p, a.bhat = bhat->p, a.Gr = Gr->p, a.P = P->p + p_off, a.ldp = ldp;
  a.invvar = INVVAR->p, a.Lprop = LPROP->p, a.seed = uint64_t(seed), a.chain0 = chain0;
  a.burn = burn, a.thin = thin, a.STATE = STATE->p + s_off, a.lds = lds;
  a.SAMPLES = (SAMPLES && slots > 0) ? SAMPLES->p + smp_off : nullptr, a.slots = slots;
  a.counters = counters, a.status = ctx->d_status;
  char nm[48];
  rom_prof_name(nm, sizeof nm, "mcmc", "_n%d_k%d_r%d", n, k, r);
  int launches = 0;
  for (int64_t done = 0; done < steps || launches == 0; done += MC_LAUNCH_STEPS) {   // (steps = 0: the start and its Phi)
    a.step0 = step0 + done;
    a.steps = int(steps - done < MC_LAUNCH_STEPS ? steps - done : MC_LAUNCH_STEPS);
    ROM_PROF(ctx, nm, 0.0, 0.0);
    k_mcmc<<<B, MC_THREADS, lds_bytes, ctx->stream>>>(a, box);
    launches += 1;
  }
  ROM_HIP(hipGetLastError());
  unsigned long long hc[2] = {0, 0};
  int status = 0;
  ROM_HIP(hipMemcpyAsync(hc, counters, sizeof hc, hipMemcpyDeviceToHost, ctx->stream));
  ROM_HIP(hipMemcpyAsync(&status, ctx->d_status, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  ROM_HIP(hipStreamSynchronize(ctx->stream));
  if (info8_host) {
    info8_host[0] = launches;
    info8_host[1] = 1;   // host synchronisations
    info8_host[2] = 2.0 * sizeof(double);
    info8_host[3] = B;
    info8_host[4] = double(hc[0]);
    info8_host[5] = double(hc[1]);
  }
  if (status) {
    // (reported once: the word is cleared, or the next call on this context -- whatever it is -- would report this failure again)
    ROM_HIP(hipMemsetAsync(ctx->d_status, 0, sizeof(int), ctx->stream));
    rom_set_error("rom_mcmc: A(theta) not positive definite at a start");
    return ROM_ERR_NOT_SPD;
  }
  return ROM_OK;
}
