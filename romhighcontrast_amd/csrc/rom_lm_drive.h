// The Levenberg-Marquardt iteration of the batched kernels (rom_lm.hip: k_lm_polish, rom_sense.hip: k_sense, rom_mlp_sense.hip:
// k_mlp_sense, the last two through rom_sense_sys.h) and the host side
// that their entry points share -- a port, line for line, of romhighcontrast_amd/inverse.py::polish_parameters (cited below as
// `py:NN`, the line numbers of that file; nonlinear.py::sense_scores runs the same loop on another model).  (internal)
//
// One workgroup of 256 threads takes one system through lm_drive.  Every control decision is taken by all threads from the same
// LDS values: control flow is uniform within a workgroup (every __syncthreads is reached by all 256 threads) and free between
// workgroups.  Every loop is bounded by max_iter, LM_TRIALS, the sizes of the system or LMS_SWEEPS; nothing waits on another
// workgroup.  No floating-point atomics: a repeated call returns the same bits.
//
// A system type Sys (LmSys, SnSys<feature policy>) supplies the model:
//   a, m, sm          its arguments (max_iter, misfit_tol, counters), its LDS map (JtJ, Hs, ldk, hinv, g, scal) and the LDS
//   cols()            the number of free columns of the Jacobian
//   jacobian()        J, J^T J -> JtJ and g = J^T rho at the current point
//   step(b, lane)     wave 0, lane = column: the trial point from the solved step b; moved -> scal[LMS_MOVED], max |new| ->
//                     scal[LMS_MAXNEW]
//   trial()           the model at the trial point: its residual, |rho|^2 -> scal[LMS_FN]; false: the point is not usable
//   keep()            the trial point becomes the current one
//   refresh()         before the final Jacobian: remakes what a rejected last trial has overwritten
//   head(out)         writes the leading part of the output row, returns its length
//   sigma_min(lane)   wave 0: the smallest singular value of the final J
//   work()            its work counter
#pragma once
#include "rom_basis_int.h"
#include "rom_block.h"
#include "rom_lm_small.h"

namespace {

constexpr int LM_TRIALS = 8;   // py:101
// (the slots LMS_* of `scal`: rom_lm_small.h)

// py:84: perp2 and the scale of a query from aux, or 0 and max |p| of its row ps; the scale is at least the smallest normal
__device__ __forceinline__ double lm_scale(const double* aux, long long query, const double* ps, int r, double& perp2) {
  double scale = 0.0;
  perp2 = 0.0;
  if (aux) {
    perp2 = aux[2 * query];
    scale = aux[2 * query + 1];
  } else {
    for (int i = 0; i < r; ++i) scale = fmax(scale, fabs(ps[i]));
  }
  return fmax(scale, 2.2250738585072014e-308);
}

// From a current point whose residual and |rho|^2 (scal[LMS_FN]) the caller has made to the output row of the system:
// head | misfit | sigma_min | converged | iterations
template <class Sys>
__device__ void lm_drive(Sys& S, double perp2, double scale, double* out) {
  double* sm = S.sm;
  const auto& m = S.m;
  const int tid = threadIdx.x, lane = tid & 63, k = S.cols(), max_iter = S.a.max_iter;
  double f = sm[m.scal + LMS_FN], lam = 1e-3;   // py:87
  bool active = max_iter > 0, stationary = false;
  int iterations = 0;
  const auto reject = [&lam] { lam *= 4.0; };   // py:117, for either reason a trial is rejected for
  __syncthreads();

  for (int it = 0; it < max_iter && active; ++it) {   // py:91
    iterations += 1;                                  // py:95
    S.jacobian();                                     // py:96-98
    double dmax = 0.0;                                // py:99, py:105
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
      if (!lm_factor(sm + m.Hs, m.ldk, k, sm + m.hinv, sm + m.scal + LMS_OKH)) {
        reject();   // a damped system that is not positive definite has no step
        continue;
      }
      if (tid < 64) {   // py:107-109
        double b[1] = {lane < k ? sm[m.g + lane] : 0.0};
        lm_solve<1>(sm + m.Hs, m.ldk, k, sm + m.hinv, b, lane);
        S.step(b[0], lane);
      }
      __syncthreads();
      const bool usable = S.trial();   // py:110-111; a point that is not usable counts as a rejected trial
      const double fn = sm[m.scal + LMS_FN], moved = sm[m.scal + LMS_MOVED], mx = sm[m.scal + LMS_MAXNEW];
      const bool ok = usable && fn < f;                      // py:112
      const bool still = moved <= 1e-13 * (1.0 + mx);        // py:113
      __syncthreads();   // (everyone has read the scalars and ok before the vectors move)
      if (ok) {                                              // py:114-116
        S.keep();
        f = fn;
        lam = fmax(lam / 3.0, 1e-12);
      } else {
        reject();
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
    if (todo) {   // py:124-126: stuck
      stationary = true;
      active = false;
    }
  }

  // py:127-129: the Jacobian at the final point; the residual and f are the accepted ones
  S.refresh();
  S.jacobian();
  const double misfit = sqrt(f + perp2);
  double* tail = out + S.head(out);
  if (tid < 64) {
    const double smin = S.sigma_min(lane);
    if (lane == 0) {
      const bool conv = (stationary || misfit <= 1e-14 * scale) && misfit <= S.a.misfit_tol * scale;   // py:132
      tail[0] = misfit;
      tail[1] = smin;
      tail[2] = conv ? 1.0 : 0.0;
      tail[3] = double(iterations);
      atomicAdd(S.a.counters, (unsigned long long)iterations);
      atomicAdd(S.a.counters + 1, S.work());
    }
  }
}

// ---- the host side -------------------------------------------------------------------------------------------------------------
// What rom_lm_polish, rom_poly_sense and rom_mlp_sense pass to lm_launch after the checks of their own model.  A start is `width` doubles (named
// width_name in the messages), an output row `lead` doubles (lead_name) | misfit | sigma_min | converged | iterations | start.
struct LmCall {
  const char* who;
  int r, K, t, tmax, max_iter;
  int width, lead;
  const char *starts_name, *width_name, *lead_name;
  rom_buf *P, *STARTS, *AUX, *OUT;
  size_t p_off, out_off;
  int64_t ldp, ldo;
  double* info8_host;
  const char *select_name, *failure;   // the profiler's name of k_lm_select; what a raised status word means
  int failure_code;
};

// The shared checks, the workspace (a row of lead + 4 doubles per system, two counters behind them), `launch(W, ldw, counters)` for
// the caller's system kernel, k_lm_select, one read-back of the counters and the status word, info8
template <class Launch>
int lm_launch(rom_ctx* ctx, const LmCall& c, Launch&& launch) {
  const int K = c.K, t = c.t, r = c.r, row = c.lead + 5;
  ROM_CHECK(t >= 1 && t <= c.tmax, "%s: t = %d starts per query, between 1 and %d", c.who, t, c.tmax);
  ROM_CHECK(K >= 0 && int64_t(K) * t <= (int64_t(1) << 30), "%s: K = %d queries (K t at most 2^30)", c.who, K);
  ROM_CHECK(c.max_iter >= 0, "%s: max_iter = %d", c.who, c.max_iter);
  ROM_CHECK(c.ldo >= int64_t(row), "%s: ldo = %lld < %s + 5 = %d", c.who, (long long)c.ldo, c.lead_name, row);
  if (c.info8_host) std::fill(c.info8_host, c.info8_host + 8, 0.0);
  if (K == 0) return ROM_OK;
  ROM_CHECK(c.P && c.STARTS && c.OUT, "%s: null argument (P, %s or OUT)", c.who, c.starts_name);
  ROM_TRY(rom_check_block(c.who, {"P", "ldp", "r"}, c.P->n, c.p_off, c.ldp, r, K));
  ROM_CHECK(c.STARTS->n >= size_t(K) * t * c.width, "%s: %s holds %zu doubles, K t %s = %zu needed", c.who, c.starts_name, c.STARTS->n,
            c.width_name, size_t(K) * t * c.width);
  ROM_CHECK(!c.AUX || c.AUX->n >= 2 * size_t(K), "%s: AUX holds %zu doubles, 2 K = %zu needed", c.who, c.AUX ? c.AUX->n : 0, 2 * size_t(K));
  ROM_TRY(rom_check_block(c.who, {"OUT", "ldo", "its row"}, c.OUT->n, c.out_off, c.ldo, row, K));   // (ldo >= row: checked above)
  ROM_HIP(hipSetDevice(ctx->device));

  const int B = K * t, ldw = c.lead + 4;
  Tmp ws;
  const size_t ws_doubles = size_t(B) * ldw + 2;
  ROM_TRY(ws.get(ctx, ws_doubles));
  unsigned long long* counters = reinterpret_cast<unsigned long long*>(ws.p() + size_t(B) * ldw);
  ROM_HIP(hipMemsetAsync(counters, 0, 2 * sizeof(unsigned long long), ctx->stream));
  ROM_HIP(hipMemsetAsync(ctx->d_status, 0, sizeof(int), ctx->stream));
  launch(ws.p(), ldw, counters);
  ROM_HIP(hipGetLastError());
  {
    ROM_PROF(ctx, c.select_name, 0.0, 8.0 * double(B) * ldw);
    k_lm_select<<<K, 64, 0, ctx->stream>>>(ws.p(), ldw, t, c.lead, c.OUT->p + c.out_off, c.ldo);
  }
  ROM_HIP(hipGetLastError());
  unsigned long long hc[2] = {0, 0};
  int status = 0;
  ROM_HIP(hipMemcpyAsync(hc, counters, sizeof hc, hipMemcpyDeviceToHost, ctx->stream));
  ROM_HIP(hipMemcpyAsync(&status, ctx->d_status, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  ROM_HIP(hipStreamSynchronize(ctx->stream));
  if (c.info8_host) {
    c.info8_host[0] = 2;   // launches
    c.info8_host[1] = 1;   // host synchronisations
    c.info8_host[2] = double(ws_doubles) * sizeof(double);
    c.info8_host[3] = B;
    c.info8_host[4] = double(hc[0]);
    c.info8_host[5] = double(hc[1]);
  }
  if (status) {
    // (reported once: the word is cleared, or the next call on this context -- whatever it is -- would report this failure again)
    ROM_HIP(hipMemsetAsync(ctx->d_status, 0, sizeof(int), ctx->stream));
    rom_set_error("%s: %s", c.who, c.failure);
    return c.failure_code;
  }
  return ROM_OK;
}

}  // namespace
