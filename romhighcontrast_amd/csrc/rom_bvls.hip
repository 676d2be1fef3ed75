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
// The iteration itself is BvSys of rom_bvls_sys.h (shared with rom_local_select.hip).
// G^T G is formed once per call by k_bvls_gram (shared by every system).  G_r (at most 48 KB) and G^T G (32 KB) are read through
// L2: with G_r in LDS beside the 33 KB factor a CU would hold one workgroup; here the LDS is 40.2 KB and four fit.
#include <cmath>

#include "rom_basis_int.h"
#include "rom_block.h"
#include "rom_bvls_sys.h"

namespace {

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

__global__ __launch_bounds__(LMS_THREADS) void k_bvls(const BvArgs a, const BvBox box) {
  __shared__ double H[BV_NMAX * BV_LD];
  __shared__ double invd[BV_NMAX], c[BV_NMAX], z[BV_NMAX], v[BV_NMAX], gn[BV_NMAX], part[LMS_THREADS], ps[BV_RMAX], rs[BV_RMAX], flag[2];
  __shared__ int st[BV_NMAX], barred[BV_NMAX], idx[BV_NMAX], ctl[3];   // ctl: the pass was infeasible; nothing left to free; free columns
  const int tid = threadIdx.x, lane = tid & 63, n = a.n, r = a.r;
  const long long sys = blockIdx.x;
  BvSys S = {n, r, a.G, a.gram, a.status, H, invd, c, z, v, gn, part, ps, rs, flag, st, barred, idx, ctl};
  const double lo = box.lo[lane], hi = box.hi[lane];

  if (tid < r) {
    const double p = a.Pq[sys * a.ldp + tid];
    if (!bv_finite(p)) atomicOr(a.status, 1);
    ps[tid] = p;
  }
  bool conv = false;
  const int passes = S.run(lo, hi, a.max_iter, &conv);   // (its first step is a barrier)
  const double f = S.misfit2();
  if (tid < 64) {
    const bool in = tid < n;
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
