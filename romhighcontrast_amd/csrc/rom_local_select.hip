// rom_local_select: sensor state estimation with kc local reduced spaces and the model selection of Cohen, Dahmen, Mula and
// Nichols (SIAM/ASA JUQ 10, 2022) -- a port, decision for decision, of romhighcontrast_amd/inverse.py::local_select_host.
// For measurement vector i and cluster j:
//   1. state      c_ij = argmin over c_lo[j] <= c <= c_hi[j] of ||p_ij - G_j c||       (BvSys, G_j and G_j^T G_j in global memory)
//   2. residual   B_ij[:, q] = sum_i' c_ij[i'] R_j[:, 1 + i' k + q]                     (rank x k, built in LDS; rho_j = R_j[:, 0])
//   3. surrogate  S_ij = min over a_lo[j] <= a <= a_hi[j] of ||rho_j - B_ij a||         (BvSys again, B_ij and B_ij^T B_ij in LDS)
//   4. selection  label_i = the j of smallest (S_ij, j) among the systems of status 0 whose S is a number, or -1
// k_bvls_gram forms the kc Gram matrices G_j^T G_j, k_local_fit runs 1 - 3 with one workgroup of 256 threads per system and both
// active-set iterations inside the launch, k_local_pick does 4 with one thread per vector: three launches whatever K and kc are.
// The grid of k_local_fit is (K, kc): workgroups are handed out along x first, so the systems that read the same R_j -- the only
// large operand, rank (1 + k n) doubles through L2 -- run together.  Control flow is uniform within a workgroup (the decisions
// of BvSys go through LDS; a system that fails leaves at a barrier all its threads reach), free between workgroups; nothing
// waits on another workgroup.  No floating-point atomics, one fixed order in every sum, no system reads what another one
// writes: the same bits on every call and for every split of the rows.
#include <cmath>
#include <cstring>

#include "rom_basis_int.h"
#include "rom_block.h"
#include "rom_bvls_sys.h"
#include "rom_local_select_host.h"

namespace {

static_assert(LS_NMAX == BV_NMAX && LS_RMAX == BV_RMAX && LS_HLD == BV_LD && LS_KMAX <= BV_NMAX, "the limits of BvSys");

struct LsArgs {
  int n, k, rank, r, kc, iter_state, iter_param;
  const double *RT, *GR, *gram, *Pq, *box;   // box: c_lo | c_hi (kc n each) | a_lo | a_hi (kc k each)
  const int* gstatus;                        // kc words of k_bvls_gram
  long long ldp, ldo;
  double* OUT;
  unsigned long long* counters;   // passes of the state solves, of the parameter solves, factorisations, systems of status != 0
};

__global__ __launch_bounds__(LMS_THREADS) void k_local_fit(const LsArgs a) {
  extern __shared__ __align__(16) double ls_lds[];
  double* sm = ls_lds;
  const int tid = threadIdx.x, lane = tid & 63, n = a.n, k = a.k, rank = a.rank, r = a.r;
  const long long vec = blockIdx.x;
  const int j = blockIdx.y;
  const LsLds m(n, k, rank, r);
  const LsRow o(n, k);
  int* ints = reinterpret_cast<int*>(sm + m.ints);
  int *st = ints, *barred = ints + m.nm, *idx = ints + 2 * m.nm, *ctl = ints + 3 * m.nm, *stat = ctl + 4, *keep = ctl + 6;
  double* out = a.OUT + (vec * a.kc + j) * a.ldo;
  const double nan = __builtin_nan("");

  if (tid == 0) stat[0] = a.gstatus[j] ? 1 : 0, stat[1] = 0;
  __syncthreads();
  for (int e = tid; e < r; e += LMS_THREADS) {
    const double p = a.Pq[vec * a.ldp + size_t(j) * r + e];
    if (!bv_finite(p)) atomicOr(stat, 1);
    sm[m.ps + e] = p;
  }
  __syncthreads();
  int status = stat[0] ? LS_BAD_STATE : 0;

  // ---- 1. the state
  unsigned long long factorisations = 0;
  if (!status) {
    BvSys S = {n,         r,         a.GR + size_t(j) * r * n, a.gram + size_t(j) * n * n, stat,        sm + m.mat, sm + m.invd,
               sm + m.c,  sm + m.z,  sm + m.v,                 sm + m.gn,                  sm + m.part, sm + m.ps,  sm + m.rs,
               sm + m.flag, st, barred, idx, ctl};
    const bool has = lane < n;
    const double lo = has ? a.box[size_t(j) * n + lane] : 0.0, hi = has ? a.box[size_t(a.kc + j) * n + lane] : 0.0;
    bool conv = false;
    const int passes = S.run(lo, hi, a.iter_state, &conv);
    const double f = S.misfit2();
    factorisations = S.factorisations;
    if (tid < n) sm[m.c1 + tid] = sm[m.c + tid];
    if (tid == 0) sm[m.scal] = sqrt(f), keep[0] = passes;
    __syncthreads();   // (the state solve is over: `mat` and the vectors are free, stat[0] is final)
    status = (stat[0] ? LS_BAD_STATE : 0) | (conv ? 0 : LS_OPEN_STATE);
  }
  if (status & LS_BAD_STATE) {   // (uniform: status comes from LDS after a barrier)
    for (int e = tid; e < o.status; e += LMS_THREADS) out[e] = e >= o.passes ? 0.0 : nan;
    if (tid == 0) {
      out[o.status] = double(LS_BAD_STATE);
      atomicAdd(a.counters + 2, factorisations);
      atomicAdd(a.counters + 3, 1ull);
    }
    return;
  }

  // ---- 2. B = sum_i' c_i' R[:, 1 + i' k + q], rho = R[:, 0]: entry (row, q) by one thread, i' ascending
  const int P = 1 + k * n;
  const double* R = a.RT + size_t(j) * rank * P;
  double* B = sm + m.B;
  for (int x = tid; x < rank * k; x += LMS_THREADS) {
    const int row = x / k, q = x - row * k;
    const double* Rr = R + size_t(row) * P + 1 + q;
    double s = 0.0;
    for (int i = 0; i < n; ++i) s = fma(sm[m.c1 + i], Rr[i * k], s);
    B[x] = s;
  }
  for (int row = tid; row < rank; row += LMS_THREADS) {
    const double rho = R[size_t(row) * P];
    if (!bv_finite(rho)) atomicOr(stat + 1, 1);
    sm[m.ps + row] = rho;
  }
  __syncthreads();
  // B^T B: entry (jj, q) by one thread, rows ascending (k_bvls_gram's order); every entry of B is looked at
  if (tid < k * k) {
    const int jj = tid / k, q = tid - jj * k;
    bool bad = false;
    double s = 0.0;
    for (int i = 0; i < rank; ++i) {
      const double bq = B[i * k + q];
      bad |= !bv_finite(bq);
      s = fma(B[i * k + jj], bq, s);
    }
    sm[m.gram3 + tid] = s;
    if (bad) atomicOr(stat + 1, 1);
  }
  __syncthreads();

  // ---- 3. the parameter and the surrogate
  int passes3 = 0;
  if (stat[1] == 0) {
    BvSys S = {k,         rank,      B,        sm + m.gram3, stat + 1,    sm + m.mat, sm + m.invd,
               sm + m.c,  sm + m.z,  sm + m.v, sm + m.gn,    sm + m.part, sm + m.ps,  sm + m.rs,
               sm + m.flag, st, barred, idx, ctl};
    const bool has = lane < k;
    const size_t ab = 2 * size_t(a.kc) * n;
    const double lo = has ? a.box[ab + size_t(j) * k + lane] : 0.0, hi = has ? a.box[ab + size_t(a.kc + j) * k + lane] : 0.0;
    bool conv = false;
    passes3 = S.run(lo, hi, a.iter_param, &conv);
    const double f = S.misfit2();
    factorisations += S.factorisations;
    if (tid == 0) sm[m.scal + 1] = sqrt(f);
    __syncthreads();
    status |= conv ? 0 : LS_OPEN_PARAM;
  }
  if (stat[1]) status |= LS_BAD_PARAM;
  const bool bad3 = (status & LS_BAD_PARAM) != 0;
  if (tid < n) out[o.c + tid] = sm[m.c1 + tid];
  if (tid < k) out[o.a + tid] = bad3 ? nan : sm[m.c + tid];
  if (tid == 0) {
    out[o.S] = bad3 ? nan : sm[m.scal + 1];
    out[o.misfit] = sm[m.scal];
    out[o.passes] = double(keep[0]);
    out[o.passes + 1] = bad3 ? 0.0 : double(passes3);
    out[o.status] = double(status);
    atomicAdd(a.counters, (unsigned long long)keep[0]);
    atomicAdd(a.counters + 1, (unsigned long long)(bad3 ? 0 : passes3));
    atomicAdd(a.counters + 2, factorisations);
    if (status) atomicAdd(a.counters + 3, 1ull);
  }
}

// label of vector i: the smallest (S, j) among its systems of status 0 whose S is a number (an S that overflowed to NaN never
// wins), or -1
__global__ __launch_bounds__(256) void k_local_pick(const double* __restrict__ OUT, long long ldo, int K, int kc, int at_S, int at_status,
                                                    int* __restrict__ label) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= K) return;
  int best = -1;
  double bs = 0.0;
  for (int j = 0; j < kc; ++j) {
    const double* row = OUT + (i * kc + j) * ldo;
    const double s = row[at_S];
    if (row[at_status] == 0.0 && s == s && (best < 0 || s < bs)) best = j, bs = s;
  }
  label[i] = best;
}

int ls_layout(const char* who, int n, int k, int rank, int r, int* rank_max) {
  const int why = ls_check_shape(n, k, rank, r, rank_max);
  ROM_CHECK(why != 1, "%s: n = %d coefficients per cluster, between 1 and %d", who, n, LS_NMAX);
  ROM_CHECK(why != 2, "%s: k = %d parameters, between 1 and %d", who, k, LS_KMAX);
  ROM_CHECK(why != 3, "%s: r = %d reduced sensor coordinates, between n = %d and %d", who, r, n, LS_RMAX);
  ROM_CHECK(why != 4, "%s: rank = %d residual rows, at least k = %d (B needs full column rank)", who, rank, k);
  ROM_CHECK(why != 5, "%s: rank = %d residual rows, at most %d at n = %d, k = %d, r = %d (B and the factor share %d bytes of LDS)", who,
            rank, *rank_max, n, k, r, LS_LDS_BYTES);
  return ROM_OK;
}

}  // namespace

extern "C" int rom_local_select_layout(int n, int k, int rank, int r, int64_t* out8) {
  ROM_CHECK(out8, "rom_local_select_layout: null argument (out8)");
  int rank_max = 0;
  ROM_TRY(ls_layout("rom_local_select_layout", n, k, rank, r, &rank_max));
  const LsLds m(n, k, rank, r);
  const LsRow o(n, k);
  const int64_t v[8] = {m.bytes, o.total, rank_max, LS_KCMAX, m.mat, m.B, m.gram3, LS_LAUNCHES};
  std::memcpy(out8, v, sizeof v);
  return ROM_OK;
}

extern "C" int rom_local_select(rom_ctx* ctx, int kc, int n, int k, int rank, int r, rom_buf* RT, rom_buf* GR, rom_buf* P, size_t p_off,
                                int64_t ldp, int K, const double* c_lo_host, const double* c_hi_host, const double* a_lo_host,
                                const double* a_hi_host, int max_iter, rom_buf* OUT, size_t out_off, int64_t ldo, int32_t* label_host,
                                double* info8_host) {
  ROM_CHECK(ctx && RT && GR && c_lo_host && c_hi_host && a_lo_host && a_hi_host,
            "rom_local_select: null argument (context, RT, GR or a box)");
  int rank_max = 0;
  ROM_TRY(ls_layout("rom_local_select", n, k, rank, r, &rank_max));
  ROM_CHECK(kc >= 1 && kc <= LS_KCMAX, "rom_local_select: kc = %d clusters, between 1 and %d", kc, LS_KCMAX);
  const size_t P1 = 1 + size_t(k) * n;
  ROM_CHECK(RT->n >= size_t(kc) * rank * P1, "rom_local_select: RT holds %zu doubles, kc rank (1 + k n) = %zu needed", RT->n,
            size_t(kc) * rank * P1);
  ROM_CHECK(GR->n >= size_t(kc) * r * n, "rom_local_select: GR holds %zu doubles, kc r n = %zu needed", GR->n, size_t(kc) * r * n);
  // (K is the grid's x extent: K workgroups of 256 threads stay below 2^31 threads)
  ROM_CHECK(K >= 0 && K <= LS_KMAX_VECTORS && K <= (1 << 30) / kc, "rom_local_select: K = %d measurement vectors, at most 2^23 and K kc at most 2^30", K);
  const LsRow o(n, k);
  ROM_CHECK(ldo >= o.total, "rom_local_select: ldo = %lld < n + k + 5 = %d", (long long)ldo, o.total);
  std::vector<double> box;
  const long long bad = ls_pack_boxes(kc, n, k, c_lo_host, c_hi_host, a_lo_host, a_hi_host, box);
  if (bad >= 0) {
    const bool of_c = bad < (long long)kc * n;
    const long long e = of_c ? bad : bad - (long long)kc * n;
    const int per = of_c ? n : k;
    ROM_CHECK(false, "rom_local_select: the boxes need lo <= hi without NaN, cluster %lld coordinate %lld of %s has [%g, %g]", e / per,
              e % per, of_c ? "c" : "a", (of_c ? c_lo_host : a_lo_host)[e], (of_c ? c_hi_host : a_hi_host)[e]);
  }
  if (info8_host) std::fill(info8_host, info8_host + 8, 0.0);
  if (K == 0) return ROM_OK;
  ROM_CHECK(P && OUT && label_host, "rom_local_select: null argument (P, OUT or label)");
  ROM_TRY(rom_check_block("rom_local_select", {"P", "ldp", "kc r"}, P->n, p_off, ldp, kc * r, K));
  ROM_TRY(rom_check_block("rom_local_select", {"OUT", "ldo", "n + k + 5"}, OUT->n, out_off, ldo, o.total, int64_t(K) * kc));
  ROM_HIP(hipSetDevice(ctx->device));

  // workspace, in doubles: the Gram matrices | the boxes | 4 counters | kc status words | K labels
  const size_t w_gram = 0, w_box = w_gram + size_t(kc) * n * n, w_cnt = w_box + box.size(), w_stat = w_cnt + 4;
  const size_t w_lab = w_stat + (size_t(kc) + 1) / 2, ws_doubles = w_lab + (size_t(K) + 1) / 2;
  Tmp ws;
  ROM_TRY(ws.get(ctx, ws_doubles));
  unsigned long long* counters = reinterpret_cast<unsigned long long*>(ws.p() + w_cnt);
  int* gstatus = reinterpret_cast<int*>(ws.p() + w_stat);
  int* label = reinterpret_cast<int*>(ws.p() + w_lab);
  ROM_HIP(hipMemsetAsync(counters, 0, (w_lab - w_cnt) * sizeof(double), ctx->stream));   // (the counters and the status words)
  ROM_HIP(hipMemcpyAsync(ws.p() + w_box, box.data(), box.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  {
    ROM_PROF(ctx, "local_select_gram", 2.0 * kc * r * n * n, 8.0 * kc * r * n);
    k_bvls_gram<<<dim3(n, kc), BV_NMAX, 0, ctx->stream>>>(GR->p, n, r, ws.p() + w_gram, gstatus);
  }
  ROM_HIP(hipGetLastError());
  const LsLds m(n, k, rank, r);
  {
    LsArgs a;
    a.n = n, a.k = k, a.rank = rank, a.r = r, a.kc = kc;
    a.iter_state = max_iter < 0 ? 5 * n + 10 : max_iter, a.iter_param = max_iter < 0 ? 5 * k + 10 : max_iter;
    a.RT = RT->p, a.GR = GR->p, a.gram = ws.p() + w_gram, a.Pq = P->p + p_off, a.box = ws.p() + w_box, a.gstatus = gstatus;
    a.ldp = ldp, a.ldo = ldo, a.OUT = OUT->p + out_off, a.counters = counters;
    char nm[64];
    rom_prof_name(nm, sizeof nm, "local_select_fit", "_n%d_k%d_rank%d_r%d", n, k, rank, r);
    ROM_PROF(ctx, nm, 2.0 * K * kc * (double(rank) * n * k + double(rank) * k * k), 8.0 * K * kc * double(rank) * P1);
    k_local_fit<<<dim3(K, kc), LMS_THREADS, size_t(m.bytes), ctx->stream>>>(a);
  }
  ROM_HIP(hipGetLastError());
  {
    ROM_PROF(ctx, "local_select_pick", 0.0, 16.0 * K * kc);
    k_local_pick<<<(K + 255) / 256, 256, 0, ctx->stream>>>(OUT->p + out_off, ldo, K, kc, o.S, o.status, label);
  }
  ROM_HIP(hipGetLastError());
  unsigned long long hc[4] = {0, 0, 0, 0};
  ROM_HIP(hipMemcpyAsync(hc, counters, sizeof hc, hipMemcpyDeviceToHost, ctx->stream));
  ROM_HIP(hipMemcpyAsync(label_host, label, size_t(K) * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  ROM_HIP(hipStreamSynchronize(ctx->stream));
  if (info8_host) {
    info8_host[0] = double(K) * kc;   // systems
    info8_host[1] = LS_LAUNCHES;
    info8_host[2] = 1;                // host synchronisations
    info8_host[3] = double(ws_doubles) * sizeof(double);
    info8_host[4] = double(hc[0] + hc[1]);   // passes of both solves
    info8_host[5] = double(hc[2]);           // factorisations
    info8_host[6] = 2.0 * K * kc * (double(rank) * n * k + double(rank) * k * k);   // executed flops of steps 2 and of B^T B
    info8_host[7] = double(hc[3]);           // systems of status != 0
  }
  return ROM_OK;
}
