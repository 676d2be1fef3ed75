// rom_poly_sense: sensor state estimation on the polynomial manifold of a fitted rom_poly map -- a port, line for line, of
// romhighcontrast_amd/nonlinear.py::sense_scores (cited below as `py:` with the names of that function) and, through it, of the
// Levenberg-Marquardt of inverse.py::polish_parameters / rom_lm.hip, with another model: in reduced sensor coordinates the sensor
// image of the decoder u(z) = mean + z V_known + g(z) V_unknown is LINEAR in the Legendre products phi(t) of rom_poly.hip,
//     F(t) = G_r phi(t),   residual rho = p - G_r phi(t),   J = d rho / d t = -G_r d phi / d t,
// with phi_p(t) = prod_j L_{alpha_pj}(t_j) and d phi_p / d t_j = L'_{alpha_pj}(t_j) prod_{i != j} L_{alpha_pi}(t_i); the Legendre
// values by (k + 1) L_{k+1} = (2k + 1) t L_k - k L_{k-1}, the derivatives by L'_{k+1} = L'_{k-1} + (2k + 1) L_k.
//
// One SYSTEM is one pair (query, start); k_sense runs one workgroup of 256 threads per system and the whole iteration inside the
// launch.  In LDS: the Legendre table (m x (d + 1) values and derivatives), phi (P), d phi (P x 16, the free coordinates packed
// to the front), J (16 columns of r, row stride r | 1), J^T J and the damped system (16 x 17), the exponent rows as bytes and
// the vectors: at most 34.7 KB (P = 91, the most terms P <= 96 admits, and r = 96), inside the default 64 KB of dynamic LDS.  G_r (at most 72 KB,
// shared by every system) is read through L2: with it resident in LDS a CU would hold one workgroup and run the systems of a
// chunk one after the other, while here four workgroups fit a CU at every shape (by registers; LDS never admits fewer).
// The product G_r [d phi] (r x P)(P x 16) runs on v_mfma_f64_16x16x4_f64: the 16 columns of d phi are one tile column, a wave
// takes the 16-row tiles w, w + 4 of G_r.  The column phi (the model value of every trial) goes by VALU, 16 lanes per row, in
// double-double arithmetic (see SnDD below): rho and f are correctly rounded, as the host's, which forms them in long double.
// A PINNED coordinate (lo_j == hi_j) stays at its clipped start bit for bit, has no column in d phi, J, J^T J and sigma_min.
// The iteration itself is lm_drive (rom_lm_drive.h, with the contract on control flow); SnSys below is its model.
#include <cmath>
#include <cstring>
#include <vector>

#include "rom_lm_drive.h"
#include "rom_mma.h"

namespace {

constexpr int SN_MMAX = 16, SN_DMAX = 8, SN_PMAX = 96, SN_RMAX = 96, SN_TMAX = 8;
constexpr int SN_THREADS = LMS_THREADS;
constexpr int SN_LDD = 16;   // row stride of d phi: a row is one MFMA operand row (16 lanes read 128 contiguous bytes)

struct SnBox {
  double lo[SN_MMAX], hi[SN_MMAX];
};
struct SnTerms {   // the exponent of coordinate j in term p at [p SN_MMAX + j]
  unsigned char pw[SN_PMAX * SN_MMAX];
};

struct SnArgs {
  int m, d, P, r, t, max_iter;
  const double* Gr;   // r P
  const double* Pq;   // query rows, ldp apart
  long long ldp;
  const double* T0;   // K t m
  const double* aux;  // K x 2 (perp2, scale) or null
  double misfit_tol;
  double* W;          // per system: t (m) | misfit | sigma_min | converged | iterations
  int ldw;
  unsigned long long* counters;   // LM iterations, feature evaluations
  int* status;
};

// the LDS map, in doubles (host and device)
struct SnLds {
  int ldr, ldk, ldl, ppad;
  int Lg, Dg, phi, dphi, Js, JtJ, Hs, hinv, rho, rhon, ps, th, thn, g, lo, hi, scal, idx, pw, total;
  __host__ __device__ SnLds(int m, int d, int P, int r) {
    ldr = r | 1, ldk = SN_MMAX + 1, ldl = d + 1, ppad = (P + 3) & ~3;
    int at = 0;
    auto take = [&](int cnt) {
      const int o = at;
      at += cnt;
      return o;
    };
    dphi = take(ppad * SN_LDD), phi = take(ppad), Lg = take(m * ldl), Dg = take(m * ldl);
    Js = take(SN_MMAX * ldr), JtJ = take(SN_MMAX * ldk), Hs = take(SN_MMAX * ldk), hinv = take(SN_MMAX);
    rho = take(r), rhon = take(r), ps = take(r);
    th = take(SN_MMAX), thn = take(SN_MMAX), g = take(SN_MMAX), lo = take(SN_MMAX), hi = take(SN_MMAX);
    scal = take(8);             // the slots LMS_* of rom_lm_drive.h; [7]: the number of free coordinates
    idx = take(SN_MMAX);        // 2 x 16 ints: the coordinate of free column c | the free column of coordinate j (-1: pinned)
    pw = take(2 * SN_PMAX);     // SN_PMAX x SN_MMAX bytes
    total = at;
  }
};

__device__ __forceinline__ bool sn_finite(double v) { return fabs(v) < __builtin_huge_val(); }

// Double-double sums for the residual and its squared norm.  Off the manifold |rho| is a few percent of |G_r phi|: in plain
// fp64 the rounding of G_r phi and of the sum of squares puts noise of eps |rho| |G_r phi| on f, the acceptance f_new < f is then
// decided by rounding once a step gains less than that, and the final t is reproducible to 1e-9 only.  With rho and f correctly
// rounded (the host forms them in long double) it is reproducible to a few 1e-11.  Error-free transformations, no contraction.
struct SnDD {
  double hi, lo;
};
__device__ __forceinline__ SnDD sn_two_sum(double a, double b) {
#pragma clang fp contract(off)
  const double s = a + b, bb = s - a;
  return {s, (a - (s - bb)) + (b - bb)};
}
__device__ __forceinline__ SnDD sn_add(SnDD x, SnDD y) {   // (symmetric in x and y: a butterfly leaves the same bits in every lane)
#pragma clang fp contract(off)
  const SnDD s = sn_two_sum(x.hi, y.hi);
  const double e = s.lo + (x.lo + y.lo), hi = s.hi + e;
  return {hi, e - (hi - s.hi)};
}
__device__ __forceinline__ SnDD sn_mac(SnDD acc, double a, double b) {   // acc + a b
#pragma clang fp contract(off)
  const double p = a * b, pe = __builtin_fma(a, b, -p);
  return sn_add(acc, SnDD{p, pe});
}
__device__ __forceinline__ SnDD sn_shfl_xor(SnDD v, int mask) { return {__shfl_xor(v.hi, mask, 64), __shfl_xor(v.lo, mask, 64)}; }

struct SnSys {
  const SnArgs& a;
  const SnLds& m;
  double* sm;
  int kf = 0;   // free coordinates
  unsigned long long evaluations = 0;
  __device__ SnSys(const SnArgs& a_, const SnLds& m_, double* sm_) : a(a_), m(m_), sm(sm_) {}
  __device__ const unsigned char* pw() const { return reinterpret_cast<const unsigned char*>(sm + m.pw); }
  __device__ const int* free_coord() const { return reinterpret_cast<const int*>(sm + m.idx); }
  __device__ const int* free_column() const { return reinterpret_cast<const int*>(sm + m.idx) + SN_MMAX; }
  __device__ int cols() const { return kf; }
  __device__ unsigned long long work() const { return evaluations; }

  // py:legendre_table: L_k and L'_k, k = 0 .. d, of the coordinates at sm[thx ..)
  __device__ void legendre(int thx) {
    const int tid = threadIdx.x, d = a.d;
    if (tid < a.m) {
#pragma clang fp contract(off)   // (no fused multiply-add here: the table, and with it phi and d phi, has the host's bits)
      const double t = sm[thx + tid];
      double* L = sm + m.Lg + tid * m.ldl;
      double* D = sm + m.Dg + tid * m.ldl;
      L[0] = 1.0, L[1] = t, D[0] = 0.0, D[1] = 1.0;
      for (int k = 1; k < d; ++k) {
        L[k + 1] = (double(2 * k + 1) * t * L[k] - double(k) * L[k - 1]) / double(k + 1);
        D[k + 1] = D[k - 1] + double(2 * k + 1) * L[k];
      }
    }
    __syncthreads();
    evaluations += 1;
  }

  // py:`F, _ = legendre_features(new, powers, False)` .. `fn`: phi(t), rho = p - G_r phi -> rhon, |rho|^2 -> scal[LMS_FN]
  __device__ void eval(int thx) {
    const int tid = threadIdx.x, lane = tid & 63, P = a.P, r = a.r, l16 = tid & 15, nm = a.m;
    legendre(thx);
    const unsigned char* e = pw();
    for (int p = tid; p < m.ppad; p += SN_THREADS) {
      double v = 0.0;
      if (p < P) {
        v = 1.0;
        for (int j = 0; j < nm; ++j) v *= sm[m.Lg + j * m.ldl + e[p * SN_MMAX + j]];
      }
      sm[m.phi + p] = v;
    }
    __syncthreads();
    for (int i0 = 0; i0 < r; i0 += 16) {   // 16 lanes per row of G_r
      const int i = i0 + (tid >> 4);
      SnDD s = {0.0, 0.0};
      if (i < r)
        for (int p = l16; p < P; p += 16) s = sn_mac(s, a.Gr[size_t(i) * P + p], sm[m.phi + p]);
#pragma unroll
      for (int x = 8; x >= 1; x >>= 1) s = sn_add(s, sn_shfl_xor(s, x));
      if (i < r && l16 == 0) {
        const SnDD dlt = sn_two_sum(sm[m.ps + i], -s.hi);
        sm[m.rhon + i] = dlt.hi + (dlt.lo - s.lo);
      }
    }
    __syncthreads();
    if (tid < 64) {
      const double v0 = lane < r ? sm[m.rhon + lane] : 0.0, v1 = lane + 64 < r ? sm[m.rhon + lane + 64] : 0.0;
      SnDD f = sn_mac(sn_mac(SnDD{0.0, 0.0}, v0, v0), v1, v1);
#pragma unroll
      for (int x = 32; x >= 1; x >>= 1) f = sn_add(f, sn_shfl_xor(f, x));
      if (lane == 0) sm[m.scal + LMS_FN] = f.hi + f.lo;
    }
    __syncthreads();
  }

  // py:`Ja`, `JtJ`, `g` at the current t (th) and its rho: d phi / d t of the free coordinates, J = -G_r d phi -> Js (column c at
  // Js + c ldr), J^T J -> JtJ, g = J^T rho
  __device__ void jacobian() {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, P = a.P, r = a.r, nm = a.m;
    double* Js = sm + m.Js;
    legendre(m.th);
    const unsigned char* e = pw();
    const int* fc = free_coord();
    for (int x = tid; x < m.ppad * SN_LDD; x += SN_THREADS) {
      const int p = x >> 4, c = x & 15;
      double v = 0.0;
      if (p < P && c < kf) {
        const int j = fc[c], aj = e[p * SN_MMAX + j];
        if (aj > 0) {   // (L'_0 = 0)
          v = 1.0;
          for (int i = 0; i < nm; ++i) v *= i == j ? sm[m.Dg + i * m.ldl + aj] : sm[m.Lg + i * m.ldl + e[p * SN_MMAX + i]];
        }
      }
      sm[m.dphi + x] = v;
    }
    __syncthreads();
    // MFMA f64 16x16x4: A operand lane l holds A[i = l & 15][k = l >> 4], B operand B[k = l >> 4][j = l & 15], the result
    // register g the element (row (l >> 4) + 4 g, column l & 15)
    for (int tile = w; tile * 16 < r; tile += 4) {
      const int row = tile * 16 + (lane & 15), kq = lane >> 4;
      const double* grow = a.Gr + size_t(row < r ? row : 0) * P;
      d4_t acc = {0.0, 0.0, 0.0, 0.0};
      for (int k0 = 0; k0 < m.ppad; k0 += 4) {
        const int p = k0 + kq;
        const double av = (row < r && p < P) ? grow[p] : 0.0;
        const double bv = sm[m.dphi + p * SN_LDD + (lane & 15)];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
      }
      const int c = lane & 15;
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int i = tile * 16 + (lane >> 4) + 4 * g4;
        if (i < r && c < kf) Js[c * m.ldr + i] = -acc[g4];
      }
    }
    __syncthreads();
    for (int x = tid; x < kf * kf; x += SN_THREADS) {
      const int q = x / kf, p = x - q * kf;
      double s = 0.0;
      for (int i = 0; i < r; ++i) s = fma(Js[q * m.ldr + i], Js[p * m.ldr + i], s);
      sm[m.JtJ + q * m.ldk + p] = s;
    }
    if (tid < kf) {
      double s = 0.0;
      for (int i = 0; i < r; ++i) s = fma(Js[tid * m.ldr + i], sm[m.rho + i], s);
      sm[m.g + tid] = s;
    }
    __syncthreads();
  }

  // py:`step`, `new`, `moved`: lane = coordinate, the step b by free column; a pinned coordinate keeps its value
  __device__ void step(double b, int lane) {
    const int nm = a.m;
    const int c = lane < nm ? free_column()[lane] : -1;
    const double st = __shfl(b, c >= 0 ? c : 0, 64);
    double moved = 0.0, mx = 0.0;
    if (lane < nm) {
      const double old = sm[m.th + lane], lo = sm[m.lo + lane], hi = sm[m.hi + lane];
      double nw = old;
      if (c >= 0) {
        const double v = old - st;
        nw = v < lo ? lo : (v > hi ? hi : v);
      }
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
  __device__ bool trial() {   // (every point of the box is usable)
    eval(m.thn);
    return true;
  }
  __device__ void keep() {
    const int tid = threadIdx.x;
    if (tid < a.m) sm[m.th + tid] = sm[m.thn + tid];
    if (tid < a.r) sm[m.rho + tid] = sm[m.rhon + tid];
  }
  __device__ void refresh() {}   // (the Jacobian needs nothing that a trial overwrites)
  __device__ int head(double* out) const {   // t
    if (threadIdx.x < a.m) out[threadIdx.x] = sm[m.th + threadIdx.x];
    return a.m;
  }
  __device__ double sigma_min(int lane) { return kf > 0 ? lm_sigma_min_wave<2>(sm + m.Js, m.ldr, kf, a.r, lane) : 0.0; }
};

__global__ __launch_bounds__(SN_THREADS) void k_sense(const SnArgs a, const SnBox box, const SnTerms terms) {
  extern __shared__ __align__(16) double sn_lds[];
  double* sm = sn_lds;
  const SnLds m(a.m, a.d, a.P, a.r);
  const int tid = threadIdx.x, nm = a.m, r = a.r;
  const long long sys = blockIdx.x, query = sys / a.t;
  SnSys S(a, m, sm);
  double* out = a.W + size_t(sys) * a.ldw;

  // the exponent rows, the box and the free coordinates; the query's row, the clipped start, the scale (py: `th = clip(..)`, `scale`)
  bool bad = false;
  {
    unsigned char* e = reinterpret_cast<unsigned char*>(sm + m.pw);
    for (int x = tid; x < a.P * SN_MMAX; x += SN_THREADS) e[x] = terms.pw[x];
    int* fc = reinterpret_cast<int*>(sm + m.idx);
    if (tid == 0) {
      int kf = 0;
      for (int j = 0; j < nm; ++j) {
        const bool is_free = box.lo[j] < box.hi[j];
        fc[SN_MMAX + j] = is_free ? kf : -1;
        if (is_free) fc[kf++] = j;
      }
      for (int c = kf; c < SN_MMAX; ++c) fc[c] = 0;
      sm[m.scal + 7] = double(kf);
    }
    if (tid < r) {
      const double v = a.Pq[query * a.ldp + tid];
      bad |= !sn_finite(v);
      sm[m.ps + tid] = v;
    }
    if (tid < nm) {
      const double v = a.T0[size_t(sys) * nm + tid], lo = box.lo[tid], hi = box.hi[tid];
      bad |= !sn_finite(v);
      sm[m.lo + tid] = lo, sm[m.hi + tid] = hi;
      sm[m.th + tid] = v < lo ? lo : (v > hi ? hi : v);
    }
    for (long long x = sys * SN_THREADS + tid; x < (long long)r * a.P; x += (long long)gridDim.x * SN_THREADS) bad |= !sn_finite(a.Gr[x]);
    if (bad) atomicOr(a.status, 1);   // NaN / Inf in G_r, P or T0: the call fails (the loops below are bounded whatever the data)
  }
  __syncthreads();
  S.kf = int(sm[m.scal + 7]);
  double perp2;
  const double scale = lm_scale(a.aux, query, sm + m.ps, r, perp2);

  S.eval(m.th);
  if (tid < r) sm[m.rho + tid] = sm[m.rhon + tid];
  lm_drive(S, perp2, scale, out);
}

}  // namespace

extern "C" int rom_poly_sense(rom_ctx* ctx, int m, int d, int r, rom_buf* Gr, rom_buf* P, size_t p_off, int64_t ldp, int K, int t,
                              rom_buf* T0, const double* lo_host, const double* hi_host, rom_buf* AUX, int max_iter, double misfit_tol,
                              rom_buf* OUT, size_t out_off, int64_t ldo, double* info8_host) {
  ROM_CHECK(ctx && Gr && lo_host && hi_host, "rom_poly_sense: null argument (context, Gr, lo or hi)");
  ROM_CHECK(m >= 1 && m <= SN_MMAX, "rom_poly_sense: m = %d coordinates, between 1 and %d", m, SN_MMAX);
  ROM_CHECK(d >= 1 && d <= SN_DMAX, "rom_poly_sense: degree d = %d, between 1 and %d", d, SN_DMAX);
  long long terms = 1;
  for (int k = 1; k <= d; ++k) terms = terms * (m + k) / k;   // C(m + k, k): exact at every step
  ROM_CHECK(terms <= SN_PMAX, "rom_poly_sense: P = C(%d + %d, %d) = %lld terms, at most %d", m, d, d, terms, SN_PMAX);
  const int np = int(terms);
  ROM_CHECK(r >= 1 && r <= SN_RMAX, "rom_poly_sense: r = %d sensor coordinates, between 1 and %d", r, SN_RMAX);
  ROM_CHECK(Gr->n >= size_t(r) * np, "rom_poly_sense: Gr holds %zu doubles, r P = %zu needed", Gr->n, size_t(r) * np);
  const SnLds map(m, d, np, r);
  const size_t lds = size_t(map.total) * sizeof(double);
  ROM_CHECK(lds <= 64 * 1024, "rom_poly_sense: %zu bytes of LDS", lds);   // (34.7 KB at most)

  SnBox box;
  for (int j = 0; j < SN_MMAX; ++j) {
    box.lo[j] = j < m ? lo_host[j] : 0.0;
    box.hi[j] = j < m ? hi_host[j] : 0.0;
  }
  SnTerms tab;
  std::memset(tab.pw, 0, sizeof tab.pw);
  {
    std::vector<int> powers(size_t(np) * m);
    int np2 = 0;
    ROM_TRY(rom_poly_terms(m, d, &np2, powers.data()));
    for (int p = 0; p < np; ++p)
      for (int j = 0; j < m; ++j) tab.pw[p * SN_MMAX + j] = (unsigned char)powers[size_t(p) * m + j];
  }
  const LmCall call = {"rom_poly_sense", r, K, t, SN_TMAX, max_iter, m, m, "T0", "m", "m", P, T0, AUX, OUT, p_off, out_off,
                       ldp, ldo, info8_host, "poly_sense_select", "NaN / Inf in Gr, P or T0", ROM_ERR_INVALID};
  return lm_launch(ctx, call, [&](double* W, int ldw, unsigned long long* counters) {
    SnArgs a;
    a.m = m, a.d = d, a.P = np, a.r = r, a.t = t, a.max_iter = max_iter;
    a.Gr = Gr->p, a.Pq = P->p + p_off, a.ldp = ldp, a.T0 = T0->p, a.aux = AUX ? AUX->p : nullptr, a.misfit_tol = misfit_tol;
    a.W = W, a.ldw = ldw, a.counters = counters, a.status = ctx->d_status;
    char nm[48];
    rom_prof_name(nm, sizeof nm, "poly_sense", "_m%d_d%d_r%d", m, d, r);
    ROM_PROF(ctx, nm, 0.0, 0.0);
    k_sense<<<K * t, SN_THREADS, lds, ctx->stream>>>(a, box, tab);
  });
}
