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
// double-double arithmetic (SnDD of rom_sense_sys.h): rho and f are correctly rounded, as the host's, which forms them in long double.
// A PINNED coordinate (lo_j == hi_j) stays at its clipped start bit for bit, has no column in d phi, J, J^T J and sigma_min.
// The iteration itself is lm_drive (rom_lm_drive.h, with the contract on control flow); its model SnSys, the residual, the MFMA
// product and the kernel's body are those of rom_sense_sys.h, shared with rom_mlp_sense.hip: SnPoly below is the feature policy.
#include <cmath>
#include <cstring>
#include <vector>

#include "rom_sense_sys.h"

namespace {

constexpr int SN_DMAX = 8;

struct SnTerms {   // the exponent of coordinate j in term p at [p SN_MMAX + j]
  unsigned char pw[SN_PMAX * SN_MMAX];
};

// the policy's LDS at m.feat: the Legendre values and derivatives (m x (d + 1) each), then the exponent rows as bytes
__host__ __device__ inline int sn_poly_lds(int m, int d) { return 2 * m * (d + 1) + 2 * SN_PMAX; }

struct SnPoly {
  int nm, d, P, ldl;
  unsigned long long evaluations = 0;
  __device__ SnPoly(int m_, int d_, int P_) : nm(m_), d(d_), P(P_), ldl(d_ + 1) {}
  __device__ int Lg(const SnLds& m) const { return m.feat; }
  __device__ int Dg(const SnLds& m) const { return m.feat + nm * ldl; }
  __device__ unsigned char* pw(double* sm, const SnLds& m) const { return reinterpret_cast<unsigned char*>(sm + m.feat + 2 * nm * ldl); }

  // py:legendre_table: L_k and L'_k, k = 0 .. d, of the coordinates at sm[thx ..)
  __device__ void legendre(double* sm, const SnLds& m, int thx) {
    const int tid = threadIdx.x;
    if (tid < nm) {
#pragma clang fp contract(off)   // (no fused multiply-add here: the table, and with it phi and d phi, has the host's bits)
      const double t = sm[thx + tid];
      double* L = sm + Lg(m) + tid * ldl;
      double* D = sm + Dg(m) + tid * ldl;
      L[0] = 1.0, L[1] = t, D[0] = 0.0, D[1] = 1.0;
      for (int k = 1; k < d; ++k) {
        L[k + 1] = (double(2 * k + 1) * t * L[k] - double(k) * L[k - 1]) / double(k + 1);
        D[k + 1] = D[k - 1] + double(2 * k + 1) * L[k];
      }
    }
    __syncthreads();
    evaluations += 1;
  }

  // py:legendre_features(.., False): phi_p = prod_j L_{alpha_pj}(t_j)
  __device__ void values(double* sm, const SnLds& m, int thx) {
    const int tid = threadIdx.x;
    legendre(sm, m, thx);
    const unsigned char* e = pw(sm, m);
    for (int p = tid; p < m.ppad; p += SN_THREADS) {
      double v = 0.0;
      if (p < P) {
        v = 1.0;
        for (int j = 0; j < nm; ++j) v *= sm[Lg(m) + j * ldl + e[p * SN_MMAX + j]];
      }
      sm[m.phi + p] = v;
    }
    __syncthreads();
  }

  // py:legendre_features: d phi_p / d t_j = L'_{alpha_pj}(t_j) prod_{i != j} L_{alpha_pi}(t_i), the free coordinates only
  __device__ void tangents(double* sm, const SnLds& m, int kf, const int* fc) {
    const int tid = threadIdx.x;
    legendre(sm, m, m.th);
    const unsigned char* e = pw(sm, m);
    for (int x = tid; x < m.ppad * SN_LDD; x += SN_THREADS) {
      const int p = x >> 4, c = x & 15;
      double v = 0.0;
      if (p < P && c < kf) {
        const int j = fc[c], aj = e[p * SN_MMAX + j];
        if (aj > 0) {   // (L'_0 = 0)
          v = 1.0;
          for (int i = 0; i < nm; ++i) v *= i == j ? sm[Dg(m) + i * ldl + aj] : sm[Lg(m) + i * ldl + e[p * SN_MMAX + i]];
        }
      }
      sm[m.dphi + x] = v;
    }
    __syncthreads();
  }
};

__global__ __launch_bounds__(SN_THREADS) void k_sense(const SnArgs a, const SnBox box, const SnTerms terms, const int d) {
  extern __shared__ __align__(16) double sn_lds[];
  double* sm = sn_lds;
  const SnLds m(a.P, a.r, sn_poly_lds(a.m, d));
  SnPoly F(a.m, d, a.P);
  unsigned char* e = F.pw(sm, m);
  for (int x = threadIdx.x; x < a.P * SN_MMAX; x += SN_THREADS) e[x] = terms.pw[x];
  sn_run(a, box, m, sm, F, false);
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
  const SnLds map(np, r, sn_poly_lds(m, d));
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
    a.m = m, a.P = np, a.r = r, a.t = t, a.max_iter = max_iter;
    a.Gr = Gr->p, a.Pq = P->p + p_off, a.ldp = ldp, a.T0 = T0->p, a.aux = AUX ? AUX->p : nullptr, a.misfit_tol = misfit_tol;
    a.W = W, a.ldw = ldw, a.counters = counters, a.status = ctx->d_status;
    char nm[48];
    rom_prof_name(nm, sizeof nm, "poly_sense", "_m%d_d%d_r%d", m, d, r);
    ROM_PROF(ctx, nm, 0.0, 0.0);
    k_sense<<<K * t, SN_THREADS, lds, ctx->stream>>>(a, box, tab, d);
  });
}
