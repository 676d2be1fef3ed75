// rom_mlp_sense: sensor state estimation on the manifold of a fitted rom_mlp map -- a port of
// romhighcontrast_amd/nonlinear.py::mlp_sense_scores (cited below as `py:` with the names of that file), the iteration of
// rom_poly_sense with another feature vector.  With t = (z - c) / h and a_L(t) the activations of the last hidden layer the
// sensor image of the decoder u(z) = mean + z V_known + g(z) V_unknown is linear in psi(t) = [1; t; a_L(t)] (P = 1 + m + H_L <= 81):
// the output layer and the target scaling are folded into the sensing matrix (py:mlp_sensing_matrix), so
//     F(t) = G_r psi(t),   rho = p - G_r psi(t),   J = -G_r d psi / d t,   d psi / d t = [0; I; D_L],
//     a_0 = t,  a_{l+1} = sigma(W_l a_l + b_l),   D_0 = I,  D_{l+1} = diag(sigma'(a_{l+1})) W_l D_l      (forward mode)
// with the free coordinates' columns only.  Everything but psi and d psi is rom_sense_sys.h: SnMlp below is its feature policy.
//
// One workgroup of 256 threads per system (query, start).  The value column goes by VALU in plain fp64: four lanes per unit take
// the inputs i = q, q + 4, .. in ascending order with fma, then two butterfly steps (xor 1, xor 2) and the bias -- one fixed
// order.  The tangent block W_l D_l, (H_{l+1} x H_l)(H_l x 16), runs on v_mfma_f64_16x16x4_f64: wave w takes the 16-row tile w of
// W_l as the A operand, D_l sits in LDS with row stride 16 like d psi.  Rows and k-steps beyond the widths are masked to exact
// zeros at the operand loads, and units beyond a width are never stored or read: a padded logistic unit (sigma(0) = 1/2) does
// not exist anywhere.  A trial evaluates the value column only; the Jacobian both (the activations a trial has overwritten are
// made again).
// The hidden weights (at most 9 216 + 192 doubles, shared by every system like G_r) are read through L2: in LDS they would add up to
// 73.5 KB to a workgroup and leave one workgroup per CU at the large shapes; here the policy's LDS is three activation columns and
// two D blocks (17.5 KB), 48.2 KB with the rest at the largest shape, so three workgroups fit a CU by LDS as by registers.  Both
// placements were measured (profiles/mlp_sense_resources.txt): the copy in LDS is 2.9 x slower at (12, (64, 64, 64), r = 40).
#include <cmath>

#include "rom_sense_sys.h"

namespace {

constexpr int MS_LMAX = 3, MS_HMAX = 64;
// The measured alternative ("rom_mlp_sense"): `make EXTRA=-DMS_STAGE_WEIGHTS=1` copies the hidden weights into LDS
// behind the map at the start of every workgroup and reads them from there.
#ifndef MS_STAGE_WEIGHTS
#define MS_STAGE_WEIGHTS 0
#endif

struct MsNet {
  int L, act;              // hidden layers; 0 tanh, 1 logistic, 2 relu
  int width[MS_LMAX + 1];  // m, H_1 .. H_L
  int woff[MS_LMAX], boff[MS_LMAX];
  const double* WH;
  long long n;             // doubles of WH
};

// the policy's LDS at m.feat: the activation columns a_1 .. a_L, then the two D blocks (64 x 16 each)
constexpr int MS_LDS = MS_LMAX * MS_HMAX + 2 * MS_HMAX * SN_LDD;

struct SnMlp {
  const MsNet& n;
  const double* wh;   // the hidden weights: n.WH (through L2), or their copy in LDS
  unsigned long long evaluations = 0;
  __device__ SnMlp(const MsNet& n_, const double* wh_) : n(n_), wh(wh_) {}

  // py:mlp_hidden_features: a_1 .. a_L at the coordinates sm[thx ..) -> the policy's columns
  __device__ void forward(double* sm, const SnLds& m, int thx) {
    const int tid = threadIdx.x, u = tid >> 2, q = tid & 3;
    for (int l = 0; l < n.L; ++l) {
      const int hin = n.width[l], hout = n.width[l + 1];
      const double* in = l == 0 ? sm + thx : sm + m.feat + (l - 1) * MS_HMAX;
      const double* wrow = wh + n.woff[l] + size_t(u < hout ? u : 0) * hin;
      double s = 0.0;
      if (u < hout)
        for (int i = q; i < hin; i += 4) s = fma(wrow[i], in[i], s);
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      if (u < hout && q == 0) {
        const double z = s + wh[n.boff[l] + u];
        sm[m.feat + l * MS_HMAX + u] = n.act == 0 ? tanh(z) : n.act == 1 ? 1.0 / (1.0 + exp(-z)) : (z > 0.0 ? z : 0.0);
      }
      __syncthreads();
    }
    evaluations += 1;
  }

  // psi = [1; t; a_L]
  __device__ void values(double* sm, const SnLds& m, int thx) {
    const int tid = threadIdx.x, nm = n.width[0], hl = n.width[n.L];
    forward(sm, m, thx);
    for (int p = tid; p < m.ppad; p += SN_THREADS) {
      double v = 0.0;
      if (p == 0)
        v = 1.0;
      else if (p <= nm)
        v = sm[thx + p - 1];
      else if (p <= nm + hl)
        v = sm[m.feat + (n.L - 1) * MS_HMAX + p - 1 - nm];
      sm[m.phi + p] = v;
    }
    __syncthreads();
  }

  // d psi / d t = [0; I; D_L] of the free coordinates at sm[m.th ..)
  __device__ void tangents(double* sm, const SnLds& m, int kf, const int* fc) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nm = n.width[0], c = lane & 15, kq = lane >> 4;
    forward(sm, m, m.th);
    double* D[2] = {sm + m.feat + MS_LMAX * MS_HMAX, sm + m.feat + MS_LMAX * MS_HMAX + MS_HMAX * SN_LDD};
    // the rows 0 .. m of d psi, the rows P .. ppad, and D_0: the unit column of its coordinate in every free column
    for (int x = tid; x < m.ppad * SN_LDD; x += SN_THREADS) {
      const int p = x >> 4, cc = x & 15;
      if (p <= nm || p > nm + n.width[n.L]) sm[m.dphi + x] = (p >= 1 && p <= nm && cc < kf && fc[cc] == p - 1) ? 1.0 : 0.0;
    }
    for (int x = tid; x < nm * SN_LDD; x += SN_THREADS) D[0][x] = ((x & 15) < kf && fc[x & 15] == (x >> 4)) ? 1.0 : 0.0;
    __syncthreads();
    for (int l = 0; l < n.L; ++l) {
      const int hin = n.width[l], hout = n.width[l + 1];
      const double* Din = D[l & 1];
      double* Dout = l + 1 == n.L ? sm + m.dphi + (1 + nm) * SN_LDD : D[(l + 1) & 1];
      const double* act = sm + m.feat + l * MS_HMAX;
      if (w * 16 < hout) {   // (MFMA layout: see SnSys::jacobian)
        const int row = w * 16 + c;
        const double* wrow = wh + n.woff[l] + size_t(row < hout ? row : 0) * hin;
        d4_t acc = {0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 < hin; k0 += 4) {
          const int k = k0 + kq;
          const double av = (row < hout && k < hin) ? wrow[k] : 0.0;
          const double bv = k < hin ? Din[k * SN_LDD + c] : 0.0;
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
        }
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const int i = w * 16 + kq + 4 * g4;
          if (i < hout) {
            const double a = act[i];
            const double ds = n.act == 0 ? 1.0 - a * a : n.act == 1 ? a * (1.0 - a) : (a > 0.0 ? 1.0 : 0.0);
            Dout[i * SN_LDD + c] = c < kf ? ds * acc[g4] : 0.0;
          }
        }
      }
      __syncthreads();
    }
  }
};

__global__ __launch_bounds__(SN_THREADS) void k_mlp_sense(const SnArgs a, const SnBox box, const MsNet net) {
  extern __shared__ __align__(16) double ms_lds[];
  const SnLds m(a.P, a.r, MS_LDS);
  const double* wh = net.WH;
  if (MS_STAGE_WEIGHTS) {   // (the first barrier of sn_run comes before the first use)
    for (int x = threadIdx.x; x < net.n; x += SN_THREADS) ms_lds[m.total + x] = net.WH[x];
    wh = ms_lds + m.total;
  }
  SnMlp F(net, wh);
  bool bad = false;
  for (long long x = (long long)blockIdx.x * SN_THREADS + threadIdx.x; x < net.n; x += (long long)gridDim.x * SN_THREADS)
    bad |= !sn_finite(net.WH[x]);
  sn_run(a, box, m, ms_lds, F, bad);
}

}  // namespace

extern "C" int rom_mlp_sense(rom_ctx* ctx, int m, int n_hidden, const int* hidden, int activation, rom_buf* WH, int r, rom_buf* Gr,
                             rom_buf* P, size_t p_off, int64_t ldp, int K, int t, rom_buf* T0, const double* lo_host,
                             const double* hi_host, rom_buf* AUX, int max_iter, double misfit_tol, rom_buf* OUT, size_t out_off,
                             int64_t ldo, double* info8_host) {
  ROM_CHECK(ctx && WH && Gr && lo_host && hi_host, "rom_mlp_sense: null argument (context, WH, Gr, lo or hi)");
  ROM_CHECK(m >= 1 && m <= SN_MMAX, "rom_mlp_sense: m = %d coordinates, between 1 and %d", m, SN_MMAX);
  ROM_CHECK(n_hidden >= 1 && n_hidden <= MS_LMAX && hidden, "rom_mlp_sense: %d hidden layers, between 1 and %d", n_hidden, MS_LMAX);
  ROM_CHECK(activation >= 0 && activation <= 2, "rom_mlp_sense: activation = %d, one of 0 (tanh), 1 (logistic), 2 (relu)", activation);
  MsNet net;
  net.L = n_hidden, net.act = activation, net.width[0] = m;
  size_t at = 0;
  for (int l = 0; l < MS_LMAX; ++l) net.width[l + 1] = 0, net.woff[l] = net.boff[l] = 0;
  for (int l = 0; l < n_hidden; ++l) {
    ROM_CHECK(hidden[l] >= 1 && hidden[l] <= MS_HMAX, "rom_mlp_sense: hidden layer %d has width = %d units, between 1 and %d", l, hidden[l],
              MS_HMAX);
    net.width[l + 1] = hidden[l];
    net.woff[l] = int(at);
    at += size_t(hidden[l]) * net.width[l];
  }
  for (int l = 0; l < n_hidden; ++l) {
    net.boff[l] = int(at);
    at += size_t(hidden[l]);
  }
  const int np = 1 + m + hidden[n_hidden - 1];
  ROM_CHECK(r >= 1 && r <= SN_RMAX, "rom_mlp_sense: r = %d sensor coordinates, between 1 and %d", r, SN_RMAX);
  ROM_CHECK(WH->n >= at, "rom_mlp_sense: WH holds %zu doubles, the hidden layers have %zu", WH->n, at);
  ROM_CHECK(Gr->n >= size_t(r) * np, "rom_mlp_sense: Gr holds %zu doubles, r (1 + m + H_L) = %zu needed", Gr->n, size_t(r) * np);
  net.WH = WH->p, net.n = (long long)at;
  const SnLds map(np, r, MS_LDS);
  const size_t lds = (size_t(map.total) + (MS_STAGE_WEIGHTS ? at : 0)) * sizeof(double);
  ROM_CHECK(lds <= (MS_STAGE_WEIGHTS ? 160 : 64) * 1024, "rom_mlp_sense: %zu bytes of LDS", lds);   // (48.2 KB at most)
  if (MS_STAGE_WEIGHTS) ROM_HIP(hipFuncSetAttribute((const void*)k_mlp_sense, hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));

  SnBox box;
  for (int j = 0; j < SN_MMAX; ++j) {
    box.lo[j] = j < m ? lo_host[j] : 0.0;
    box.hi[j] = j < m ? hi_host[j] : 0.0;
  }
  const LmCall call = {"rom_mlp_sense", r, K, t, SN_TMAX, max_iter, m, m, "T0", "m", "m", P, T0, AUX, OUT, p_off, out_off,
                       ldp, ldo, info8_host, "mlp_sense_select", "NaN / Inf in WH, Gr, P or T0", ROM_ERR_INVALID};
  return lm_launch(ctx, call, [&](double* W, int ldw, unsigned long long* counters) {
    SnArgs a;
    a.m = m, a.P = np, a.r = r, a.t = t, a.max_iter = max_iter;
    a.Gr = Gr->p, a.Pq = P->p + p_off, a.ldp = ldp, a.T0 = T0->p, a.aux = AUX ? AUX->p : nullptr, a.misfit_tol = misfit_tol;
    a.W = W, a.ldw = ldw, a.counters = counters, a.status = ctx->d_status;
    char nm[48];
    rom_prof_name(nm, sizeof nm, "mlp_sense", "_m%d_h%d_r%d", m, hidden[n_hidden - 1], r);
    ROM_PROF(ctx, nm, 0.0, 0.0);
    k_mlp_sense<<<K * t, SN_THREADS, lds, ctx->stream>>>(a, box, net);
  });
}
