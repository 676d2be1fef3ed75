// The system of the sensor state estimation on a manifold whose sensor image is LINEAR in a feature vector psi(t) (internal):
//     F(t) = G_r psi(t),   residual rho = p - G_r psi(t),   J = d rho / d t = -G_r d psi / d t.
// rom_sense.hip (psi: the Legendre products of a rom_poly map) and rom_mlp_sense.hip (psi = [1; t; the last hidden layer of a
// rom_mlp map]) share everything but the production of psi and d psi / d t: the double-double residual and |rho|^2, the product
// G_r [d psi] on v_mfma_f64_16x16x4_f64, J^T J, g, the step, sigma_min, the start of a system and the kernel's body.  A FEATURE
// POLICY Feat supplies the rest:
//   values(sm, m, thx)             psi at the coordinates sm[thx ..) -> sm[m.phi ..), the rows P .. ppad exact zeros; ends with a
//                                  barrier
//   tangents(sm, m, kf, fc)        d psi / d t at sm[m.th ..) of the free coordinates fc[0 .. kf) -> sm[m.dphi ..) (ppad x 16, row
//                                  stride SN_LDD; the columns kf .. 16 and the rows P .. ppad exact zeros); ends with a barrier
//   evaluations                    its work counter
// and owns `feat` doubles of the LDS map at m.feat.  The iteration itself is lm_drive (rom_lm_drive.h); SnSys below is its model.
#pragma once
#include "rom_lm_drive.h"
#include "rom_mma.h"

namespace {

constexpr int SN_MMAX = 16, SN_PMAX = 96, SN_RMAX = 96, SN_TMAX = 8;
constexpr int SN_THREADS = LMS_THREADS;
constexpr int SN_LDD = 16;   // row stride of d psi: a row is one MFMA operand row (16 lanes read 128 contiguous bytes)

struct SnBox {
  double lo[SN_MMAX], hi[SN_MMAX];
};

struct SnArgs {
  int m, P, r, t, max_iter;
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

// the LDS map, in doubles (host and device); `feat` doubles at `feat` belong to the feature policy
struct SnLds {
  int ldr, ldk, ppad;
  int phi, dphi, feat, Js, JtJ, Hs, hinv, rho, rhon, ps, th, thn, g, lo, hi, scal, idx, total;
  __host__ __device__ SnLds(int P, int r, int feat_doubles) {
    ldr = r | 1, ldk = SN_MMAX + 1, ppad = (P + 3) & ~3;
    int at = 0;
    auto take = [&](int cnt) {
      const int o = at;
      at += cnt;
      return o;
    };
    dphi = take(ppad * SN_LDD), phi = take(ppad), feat = take(feat_doubles);
    Js = take(SN_MMAX * ldr), JtJ = take(SN_MMAX * ldk), Hs = take(SN_MMAX * ldk), hinv = take(SN_MMAX);
    rho = take(r), rhon = take(r), ps = take(r);
    th = take(SN_MMAX), thn = take(SN_MMAX), g = take(SN_MMAX), lo = take(SN_MMAX), hi = take(SN_MMAX);
    scal = take(8);             // the slots LMS_* of rom_lm_drive.h; [7]: the number of free coordinates
    idx = take(SN_MMAX);        // 2 x 16 ints: the coordinate of free column c | the free column of coordinate j (-1: pinned)
    total = at;
  }
};

__device__ __forceinline__ bool sn_finite(double v) { return fabs(v) < __builtin_huge_val(); }

// Double-double sums for the residual and its squared norm.  Off the manifold |rho| is a few percent of |G_r psi|: in plain
// fp64 the rounding of G_r psi and of the sum of squares puts noise of eps |rho| |G_r psi| on f, the acceptance f_new < f is then
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

template <class Feat>
struct SnSys {
  const SnArgs& a;
  const SnLds& m;
  double* sm;
  Feat& F;
  int kf = 0;   // free coordinates
  __device__ SnSys(const SnArgs& a_, const SnLds& m_, double* sm_, Feat& F_) : a(a_), m(m_), sm(sm_), F(F_) {}
  __device__ const int* free_coord() const { return reinterpret_cast<const int*>(sm + m.idx); }
  __device__ const int* free_column() const { return reinterpret_cast<const int*>(sm + m.idx) + SN_MMAX; }
  __device__ int cols() const { return kf; }
  __device__ unsigned long long work() const { return F.evaluations; }

  // py:`F, _ = features(new, False)` .. `fn`: psi(t), rho = p - G_r psi -> rhon, |rho|^2 -> scal[LMS_FN]
  __device__ void eval(int thx) {
    const int tid = threadIdx.x, lane = tid & 63, P = a.P, r = a.r, l16 = tid & 15;
    F.values(sm, m, thx);
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

  // py:`Ja`, `JtJ`, `g` at the current t (th) and its rho: d psi / d t of the free coordinates, J = -G_r d psi -> Js (column c at
  // Js + c ldr), J^T J -> JtJ, g = J^T rho
  __device__ void jacobian() {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, P = a.P, r = a.r;
    double* Js = sm + m.Js;
    F.tangents(sm, m, kf, free_coord());
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

// The body of a kernel, one workgroup of SN_THREADS per system, after the policy has set up its own part of the LDS (no barrier
// needed in between: the first one is below): the box and the free coordinates, the query's row, the clipped start, the scale
// (py: `th = clip(..)`, `scale`), the checks of G_r, P and T0, the start's residual and the iteration.  `bad`: what the caller
// has found in its own operands.
template <class Feat>
__device__ void sn_run(const SnArgs& a, const SnBox& box, const SnLds& m, double* sm, Feat& F, bool bad) {
  const int tid = threadIdx.x, nm = a.m, r = a.r;
  const long long sys = blockIdx.x, query = sys / a.t;
  SnSys<Feat> S(a, m, sm, F);
  double* out = a.W + size_t(sys) * a.ldw;
  {
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
    if (bad) atomicOr(a.status, 1);   // NaN / Inf in an operand: the call fails (the loops below are bounded whatever the data)
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
