// The small dense layer of the basis stage: symmetric eigenproblems of at most a few hundred unknowns (up to SE_GRID_MAX for
// the POD's whole-matrix fallback) and the whitening of small Gram matrices, all on the device.  Three routes by order --
// kb_jacobi32 (n <= 32, eigenvectors), kb_small_eig (n <= SE_LDS_MAX, one workgroup, every mode), jacobi_grid (beyond: one
// launch per round over the whole chip) -- and the pivoted-Cholesky whitening (kb_pivchol_whiten32 / kb_pivchol_whiten).
// Callers: romb_gram_transform and the orthonormalisation entries of rom_basis.hip, rom_pod.hip, rom_pca_tall.hip, rom_poly.hip,
// rom_sensors.hip.  Reference counterparts: LAPACK's dsyevd / dpotrf inside the host-side steps of ReducedBasisPCA.build
// (src/lib/ReducedBasis.py:189-200).
#include <algorithm>
#include <cmath>
#include <vector>

#include "rom_ops.h"

#include "rom_basis_int.h"
#include "rom_small_dense.h"

// =====================================================================================================================
// symmetric eigenproblem of a small matrix: cyclic Jacobi, one workgroup
// =====================================================================================================================
// A (n x n, leading dimension lda, symmetrised on entry) = sum_i lam_i q_i q_i^T.  Rotations of a round act on disjoint
// index pairs (round-robin tournament ordering), so a round is three workgroup-wide phases: angles, row rotations of A
// and of the accumulated eigenvector rows, column rotations of A.  A rotation is skipped when |a_pq| <= eps sqrt(a_pp a_qq)
// -- the criterion under which Jacobi computes the small eigenvalues of a graded positive definite matrix to high
// RELATIVE accuracy (Demmel-Veselic), which is what the whitening of nearly dependent sketches and the Rayleigh-Ritz
// rounds of the POD rely on.  512 threads; the matrix and the eigenvector rows live in LDS (n <= SE_LDS_MAX, 160 KB opted
// in), addressed with ds_read / ds_write; larger orders take jacobi_grid below.
// Output (mode): eigenvalues descending in lam, and in T (ld ldt)
//   SE_EIG     rows = eigenvectors q_i^T
//   SE_WHITEN  row i = q_i^T / sqrt(lam_i) for lam_i > rel_tol * lam_0, zero rows otherwise
//              (T X has orthonormal rows spanning the numerical row space of X when A = X X^T)
//   SE_LOWDIN  sum_i q_i q_i^T / sqrt(lam_i) over the same i: the symmetric inverse square root (nearest orthonormal rows)
constexpr int SE_TPB = 512, SE_WAVES = SE_TPB / 64;

// kb_small_eig's LDS as pointers (SmallEigLds has the offsets), with the sizes every step needs: order, row stride, order
// rounded up to even, pairs per round.  As: the matrix; Vt: the eigenvector rows; cs, sn [half]: the rotations of a round;
// ev, nu2 [n]: eigenvalues, noise levels; red [SE_WAVES]: partials of a reduction; pp, qq [half]: the pairs of a round
// (qq = -1: the dummy index of an odd n); perm [n]: perm[i] = index of the i-th largest eigenvalue; flag: the sweep rotated
struct SmallEig {
  int n, ld, ne, half;
  double *As, *Vt, *cs, *sn, *ev, *nu2, *red;
  int *pp, *qq, *perm, *flag;
  __device__ SmallEig(double* sm, int n_) : n(n_), ld(n_ | 1), ne(n_ + (n_ & 1)), half((n_ + (n_ & 1)) / 2) {
    const SmallEigLds L(n);
    auto dbl = [sm](unsigned off) { return reinterpret_cast<double*>(reinterpret_cast<char*>(sm) + off); };
    auto integer = [sm](unsigned off) { return reinterpret_cast<int*>(reinterpret_cast<char*>(sm) + off); };
    As = dbl(L.As), Vt = dbl(L.Vt), cs = dbl(L.cs), sn = dbl(L.sn), ev = dbl(L.ev), nu2 = dbl(L.nu2), red = dbl(L.red);
    pp = integer(L.pp), qq = integer(L.qq), perm = integer(L.perm), flag = integer(L.flag);
  }
};

// As <- (A + A^T) / 2, Vt <- I; returns this thread's share of max |a_ii| (no barrier)
static __device__ double se_load(const SmallEig& S, const double* A, int lda) {
  const int t = threadIdx.x, n = S.n, ld = S.ld;
  double dmax = 0.0;
  for (int idx = t; idx < n * n; idx += SE_TPB) {
    const int r = idx / n, c = idx % n;
    const double v = 0.5 * (A[size_t(r) * lda + c] + A[size_t(c) * lda + r]);
    S.As[r * ld + c] = v;
    S.Vt[r * ld + c] = r == c ? 1.0 : 0.0;
    if (r == c) dmax = fmax(dmax, fabs(v));
  }
  return dmax;
}

// Rows that are orthogonal up to a moderate defect -- G = g (I + E), g = mean diagonal, ||E|| < 1/2: rotated Ritz
// vectors of a subspace iteration, lifted modes, a Gaussian start block -- need no eigen-decomposition: the inverse
// square root comes from the coupled Newton-Schulz iteration
//     W = (3 I - Z Y) / 2 ,  Y <- Y W ,  Z <- W Z        (Y_0 = I + E, Z_0 = I;  Y -> (I+E)^(1/2), Z -> (I+E)^(-1/2))
// which converges quadratically: a handful of n^3 products in LDS instead of ten Jacobi sweeps of n - 1 dependent
// rounds each.  The transform is symmetric, so it serves the whitening and the symmetric orthonormalisation alike.
// Eigenvalues reported: the diagonal of G.  (W lives in the caller's T, which is overwritten at the end anyway; ns_ws:
// 2 n^2 doubles of global scratch for the next iterates.)
// SE_NS_DONE: lam and T are written.  SE_NS_ABANDONED: As and Vt are spent and the caller loads the matrix again.
enum SeNs { SE_NS_SKIPPED, SE_NS_DONE, SE_NS_ABANDONED };
static __device__ SeNs se_newton_schulz(const SmallEig& S, double* lam, double* T, int ldt, double* ns_ws) {
  const int t = threadIdx.x, n = S.n, ld = S.ld;
  double *As = S.As, *Vt = S.Vt, *red = S.red;
  double tr = 0.0;
  for (int i = t; i < n; i += SE_TPB) tr += As[i * ld + i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) tr += __shfl_down(tr, o, 64);
  __syncthreads();
  if ((t & 63) == 0) red[t >> 6] = tr;
  __syncthreads();
  double gmean = 0.0;
#pragma unroll
  for (int w = 0; w < SE_WAVES; ++w) gmean += red[w];
  gmean /= double(n);
  double esum = 0.0;  // max row sum of |E|: an upper bound of ||E||_2
  for (int r = t; r < n; r += SE_TPB) {
    double rs = 0.0;
    for (int c = 0; c < n; ++c) rs += fabs(As[r * ld + c] / gmean - (r == c ? 1.0 : 0.0));
    esum = fmax(esum, rs);
  }
  esum = block_max<SE_WAVES>(esum, red);
  // (||E||_2 < 1 is what the theory asks for; the iteration is tried up to a row-sum bound of 2 and abandoned -- matrix
  // reloaded, Jacobi instead -- if the defect ||Z Y - I|| stops falling: a singular G.  Not beyond 2: an eigenvalue of G / g
  // above 3 makes W_0 = (3 I - G / g) / 2 indefinite, and the iteration then CONVERGES, its defect falling all the way, to an
  // inverse square root with a negative eigenvalue -- a whitening, but not the symmetric positive definite one.  Below 2
  // the spectrum of G / g lies in (0, 3), every W stays positive definite and only the principal root can be reached)
  if (!(gmean > 0.0 && esum < 2.0)) return SE_NS_SKIPPED;
  double dev_prev = 1e300;
  for (int i = t; i < n; i += SE_TPB) lam[i] = As[i * ld + i];
  __syncthreads();
  for (int idx = t; idx < n * n; idx += SE_TPB) {
    const int r = idx / n, c = idx % n;
    As[r * ld + c] /= gmean;
  }
  __syncthreads();
  double* Yn = ns_ws;                    // new Y, Z of an iteration (global scratch, L2 resident)
  double* Zn = ns_ws + size_t(n) * n;
  for (int itn = 0; itn < 20; ++itn) {
    double dev = 0.0;
    for (int idx = t; idx < n * n; idx += SE_TPB) {
      const int r = idx / n, c = idx % n;
      double acc = 0.0;
      for (int k = 0; k < n; ++k) acc += Vt[r * ld + k] * As[k * ld + c];   // (Z Y)_rc
      dev = fmax(dev, fabs(acc - (r == c ? 1.0 : 0.0)));
      T[size_t(r) * ldt + c] = 0.5 * ((r == c ? 3.0 : 0.0) - acc);
    }
    dev = block_max<SE_WAVES>(dev, red);   // ||Z Y - I||_max; its barriers also order the writes of W before the reads below
    if (dev < 4e-16 * n) break;
    if (!(dev < dev_prev) || itn == 19) return SE_NS_ABANDONED;
    dev_prev = dev;
    for (int idx = t; idx < n * n; idx += SE_TPB) {
      const int r = idx / n, c = idx % n;
      double ay = 0.0, az = 0.0;
      for (int k = 0; k < n; ++k) {
        ay += As[r * ld + k] * T[size_t(k) * ldt + c];   // (Y W)_rc
        az += T[size_t(r) * ldt + k] * Vt[k * ld + c];   // (W Z)_rc
      }
      Yn[idx] = ay;
      Zn[idx] = az;
    }
    __syncthreads();   // every thread has read the old Y, Z (and written its part of the new ones)
    for (int idx = t; idx < n * n; idx += SE_TPB) {
      const int r = idx / n, c = idx % n;
      As[r * ld + c] = Yn[idx];
      Vt[r * ld + c] = Zn[idx];
    }
    __syncthreads();
  }
  const double sc = 1.0 / sqrt(gmean);
  for (int idx = t; idx < n * n; idx += SE_TPB) {
    const int r = idx / n, c = idx % n;
    T[size_t(r) * ldt + c] = sc * 0.5 * (Vt[r * ld + c] + Vt[c * ld + r]);
  }
  return SE_NS_DONE;
}

// Eigenvector rows under the rotations of a round, Vt <- J^T Vt: the four items base + u SE_TPB + t of this thread, item
// (k, j) = entries j of the rows (p_k, q_k) -- all loads, then all stores, as for the blocks of the matrix below
static __device__ void se_rotate_vt_items(const SmallEig& S, int base) {
  const int t = threadIdx.x, n = S.n, ld = S.ld;
  double* Vt = S.Vt;
  double op[4], oq[4];
  int ap[4], aq[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int idx = base + u * SE_TPB + t;
    ap[u] = -1;
    if (idx < S.half * n) {
      const int k = idx / n, j = idx - k * n;
      const double s = S.sn[k];
      if (s != 0.0) {  // (also every pair with the dummy index)
        const int p = S.pp[k], q = S.qq[k];
        const double c = S.cs[k];
        const double vp = Vt[p * ld + j], vq = Vt[q * ld + j];
        ap[u] = p * ld + j;
        aq[u] = q * ld + j;
        op[u] = c * vp - s * vq;
        oq[u] = s * vp + c * vq;
      }
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (ap[u] >= 0) {
      Vt[ap[u]] = op[u];
      Vt[aq[u]] = oq[u];
    }
}

// The sweeps: As <- diagonal, Vt <- eigenvector rows.  A rotation is applied when |a_pq| > tol sqrt(|a_pp a_qq|) -- the
// relative criterion under which graded matrices keep their small eigenvalues -- AND |a_pq| > tol nu_p nu_q, the rounding
// noise of the entry: nu_i^2 is what a_ii would be had no cancellation happened (initially |a_ii| for a Gram-like matrix;
// under a rotation c^2 nu_p^2 + s^2 nu_q^2).  A direction that rank deficiency has cancelled to nothing keeps its nu, so the
// rounding residue that couples it to the rest is recognised as such and the sweeps end; without it they never do (each
// rotation re-creates the residue).  gram_like == 0 (a general symmetric matrix such as Y G Y^T: all entries carry
// eps ||A||): nu_i^2 = max |a_ii|.
static __device__ void se_jacobi_sweeps(const SmallEig& S, int gram_like, double dmax) {
  const int t = threadIdx.x, n = S.n, ld = S.ld, ne = S.ne, half = S.half;
  double *As = S.As, *cs = S.cs, *sn = S.sn, *nu2 = S.nu2;
  int *pp = S.pp, *qq = S.qq, *flag = S.flag;
  const double tol2 = jacobi_tol2(n, gram_like), floor_abs = jacobi_floor(dmax);
  for (int i = t; i < n; i += SE_TPB) nu2[i] = jacobi_nu2_init(gram_like, As[i * ld + i], dmax);
  __syncthreads();
  for (int sweep = 0; sweep < 40; ++sweep) {
    if (t == 0) *flag = 0;
    __syncthreads();
    for (int r = 0; r < ne - 1; ++r) {
      if (t < half) {
        const JacobiPair pr = jacobi_pair(t, r, ne - 1);
        int p = pr.p, q = pr.q;
        double c = 1.0, s = 0.0;
        if (q < n) {
          const double app = As[p * ld + p], aqq = As[q * ld + q], apq = As[p * ld + q];
          const double np2 = nu2[p], nq2 = nu2[q], apq2 = apq * apq;
          if (apq2 > tol2 * fabs(app * aqq) && fabs(apq) > floor_abs && apq2 > tol2 * np2 * nq2) {
            // t = tan(phi) = sign(a) b / (|a| + sqrt(a^2 + b^2)), a = a_qq - a_pp, b = 2 a_pq (the smaller root of
            // t^2 + 2 theta t - 1 = 0, theta = a / b); c = 1 / sqrt(1 + t^2), s = t c.  (This kernel's own formula, with its
            // square root and its division: jacobi_rotation rounds differently.)
            const double a = aqq - app, bb = 2.0 * apq;
            const double tt = (a >= 0 ? bb : -bb) / (fabs(a) + sqrt(a * a + bb * bb));
            c = se_rsqrt(1.0 + tt * tt);
            s = tt * c;
            nu2[p] = c * c * np2 + s * s * nq2;
            nu2[q] = s * s * np2 + c * c * nq2;
            *flag = 1;
          }
        } else {
          q = -1;  // p is paired with the dummy index of an odd n: no rotation, but its row / column still takes the others'
        }
        cs[t] = c;
        sn[t] = s;
        pp[t] = p;
        qq[t] = q;
      }
      __syncthreads();
      // A <- J^T A J as disjoint 2 x 2 blocks: block (k, l) = rows (p_k, q_k) x columns (p_l, q_l) becomes R_k B R_l^T;
      // one pass, no barrier between the row and the column rotations.  (c, s) = (1, 0) for pairs that do not rotate.
      // Items are taken four at a time -- all loads, then all stores: the blocks are disjoint, but the compiler cannot
      // know that, and one item at a time is a chain of LDS round trips.
      for (int base = 0; base < half * half; base += 4 * SE_TPB) {
        double o00[4], o01[4], o10[4], o11[4];
        int a00[4], a01[4], a10[4], a11[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int idx = base + u * SE_TPB + t;
          a00[u] = a01[u] = a10[u] = a11[u] = -1;
          if (idx < half * half) {
            const int k = idx / half, l = idx - k * half;
            const double sk = sn[k], sl = sn[l];
            if (sk != 0.0 || sl != 0.0) {  // (s, not c, is the test: c rounds to 1 for tiny angles)
              const int pk = pp[k], qk = qq[k], pl = pp[l], ql = qq[l];
              const double ck = cs[k], cl = cs[l];
              const bool vk = qk >= 0, vl = ql >= 0;  // (a pair with the dummy index has one real row / column)
              const double b00 = As[pk * ld + pl], b01 = vl ? As[pk * ld + ql] : 0.0;
              const double b10 = vk ? As[qk * ld + pl] : 0.0, b11 = (vk && vl) ? As[qk * ld + ql] : 0.0;
              double n00, n01, n10, n11;
              jacobi_block_update(ck, sk, cl, sl, b00, b01, b10, b11, n00, n01, n10, n11);
              a00[u] = pk * ld + pl;
              o00[u] = n00;
              if (vl) { a01[u] = pk * ld + ql; o01[u] = n01; }
              if (vk) { a10[u] = qk * ld + pl; o10[u] = n10; }
              if (vk && vl) { a11[u] = qk * ld + ql; o11[u] = n11; }
            }
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (a00[u] >= 0) As[a00[u]] = o00[u];
          if (a01[u] >= 0) As[a01[u]] = o01[u];
          if (a10[u] >= 0) As[a10[u]] = o10[u];
          if (a11[u] >= 0) As[a11[u]] = o11[u];
        }
      }
      for (int base = 0; base < half * n; base += 4 * SE_TPB) se_rotate_vt_items(S, base);
      __syncthreads();
    }
    const int any = *flag;
    __syncthreads();
    if (!any) break;
  }
}

// ev <- diagonal of As, perm <- its descending order, lam <- the eigenvalues in that order
static __device__ void se_rank(const SmallEig& S, double* lam) {
  const int t = threadIdx.x, n = S.n;
  for (int i = t; i < n; i += SE_TPB) S.ev[i] = S.As[i * S.ld + i];
  __syncthreads();
  for (int i = t; i < n; i += SE_TPB) S.perm[rank_descending(S.ev, n, i)] = i;
  __syncthreads();
  for (int i = t; i < n; i += SE_TPB) lam[i] = S.ev[S.perm[i]];
}

// T by mode from the ranked eigenpairs (ev, perm, Vt)
static __device__ void se_write_T(const SmallEig& S, int mode, double rel_tol, double* T, int ldt) {
  const int t = threadIdx.x, n = S.n, ld = S.ld;
  const double *Vt = S.Vt, *ev = S.ev;
  const int* perm = S.perm;
  const double lmax = ev[perm[0]];
  if (mode == SE_LOWDIN) {
    for (int idx = t; idx < n * n; idx += SE_TPB) {
      const int r = idx / n, c = idx % n;
      double s = 0.0;
      for (int i = 0; i < n; ++i) {
        const double l = ev[i];
        if (l > rel_tol * lmax && l > 0.0) s += Vt[i * ld + r] * Vt[i * ld + c] / sqrt(l);
      }
      T[size_t(r) * ldt + c] = s;
    }
  } else {
    for (int idx = t; idx < n * n; idx += SE_TPB) {
      const int r = idx / n, c = idx % n, src = perm[r];
      double v = Vt[src * ld + c];
      if (mode == SE_WHITEN) {
        const double l = ev[src];
        v = (l > rel_tol * lmax && l > 0.0) ? v / sqrt(l) : 0.0;
      }
      T[size_t(r) * ldt + c] = v;
    }
  }
}

// The kernel: one workgroup of SE_TPB threads, SmallEigLds(n).bytes of dynamic LDS, the steps above in order (static
// functions, all inlined: the kernel makes no call).  ns_ws: 2 n^2 doubles of global scratch for se_newton_schulz.
__global__ __launch_bounds__(SE_TPB) void kb_small_eig(int n, const double* __restrict__ A, int lda, double* __restrict__ lam,
                                                       double* __restrict__ T, int ldt, int mode, double rel_tol, int gram_like,
                                                       double* __restrict__ ns_ws) {
  extern __shared__ __align__(16) double sm[];
  const SmallEig S(sm, n);
  const double dmax = block_max<SE_WAVES>(se_load(S, A, lda), S.red);
  if (mode != SE_EIG && dmax > 0.0) {   // the whitenings of nearly orthonormal rows: no eigen-decomposition
    const SeNs ns = se_newton_schulz(S, lam, T, ldt, ns_ws);
    if (ns == SE_NS_DONE) return;
    if (ns == SE_NS_ABANDONED) {   // start over for the eigen-decomposition
      __syncthreads();
      (void)se_load(S, A, lda);
      __syncthreads();
    }
  }
  se_jacobi_sweeps(S, gram_like, dmax);
  se_rank(S, lam);
  se_write_T(S, mode, rel_tol, T, ldt);
}

// Eigen-decomposition (SE_EIG) of a symmetric matrix of order n <= 32: jacobi32_run (rom_small_dense.h), 256 threads.
// The eigenproblems of the POD's Rayleigh-Ritz steps (b = 20 ... 32, graded, 5 ... 10 sweeps) are latency chains of a few
// hundred rounds each; same rotation criterion, same sweep order as kb_small_eig.
__global__ __launch_bounds__(256) void kb_jacobi32(int n, const double* __restrict__ A, int lda, double* __restrict__ lam,
                                                   double* __restrict__ T, int ldt, int gram_like) {
  __shared__ Jacobi32Lds L;
  __shared__ double red[4];
  const int t = threadIdx.x;
  double dmax = 0.0;
  for (int idx = t; idx < n * n; idx += 256) {
    const int r = idx / n, c = idx - r * n;
    const double v = 0.5 * (A[size_t(r) * lda + c] + A[size_t(c) * lda + r]);
    L.As[r * J32_LD + c] = v;
    L.Vt[r * J32_LD + c] = r == c ? 1.0 : 0.0;
    if (r == c) dmax = fmax(dmax, fabs(v));
  }
  dmax = block_max<4>(dmax, red);
  jacobi32_run<256>(n, L, gram_like, dmax);
  if (t < n) lam[t] = L.ev[L.perm[t]];
  for (int idx = t; idx < n * n; idx += 256) {
    const int r = idx / n, c = idx - r * n;
    T[size_t(r) * ldt + c] = L.Vt[L.perm[r] * J32_LD + c];
  }
}

// Rank-revealing whitening transform by PIVOTED CHOLESKY: A = X X^T (n x n Gram matrix, symmetrised on entry),
// P A P^T = L L^T with diagonal pivoting, stopped at the first pivot below rel_tol x the largest one (rank r);
// T = [L_r^-1  0] P, so that the first r rows of T X are orthonormal and the rest are zero.  The rows come out graded
// (row k is orthogonal to the k - 1 stronger ones) -- what the power steps of the range finder need -- and the whole
// thing is n dependent steps of one column each: tens of microseconds, where the eigen-decomposition of an
// ill-conditioned Gram matrix takes ten Jacobi sweeps of n - 1 rounds (1-2 ms).  Like every Gram-based orthonormalisation
// it resolves directions down to ~1e-8 of the strongest per round; callers run two rounds where that matters.
// lam: the squared pivots (descending), zeros behind the rank.  One workgroup, matrix in LDS (n <= SE_LDS_MAX).
__global__ __launch_bounds__(256) void kb_pivchol_whiten(int n, const double* __restrict__ A, int lda, double* __restrict__ lam,
                                                         double* __restrict__ T, int ldt, double rel_tol) {
  extern __shared__ __align__(16) double sm[];
  const int t = threadIdx.x, ld = n | 1;
  const PivcholLds lay(n);
  char* b = reinterpret_cast<char*>(sm);
  double* As = reinterpret_cast<double*>(b + lay.As);     // working matrix, lower triangle used
  double* Li = reinterpret_cast<double*>(b + lay.Li);     // L^-1 (r x r, lower)
  double* red = reinterpret_cast<double*>(b + lay.red);   // [4] values
  int* redi = reinterpret_cast<int*>(b + lay.redi);       // [4] indices
  int* perm = reinterpret_cast<int*>(b + lay.perm);       // perm[k] = original index of pivot k
  __shared__ int s_rank, s_piv;
  __shared__ double s_first;
  for (int idx = t; idx < n * n; idx += 256) {
    const int r = idx / n, c = idx % n;
    As[r * ld + c] = 0.5 * (A[size_t(r) * lda + c] + A[size_t(c) * lda + r]);
    Li[r * ld + c] = 0.0;
  }
  for (int i = t; i < n; i += 256) perm[i] = i;
  if (t == 0) s_rank = n;
  __syncthreads();
  for (int k = 0; k < n; ++k) {
    // pivot: largest remaining diagonal entry (first one on ties)
    double best = -1e300;
    int at = k;
    for (int j = k + t; j < n; j += 256) {
      const double d = As[j * ld + j];
      if (d > best) { best = d; at = j; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ob = __shfl_down(best, o, 64);
      const int oa = __shfl_down(at, o, 64);
      if (ob > best || (ob == best && oa < at)) { best = ob; at = oa; }
    }
    if ((t & 63) == 0) { red[t >> 6] = best; redi[t >> 6] = at; }
    __syncthreads();
    if (t == 0) {
      double bb = red[0];
      int ba = redi[0];
      for (int w = 1; w < 4; ++w)
        if (red[w] > bb || (red[w] == bb && redi[w] < ba)) { bb = red[w]; ba = redi[w]; }
      if (k == 0) s_first = bb;
      s_piv = (bb > rel_tol * s_first && bb > 0.0) ? ba : -1;
      if (s_piv < 0 && s_rank == n) s_rank = k;
    }
    __syncthreads();
    const int pv = s_piv;
    if (pv < 0) break;
    if (pv != k) {  // symmetric swap of rows / columns k and pv (full storage: both triangles kept consistent)
      for (int j = t; j < n; j += 256) {
        const double x = As[k * ld + j];
        As[k * ld + j] = As[pv * ld + j];
        As[pv * ld + j] = x;
      }
      __syncthreads();
      for (int i = t; i < n; i += 256) {
        const double x = As[i * ld + k];
        As[i * ld + k] = As[i * ld + pv];
        As[i * ld + pv] = x;
      }
      if (t == 0) { const int x = perm[k]; perm[k] = perm[pv]; perm[pv] = x; }
      __syncthreads();
    }
    const double lkk = sqrt(As[k * ld + k]);
    __syncthreads();
    for (int i = k + t; i < n; i += 256) As[i * ld + k] = i == k ? lkk : As[i * ld + k] / lkk;   // column k of L
    __syncthreads();
    const int m = n - k - 1;  // trailing update, full square (symmetric storage)
    for (int idx = t; idx < m * m; idx += 256) {
      const int i = k + 1 + idx / m, j = k + 1 + idx % m;
      As[i * ld + j] -= As[i * ld + k] * As[j * ld + k];
    }
    __syncthreads();
  }
  const int r = s_rank;
  // L^-1 by forward substitution, one column per thread: L x = e_j
  for (int j = t; j < r; j += 256) {
    for (int i = j; i < r; ++i) {
      double sacc = i == j ? 1.0 : 0.0;
      for (int q = j; q < i; ++q) sacc -= As[i * ld + q] * Li[q * ld + j];
      Li[i * ld + j] = sacc / As[i * ld + i];
    }
  }
  __syncthreads();
  // T[i, perm[q]] = Li[i, q] (q <= i < r), zero elsewhere
  for (int idx = t; idx < n * n; idx += 256) T[size_t(idx / n) * ldt + idx % n] = 0.0;
  __syncthreads();
  for (int idx = t; idx < r * r; idx += 256) {
    const int i = idx / r, q = idx % r;
    if (q <= i) T[size_t(i) * ldt + perm[q]] = Li[i * ld + q];
  }
  for (int i = t; i < n; i += 256) lam[i] = i < r ? As[i * ld + i] * As[i * ld + i] : 0.0;
}


// The same factorisation for n <= 32 (the row blocks of the POD's sketch passes, six calls per pass): ONE barrier per step.
// No row / column is moved -- a bit mask of the indices still in play replaces the symmetric swap, the factor's column k is
// stored by ORIGINAL row index (Lc[i][k]) -- every wave finds the pivot for itself (an LDS atomic max over keys that
// carry the index: no shuffle chain, no barrier), the trailing update and the factor's
// column are one phase (the update reads row / column pv only, which it does not write), and L^-1 is one forward substitution
// per lane on REGISTERS (fully unrolled; the generic kernel's column-per-thread loop reads back what it has just stored to
// LDS, 500 dependent round trips for the first column).  Same pivots (largest remaining diagonal entry, first on ties), same
// stopping rule, same outputs as kb_pivchol_whiten up to the rounding of x / sqrt(d) against x * (1 / sqrt(d)).
__global__ __launch_bounds__(256) void kb_pivchol_whiten32(int n, const double* __restrict__ A, int lda, double* __restrict__ lam,
                                                           double* __restrict__ T, int ldt, double rel_tol) {
  constexpr int LD = 33;
  __shared__ double As[32 * LD], Lc[32 * LD], dpiv[32];
  __shared__ unsigned long long smax[4];
  __shared__ int perm[32];
  const int t = threadIdx.x;
  for (int idx = t; idx < 32 * 32; idx += 256) {
    const int r = idx >> 5, c = idx & 31;
    As[r * LD + c] = (r < n && c < n) ? 0.5 * (A[size_t(r) * lda + c] + A[size_t(c) * lda + r]) : 0.0;
    Lc[r * LD + c] = 0.0;
  }
  __syncthreads();
  unsigned active = n >= 32 ? 0xffffffffu : ((1u << n) - 1u);
  double first = 0.0;
  int rank = n;
  const int w = t >> 6, lane = t & 63;
  const int j = t & 31, i0 = t >> 5;   // the four entries of a thread: (i0 + 8 u, j) -- the same for every step (nothing moves)
  const unsigned mj = 1u << j;
  for (int k = 0; k < n; ++k) {
    // pivot = largest remaining diagonal entry: one LDS atomic max per lane on a key = the entry's bits with the low five
    // replaced by 31 - index (positive doubles order like their bit patterns; entries that agree to 2^-47 count as ties and
    // the lower index wins, like the first-on-ties rule of the generic kernel).  Each wave does this for itself.
    if (lane == 0) smax[w] = 0ull;
    __builtin_amdgcn_wave_barrier();
    if (lane < 32 && ((active >> lane) & 1u)) {
      const double d = As[lane * LD + lane];
      if (d > 0.0) atomicMax(&smax[w], (static_cast<unsigned long long>(__double_as_longlong(d)) & ~31ull) | unsigned(31 - lane));
    }
    __builtin_amdgcn_wave_barrier();
    const unsigned long long best = *const_cast<volatile unsigned long long*>(&smax[w]);
    const int pv = best ? 31 - int(best & 31ull) : -1;
    const double dk = pv >= 0 ? As[pv * LD + pv] : 0.0;
    if (k == 0) first = dk;
    if (!(pv >= 0 && dk > rel_tol * first && dk > 0.0)) { rank = k; break; }   // (uniform: every thread sees the same values)
    const double lkk = sqrt(dk), rs = 1.0 / lkk;
    active &= ~(1u << pv);
    const double lj = As[j * LD + pv] * rs;
    if (active & mj) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + 8 * u;
        if ((active >> i) & 1u) As[i * LD + j] -= (As[i * LD + pv] * rs) * lj;
      }
    }
    if (t < 32) Lc[t * LD + k] = t == pv ? lkk : ((active & mj) ? lj : 0.0);
    if (t == 0) { perm[k] = pv; dpiv[k] = lkk; }
    __syncthreads();
  }
  if (t == 0) {   // the indices that never became a pivot complete the permutation (their columns of T are zero)
    int at = rank;
    for (int j = 0; j < n; ++j)
      if ((active >> j) & 1u) perm[at++] = j;
  }
  __syncthreads();
  if (t < 32) {
    // column t of L^-1 in pivot order: x_i = (delta_it - sum_{q < i} L[i][q] x_q) / L[i][i]  (x_q = 0 for q < t by itself)
    double x[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      const int pi = i < n ? perm[i] : 0;
      double s = i == t ? 1.0 : 0.0;
#pragma unroll
      for (int q = 0; q < i; ++q) s -= Lc[pi * LD + q] * x[q];
      x[i] = (i < rank && t < rank) ? s / dpiv[i] : 0.0;
    }
    // T[i, perm[t]] = Li[i, t]
    if (t < n) {
      const int col = perm[t];
#pragma unroll
      for (int i = 0; i < 32; ++i)
        if (i < n) T[size_t(i) * ldt + col] = x[i];
      lam[t] = t < rank ? dpiv[t] * dpiv[t] : 0.0;
    }
  }
}

int romb_pivchol_whiten(rom_ctx* ctx, int n, const double* A, int lda, double* lam, double* T, int ldt, double rel_tol) {
  if (n <= 0) return ROM_OK;
  if (n <= 32) {
    ROM_PROF(ctx, "pivchol_whiten", 1.0 * n * n * n, 16.0 * n * n);
    kb_pivchol_whiten32<<<1, 256, 0, ctx->stream>>>(n, A, lda, lam, T, ldt, rel_tol);
    ROM_HIP(hipGetLastError());
    return ROM_OK;
  }
  const size_t lds = PivcholLds(n).bytes;
  if (lds > 64 * 1024)
    ROM_TRY(rom_lds_optin(ctx->lds_optin_pivchol, reinterpret_cast<const void*>(kb_pivchol_whiten), 160 * 1024 - 256, ctx->device));
  {
    ROM_PROF(ctx, "pivchol_whiten", 1.0 * n * n * n, 16.0 * n * n);
    kb_pivchol_whiten<<<1, 256, lds, ctx->stream>>>(n, A, lda, lam, T, ldt, rel_tol);
  }
  ROM_HIP(hipGetLastError());
  return ROM_OK;
}

// =====================================================================================================================
// Cyclic Jacobi of a symmetric matrix of order 97 ... SE_MAX over the WHOLE chip: one launch per round
// =====================================================================================================================
// kb_small_eig is ONE workgroup and stops at the 96 rows that fit its LDS; on one workgroup the whole-matrix diagonalisation
// that rom_pod falls back to for a flat spectrum (n = 900-1000) would take seconds.  The
// rotations of a round act on disjoint index pairs, so a round is a grid: thread (k, l) of the first half * half threads owns
// the 2 x 2 block rows (p_k, q_k) x columns (p_l, q_l) and computes the rotations of its two pairs itself from the pivot
// blocks (jacobi_rotation of rom_small_dense.h: a pure function, the same bits in every thread -- no phase that computes
// rotations for the others, hence no synchronisation inside a round), the other half * ne threads rotate the eigenvector rows;
// everything is read from the buffers the previous round wrote and written to the other pair (every entry is written every
// round).  Same criterion (relative, with the noise levels of a Gram matrix rotated along), same round-robin order as
// jacobi32_run.  n = 1000: 999 launches of a few microseconds per sweep.
__global__ __launch_bounds__(256) void kb_jgrid_round(int ne, int half, int r, const double* __restrict__ Ac, double* __restrict__ An,
                                                      const double* __restrict__ Vc, double* __restrict__ Vn,
                                                      const double* __restrict__ nuc, double* __restrict__ nun,
                                                      const double* __restrict__ par, int* __restrict__ any) {
  const long long gid = blockIdx.x * 256LL + threadIdx.x;
  const int nm1 = ne - 1;
  const double tol2 = par[1], floor_abs = par[2];
  if (gid < (long long)half * half) {
    const int k = int(gid / half), l = int(gid - (long long)k * half);
    const auto [pk, qk] = jacobi_pair(k, r, nm1);
    const auto [pl, ql] = jacobi_pair(l, r, nm1);
    const size_t rk = size_t(pk) * ne, sk = size_t(qk) * ne, rl = size_t(pl) * ne;
    const double kpp = Ac[rk + pk], kqq = Ac[sk + qk], kpq = Ac[rk + qk];
    const double lpp = Ac[rl + pl], lqq = Ac[size_t(ql) * ne + ql], lpq = Ac[rl + ql];
    const double b00 = Ac[rk + pl], b01 = Ac[rk + ql], b10 = Ac[sk + pl], b11 = Ac[sk + ql];
    double ck, s_k, cl, sl, nkpo, nkqo, nlpo, nlqo;
    const bool rot = jacobi_rotation(kpp, kqq, kpq, nuc[pk], nuc[qk], tol2, floor_abs, ck, s_k, nkpo, nkqo);
    (void)jacobi_rotation(lpp, lqq, lpq, nuc[pl], nuc[ql], tol2, floor_abs, cl, sl, nlpo, nlqo);
    jacobi_block_update(ck, s_k, cl, sl, b00, b01, b10, b11, An[rk + pl], An[rk + ql], An[sk + pl], An[sk + ql]);
    if (l == 0) {
      nun[pk] = nkpo;
      nun[qk] = nkqo;
      if (rot) *any = 1;
    }
    return;
  }
  const long long idx = gid - (long long)half * half;
  if (idx >= (long long)half * ne) return;
  const int k = int(idx / ne), j = int(idx - (long long)k * ne);
  const auto [pk, qk] = jacobi_pair(k, r, nm1);
  const size_t rk = size_t(pk) * ne, sk = size_t(qk) * ne;
  double ck, s_k, a, b;
  (void)jacobi_rotation(Ac[rk + pk], Ac[sk + qk], Ac[rk + qk], nuc[pk], nuc[qk], tol2, floor_abs, ck, s_k, a, b);
  const double vp = Vc[rk + j], vq = Vc[sk + j];
  Vn[rk + j] = ck * vp - s_k * vq;
  Vn[sk + j] = s_k * vp + ck * vq;
}

// A0 <- symmetrised copy of A with zero padding to the even order ne, V0 <- identity
__global__ void kb_jgrid_init(int n, int ne, const double* __restrict__ A, int lda, double* __restrict__ A0, double* __restrict__ V0) {
  const long long idx = blockIdx.x * 256LL + threadIdx.x;
  if (idx >= (long long)ne * ne) return;
  const int r = int(idx / ne), c = int(idx - (long long)r * ne);
  A0[idx] = (r < n && c < n) ? 0.5 * (A[size_t(r) * lda + c] + A[size_t(c) * lda + r]) : 0.0;
  V0[idx] = r == c ? 1.0 : 0.0;
}

// par[0] = max |a_ii|, par[1] = tol^2, par[2] = smallest entry that is rotated; nu^2 (noise levels) of the rows
__global__ __launch_bounds__(256) void kb_jgrid_params(int n, int ne, const double* __restrict__ A0, int gram_like, double* __restrict__ par,
                                                       double* __restrict__ nu) {
  __shared__ double red[4];
  const int t = threadIdx.x;
  double dmax = 0.0;
  for (int i = t; i < n; i += 256) dmax = fmax(dmax, fabs(A0[size_t(i) * ne + i]));
  dmax = block_max<4>(dmax, red);
  if (t == 0) {
    par[0] = dmax;
    par[1] = jacobi_tol2(n, gram_like);
    par[2] = jacobi_floor(dmax);
  }
  for (int i = t; i < ne; i += 256) nu[i] = i < n ? jacobi_nu2_init(gram_like, A0[size_t(i) * ne + i], dmax) : 0.0;
}

__global__ void kb_jgrid_diag(int n, int ne, const double* __restrict__ Ac, double* __restrict__ d) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) d[i] = Ac[size_t(i) * ne + i];
}

// T[i, :] = scale[i] V[perm[i], :], lam[i] = d[perm[i]]
__global__ void kb_jgrid_gather(int n, int ne, const double* __restrict__ Vc, const double* __restrict__ d, const int* __restrict__ perm,
                                const double* __restrict__ scale, double* __restrict__ T, int ldt, double* __restrict__ lam) {
  const long long idx = blockIdx.x * 256LL + threadIdx.x;
  if (idx >= (long long)n * n) return;
  const int i = int(idx / n), c = int(idx - (long long)i * n);
  const int src = perm[i];
  T[size_t(i) * ldt + c] = scale[i] * Vc[size_t(src) * ne + c];
  if (c == 0) lam[i] = d[src];
}

// (mode / rel_tol as kb_small_eig: SE_EIG rows = eigenvectors, SE_WHITEN rows / sqrt(lam) -- zero rows below rel_tol x the
// largest eigenvalue --, SE_LOWDIN the symmetric inverse square root over the same eigenpairs)
static int jacobi_grid(rom_ctx* ctx, int n, const double* A, int lda, double* lam, double* T, int ldt, int mode, double rel_tol,
                       int gram_like) {
  const int ne = n + (n & 1), half = ne / 2;
  const size_t nn = size_t(ne) * ne;
  Tmp A0, A1, V0, V1, nu0, nu1, par, diag, anyb, permb;
  ROM_TRY(A0.get(ctx, nn));
  ROM_TRY(A1.get(ctx, nn));
  ROM_TRY(V0.get(ctx, nn));
  ROM_TRY(V1.get(ctx, nn));
  ROM_TRY(nu0.get(ctx, ne));
  ROM_TRY(nu1.get(ctx, ne));
  ROM_TRY(par.get(ctx, 4));
  ROM_TRY(diag.get(ctx, n));
  ROM_TRY(anyb.get(ctx, 1));
  ROM_TRY(permb.get(ctx, (size_t(n) + 1) / 2 + 1));
  int* d_any = reinterpret_cast<int*>(anyb.p());
  int* d_perm = reinterpret_cast<int*>(permb.p());
  ROM_PROF(ctx, "jacobi_grid", 30.0 * n * double(n) * n, 16.0 * double(n) * n);
  kb_jgrid_init<<<unsigned((nn + 255) / 256), 256, 0, ctx->stream>>>(n, ne, A, lda, A0, V0);
  kb_jgrid_params<<<1, 256, 0, ctx->stream>>>(n, ne, A0, gram_like, par, nu0);
  ROM_HIP(hipGetLastError());
  double *Ac = A0, *An = A1, *Vc = V0, *Vn = V1, *nuc = nu0, *nun = nu1;
  const long long threads = (long long)half * half + (long long)half * ne;
  const unsigned grid = unsigned((threads + 255) / 256);
  for (int sweep = 0; sweep < 60; ++sweep) {
    ROM_HIP(hipMemsetAsync(d_any, 0, sizeof(int), ctx->stream));
    for (int r = 0; r < ne - 1; ++r) {
      kb_jgrid_round<<<grid, 256, 0, ctx->stream>>>(ne, half, r, Ac, An, Vc, Vn, nuc, nun, par, d_any);
      std::swap(Ac, An);
      std::swap(Vc, Vn);
      std::swap(nuc, nun);
    }
    ROM_HIP(hipGetLastError());
    int any = 0;
    ROM_HIP(hipMemcpyAsync(&any, d_any, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ROM_HIP(hipStreamSynchronize(ctx->stream));
    ctx->host_syncs += 1;
    if (!any) break;
  }
  kb_jgrid_diag<<<unsigned((n + 255) / 256), 256, 0, ctx->stream>>>(n, ne, Ac, diag);
  ROM_HIP(hipGetLastError());
  std::vector<double> d(n);
  ROM_TRY(download(ctx, diag, d.data(), n));
  ctx->host_syncs += 1;
  std::vector<int> perm(n);
  for (int i = 0; i < n; ++i) perm[rank_descending(d.data(), n, i)] = i;
  ROM_HIP(hipMemcpyAsync(d_perm, perm.data(), size_t(n) * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  const double lmax = d[perm[0]];
  std::vector<double> scale(n, 1.0);
  if (mode != SE_EIG)
    for (int i = 0; i < n; ++i) {
      const double l = d[perm[i]];
      const bool keep = l > rel_tol * lmax && l > 0.0;
      scale[i] = !keep ? 0.0 : mode == SE_WHITEN ? 1.0 / std::sqrt(l) : 1.0 / std::sqrt(std::sqrt(l));
    }
  Tmp scb;
  ROM_TRY(scb.get(ctx, n));
  ROM_HIP(hipMemcpyAsync(scb.p(), scale.data(), size_t(n) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  const unsigned gg = unsigned((size_t(n) * n + 255) / 256);
  if (mode != SE_LOWDIN) {
    kb_jgrid_gather<<<gg, 256, 0, ctx->stream>>>(n, ne, Vc, diag, d_perm, scb, T, ldt, lam);
    ROM_HIP(hipGetLastError());
  } else {
    // sum_i q_i q_i^T / sqrt(lam_i) = S^T S with S = rows q_i^T lam_i^(-1/4): gathered into one ping-pong buffer, transposed
    // into the other, one small product
    double* S = An;
    double* St = Vn;
    kb_jgrid_gather<<<gg, 256, 0, ctx->stream>>>(n, ne, Vc, diag, d_perm, scb, S, n, lam);
    ROM_HIP(hipGetLastError());
    ROM_TRY(romb_transpose(ctx, St, n, S, n, n, n));
    ROM_TRY(rom_launch_gemm_nt(ctx, n, n, n, 1.0, St, n, St, n, 0.0, T, ldt, "gemm_nt"));
  }
  ROM_HIP(hipStreamSynchronize(ctx->stream));   // (perm / scale are host memory of this frame)
  ctx->host_syncs += 1;
  return ROM_OK;
}

int romb_small_eig(rom_ctx* ctx, int n, const double* A, int lda, double* lam, double* T, int ldt, int mode, double rel_tol,
                     bool gram_like, bool tight) {
  if (n <= 0) return ROM_OK;
  // what the kernels get: 0 general symmetric, 1 Gram-like, 2 Gram-like with the rotation threshold 16 eps instead of n eps
  // (rom_pca_tall: its own convergence test, 64 eps max(d) max(d_i, d_j), must lie above what the sweeps leave behind)
  const int gl = gram_like ? (tight ? 2 : 1) : 0;
  ROM_CHECK(n <= SE_GRID_MAX, "small symmetric eigenproblem: n = %d beyond %d", n, SE_GRID_MAX);
  if (n > SE_LDS_MAX) return jacobi_grid(ctx, n, A, lda, lam, T, ldt, mode, rel_tol, gl);   // (one launch per round, the whole chip)
  const size_t lds = SmallEigLds(n).bytes;   // (n <= SE_LDS_MAX here: matrix + eigenvector rows in LDS)
  double* ns_ws = nullptr;
  ROM_TRY(rom_ctx_scratch(ctx, 2 * size_t(n) * n, &ns_ws));   // Newton-Schulz fast path: next iterates
  if (lds > 64 * 1024)
    ROM_TRY(rom_lds_optin(ctx->lds_optin_small_eig, reinterpret_cast<const void*>(kb_small_eig), 160 * 1024, ctx->device));
  {
    char nm[48];
    rom_prof_name(nm, sizeof nm, "small_eig", "_n%d_mode%d_%s", n, mode, gram_like ? "gram" : "sym");
    ROM_PROF(ctx, nm, 30.0 * n * n * n, 16.0 * n * n);
    // n <= 32, eigenvectors: kb_jacobi32 -- 256 threads, every thread computes the rotations of its block itself, ONE barrier
    // per round: several times the rounds per microsecond of the three-phase 512-thread form
    if (n <= 32 && mode == SE_EIG) kb_jacobi32<<<1, 256, 0, ctx->stream>>>(n, A, lda, lam, T, ldt, gl);
    else kb_small_eig<<<1, SE_TPB, lds, ctx->stream>>>(n, A, lda, lam, T, ldt, mode, rel_tol, gl, ns_ws);
  }
  ROM_HIP(hipGetLastError());
  return ROM_OK;
}

// test / diagnostic entry: eigen-decomposition of a small symmetric matrix given on the host
extern "C" int rom_small_eig_host(rom_ctx* ctx, int n, const double* A_host, int mode, double rel_tol, int gram_like,
                                  double* lam_host, double* T_host) {
  ROM_CHECK(ctx && A_host && lam_host && T_host && n >= 1 && n <= SE_MAX, "rom_small_eig_host: bad arguments");
  ROM_CHECK(mode >= 0 && mode <= 3, "rom_small_eig_host: mode must be 0, 1, 2 or 3");
  ROM_CHECK(mode != 3 || n <= SE_LDS_MAX, "rom_small_eig_host: the pivoted-Cholesky whitening takes n <= %d", SE_LDS_MAX);
  Tmp A, lam, T;
  ROM_TRY(A.get(ctx, size_t(n) * n));
  ROM_TRY(lam.get(ctx, n));
  ROM_TRY(T.get(ctx, size_t(n) * n));
  ROM_HIP(hipMemcpyAsync(A.p(), A_host, size_t(n) * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  if (mode == 3) ROM_TRY(romb_pivchol_whiten(ctx, n, A, n, lam, T, n, rel_tol));
  else ROM_TRY(romb_small_eig(ctx, n, A, n, lam, T, n, mode, rel_tol, gram_like != 0, gram_like == 2));
  ROM_TRY(download(ctx, lam, lam_host, n));
  return download(ctx, T, T_host, size_t(n) * n);
}
