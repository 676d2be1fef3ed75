// rom_kmeans: Lloyd's algorithm on a tall block X (M rows, r <= 128 columns) against kc <= 256 centroids -- the clustering of the
// local reduced bases (romhighcontrast_amd/local.py): the parameter domain is split and every part gets its own small basis.
//
// The ANSWER is defined the way rom_nearest defines its own: the distance is the one device function nn_dist2 (rom_dist.h:
// differences of the original operands, one fma chain in column order), and the label of a row is the centroid that is smallest
// under the total order (that value, centroid index) -- what the exhaustive scan k_km_exhaust returns (mode 1, test hook and
// definition).  Mode 0, the product path, returns the same bits from one fused kernel per iteration on the slab engine of
// rom_slab.h (k_km_step, 512 threads, slabs of 32 rows, a chunk of slabs per workgroup):
//   screen      the kc centroids, shifted by the block's column means mu, are the LDS-resident NT operand B; for the rows of a
//               slab slab_nt forms all scores s_j = |c~_j|^2 - 2 x~ . c~_j (x~ = fl(x - mu), c~ = fl(c - mu)) and leaves them in LDS.
//   rescore     four rows per wave, sixteen lanes per row.  The lanes scan the row's scores; every centroid whose score lies within
//               2 delta of the smallest is rescored with nn_dist2 on the ORIGINAL operands, the label is the smallest of those under
//               (d2, j).  delta = 4 (r + 4) (eps (|x~|^2 + max_j |c~_j|^2) + 2^-1022), eps = 2^-52.  With u = eps / 2 and
//               S = |x~|^2 + |c~_j|^2 the computed s_j + |x~|^2 differs from the exact squared distance D_j of the original
//               operands by at most
//                     the r-term fma dot product of the MFMA, in any order, times 2:     r u 2 |x~| |c~|  <=  r u S
//                     |c~_j|^2 and |x~|^2, r-term fma chains:                                                r u S
//                     the fma that forms s_j and the (virtual) addition of |x~|^2:                           4 u S
//                     one rounding of each centred entry, |(x~ - c~) - (x - c)| <= u (|x~| + |c~|):          4 u S
//               in all (2 r + 8) u S = (r + 4) eps S <= delta / 4 (the second term of delta covers operations that underflow).
//               Let j0 carry the smallest score m and j1 be the label of the exhaustive scan: nn_dist2 (relative error below
//               (r + 2) u) has d2_j1 <= d2_j0, hence D_j1 <= D_j0 (1 + (r + 2) eps), and with D_j0 <= 2 S (1 + eps)
//                     s_j1 <= D_j1 - |x~|^2 + delta / 4 <= s_j0 + delta / 2 + (r + 2) eps D_j0 < m + delta:
//               j1 -- and every centroid that ties with it -- is among the rescored ones; the threshold m + 2 delta leaves a
//               whole delta for its own rounding.  The sixteen lanes of a row rescore a centroid together: each forms the
//               differences of its own columns from the original entries it holds in registers, and nn_dist2_lanes16 (rom_dist.h)
//               runs nn_dist2's chain over them by lane broadcasts -- no operand is read again.  The bound decides which centroids are rescored, never the answer: a NaN or
//               an overflow in a row's screen makes the kernel rescore all kc centroids for that row.  Usually one exact
//               distance per row, which dist2 and the inertia need anyway.
//   accumulate  the scores make way for the slab's one-hot label matrix Z (32 x kc) beside the shifted rows and a column of ones
//               in the TN layout; Z^T [X~ | 1] goes to register accumulators by slab_tn_acc, the 16 x 16 tiles dealt to the waves
//               (w + 8 q).  One-hot products are exact, the counts come out of the same MFMAs as exact integers, the order of
//               the sums is fixed.
//   epilogue    one partial kc x (r + 1) per workgroup; k_km_update adds the partials in chunk order and forms
//               c_j = mu + sum / n_j (the previous centroid bit for bit where n_j = 0); k_km_control adds the inertia partials
//               in chunk order, reads the integer count of changed labels and decides whether to stop.
// Mode 1 runs k_km_exhaust for the labels and distances and the same accumulation (k_km_step with the labels given).
// The stop test lives on the device: every kernel of an iteration returns at once when the done flag is set; the host
// enqueues iterations in groups of 8 and reads the status word once per group.  The call ends with an assignment pass against
// the centroids it returns.  No floating-point atomics anywhere: a repeated call returns the same bits.
//
// LDS of k_km_step (rom_kmeans_layout, the single place that decides it; doubles, rpad = r up to a multiple of 4, kcp = kc up to
// 16, rcp = r + 1 up to 16): Bs kcp (rpad + 2) | |c~|^2 kcp | As 32 (rpad + 2) (NT copy of the slab) | T 32 slab_ld_tn(kcp + rcp)
// (scores, then Z | X~ | 1: the TN copy) | 16 | mu 128 | the original centroids kc r where all of it stays within 160 KB.  kcp rpad <= 8192 keeps it within 160 KB: (64, 128) 151 KB, (256, 32) 156 KB.
#include <climits>
#include <cmath>
#include <cstring>

#include "rom_basis_int.h"
#include "rom_block.h"
#include "rom_dist.h"
#include "rom_slab.h"

struct rom_kmeans {
  rom_ctx* ctx = nullptr;
  int r = 0, kc = 0, iterations = 0, converged = 0, stop = 0;
  long long M_train = 0, launches = 0, syncs = 0;
  rom_buf* C = nullptr;       // kc x r centroids
  rom_buf* stat = nullptr;    // KM_STAT: the shift mu (128) | non-finite entries of the block
  rom_buf* counts = nullptr;  // kc
  rom_buf* hist = nullptr;    // inertia of the assignment of every iteration, then of the final one
  rom_buf* labels = nullptr;  // M_train int32
};

namespace {

constexpr int KM_KCMAX = 256, KM_BUDGET = 8192, KM_TILES = 6, KM_GROUP = 8;
constexpr int KM_STAT = NN_RMAX + 2;
constexpr int KM_LDS_MAX = 160 * 1024;
constexpr int KM_GIVEN = 1, KM_FORCE = 2, KM_NOACC = 4;   // flags of k_km_step / k_km_update
constexpr double KM_DBL_MAX = 1.7976931348623157e308, KM_TINY = 2.2250738585072014e-308;
// control block (doubles): ints st[4] = done, iterations, converged, stop reason | counters (unsigned long long) changed labels
// of the iteration, rows rescored beyond the first candidate | mean column variance | final inertia
constexpr int KM_CTL = 8;

struct KmLayout {
  int rpad, kcp, rcp, LX, LT, ntiles;
  int corig;   // the original centroids (kc x r) have room in LDS too: the rescoring reads them there, not through L2
  size_t lds_doubles;
};
bool km_layout(int r, int kc, KmLayout* L) {
  if (r < 1 || r > NN_RMAX || kc < 1 || kc > KM_KCMAX) return false;
  L->rpad = (r + 3) / 4 * 4;
  L->kcp = (kc + 15) / 16 * 16;
  L->rcp = (r + 1 + 15) / 16 * 16;
  L->LX = slab_ld_nt(L->rpad);
  L->LT = slab_ld_tn(L->kcp + L->rcp);
  L->ntiles = (L->kcp / 16) * (L->rcp / 16);
  L->lds_doubles = size_t(L->kcp) * L->LX + L->kcp + size_t(SLAB_ROWS) * L->LX + size_t(SLAB_ROWS) * L->LT + 16 + NN_RMAX;
  L->corig = (L->lds_doubles + size_t(kc) * r) * sizeof(double) <= size_t(KM_LDS_MAX);
  if (L->corig) L->lds_doubles += size_t(kc) * r;
  return true;
}

// ---- the exhaustive scan: the definition of the labels (mode 1) -----------------------------------------------------------------
// a thread per row (grid-stride), the centroids in LDS (read by every lane at once); labels, dist2 and the count of changed labels
__global__ __launch_bounds__(256) void k_km_exhaust(const double* __restrict__ X, long long ldx, long long M, int r, int kc,
                                                    const double* __restrict__ C, int* __restrict__ labels, double* __restrict__ dist2,
                                                    unsigned long long* __restrict__ cnt, const int* __restrict__ done, int flags) {
  extern __shared__ double km_lds[];
  if (!(flags & KM_FORCE) && *done) return;
  for (int e = threadIdx.x; e < kc * r; e += 256) km_lds[e] = C[e];
  __syncthreads();
  int changed = 0;
  for (long long row0 = (long long)blockIdx.x * 256; row0 < M; row0 += (long long)gridDim.x * 256) {
    const long long row = row0 + threadIdx.x;
    bool ch = false;
    if (row < M) {
      double bd = NN_INF;
      long long bj = LLONG_MAX;
      for (int j = 0; j < kc; ++j) {
        double d[1];
        nn_dist2<1>(X + row * ldx, 0, km_lds + j * r, r, d);
        if (nn_less(d[0], j, bd, bj)) {
          bd = d[0];
          bj = j;
        }
      }
      ch = labels[row] != int(bj);
      labels[row] = int(bj);
      dist2[row] = bd;
    }
    changed += __popcll(__ballot(ch));
  }
  if ((threadIdx.x & 63) == 0 && changed) atomicAdd(cnt, (unsigned long long)changed);
}

// ---- one Lloyd iteration on the slab engine ----------------------------------------------------------------------------------
// Workgroup b owns the slabs [b per_chunk, (b + 1) per_chunk).  Thread t stages row t >> 4 of a slab, columns (t & 15) + 16 u --
// and those sixteen lanes are the ones that scan and rescore that row: wave w owns rows 4 w .. 4 w + 3.
// part[b] (kcp x rcp) = Z^T [X~ | 1] over the chunk, ipart[b] = its sum of dist2, row after row.
__global__ __launch_bounds__(SLAB_THREADS) void k_km_step(const double* __restrict__ X, long long ldx, long long M, int r, int kc,
                                                         int rpad, int kcp, int rcp, int corig, const double* __restrict__ C,
                                                         const double* __restrict__ mean, long long per_chunk, int* __restrict__ labels,
                                                         double* __restrict__ dist2, double* __restrict__ part,
                                                         double* __restrict__ ipart, unsigned long long* __restrict__ cnt,
                                                         const int* __restrict__ done, int flags) {
  extern __shared__ double km_lds[];
  if (!(flags & KM_FORCE) && *done) return;
  const int LX = slab_ld_nt(rpad), LT = slab_ld_tn(kcp + rcp);
  double* Bs = km_lds;                    // kcp x LX
  double* cn = Bs + kcp * LX;             // kcp
  double* As = cn + kcp;                  // 32 x LX
  double* T = As + SLAB_ROWS * LX;        // 32 x LT
  double* iws = T + SLAB_ROWS * LT;       // 8 (of 16)
  double* mus = iws + 16;                 // 128: the shift, zero from column r on
  double* Cl = mus + NN_RMAX;             // kc x r original centroids, where the layout has room for them
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, i = lane & 15, k4 = lane >> 4;
  const int rt = w & 1, ct0 = w >> 1, nct = kcp >> 4, ncr = rcp >> 4, ntiles = nct * ncr;
  const int srow = t >> 4, scl = t & 15;
  const bool given = flags & KM_GIVEN, acc_on = !(flags & KM_NOACC);

  for (int e = t; e < kcp * LX; e += SLAB_THREADS) {
    const int j = e / LX, c = e - j * LX;
    Bs[e] = (j < kc && c < r) ? C[j * r + c] - mean[c] : 0.0;
  }
  if (t < NN_RMAX) mus[t] = t < r ? mean[t] : 0.0;
  if (corig)
    for (int e = t; e < kc * r; e += SLAB_THREADS) Cl[e] = C[e];
  const double* Co = corig ? Cl : C;
  __syncthreads();
  if (t < kcp) {
    double s = 0.0;
    for (int c = 0; c < rpad; ++c) s = fma(Bs[t * LX + c], Bs[t * LX + c], s);
    cn[t] = s;
  }
  __syncthreads();
  double cmax = 0.0;   // max_j |c~_j|^2 (a NaN stays: the row then rescores everything)
  for (int j = lane; j < kc; j += 64) cmax = cn[j] > cmax || cn[j] != cn[j] ? cn[j] : cmax;
#pragma unroll
  for (int o = 1; o < 64; o *= 2) {
    const double v = __shfl_xor(cmax, o, 64);
    cmax = v > cmax || v != v ? v : cmax;
  }

  // this thread's entries of the slab and of the next one: the ORIGINAL values (the rescoring wants them); the shifted ones are
  // formed from them wherever they are written.  A row past M holds mu: it shifts to exactly zero.
  double xo[8], xnext[8];
  int lab_next = -1;   // (lanes scl == 0: the row's label so far, fetched with the slab)
  const double* mu = mus + scl;   // (mu[16 u]: the shift of this thread's column scl + 16 u, 0.0 from column r on)
  long long slab0, slab1;
  slab_chunk_range(M, per_chunk, &slab0, &slab1);
  auto load_slab = [&](long long s) {
    const long long row = s * SLAB_ROWS + srow;
#pragma unroll
    for (int u = 0; u < 8; ++u) xnext[u] = (row < M && scl + 16 * u < r) ? X[row * ldx + scl + 16 * u] : mu[16 * u];
    if (!given && scl == 0 && row < M) lab_next = labels[row];
  };
  d4_t acc[KM_TILES];
#pragma unroll
  for (int q = 0; q < KM_TILES; ++q) acc[q] = d4_t{0.0, 0.0, 0.0, 0.0};
  double iw = 0.0;
  int changed = 0, extra = 0;

  if (slab0 < slab1) load_slab(slab0);
  for (long long s = slab0; s < slab1; ++s) {
    const long long grow = s * SLAB_ROWS + srow;
    const int lab_old = lab_next;
    // the slab's NT copy (the last reads of As and T lie before the two barriers of the previous slab's second half)
    double xn = 0.0;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      xo[u] = xnext[u];
      const double xs = xo[u] - mu[16 * u];
      if (scl + 16 * u < rpad) As[srow * LX + scl + 16 * u] = xs;
      xn = fma(xs, xs, xn);
    }
    xn += __shfl_xor(xn, 1, 64);
    xn += __shfl_xor(xn, 2, 64);
    xn += __shfl_xor(xn, 4, 64);
    xn += __shfl_xor(xn, 8, 64);
    __syncthreads();
    if (s + 1 < slab1) load_slab(s + 1);
    if (!given) {
      for (int h = 0; 8 * h < nct; ++h) {
        d4_t y[2];
        slab_nt(As, LX, Bs + h * 128 * LX, LX, rpad, nct - 8 * h, y);
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
          const int ct = 8 * h + ct0 + 4 * jj;
          if (ct < nct) {
            const int col = ct * 16 + i;
#pragma unroll
            for (int g = 0; g < 4; ++g) T[(rt * 16 + k4 + 4 * g) * LT + col] = fma(-2.0, y[jj][g], cn[col]);
          }
        }
      }
    }
    __syncthreads();
    // scan and rescore: row srow by the sixteen lanes scl = 0 .. 15, centroids scl + 16 u each
    double bd = NN_INF;
    long long bj = LLONG_MAX;
    if (given) {
      if (grow < M) {
        bd = dist2[grow];
        bj = labels[grow];
      }
    } else {
      double m = NN_INF;
      int bad = 0;
      for (int u = 0; u < nct; ++u) {
        const int col = scl + 16 * u;
        const double sc = T[srow * LT + col];
        if (col < kc) {
          bad |= fabs(sc) <= KM_DBL_MAX ? 0 : 1;
          m = sc < m ? sc : m;
        }
      }
#pragma unroll
      for (int o = 1; o < 16; o *= 2) {
        const double v = __shfl_xor(m, o, 64);
        m = v < m ? v : m;
        bad |= __shfl_xor(bad, o, 64);
      }
      const double delta = 4.0 * double(r + 4) * (NN_EPS * (xn + cmax) + KM_TINY);
      const double thr = m + 2.0 * delta;
      const bool all = bad || !(fabs(thr) <= KM_DBL_MAX);
      unsigned mask = 0;   // bit u: centroid scl + 16 u is to be rescored
      if (grow < M)
        for (int u = 0; u < nct; ++u) {
          const int col = scl + 16 * u;
          if (col < kc && (all || T[srow * LT + col] <= thr)) mask |= 1u << u;
        }
      int ncand = __popc(mask);
#pragma unroll
      for (int o = 1; o < 16; o *= 2) ncand += __shfl_xor(ncand, o, 64);
      // a round rescores the lowest centroid left of each of the wave's four rows, its sixteen lanes together (nn_dist2_lanes16)
      while (__any(mask != 0)) {
        int j = mask ? scl + 16 * (__ffs(int(mask)) - 1) : INT_MAX;
#pragma unroll
        for (int o = 1; o < 16; o *= 2) j = min(j, __shfl_xor(j, o, 64));
        const bool live = j != INT_MAX;
        double dreg[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) dreg[u] = (live && scl + 16 * u < r) ? xo[u] - Co[j * r + scl + 16 * u] : 0.0;
        const double d = nn_dist2_lanes16(dreg, r);
        if (live && nn_less(d, j, bd, bj)) {
          bd = d;
          bj = j;
        }
        if (live && (j & 15) == scl) mask &= ~(1u << (j >> 4));
      }
      bool ch = false;
      if (scl == 0 && grow < M) {
        ch = lab_old != int(bj);
        labels[grow] = int(bj);
        dist2[grow] = bd;
      }
      changed += __popcll(__ballot(ch));
      extra += __popcll(__ballot(scl == 0 && ncand > 1));
    }
    {
      // the wave's four rows in row order
      const double dv = grow < M ? bd : 0.0;
      iw += __shfl(dv, 0, 64);
      iw += __shfl(dv, 16, 64);
      iw += __shfl(dv, 32, 64);
      iw += __shfl(dv, 48, 64);
    }
    if (acc_on) {
      // Z over the scores (each lane rewrites the columns it has read), X~ | 1 | 0 beside it
      for (int u = 0; u < nct; ++u) {
        const int col = scl + 16 * u;
        T[srow * LT + col] = (grow < M && col == bj) ? 1.0 : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 9; ++u) {
        const int c = scl + 16 * u;
        if (c < rcp) T[srow * LT + kcp + c] = c < r ? xo[u & 7] - mu[16 * (u & 7)] : (c == r && grow < M) ? 1.0 : 0.0;
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < KM_TILES; ++q) {
        const int tt = w + 8 * q;
        if (tt < ntiles) slab_tn_acc(T, LT, (tt / ncr) * 16, kcp + (tt % ncr) * 16, acc[q]);
      }
    }
  }
  if (acc_on) {
    double* Pb = part + size_t(blockIdx.x) * kcp * rcp;
#pragma unroll
    for (int q = 0; q < KM_TILES; ++q) {
      const int tt = w + 8 * q;
      if (tt < ntiles) slab_tn_store(Pb, rcp, (tt / ncr) * 16, (tt % ncr) * 16, acc[q]);
    }
  }
  if (lane == 0) {
    iws[w] = iw;
    if (changed) atomicAdd(cnt, (unsigned long long)changed);
    if (extra) atomicAdd(cnt + 1, (unsigned long long)extra);
  }
  __syncthreads();
  if (t == 0) {
    double sum = iws[0];
    for (int q = 1; q < 8; ++q) sum += iws[q];
    ipart[blockIdx.x] = sum;
  }
}

// ---- the update: one workgroup per centroid adds the partials in chunk order ---------------------------------------------------
// counts[j] = n_j; C[j] = mu + sum / n_j, or C[j] as it is where n_j = 0; shift2[j] = |C_new[j] - C_old[j]|^2.  With KM_NOACC only
// the counts are written.
__global__ __launch_bounds__(256) void k_km_update(const double* __restrict__ part, int chunks, int kcp, int rcp, int r,
                                                   const double* __restrict__ mean, double* __restrict__ C, double* __restrict__ counts,
                                                   double* __restrict__ shift2, const int* __restrict__ done, int flags) {
  __shared__ double sums[NN_RMAX + 1], sq[NN_RMAX];
  if (!(flags & KM_FORCE) && *done) return;
  const int j = blockIdx.x, t = threadIdx.x;
  if (t <= r) {
    double s = 0.0;
    for (int q = 0; q < chunks; ++q) s += part[(size_t(q) * kcp + j) * rcp + t];
    sums[t] = s;
  }
  __syncthreads();
  const double n = sums[r];
  if (t == 0) counts[j] = n;
  if (flags & KM_NOACC) return;
  if (t < r) {
    const double old = C[j * r + t];
    const double nw = n > 0.0 ? mean[t] + sums[t] / n : old;
    C[j * r + t] = nw;
    sq[t] = (nw - old) * (nw - old);
  }
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    for (int c = 0; c < r; ++c) s += sq[c];
    shift2[j] = s;
  }
}

// ---- the stop test (one thread) -----------------------------------------------------------------------------------------------
// hist[iteration] = the inertia partials added in chunk order.  final: that only, whatever the done flag says.
__global__ void k_km_control(const double* __restrict__ ipart, int chunks, const double* __restrict__ shift2, int kc,
                             double* __restrict__ ctl, double* __restrict__ hist, double tol, int max_iter, int final) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int* st = reinterpret_cast<int*>(ctl);
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(ctl + 2);
  if (!final && st[0]) return;
  double inertia = 0.0;
  for (int q = 0; q < chunks; ++q) inertia += ipart[q];
  const int it = st[1];
  hist[it] = inertia;
  if (final) return;
  const unsigned long long changed = cnt[0];
  cnt[0] = 0;
  double ms = 0.0;
  for (int j = 0; j < kc; ++j) ms = shift2[j] > ms ? shift2[j] : ms;
  st[1] = it + 1;
  if (changed == 0) {
    st[0] = 1;
    st[2] = 1;
    st[3] = 0;
  } else if (ms <= tol * ctl[4]) {
    st[0] = 1;
    st[3] = 1;
  } else if (it + 1 >= max_iter) {
    st[0] = 1;
    st[3] = 2;
  }
}

// ---- mean column variance of the block: fixed-order partials ---------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_km_var_partial(const double* __restrict__ X, long long ldx, long long M, int r,
                                                        const double* __restrict__ mean, long long rows_per_chunk,
                                                        double* __restrict__ vpart) {
  __shared__ double sv[256];
  const long long r0 = (long long)blockIdx.x * rows_per_chunk, r1 = min(M, r0 + rows_per_chunk);
  double s = 0.0;
  for (long long row = r0 + threadIdx.x; row < r1; row += 256)
    for (int c = 0; c < r; ++c) {
      const double d = X[row * ldx + c] - mean[c];
      s = fma(d, d, s);
    }
  sv[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 1; q < 256; ++q) s += sv[q];
    vpart[blockIdx.x] = s;
  }
}
__global__ void k_km_var_finish(const double* __restrict__ vpart, int chunks, double divisor, double* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double s = 0.0;
  for (int q = 0; q < chunks; ++q) s += vpart[q];
  *out = s / divisor;
}

// ---- farthest-point start -------------------------------------------------------------------------------------------------------
// Launch s first reduces the (value, row) partials of launch s - 1 to the centre they chose (launch 0: the centre is mu and the
// rule "smallest distance"; later launches: "largest D"; lowest row among equals in both), then D <- min(D, d2 to that centre)
// and writes its own partials.  Launch kc only reduces.
__device__ __forceinline__ bool mm_better(bool smallest, double v, long long row, double bv, long long brow) {
  return smallest ? (v < bv || (v == bv && row < brow)) : (v > bv || (v == bv && row < brow));
}
__global__ __launch_bounds__(256) void k_km_maximin(const double* __restrict__ X, long long ldx, long long M, int r,
                                                    const double* __restrict__ mean, double* __restrict__ D, int step, int kc,
                                                    const double* __restrict__ pv_in, const long long* __restrict__ pr_in, int nb_in,
                                                    double* __restrict__ pv_out, long long* __restrict__ pr_out,
                                                    long long* __restrict__ rows_out) {
  __shared__ double rv[256], cs[NN_RMAX];
  __shared__ long long rr[256];
  const int t = threadIdx.x;
  if (step > 0) {
    const bool smallest = step == 1;
    double bv = smallest ? NN_INF : -1.0;
    long long br = LLONG_MAX;
    for (int q = t; q < nb_in; q += 256)
      if (mm_better(smallest, pv_in[q], pr_in[q], bv, br)) {
        bv = pv_in[q];
        br = pr_in[q];
      }
    rv[t] = bv;
    rr[t] = br;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (t < o && mm_better(smallest, rv[t + o], rr[t + o], rv[t], rr[t])) {
        rv[t] = rv[t + o];
        rr[t] = rr[t + o];
      }
      __syncthreads();
    }
    const long long centre = rr[0];
    if (blockIdx.x == 0 && t == 0) rows_out[step - 1] = centre;
    if (step == kc) return;
    __syncthreads();
    if (t < r) cs[t] = (centre >= 0 && centre < M) ? X[centre * ldx + t] : 0.0;
  } else if (t < r) {
    cs[t] = mean[t];
  }
  __syncthreads();
  const bool smallest = step == 0;
  double bv = smallest ? NN_INF : -1.0;
  long long br = LLONG_MAX;
  for (long long row = (long long)blockIdx.x * 256 + t; row < M; row += (long long)gridDim.x * 256) {
    double d[1];
    nn_dist2<1>(X + row * ldx, 0, cs, r, d);
    double v = d[0];
    if (step > 0) {
      if (step > 1) v = D[row] < v ? D[row] : v;
      D[row] = v;
    }
    if (mm_better(smallest, v, row, bv, br)) {
      bv = v;
      br = row;
    }
  }
  rv[t] = bv;
  rr[t] = br;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o && mm_better(smallest, rv[t + o], rr[t + o], rv[t], rr[t])) {
      rv[t] = rv[t + o];
      rr[t] = rr[t + o];
    }
    __syncthreads();
  }
  if (t == 0) {
    pv_out[blockIdx.x] = rv[0];
    pr_out[blockIdx.x] = rr[0];
  }
}

// ---- host helpers -----------------------------------------------------------------------------------------------------------------
int km_check_shape(const char* who, int r, int kc, KmLayout* L) {
  ROM_CHECK(r >= 1 && r <= NN_RMAX, "%s: r = %d columns, between 1 and %d", who, r, NN_RMAX);
  ROM_CHECK(kc >= 1 && kc <= KM_KCMAX, "%s: kc = %d centroids, between 1 and %d", who, kc, KM_KCMAX);
  km_layout(r, kc, L);
  ROM_CHECK(L->kcp * L->rpad <= KM_BUDGET, "%s: padded kc x padded r = %d x %d = %d doubles, at most %d", who, L->kcp, L->rpad,
            L->kcp * L->rpad, KM_BUDGET);
  ROM_CHECK(L->lds_doubles * sizeof(double) <= size_t(KM_LDS_MAX) && L->ntiles <= 8 * KM_TILES,
            "%s: the LDS of the fused kernel, %zu bytes for r = %d, kc = %d, exceeds %d", who, L->lds_doubles * sizeof(double), r, kc,
            KM_LDS_MAX);
  return ROM_OK;
}

// column means (mean != 0) and the count of non-finite entries of a block into stat[0 .. 128) and stat[bad_at]
int km_stats(rom_ctx* ctx, const double* x, int64_t ldx, int64_t M, int r, int mean, int bad_at, Tmp& spart, double* stat, int* launches) {
  int rp = 1;
  while (rp < r) rp *= 2;
  const int qc = int(std::min<int64_t>(512, (M + 63) / 64));
  ROM_TRY(spart.get(ctx, size_t(qc) * (NN_RMAX + 1)));
  ROM_PROF(ctx, "km_stats", 2.0 * double(M) * r, 8.0 * double(M) * r);
  k_nn_stats_partial<<<qc, 256, 0, ctx->stream>>>(x, ldx, M, r, rp, (M + qc - 1) / qc, spart);
  k_nn_stats_finish<<<1, 1024, 0, ctx->stream>>>(spart, qc, r, M, mean, bad_at, stat);
  ROM_HIP(hipGetLastError());
  *launches += 2;
  return ROM_OK;
}

// what one assignment (and accumulation) pass needs
struct KmPass {
  rom_ctx* ctx;
  const double* x;
  int64_t ldx, M;
  int r, kc, mode;
  KmLayout L;
  SlabPlan plan;
  size_t lds;
  const double *C, *mean;
  int* labels;
  double *dist2, *part, *ipart, *ctl;
};
int km_pass(const KmPass& p, int flags, int* launches, double* executed) {
  rom_ctx* ctx = p.ctx;
  const int* done = reinterpret_cast<const int*>(p.ctl);
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(p.ctl + 2);
  const double nrows = double((p.M + SLAB_ROWS - 1) / SLAB_ROWS) * SLAB_ROWS;
  if (p.mode == 1) {
    const unsigned grid = unsigned(std::min<int64_t>((p.M + 255) / 256, 1 << 20));
    ROM_PROF(ctx, "km_exhaust", 3.0 * double(p.M) * p.kc * p.r, 8.0 * double(p.M) * p.r);
    k_km_exhaust<<<grid, 256, size_t(p.kc) * p.r * sizeof(double), ctx->stream>>>(p.x, p.ldx, p.M, p.r, p.kc, p.C, p.labels, p.dist2, cnt,
                                                                                 done, flags);
    ROM_HIP(hipGetLastError());
    *launches += 1;
    *executed += 3.0 * double(p.M) * p.kc * p.r;
    flags |= KM_GIVEN;
  }
  const double fl = (flags & KM_GIVEN ? 0.0 : 2.0 * nrows * p.L.rpad * p.L.kcp + 3.0 * double(p.M) * p.r) +
                    (flags & KM_NOACC ? 0.0 : 2.0 * nrows * p.L.kcp * p.L.rcp);
  char nm[48];
  rom_prof_name(nm, sizeof nm, "km_step", "_r%d_kc%d", p.r, p.kc);
  ROM_PROF(ctx, nm, fl, 8.0 * double(p.M) * (p.r + 2));
  k_km_step<<<p.plan.chunks, SLAB_THREADS, p.lds, ctx->stream>>>(p.x, p.ldx, p.M, p.r, p.kc, p.L.rpad, p.L.kcp, p.L.rcp, p.L.corig, p.C, p.mean,
                                                                p.plan.per_chunk, p.labels, p.dist2, p.part, p.ipart, cnt, done, flags);
  ROM_HIP(hipGetLastError());
  *launches += 1;
  *executed += fl;
  return ROM_OK;
}
int km_prepare_pass(rom_ctx* ctx, KmPass* p) {
  ROM_TRY(km_check_shape("rom_kmeans", p->r, p->kc, &p->L));
  p->plan = rom_slab_plan(ctx, p->M, p->r);
  p->lds = p->L.lds_doubles * sizeof(double);
  if (p->lds > 64 * 1024) ROM_TRY(rom_lds_optin(ctx->lds_optin_km_step, reinterpret_cast<const void*>(k_km_step), KM_LDS_MAX));
  return ROM_OK;
}

bool all_finite(const double* v, size_t n) {
  for (size_t e = 0; e < n; ++e)
    if (!(std::fabs(v[e]) <= KM_DBL_MAX)) return false;
  return true;
}

using KmGuard = HandleGuard<rom_kmeans, rom_kmeans_destroy>;

}  // namespace

extern "C" int rom_kmeans_layout(int r, int kc, int64_t* out8) {
  ROM_CHECK(out8, "rom_kmeans_layout: null argument (out8)");
  KmLayout L;
  ROM_TRY(km_check_shape("rom_kmeans_layout", r, kc, &L));
  out8[0] = L.rpad;
  out8[1] = L.kcp;
  out8[2] = int64_t(L.lds_doubles * sizeof(double));
  out8[3] = SLAB_ROWS;
  out8[4] = L.rcp;
  out8[5] = L.LT;
  out8[6] = int64_t(L.kcp) * L.rcp;
  out8[7] = (L.ntiles + 7) / 8;
  return ROM_OK;
}

extern "C" int rom_kmeans_destroy(rom_kmeans* h) {
  if (!h) return ROM_OK;
  for (rom_buf* b : {h->C, h->stat, h->counts, h->hist, h->labels})
    if (b) rom_buf_free(b);
  delete h;
  return ROM_OK;
}

extern "C" int rom_kmeans_init_maximin(rom_ctx* ctx, rom_buf* X, size_t x_off, int64_t ldx, int r, int64_t M, int kc, int64_t* rows_host) {
  ROM_CHECK(ctx && X && rows_host, "rom_kmeans_init_maximin: null argument (context, X or rows_host)");
  KmLayout L;
  ROM_TRY(km_check_shape("rom_kmeans_init_maximin", r, kc, &L));
  ROM_CHECK(M >= kc && M <= int64_t(INT_MAX), "rom_kmeans_init_maximin: M = %lld rows, at least kc = %d", (long long)M, kc);
  ROM_TRY(rom_check_block("rom_kmeans_init_maximin", {"X", "ldx", "r"}, X->n, x_off, ldx, r, M));
  ROM_HIP(hipSetDevice(ctx->device));
  const double* x = X->p + x_off;
  Tmp stat, spart, D, pbest, rows;
  int launches = 0;
  ROM_TRY(stat.get(ctx, KM_STAT));
  ROM_TRY(km_stats(ctx, x, ldx, M, r, 1, NN_RMAX, spart, stat, &launches));
  const int nb = int(std::min<int64_t>(512, (M + 255) / 256));
  ROM_TRY(D.get(ctx, size_t(M)));
  ROM_TRY(pbest.get(ctx, 4 * size_t(nb)));   // two sets of (values | rows): a launch reads one and writes the other
  ROM_TRY(rows.get(ctx, size_t(kc)));
  long long* d_rows = reinterpret_cast<long long*>(rows.p());
  {
    ROM_PROF(ctx, "km_maximin", 3.0 * double(M) * r * kc, 8.0 * double(M) * (r + 2) * kc);
    for (int s = 0; s <= kc; ++s) {
      double* in = pbest.p() + size_t((s + 1) & 1) * 2 * nb;
      double* out = pbest.p() + size_t(s & 1) * 2 * nb;
      k_km_maximin<<<s == kc ? 1 : nb, 256, 0, ctx->stream>>>(x, ldx, M, r, stat, D, s, kc, in, reinterpret_cast<const long long*>(in + nb), nb,
                                                            out, reinterpret_cast<long long*>(out + nb), d_rows);
    }
  }
  ROM_HIP(hipGetLastError());
  double bad = 0.0;
  ROM_HIP(hipMemcpyAsync(&bad, stat.p() + NN_RMAX, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ROM_HIP(hipMemcpyAsync(rows_host, d_rows, size_t(kc) * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  ROM_HIP(hipStreamSynchronize(ctx->stream));
  ROM_CHECK(bad == 0.0, "rom_kmeans_init_maximin: NaN / Inf in the block (%.0f entries)", bad);
  return ROM_OK;
}

extern "C" int rom_kmeans_fit(rom_ctx* ctx, rom_buf* X, size_t x_off, int64_t ldx, int r, int64_t M, int kc, const double* init_host,
                              int max_iter, double tol, int mode, rom_kmeans** out, double* info_host) {
  ROM_CHECK(ctx && X && init_host && out, "rom_kmeans_fit: null argument (context, X, init_host or out)");
  *out = nullptr;
  KmPass p{};
  p.ctx = ctx;
  p.r = r;
  p.kc = kc;
  p.mode = mode;
  ROM_TRY(km_check_shape("rom_kmeans_fit", r, kc, &p.L));
  ROM_CHECK(M >= kc && M <= int64_t(INT_MAX), "rom_kmeans_fit: M = %lld rows, at least kc = %d", (long long)M, kc);
  ROM_CHECK(max_iter >= 0 && max_iter <= (1 << 20), "rom_kmeans_fit: max_iter = %d", max_iter);
  ROM_CHECK(tol >= 0.0, "rom_kmeans_fit: tol = %g is negative or NaN", tol);
  ROM_CHECK(mode == 0 || mode == 1, "rom_kmeans_fit: mode = %d, 0 (fused screen) or 1 (exhaustive scan)", mode);
  ROM_TRY(rom_check_block("rom_kmeans_fit", {"X", "ldx", "r"}, X->n, x_off, ldx, r, M));
  ROM_CHECK(all_finite(init_host, size_t(kc) * r), "rom_kmeans_fit: NaN / Inf in the initial centroids");
  ROM_HIP(hipSetDevice(ctx->device));
  p.x = X->p + x_off;
  p.ldx = ldx;
  p.M = M;
  ROM_TRY(km_prepare_pass(ctx, &p));

  KmGuard guard{new rom_kmeans};
  rom_kmeans* h = guard.h;
  h->ctx = ctx;
  h->r = r;
  h->kc = kc;
  h->M_train = M;
  size_t ws_doubles = 0;
  auto keep = [&](rom_buf** b, size_t n) -> int {
    ws_doubles += n;
    return rom_buf_alloc(ctx, std::max<size_t>(n, 1), b);
  };
  auto take = [&](Tmp& tmp, size_t n) -> int {
    ws_doubles += n;
    return tmp.get(ctx, n);
  };
  ROM_TRY(keep(&h->C, size_t(kc) * r));
  ROM_TRY(keep(&h->stat, KM_STAT));
  ROM_TRY(keep(&h->counts, kc));
  ROM_TRY(keep(&h->hist, size_t(max_iter) + 1));
  ROM_TRY(keep(&h->labels, (size_t(M) + 1) / 2));
  Tmp spart, vpart, dist2, part, ipart, shift2, ctl;
  ROM_TRY(take(dist2, size_t(M)));
  ROM_TRY(take(part, size_t(p.plan.chunks) * p.L.kcp * p.L.rcp));
  ROM_TRY(take(ipart, p.plan.chunks));
  ROM_TRY(take(shift2, kc));
  ROM_TRY(take(ctl, KM_CTL));
  p.C = h->C->p;
  p.mean = h->stat->p;
  p.labels = reinterpret_cast<int*>(h->labels->p);
  p.dist2 = dist2;
  p.part = part;
  p.ipart = ipart;
  p.ctl = ctl;

  int launches = 0, syncs = 0;
  double executed = 0.0;
  ROM_HIP(hipMemcpyAsync(h->C->p, init_host, size_t(kc) * r * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  ROM_HIP(hipMemsetAsync(h->labels->p, 0xff, (size_t(M) + 1) / 2 * sizeof(double), ctx->stream));   // (no label yet: -1)
  ROM_HIP(hipMemsetAsync(ctl.p(), 0, KM_CTL * sizeof(double), ctx->stream));
  ROM_TRY(km_stats(ctx, p.x, ldx, M, r, 1, NN_RMAX, spart, h->stat->p, &launches));
  ws_doubles += spart.b->n;
  if (tol > 0.0 && max_iter > 0) {
    const int vc = int(std::min<int64_t>(512, (M + 255) / 256));
    ROM_TRY(take(vpart, vc));
    k_km_var_partial<<<vc, 256, 0, ctx->stream>>>(p.x, ldx, M, r, p.mean, (M + vc - 1) / vc, vpart);
    k_km_var_finish<<<1, 1, 0, ctx->stream>>>(vpart, vc, double(M) * r, ctl.p() + 4);
    ROM_HIP(hipGetLastError());
    launches += 2;
  }
  double hctl[KM_CTL], bad = 0.0;
  int st[4] = {0, 0, 0, 0};
  auto read_status = [&]() -> int {
    ROM_HIP(hipMemcpyAsync(hctl, ctl.p(), sizeof hctl, hipMemcpyDeviceToHost, ctx->stream));
    ROM_HIP(hipMemcpyAsync(&bad, h->stat->p + NN_RMAX, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ROM_HIP(hipStreamSynchronize(ctx->stream));
    syncs += 1;
    std::memcpy(st, hctl, sizeof st);
    ROM_CHECK(bad == 0.0, "rom_kmeans_fit: NaN / Inf in the block (%.0f entries)", bad);
    return ROM_OK;
  };
  for (int it0 = 0; it0 < max_iter && !st[0]; it0 += KM_GROUP) {
    for (int it = it0; it < std::min(max_iter, it0 + KM_GROUP); ++it) {
      ROM_TRY(km_pass(p, 0, &launches, &executed));
      k_km_update<<<kc, 256, 0, ctx->stream>>>(part, p.plan.chunks, p.L.kcp, p.L.rcp, r, p.mean, h->C->p, h->counts->p, shift2,
                                              reinterpret_cast<const int*>(ctl.p()), 0);
      k_km_control<<<1, 64, 0, ctx->stream>>>(ipart, p.plan.chunks, shift2, kc, ctl, h->hist->p, tol, max_iter, 0);
      ROM_HIP(hipGetLastError());
      launches += 2;
    }
    ROM_TRY(read_status());
  }
  // the assignment against the centroids that are returned, its counts and its inertia
  ROM_TRY(km_pass(p, KM_FORCE, &launches, &executed));
  k_km_update<<<kc, 256, 0, ctx->stream>>>(part, p.plan.chunks, p.L.kcp, p.L.rcp, r, p.mean, h->C->p, h->counts->p, shift2,
                                          reinterpret_cast<const int*>(ctl.p()), KM_FORCE | KM_NOACC);
  k_km_control<<<1, 64, 0, ctx->stream>>>(ipart, p.plan.chunks, shift2, kc, ctl, h->hist->p, tol, max_iter, 1);
  ROM_HIP(hipGetLastError());
  launches += 2;
  ROM_TRY(read_status());
  h->iterations = st[1];
  h->converged = st[2];
  h->stop = st[3];
  h->launches = launches;
  h->syncs = syncs;
  if (info_host) {
    unsigned long long cnt[2];
    std::memcpy(cnt, hctl + 2, sizeof cnt);
    info_host[0] = st[1];
    info_host[1] = st[2];
    info_host[2] = launches;
    info_host[3] = syncs;
    info_host[4] = double(ws_doubles) * sizeof(double);
    info_host[5] = p.plan.chunks;
    info_host[6] = double(cnt[1]);
    info_host[7] = executed;
  }
  *out = guard.release();
  return ROM_OK;
}

extern "C" int rom_kmeans_assign(rom_kmeans* h, rom_buf* X, size_t x_off, int64_t ldx, int64_t M, int mode, int32_t* labels_host,
                                 double* dist2_host, double* inertia_host) {
  ROM_CHECK(h && X && labels_host, "rom_kmeans_assign: null argument (handle, X or labels_host)");
  ROM_CHECK(M >= 1 && M <= int64_t(INT_MAX), "rom_kmeans_assign: M = %lld rows, at least 1", (long long)M);
  ROM_CHECK(mode == 0 || mode == 1, "rom_kmeans_assign: mode = %d, 0 (fused screen) or 1 (exhaustive scan)", mode);
  ROM_TRY(rom_check_block("rom_kmeans_assign", {"X", "ldx", "r"}, X->n, x_off, ldx, h->r, M));
  rom_ctx* ctx = h->ctx;
  ROM_HIP(hipSetDevice(ctx->device));
  KmPass p{};
  p.ctx = ctx;
  p.x = X->p + x_off;
  p.ldx = ldx;
  p.M = M;
  p.r = h->r;
  p.kc = h->kc;
  p.mode = mode;
  ROM_TRY(km_prepare_pass(ctx, &p));
  Tmp spart, stat, labels, dist2, ipart, ctl;
  ROM_TRY(stat.get(ctx, KM_STAT));
  ROM_TRY(labels.get(ctx, (size_t(M) + 1) / 2));
  ROM_TRY(dist2.get(ctx, size_t(M)));
  ROM_TRY(ipart.get(ctx, p.plan.chunks));
  ROM_TRY(ctl.get(ctx, KM_CTL + 1));
  p.C = h->C->p;
  p.mean = h->stat->p;
  p.labels = reinterpret_cast<int*>(labels.p());
  p.dist2 = dist2;
  p.part = nullptr;
  p.ipart = ipart;
  p.ctl = ctl;
  int launches = 0;
  double executed = 0.0;
  ROM_HIP(hipMemsetAsync(ctl.p(), 0, (KM_CTL + 1) * sizeof(double), ctx->stream));
  ROM_HIP(hipMemsetAsync(labels.p(), 0xff, (size_t(M) + 1) / 2 * sizeof(double), ctx->stream));
  ROM_TRY(km_stats(ctx, p.x, ldx, M, h->r, 0, NN_RMAX, spart, stat, &launches));
  ROM_TRY(km_pass(p, KM_FORCE | KM_NOACC, &launches, &executed));
  k_km_control<<<1, 64, 0, ctx->stream>>>(ipart, p.plan.chunks, nullptr, h->kc, ctl, ctl.p() + KM_CTL, 0.0, 0, 1);
  ROM_HIP(hipGetLastError());
  double bad = 0.0, inertia = 0.0;
  ROM_HIP(hipMemcpyAsync(&bad, stat.p() + NN_RMAX, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ROM_HIP(hipMemcpyAsync(&inertia, ctl.p() + KM_CTL, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ROM_HIP(hipMemcpyAsync(labels_host, labels.p(), size_t(M) * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (dist2_host) ROM_HIP(hipMemcpyAsync(dist2_host, dist2.p(), size_t(M) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ROM_HIP(hipStreamSynchronize(ctx->stream));
  h->launches += launches + 1;
  h->syncs += 1;
  ROM_CHECK(bad == 0.0, "rom_kmeans_assign: NaN / Inf in the block (%.0f entries)", bad);
  if (inertia_host) *inertia_host = inertia;
  return ROM_OK;
}

extern "C" int rom_kmeans_query(rom_kmeans* h, int64_t* out8) {
  ROM_CHECK(h && out8, "rom_kmeans_query: null argument");
  out8[0] = h->r;
  out8[1] = h->kc;
  out8[2] = h->M_train;
  out8[3] = h->iterations;
  out8[4] = h->converged;
  out8[5] = h->stop;
  out8[6] = h->launches;
  out8[7] = h->syncs;
  return ROM_OK;
}

extern "C" int rom_kmeans_download(rom_kmeans* h, int what, double* host, size_t count) {
  ROM_CHECK(h && host, "rom_kmeans_download: null argument");
  ROM_CHECK(what >= 0 && what <= 4, "rom_kmeans_download: what = %d, 0 centroids, 1 counts, 2 inertia, 3 shift, 4 labels", what);
  const size_t sizes[5] = {size_t(h->kc) * h->r, size_t(h->kc), size_t(h->iterations) + 1, size_t(h->r), size_t(h->M_train)};
  ROM_CHECK(count == sizes[what], "rom_kmeans_download: part %d holds %zu values, count = %zu", what, sizes[what], count);
  rom_ctx* ctx = h->ctx;
  ROM_HIP(hipSetDevice(ctx->device));
  h->syncs += 1;
  if (what == 4) {
    std::vector<int32_t> lab(count);
    ROM_HIP(hipMemcpyAsync(lab.data(), h->labels->p, count * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    ROM_HIP(hipStreamSynchronize(ctx->stream));
    for (size_t e = 0; e < count; ++e) host[e] = double(lab[e]);
    return ROM_OK;
  }
  const rom_buf* src[4] = {h->C, h->counts, h->hist, h->stat};
  return download(ctx, src[what]->p, host, count);
}
