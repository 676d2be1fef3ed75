// Residual error bounds of the Galerkin ROM without truth snapshots, and the weak greedy built on them
// (rom_resid_*, rom_weak_greedy; include/romhc.h).
//
// The problem is affine, A(a) = sum_q a_q A_q with A_q positive semidefinite and sum_q A_q = A_1, so for u_n = W^T c
//     r(a) = f - A(a) u_n = sum_j z_j g_j ,   g_0 = f, g_{1 + i k + q} = A_q w_i ,   z = (1, -c_i a_q) ,
// and  ||r|| / max_q a_q <= ||u(a) - u_n(a)||_{H^1_0} <= ||r|| / min_q a_q  with the H^-1 norm ||r||^2 = r^T A_1^-1 r.
// With A_1 = S Lambda S (rom_spectral.hip) and g^_j = Lambda^-1/2 o (S_r g_j S_c) -- rom_launch_sine_transform, (0, -1) --
// the H^-1 norm of a combination of the g_j is the Euclidean norm of the same combination of the g^_j.
//
// The textbook form ||r||^2 = z^T G z, G the Gram matrix of the g^_j, cancels down to sqrt(eps) ||f||; the Galerkin errors at
// contrasts 1e6 .. 1e8 lie below that.  So the g^_j are orthonormalised as they arrive (two Gram-Schmidt rounds against the
// rows of Q found so far; g^_j = sum_i R_ij q_i) and the estimator is ||R z||_2: no P x P Gram matrix is ever formed.
// The functionals are rank deficient by construction (after the first pick f = sum_q a_q A_q u_1 lies in their span): a
// functional whose remainder is at roundoff of its norm (RS_DROP) adds no row to Q and keeps its column of R.
//
// Offline (rom_resid_append), per basis row: CGS2 in the A_1 inner product with the dead-row rule (romb_a1_append); the
// reduced tensor W A_q W^T and W f grown by kb_grow_ahat; the k new functionals by the per-block stencil
// apply; their transform; their orthonormalisation.  The decision whether a functional adds a row is taken on the host: one
// synchronisation per functional (the rank sizes the next products).
// Online (rom_resid_eval): the reduced solves (rom_launch_reduced_solve on the leading n x n blocks; a dead direction has a
// unit diagonal and coefficient 0), then kr_resid_eval on the rom_mma.h tile engine: one workgroup owns 64 parameters and
// walks the column tiles of R in order.  The A operand is never stored: z_mj = -c[m, i(j)] a[m, q(j)] is formed from the
// (M, n) and (M, k) arrays as it is staged.  B = R (rank x P, row stride a multiple of 4 doubles) stays in L2.  Each thread
// adds the squares of its accumulators over the column tiles in tile order, the 16 lanes of a row are summed by a fixed
// butterfly and the two wave columns through LDS: no floating-point atomics, the same bits on every call.
#include <algorithm>
#include <cmath>
#include <vector>

#include "rom_mma.h"
#include "rom_ops.h"

#include "rom_basis_int.h"

// a functional adds a row to Q when ||remainder||^2 > RS_DROP ||g^||^2 (1e-14 of its norm: ten times the roundoff of the two
// rounds, a tenth of what the bound C eps (P + nr + nc) S of the tests allows a dropped remainder to be)
constexpr double RS_DROP = 1e-28;
constexpr int64_t RS_CHUNK = int64_t(1) << 18;  // parameters per reduced-solve launch of rom_resid_eval

struct rom_resid {
  rom_fem* f = nullptr;
  int n_cap = 0, n = 0, n_live = 0, k = 0, P = 1, rank = 0, p_cap = 0, rank_cap = 0, ldR = 0;
  unsigned long long syncs = 0;
  rom_buf *W = nullptr, *AW = nullptr, *Ahat = nullptr, *bhat = nullptr, *dead = nullptr, *Q = nullptr, *R = nullptr;
  rom_buf *onehot = nullptr, *Bt = nullptr, *ZB = nullptr, *GH = nullptr, *col = nullptr, *t1 = nullptr, *t2 = nullptr;
  rom_buf *norm0 = nullptr, *nrm1 = nullptr, *nrm2 = nullptr, *s = nullptr;
  std::vector<int> rank_at;  // rank after the functionals of the first n rows, n = 0 .. n_cap
  std::vector<int> dead_host;
};

namespace {

// q = g / sqrt(s2)
__global__ void kr_unit_row(double* __restrict__ q, const double* __restrict__ g, long long dim, const double* __restrict__ s2) {
  const double a = 1.0 / sqrt(*s2);
  for (long long j = blockIdx.x * (long long)blockDim.x + threadIdx.x; j < dim; j += (long long)gridDim.x * blockDim.x) q[j] = a * g[j];
}

// column j of R: R[i, j] = t1[i] + t2[i] for i < rank; with a new row, R[rank, j] = sqrt(s2)
__global__ void kr_rcol(double* __restrict__ R, int ldR, int j, int rank, const double* __restrict__ t1,
                        const double* __restrict__ t2, const double* __restrict__ s2, int live) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < rank) R[size_t(i) * ldR + j] = t1[i] + t2[i];
  else if (i == rank && live) R[size_t(i) * ldR + j] = sqrt(*s2);
}

// dst[(b * n + i) * n + j] = src[(b * ld + i) * ld + j]
__global__ void kr_compact_ahat(double* __restrict__ dst, const double* __restrict__ src, int k, int n, int ld) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= k * n * n) return;
  const int b = idx / (n * n), r = idx % (n * n);
  dst[idx] = src[(size_t(b) * ld + r / n) * ld + r % n];
}

// dst[i * P + j] = R[i * ldR + j], i < rank, j < P
__global__ void kr_compact_r(double* __restrict__ dst, const double* __restrict__ R, int rank, int P, int ldR) {
  const long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (idx >= (long long)rank * P) return;
  dst[idx] = R[(idx / P) * ldR + idx % P];
}

// ---- the estimator ------------------------------------------------------------------------------------------------------
// DELTA[m] = w_m || R[0..rank, 0..P) z_m ||_2,  z_m0 = 1, z_m,1+ik+q = -c[m, i] a[m, q].  grid ceil(M / 64) x 256.
// Rows m >= M, columns j >= P and rows of R >= rank are staged as zeros and never read.
__global__ __launch_bounds__(256) void kr_resid_eval(long long M, int n, int k, int P, int rank, const double* __restrict__ c,
                                                     const double* __restrict__ a, const double* __restrict__ R, int ldR,
                                                     const double* __restrict__ w, double* __restrict__ delta) {
  __shared__ __align__(16) double stage[STAGE_TOTAL];
  __shared__ double red[64][2];
  const WavePos wp;
  const long long m0 = blockIdx.x * 64ll;
  const int srow = stage_row(), seg = stage_seg();
  const long long m = m0 + srow;
  const bool m_ok = m < M;
  const double* __restrict__ cm = c + (m_ok ? m : 0) * n;
  const double* __restrict__ am = a + (m_ok ? m : 0) * k;
  auto loadA = [&](int ch, double v[4]) {
    const int j0 = ch * BK + seg;
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      const int j = j0 + x;
      double z = 0.0;
      if (m_ok && j < P) {
        if (j == 0) {
          z = 1.0;
        } else {
          const int i = (j - 1) / k, q = (j - 1) - i * k;
          z = -cm[i] * am[q];
        }
      }
      v[x] = z;
    }
  };
  const int nch = (P + BK - 1) / BK;
  const int ntiles = (rank + 63) / 64;
  double ss[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int g = 0; g < 4; ++g) ss[i][g] = 0.0;
  for (int ct = 0; ct < ntiles; ++ct) {
    const int r = ct * 64 + srow;
    const double* __restrict__ Rr = R + size_t(r < rank ? r : 0) * ldR;
    auto loadB = [&](int ch, double v[4]) {
      const int j0 = ch * BK + seg;
      load4_aligned((r < rank && j0 < ldR) ? Rr + j0 : nullptr, v);  // (j0 and ldR are multiples of 4: the four lie inside the row)
#pragma unroll
      for (int x = 0; x < 4; ++x)
        if (j0 + x >= P) v[x] = 0.0;
    };
    Acc acc;
    acc_zero(acc);
    gemm_loop(nch, loadA, loadB, acc, stage, wp);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const double x0 = acc.c[i][0][g], x1 = acc.c[i][1][g];
        ss[i][g] += x0 * x0 + x1 * x1;
      }
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      double v = ss[i][g];
      v += __shfl_xor(v, 1, 64);
      v += __shfl_xor(v, 2, 64);
      v += __shfl_xor(v, 4, 64);
      v += __shfl_xor(v, 8, 64);
      if ((wp.lane & 15) == 0) red[acc_row(wp, i, g)][wp.wc] = v;
    }
  __syncthreads();
  if (threadIdx.x < 64) {
    const long long mo = m0 + threadIdx.x;
    if (mo < M) delta[mo] = (w ? w[mo] : 1.0) * sqrt(red[threadIdx.x][0] + red[threadIdx.x][1]);
  }
}

// the parameters already picked leave the competition (their residual is noise)
__global__ void kr_mask_picked(double* __restrict__ delta, const long long* __restrict__ picks, int count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) delta[picks[i]] = -1.0;
}

// first maximum of v[0..M) (np.argmax; NaN never wins): out[0] = index (-1: nothing non-negative), out[1] = value,
// out[2] = status word; the pick is appended to picks[step] when there is one.  One workgroup.
__global__ __launch_bounds__(1024) void kr_argmax(long long M, const double* __restrict__ v, double* __restrict__ out,
                                                  long long* __restrict__ picks, int step, const int* __restrict__ status) {
  __shared__ double bv[1024];
  __shared__ long long bi[1024];
  double best = -1.0;
  long long at = -1;
  for (long long m = threadIdx.x; m < M; m += 1024) {
    const double x = v[m];
    if (x > best) { best = x; at = m; }
  }
  bv[threadIdx.x] = best;
  bi[threadIdx.x] = at;
  __syncthreads();
  for (int s = 512; s > 0; s >>= 1) {
    if (int(threadIdx.x) < s) {
      const double o = bv[threadIdx.x + s];
      const long long oi = bi[threadIdx.x + s];
      if (oi >= 0 && (o > bv[threadIdx.x] || bi[threadIdx.x] < 0 || (o == bv[threadIdx.x] && oi < bi[threadIdx.x]))) {
        bv[threadIdx.x] = o;
        bi[threadIdx.x] = oi;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = double(bi[0]);
    out[1] = bv[0];
    out[2] = double(*status);
    if (bi[0] >= 0) picks[step] = bi[0];
  }
}

int alloc(rom_ctx* ctx, size_t n, rom_buf** out) { return rom_buf_alloc(ctx, std::max<size_t>(n, 1), out); }

// orthonormalise the transformed functional g (dim doubles, overwritten) against Q and append column j of R
int add_functional(rom_resid* h, double* g, int j) {
  rom_fem* f = h->f;
  rom_ctx* ctx = f->ctx;
  const int64_t dim = f->dim;
  const int rank = h->rank;
  double* s = h->s->p;
  ROM_TRY(rom_launch_l2norm(ctx, g, 1, dim, s, false));
  if (rank > 0) {
    for (int round = 0; round < 2; ++round) {
      double* t = round == 0 ? h->t1->p : h->t2->p;
      ROM_TRY(rom_launch_rowdot(ctx, h->Q->p, rank, dim, g, t));
      ROM_TRY(rom_launch_gemm_nn(ctx, 1, dim, rank, -1.0, t, rank, h->Q->p, dim, 1.0, g, dim));
    }
  }
  ROM_TRY(rom_launch_l2norm(ctx, g, 1, dim, s + 1, false));
  double host[2] = {0.0, 0.0};
  ROM_TRY(download(ctx, s, host, 2));
  ++h->syncs;
  const bool live = host[1] > RS_DROP * host[0] && host[1] > 0.0 && rank < h->rank_cap;
  if (live) {
    kr_unit_row<<<vector_grid(dim), 256, 0, ctx->stream>>>(h->Q->p + size_t(rank) * dim, g, dim, s + 1);
    ROM_HIP(hipGetLastError());
  }
  kr_rcol<<<blocks_for(size_t(rank) + 1), 256, 0, ctx->stream>>>(h->R->p, h->ldR, j, rank, h->t1->p, h->t2->p, s + 1, live ? 1 : 0);
  ROM_HIP(hipGetLastError());
  if (live) ++h->rank;
  return ROM_OK;
}

void free_all(rom_resid* h) {
  rom_buf* bufs[] = {h->W, h->AW, h->Ahat, h->bhat, h->dead, h->Q, h->R, h->onehot, h->Bt, h->ZB, h->GH, h->col, h->t1, h->t2,
                     h->norm0, h->nrm1, h->nrm2, h->s};
  for (rom_buf* b : bufs)
    if (b) rom_buf_free(b);
  delete h;
}

int create_body(rom_resid* h) {
  rom_fem* f = h->f;
  rom_ctx* ctx = f->ctx;
  const int64_t dim = f->dim;
  const int nb = std::max(h->n_cap, 1), k = h->k;
  ROM_TRY(alloc(ctx, size_t(nb) * dim, &h->W));
  ROM_TRY(alloc(ctx, size_t(nb) * dim, &h->AW));
  ROM_TRY(alloc(ctx, size_t(k) * nb * nb, &h->Ahat));
  ROM_TRY(alloc(ctx, nb, &h->bhat));
  ROM_TRY(alloc(ctx, nb, &h->dead));  // n_cap ints in a block of n_cap doubles
  ROM_TRY(alloc(ctx, size_t(h->rank_cap) * dim, &h->Q));
  ROM_TRY(alloc(ctx, size_t(h->rank_cap) * h->ldR, &h->R));
  ROM_TRY(alloc(ctx, size_t(k) * k, &h->onehot));
  ROM_TRY(alloc(ctx, dim, &h->Bt));
  ROM_TRY(alloc(ctx, size_t(k) * dim, &h->ZB));
  ROM_TRY(alloc(ctx, size_t(k) * dim, &h->GH));
  ROM_TRY(alloc(ctx, size_t(nb) * k, &h->col));
  ROM_TRY(alloc(ctx, std::max(h->rank_cap, nb), &h->t1));
  ROM_TRY(alloc(ctx, std::max(h->rank_cap, nb), &h->t2));
  ROM_TRY(alloc(ctx, nb, &h->norm0));
  ROM_TRY(alloc(ctx, nb, &h->nrm1));
  ROM_TRY(alloc(ctx, nb, &h->nrm2));
  ROM_TRY(alloc(ctx, 4, &h->s));
  ROM_HIP(hipMemsetAsync(h->R->p, 0, size_t(h->rank_cap) * h->ldR * sizeof(double), ctx->stream));
  ROM_HIP(hipMemsetAsync(h->Ahat->p, 0, size_t(k) * nb * nb * sizeof(double), ctx->stream));
  ROM_HIP(hipMemsetAsync(h->bhat->p, 0, size_t(nb) * sizeof(double), ctx->stream));
  ROM_HIP(hipMemsetAsync(h->dead->p, 0, size_t(nb) * sizeof(double), ctx->stream));
  ROM_HIP(hipMemsetAsync(h->t1->p, 0, size_t(std::max(h->rank_cap, nb)) * sizeof(double), ctx->stream));
  ROM_HIP(hipMemsetAsync(h->t2->p, 0, size_t(std::max(h->rank_cap, nb)) * sizeof(double), ctx->stream));
  ROM_TRY(romb_onehot(ctx, k, h->onehot->p));
  ROM_TRY(romb_load_vector(f, h->Bt->p));
  // g_0 = f
  ROM_TRY(rom_launch_sine_transform(f, h->Bt->p, 1, 0, -1, h->GH->p));
  ROM_TRY(add_functional(h, h->GH->p, 0));
  h->rank_at[0] = h->rank;
  return ROM_OK;
}

// enqueue the evaluation of M parameters at basis size n (no status read-back); c: M x n coefficients (n > 0)
int eval_enqueue(rom_resid* h, const double* a, int64_t M, int n, const double* w, double* delta, double* c) {
  rom_ctx* ctx = h->f->ctx;
  const int k = h->k, P = 1 + k * n, rank = h->rank_at[n];
  if (n > 0) {
    for (int64_t m0 = 0; m0 < M; m0 += RS_CHUNK) {
      const int Mc = int(std::min<int64_t>(RS_CHUNK, M - m0));
      ROM_TRY(rom_launch_reduced_solve(ctx, n, std::max(h->n_cap, 1), k, Mc, h->Ahat->p, a + m0 * k, h->bhat->p, 0, c + m0 * n));
    }
  }
  {
    ROM_PROF(ctx, "resid_eval", 2.0 * double(M) * P * rank, 8.0 * double(M) * (n + k + 1));
    kr_resid_eval<<<unsigned((M + 63) / 64), 256, 0, ctx->stream>>>(M, n, k, P, rank, c, a, h->R->p, h->ldR, w, delta);
  }
  ROM_HIP(hipGetLastError());
  return ROM_OK;
}

}  // namespace

extern "C" int rom_resid_create(rom_fem* f, int n_cap, rom_resid** out) {
  ROM_CHECK(f && out, "rom_resid_create: null argument");
  ROM_CHECK(n_cap >= 0 && n_cap <= 2048, "rom_resid_create: capacity %d outside [0, 2048]", n_cap);
  const int k = f->nrb * f->ncb;
  const int64_t p_cap = 1 + int64_t(k) * n_cap;
  ROM_CHECK(p_cap <= 65535, "rom_resid_create: %lld functionals (at most 65535)", (long long)p_cap);
  *out = nullptr;
  rom_resid* h = new rom_resid;
  h->f = f;
  h->n_cap = n_cap;
  h->k = k;
  h->p_cap = int(p_cap);
  h->rank_cap = int(std::min<int64_t>(p_cap, f->dim));
  h->ldR = (h->p_cap + 3) / 4 * 4;
  h->rank_at.assign(size_t(n_cap) + 1, 0);
  h->dead_host.assign(size_t(std::max(n_cap, 1)), 0);
  const int st = create_body(h);
  if (st != ROM_OK) {
    free_all(h);
    return st;
  }
  *out = h;
  return ROM_OK;
}

extern "C" int rom_resid_destroy(rom_resid* h) {
  if (!h) return ROM_OK;
  hipStreamSynchronize(h->f->ctx->stream);
  free_all(h);
  return ROM_OK;
}

extern "C" int rom_resid_append(rom_resid* h, rom_buf* C, int64_t c_row0, int rows) {
  ROM_CHECK(h && (C || rows == 0), "rom_resid_append: null argument");
  ROM_CHECK(rows >= 0 && c_row0 >= 0, "rom_resid_append: negative size or offset");
  ROM_CHECK(h->n + rows <= h->n_cap, "rom_resid_append: %d rows beyond the capacity %d", h->n + rows, h->n_cap);
  rom_fem* f = h->f;
  rom_ctx* ctx = f->ctx;
  const int64_t dim = f->dim;
  const int k = h->k;
  ROM_CHECK(rows == 0 || size_t(c_row0 + rows) * dim <= C->n, "rom_resid_append: rows out of range");
  int* d_dead = reinterpret_cast<int*>(h->dead->p);
  double *W = h->W->p, *AW = h->AW->p, *norm0 = h->norm0->p;
  for (int rr = 0; rr < rows; ++rr) {
    const int i = h->n;
    double* wi = W + size_t(i) * dim;
    // 1. w_i: CGS2 in the A_1 inner product
    ROM_HIP(hipMemcpyAsync(wi, C->p + (c_row0 + rr) * dim, size_t(dim) * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    ROM_TRY(rom_launch_h10norm(f, wi, nullptr, 1, norm0 + i, false));
    ROM_TRY(romb_a1_append(f, W, AW, i, norm0, h->t1->p, h->t2->p, h->nrm1->p + i, h->nrm2->p + i, d_dead));
    // 2. the reduced tensor and load grow by one row
    ROM_TRY(rom_launch_stencil_apply_blocks(f, h->onehot->p, wi, h->ZB->p));                                      // A_q w_i, all q
    ROM_TRY(rom_launch_gemm_nt(ctx, i + 1, k, dim, 1.0, W, dim, h->ZB->p, dim, 0.0, h->col->p, k, "gemm_nt"));    // w_l . A_q w_i
    kb_grow_ahat<<<blocks_for(size_t(i + 1) * k), 256, 0, ctx->stream>>>(h->Ahat->p, k, std::max(h->n_cap, 1), i, h->col->p, d_dead, i);
    ROM_HIP(hipGetLastError());
    ROM_TRY(rom_launch_rowdot(ctx, wi, 1, dim, h->Bt->p, h->bhat->p + i));                                        // w_i . f
    // 3. the k new functionals in H^-1 coordinates, orthonormalised against what is there
    ROM_TRY(rom_launch_sine_transform(f, h->ZB->p, k, 0, -1, h->GH->p));
    for (int q = 0; q < k; ++q) ROM_TRY(add_functional(h, h->GH->p + size_t(q) * dim, 1 + i * k + q));
    kb_ints_to_doubles<<<1, 1, 0, ctx->stream>>>(d_dead + i, h->s->p + 2, 1);
    ROM_HIP(hipGetLastError());
    double dead = 0.0;
    ROM_TRY(download(ctx, h->s->p + 2, &dead, 1));
    ++h->syncs;
    h->dead_host[i] = dead != 0.0 ? 1 : 0;
    h->n = i + 1;
    h->n_live += dead != 0.0 ? 0 : 1;
    h->P = 1 + k * h->n;
    h->rank_at[h->n] = h->rank;
  }
  return ROM_OK;
}

extern "C" int rom_resid_query(rom_resid* h, int64_t* out8) {
  ROM_CHECK(h && out8, "rom_resid_query: null argument");
  out8[0] = h->n;
  out8[1] = h->n_live;
  out8[2] = h->P;
  out8[3] = h->rank;
  out8[4] = h->n_cap;
  out8[5] = h->k;
  out8[6] = h->f->dim;
  out8[7] = int64_t(h->syncs);
  return ROM_OK;
}

extern "C" int rom_resid_download(rom_resid* h, int what, double* host, size_t count) {
  ROM_CHECK(h && (host || count == 0), "rom_resid_download: null argument");
  rom_ctx* ctx = h->f->ctx;
  const int64_t dim = h->f->dim;
  const int n = h->n, k = h->k;
  size_t need = 0;
  switch (what) {
    case 0: need = size_t(h->rank) * h->P; break;
    case 1: need = size_t(h->rank) * dim; break;
    case 2: need = size_t(k) * n * n; break;
    case 3: need = size_t(n); break;
    case 4: need = size_t(n) * dim; break;
    case 5: need = size_t(n) + 1; break;
    case 6: need = size_t(n); break;
    default: ROM_CHECK(false, "rom_resid_download: what = %d outside 0 .. 6", what);
  }
  ROM_CHECK(count == need, "rom_resid_download: part %d holds %zu doubles, not %zu", what, need, count);
  if (need == 0) return ROM_OK;
  if (what == 0 || what == 2) {
    Tmp tmp;
    ROM_TRY(tmp.get(ctx, need));
    if (what == 0) kr_compact_r<<<blocks_for(need), 256, 0, ctx->stream>>>(tmp, h->R->p, h->rank, h->P, h->ldR);
    else kr_compact_ahat<<<blocks_for(need), 256, 0, ctx->stream>>>(tmp, h->Ahat->p, k, n, std::max(h->n_cap, 1));
    ROM_HIP(hipGetLastError());
    return download(ctx, tmp, host, need);
  }
  if (what == 1) return download(ctx, h->Q->p, host, need);
  if (what == 3) return download(ctx, h->bhat->p, host, need);
  if (what == 4) return download(ctx, h->W->p, host, need);
  if (what == 5) {
    for (int i = 0; i <= n; ++i) host[i] = double(h->rank_at[i]);
    return ROM_OK;
  }
  for (int i = 0; i < n; ++i) host[i] = double(h->dead_host[i]);
  return ROM_OK;
}

extern "C" int rom_resid_basis(rom_resid* h, rom_buf* OUT, int64_t out_row0) {
  ROM_CHECK(h && OUT, "rom_resid_basis: null argument");
  const int64_t dim = h->f->dim;
  ROM_CHECK(out_row0 >= 0 && size_t(out_row0 + h->n) * dim <= OUT->n, "rom_resid_basis: rows out of range");
  if (h->n == 0) return ROM_OK;
  rom_ctx* ctx = h->f->ctx;
  ROM_HIP(hipMemcpyAsync(OUT->p + out_row0 * dim, h->W->p, size_t(h->n) * dim * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  ROM_HIP(hipStreamSynchronize(ctx->stream));
  return ROM_OK;
}

extern "C" int rom_resid_eval(rom_resid* h, rom_buf* a, int64_t a_row0, int64_t M, int n, rom_buf* weights, rom_buf* DELTA,
                              int64_t d_off, rom_buf* COEF, int64_t coef_row0) {
  ROM_CHECK(h && a && DELTA, "rom_resid_eval: null argument");
  ROM_CHECK(M >= 0 && a_row0 >= 0 && d_off >= 0 && coef_row0 >= 0, "rom_resid_eval: negative size or offset");
  ROM_CHECK(n >= 0 && n <= h->n, "rom_resid_eval: n = %d outside [0, %d]", n, h->n);
  ROM_CHECK(M <= (int64_t(1) << 36), "rom_resid_eval: at most 2^36 parameters");
  const int k = h->k;
  ROM_CHECK(size_t(a_row0 + M) * k <= a->n && size_t(d_off + M) <= DELTA->n && (!weights || size_t(M) <= weights->n) &&
                (!COEF || size_t(coef_row0 + M) * n <= COEF->n),
            "rom_resid_eval: buffer too small");
  if (M == 0) return ROM_OK;
  rom_ctx* ctx = h->f->ctx;
  Tmp ctmp;
  double* c = nullptr;
  if (n > 0) {
    if (COEF) c = COEF->p + coef_row0 * n;
    else {
      ROM_TRY(ctmp.get(ctx, size_t(M) * n));
      c = ctmp.p();
    }
  }
  ROM_HIP(hipMemsetAsync(ctx->d_status, 0, sizeof(int), ctx->stream));
  ROM_TRY(eval_enqueue(h, a->p + a_row0 * k, M, n, weights ? weights->p : nullptr, DELTA->p + d_off, c));
  return read_status(ctx, "rom_resid_eval");
}

extern "C" int rom_weak_greedy(rom_fem* f, rom_buf* a, int64_t M, rom_buf* weights, int n_max, double rel_tol, rom_resid* h,
                               rom_buf* BASIS, int64_t basis_row0, int64_t* picks_out, double* crit_out, double* info_host) {
  ROM_CHECK(f && a && h && BASIS && (picks_out || n_max == 0) && (crit_out || n_max == 0), "rom_weak_greedy: null argument");
  ROM_CHECK(h->f == f, "rom_weak_greedy: the handle belongs to another FE space");
  ROM_CHECK(h->n == 0, "rom_weak_greedy: the handle already holds %d rows (a fresh one is needed)", h->n);
  ROM_CHECK(M >= 1 && M <= (int64_t(1) << 36) && n_max >= 0 && basis_row0 >= 0, "rom_weak_greedy: bad sizes");
  ROM_CHECK(n_max <= h->n_cap, "rom_weak_greedy: n_max = %d beyond the capacity %d of the handle", n_max, h->n_cap);
  const int64_t dim = f->dim;
  const int k = h->k;
  ROM_CHECK(size_t(M) * k <= a->n && (!weights || size_t(M) <= weights->n) && size_t(basis_row0 + n_max) * dim <= BASIS->n,
            "rom_weak_greedy: buffer too small");
  rom_ctx* ctx = f->ctx;
  Tmp delta, coef, out, dpicks;
  rom_buf* a1 = nullptr;
  ROM_TRY(delta.get(ctx, size_t(M)));
  ROM_TRY(coef.get(ctx, size_t(M) * std::max(n_max, 1)));
  ROM_TRY(out.get(ctx, 4));
  ROM_TRY(dpicks.get(ctx, size_t(std::max(n_max, 1))));  // int64 picks in a block of doubles
  ROM_TRY(rom_buf_alloc(ctx, size_t(k), &a1));
  long long* d_picks = reinterpret_cast<long long*>(dpicks.p());
  const unsigned long long syncs0 = h->syncs;
  unsigned long long syncs = 0;
  int step = 0, stop = 0, st = ROM_OK;
  double crit0 = 0.0, last = 0.0;
  auto body = [&]() -> int {
    for (; step < n_max; ++step) {
      ROM_HIP(hipMemsetAsync(ctx->d_status, 0, sizeof(int), ctx->stream));
      ROM_TRY(eval_enqueue(h, a->p, M, step, weights ? weights->p : nullptr, delta, coef));
      if (step > 0) {
        kr_mask_picked<<<blocks_for(size_t(step)), 256, 0, ctx->stream>>>(delta, d_picks, step);
        ROM_HIP(hipGetLastError());
      }
      kr_argmax<<<1, 1024, 0, ctx->stream>>>(M, delta, out, d_picks, step, ctx->d_status);
      ROM_HIP(hipGetLastError());
      double host[3] = {0.0, 0.0, 0.0};
      ROM_TRY(download(ctx, out, host, 3));
      ++syncs;
      if (host[2] != 0.0) {
        ROM_HIP(hipMemsetAsync(ctx->d_status, 0, sizeof(int), ctx->stream));
        rom_set_error("rom_weak_greedy: reduced matrix not positive definite");
        return ROM_ERR_NOT_SPD;
      }
      if (host[0] < 0.0) {  // every parameter has been picked
        stop = 2;
        return ROM_OK;
      }
      last = host[1];
      if (step == 0) crit0 = last;
      if (last <= rel_tol * crit0) {
        stop = 1;
        return ROM_OK;
      }
      const int64_t pick = int64_t(host[0]);
      picks_out[step] = pick;
      crit_out[step] = last;
      ROM_HIP(hipMemcpyAsync(a1->p, a->p + pick * k, size_t(k) * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
      ROM_TRY(rom_solve_batch(f, a1, 1, BASIS, basis_row0 + step));
      ++syncs;
      ROM_TRY(rom_resid_append(h, BASIS, basis_row0 + step, 1));
    }
    return ROM_OK;
  };
  st = body();
  hipStreamSynchronize(ctx->stream);
  rom_buf_free(a1);
  if (st != ROM_OK) return st;
  if (info_host) {
    int dead = 0;
    for (int i = 0; i < h->n; ++i) dead += h->dead_host[i];
    info_host[0] = double(step);
    info_host[1] = double(dead);
    info_host[2] = double(stop);
    info_host[3] = double(h->rank);
    info_host[4] = double(syncs + (h->syncs - syncs0));
    info_host[5] = last;
  }
  return ROM_OK;
}
