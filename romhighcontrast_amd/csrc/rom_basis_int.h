// Pieces of the basis stage shared by the files built on rom_basis.hip and rom_small_dense.hip (internal).
#pragma once
#include <algorithm>

#include "rom_ops.h"

namespace {

// ---- launch grids ---------------------------------------------------------------------------------------------------
unsigned blocks_for(size_t n, int threads = 256) { return unsigned(std::max<size_t>(1, (n + threads - 1) / threads)); }
// grid of the grid-stride kernels over one vector of dim entries (kb_renormalise, kb_take_pick, ...)
unsigned vector_grid(int64_t dim) { return unsigned(std::min<int64_t>((dim + 255) / 256, 512)); }

// ---- temporaries from the context's caching allocator ---------------------------------------------------------------
struct Tmp {
  rom_buf* b = nullptr;
  Tmp() = default;
  Tmp(const Tmp&) = delete;
  Tmp& operator=(const Tmp&) = delete;
  ~Tmp() { release(); }
  void release() {
    if (b) rom_buf_free(b);
    b = nullptr;
  }
  int get(rom_ctx* ctx, size_t n) {
    release();
    return rom_buf_alloc(ctx, std::max<size_t>(n, 1), &b);
  }
  double* p() const { return b->p; }
  operator double*() const { return b->p; }
};

int read_status(rom_ctx* ctx, const char* who) {
  int status = 0;
  ROM_HIP(hipMemcpyAsync(&status, ctx->d_status, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  ROM_HIP(hipStreamSynchronize(ctx->stream));
  if (status) {
    // (reported once: the word is cleared, or the next call on this context -- whatever it is -- would report this failure again)
    ROM_HIP(hipMemsetAsync(ctx->d_status, 0, sizeof(int), ctx->stream));
    rom_set_error("%s: reduced matrix not positive definite", who);
    return ROM_ERR_NOT_SPD;
  }
  return ROM_OK;
}

int download(rom_ctx* ctx, const double* d, double* h, size_t n) {
  if (n == 0) return ROM_OK;
  ROM_HIP(hipMemcpyAsync(h, d, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ROM_HIP(hipStreamSynchronize(ctx->stream));
  return ROM_OK;
}

// destroys a half-built handle on every way out of its *_fit but the one that releases it
template <class H, int (*Destroy)(H*)>
struct HandleGuard {
  H* h;
  ~HandleGuard() {
    if (h) Destroy(h);
  }
  H* release() {
    H* r = h;
    h = nullptr;
    return r;
  }
};

// the points on the device: [ix | iy] as ints, then [tx | ty] (the host arrays are free after the next synchronisation)
struct DevPoints {
  Tmp buf;
  int* ix = nullptr;
  int* iy = nullptr;
  double* tx = nullptr;
  double* ty = nullptr;
  int upload(rom_ctx* ctx, int npts, const int* ix_host, const int* iy_host, const double* tx_host, const double* ty_host) {
    const size_t n_idx = (2 * size_t(npts) * sizeof(int) + sizeof(double) - 1) / sizeof(double);
    ROM_TRY(buf.get(ctx, n_idx + 2 * size_t(npts)));
    ix = reinterpret_cast<int*>(buf.p());
    iy = ix + npts;
    tx = buf.p() + n_idx;
    ty = tx + npts;
    ROM_HIP(hipMemcpyAsync(ix, ix_host, npts * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    ROM_HIP(hipMemcpyAsync(iy, iy_host, npts * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    ROM_HIP(hipMemcpyAsync(tx, tx_host, npts * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ROM_HIP(hipMemcpyAsync(ty, ty_host, npts * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    return ROM_OK;
  }
};

}  // namespace

// ---- small utilities of rom_basis.hip -------------------------------------------------------------------------------
// p[0..n) = v (a memset for +0.0)
int romb_fill(rom_ctx* ctx, double* p, size_t n, double v);
// out = the k x k identity: row b is the one-hot block coefficient vector that selects A_b
int romb_onehot(rom_ctx* ctx, int k, double* out);
// out[0..dim) = h^2: the load vector B_total of the unit right-hand side
int romb_load_vector(rom_fem* f, double* out);
// dst (cols x rows, ld ldd) = transpose of src (rows x cols, ld lds): small matrices only
int romb_transpose(rom_ctx* ctx, double* dst, long long ldd, const double* src, long long lds, int rows, int cols);
__global__ void kb_ints_to_doubles(const int* __restrict__ src, double* __restrict__ dst, int n);
// fixed-order sums of per-chunk partials: G (mirrored lower triangle, or NULL) and the rectangle B of Part[chunk] (ppad x ldp);
// out[j] = (column sum of part[chunk][j] over the chunks) / divisor
__global__ void kb_partials_reduce(const double* __restrict__ Part, int chunks, int ppad, int ldp, int P, int qg,
                                   double* __restrict__ G, double* __restrict__ B, int q, int c0);
__global__ void kb_partials_colsum(const double* __restrict__ part, int chunks, int n, double divisor, double* __restrict__ out);

namespace {
// The tail of the *_predict entry points.  With sums of squares wanted: get() before the launch, whose kernel writes one row of q
// partials per chunk to partials(); finish() adds them in chunk order and copies the q sums to the host.  finish() ends the call
// either way: it waits for the stream.  (The callers count their own launches and synchronisations.)
struct SumsqTail {
  Tmp SS, sums;
  int get(rom_ctx* ctx, int chunks, int q) {
    ROM_TRY(SS.get(ctx, size_t(chunks) * q));
    return sums.get(ctx, q);
  }
  double* partials() const { return SS.b ? SS.p() : nullptr; }
  int finish(rom_ctx* ctx, int chunks, int q, double* sumsq_host) {
    if (SS.b) {
      kb_partials_colsum<<<blocks_for(q), 256, 0, ctx->stream>>>(SS, chunks, q, 1.0, sums);
      ROM_HIP(hipGetLastError());
      ROM_HIP(hipMemcpyAsync(sumsq_host, sums.p(), size_t(q) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    ROM_HIP(hipStreamSynchronize(ctx->stream));
    return ROM_OK;
  }
};
}  // namespace
// (rom_pod.hip) out[0] = bits of the largest |x| among the finite entries, out[1] = number of entries that are not finite
__global__ void kp_block_amax(const double* __restrict__ X, size_t count, unsigned long long* __restrict__ out);

// ---- the A_1-orthonormal basis --------------------------------------------------------------------------------------
// A row is dead -- it adds no direction: w = 0 -- when its residual against the rows before it is at roundoff of the row:
// e2 = ||residual||_A^2 <= A1_DEAD_REL ||row||_A^2 (1e-13 of its norm), or is not positive at all (NaN included).  The one
// rule of the greedy's picks, the error curves, the sensor selection and the residual bounds.
constexpr double A1_DEAD_REL = 1e-26;
__device__ inline bool a1_dead(double e2, double norm0sq) { return !(e2 > A1_DEAD_REL * norm0sq) || !(e2 > 0.0); }
// One CGS2 step in the A_1 inner product.  On entry rows 0..i-1 of W (A_1-orthonormal or 0) and of AW = A_1 W are finished,
// row i of W holds the raw vector and norm0[i] its squared A_1 norm.  Round one leaves its coefficients in t1[0..i) and the
// squared norm of the remainder in *nrm1 (i = 0: no rounds, *nrm1 = norm0[0]); dead[i] is decided on it; the row is
// normalised (or zeroed), round two leaves t2[0..i) and *nrm2, and row i of AW is written.  t1 and t2 may
// be the same scratch when the caller does not read them.  Enqueued only.
int romb_a1_append(rom_fem* f, double* W, double* AW, int i, const double* norm0, double* t1, double* t2, double* nrm1,
                   double* nrm2, int* dead);
// reduced tensor Ahat[b] = C A_b C^T (k, n, n) and bhat = C B_total; AC: n x dim scratch for A_b C^T (overwritten)
int romb_reduced_tensor(rom_fem* f, const double* c, int n, double* AC, double* Ahat, double* bhat);

// kernels of rom_basis.hip that the factored greedy launches as well
__global__ void kb_greedy_select(int M, const double* __restrict__ err2, const double* __restrict__ extra2,
                                 const double* __restrict__ h1, int it, int* __restrict__ picks, double* __restrict__ maxerr);
__global__ void kb_grow_ahat(double* __restrict__ Ahat, int k, int ld, int j, const double* __restrict__ col,
                             const int* __restrict__ degenerate, int it);
__global__ void kb_galerkin_gap(int M, int n, const double* __restrict__ P, const double* __restrict__ c, double* __restrict__ extra2);

// ---- small dense problems (rom_small_dense.hip): SE_* modes and limits, romb_small_eig, romb_pivchol_whiten ---------
#include "rom_small_dense_host.h"

// ---- orthonormalisation helpers of rom_basis.hip, shared with rom_pod.hip -------------------------------------------
__global__ void kb_rows_axpy(double* __restrict__ out, const double* __restrict__ x, const double* __restrict__ y,
                             const double* __restrict__ f, double s, long long dim);
int romb_fill_random(rom_ctx* ctx, double* p, size_t n, unsigned long long seed, bool gaussian);
int romb_gram_transform(rom_ctx* ctx, double* X, double* Y, int b, int64_t dim, int mode, double rel_tol, int rounds);
int romb_orthonormalize_against(rom_ctx* ctx, double* V, int found, int take, int64_t dim);
