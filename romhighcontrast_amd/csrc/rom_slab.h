// Slab engine of the tall-block kernels (k_pca_tall_fused, k_poly_pass, k_poly_predict, k_mlp_eval, k_mlp_predict): a 512-thread
// workgroup (8 waves) walks a chunk of 32-row slabs that it keeps in LDS and runs products of v_mfma_f64_16x16x4_f64 on each,
//   NT:  Y (32 x 16 nct) = A (32 x K) B^T, B a table of 16 nct rows, both operands K-contiguous with the same kind of stride;
//   NN:  Y (32 x 16 nct) = A (32 x K) B, B a table of K rows (k_mlp_eval's backward pass: the NT table of the forward pass);
//   TN:  acc += Ys^T Ys over the 32 rows, by 16 x 16 tiles given as column offsets (ca, cb) into one slab Ys.
// Device inline functions only: the kernels keep their own LDS carve-up, prefetch, barriers, epilogues and the list of TN
// tiles a wave owns (w + 8 u of the workgroup's tiles, accumulators in registers over all slabs of the chunk).
//
// Operand maps (rom_mma.h): lane l = (i = l & 15, k = l >> 4) holds A[i][k] and B[k][i]; result register g of lane l is
// (row k + 4 g, column i) of the tile.
#pragma once
#include "rom_mma.h"

constexpr int SLAB_THREADS = 512;   // 8 waves: one workgroup per CU (LDS), two waves per SIMD

// LDS row strides (doubles).  An NT operand read (lane -> row l & 15, k = l >> 4) wants rows 4 banks apart: stride = 2 mod 4
// doubles.  A TN operand read (lane -> column l & 15, row k = l >> 4: 16 consecutive doubles of four rows) wants
// consecutive rows half the banks apart: stride = 16 mod 32 doubles.
__host__ __device__ inline int slab_ld_nt(int n) { return n + 2; }
__host__ __device__ inline int slab_ld_tn(int n) { return (n & 31) == 0 ? n + 16 : n; }

// tile tt of the lower triangle listed by rows: (0,0) (1,0) (1,1) (2,0) ...
__host__ __device__ inline void lower_tile(int tt, int* ti, int* tj) {
  int r = 0;
  while ((r + 1) * (r + 2) / 2 <= tt) ++r;
  *ti = r;
  *tj = tt - r * (r + 1) / 2;
}

// slabs [*slab0, *slab1) of workgroup blockIdx.x: per_chunk slabs each, the last chunk ends with the block's M rows
__device__ inline void slab_chunk_range(long long M, long long per_chunk, long long* slab0, long long* slab1) {
  const long long nslabs = (M + SLAB_ROWS - 1) / SLAB_ROWS;
  *slab0 = (long long)blockIdx.x * per_chunk;
  *slab1 = min(nslabs, *slab0 + per_chunk);
}

// NT product of one slab.  Wave w owns row tile w & 1 and column tiles ct = (w >> 1) + 4 jj < nct, jj = 0, 1: y[jj] is tile
// (w & 1, ct) of A B^T over k < kpad (a multiple of 4; the padding of both operands is zero).  A tile at or beyond nct is
// left zero.  No barrier inside: the caller has one between the writes of A and B and this call.
__device__ __forceinline__ void slab_nt(const double* A, int lda, const double* B, int ldb, int kpad, int nct, d4_t (&y)[2]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, i = lane & 15, k = lane >> 4;
  const int rt = w & 1, ct0 = w >> 1, ct1 = ct0 + 4;
  y[0] = d4_t{0.0, 0.0, 0.0, 0.0};
  y[1] = d4_t{0.0, 0.0, 0.0, 0.0};
  const double* pa = A + (rt * 16 + i) * lda + k;
  const double* pb0 = B + (ct0 * 16 + i) * ldb + k;
  const double* pb1 = B + (ct1 * 16 + i) * ldb + k;
  if (ct1 < nct) {
    for (int kk = 0; kk < kpad; kk += 4) {
      const double a = pa[kk];
      y[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, pb0[kk], y[0], 0, 0, 0);
      y[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, pb1[kk], y[1], 0, 0, 0);
    }
  } else if (ct0 < nct) {
    for (int kk = 0; kk < kpad; kk += 4) y[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[kk], pb0[kk], y[0], 0, 0, 0);
  }
}

// NN product of one slab (k_mlp_eval's backward pass).  The tile ownership of slab_nt, but B is read "transposed": a table of
// kpad rows (the contraction index) and 16 nct columns with stride ldb, so that y[jj] is tile (w & 1, ct) of A B.  Lane
// (i, k) takes B[kk + k][16 ct + i]: the access pattern of a TN operand (rows of 16 consecutive doubles).
__device__ __forceinline__ void slab_nn(const double* A, int lda, const double* B, int ldb, int kpad, int nct, d4_t (&y)[2]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, i = lane & 15, k = lane >> 4;
  const int rt = w & 1, ct0 = w >> 1, ct1 = ct0 + 4;
  y[0] = d4_t{0.0, 0.0, 0.0, 0.0};
  y[1] = d4_t{0.0, 0.0, 0.0, 0.0};
  const double* pa = A + (rt * 16 + i) * lda + k;
  const double* pb0 = B + k * ldb + ct0 * 16 + i;
  const double* pb1 = B + k * ldb + ct1 * 16 + i;
  if (ct1 < nct) {
    for (int kk = 0; kk < kpad; kk += 4) {
      const double a = pa[kk];
      y[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, pb0[kk * ldb], y[0], 0, 0, 0);
      y[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, pb1[kk * ldb], y[1], 0, 0, 0);
    }
  } else if (ct0 < nct) {
    for (int kk = 0; kk < kpad; kk += 4) y[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[kk], pb0[kk * ldb], y[0], 0, 0, 0);
  }
}

// acc += Ys[:, ca .. ca + 16)^T Ys[:, cb .. cb + 16) over the 32 rows of the slab (stride LY): eight MFMAs
__device__ __forceinline__ void slab_tn_acc(const double* Ys, int LY, int ca, int cb, d4_t& acc) {
  const int lane = threadIdx.x & 63, i = lane & 15, k = lane >> 4;
  const double* pa = Ys + k * LY + ca + i;
  const double* pb = Ys + k * LY + cb + i;
#pragma unroll
  for (int r = 0; r < SLAB_ROWS; r += 4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[r * LY], pb[r * LY], acc, 0, 0, 0);
}
// ... and the tile goes to rows ca .., columns cb .. of the partial Pb (stride ldp)
__device__ __forceinline__ void slab_tn_store(double* Pb, int ldp, int ca, int cb, const d4_t& acc) {
  const int lane = threadIdx.x & 63, i = lane & 15, k = lane >> 4;
#pragma unroll
  for (int g = 0; g < 4; ++g) Pb[size_t(ca + k + 4 * g) * ldp + cb + i] = acc[g];
}
