// rom_mlp_fit / rom_mlp_predict: fully connected networks between columns of a tall device block -- the "NN" entry of the
// reference's model list (src/experiments/NonLinearROM.py:54-70,138: FNNModel(hidden_layer_sizes=(20, 20), activation=
// "sigmoid")) and the regressor of src/lib/Estimators.py:75-97 (EstimatorNN: one MLPRegressor per parameter).
//
// Model: m inputs -> 1 .. 3 hidden layers of 1 .. 64 units (tanh, logistic or relu) -> q linear outputs.  Inputs scaled as in
// rom_poly_fit (mid-range c, half-range h over the training rows), targets centred and scaled by their mean and standard
// deviation.  Loss: scikit-learn's, L(w) = 1/(2M) sum_rows |net(t) - y_scaled|^2 + alpha/(2M) sum_l |W_l|_F^2.
//
// Kernels:
//   k_mlp_eval     one workgroup per chunk of 32-row slabs (rom_slab.h).  The weights sit in LDS (W_l as N_l rows of K_l, the
//                  K-contiguous table of slab_nt).  ONE slab buffer holds [A_0 | .. | A_{L} | Delta_1 | .. | Delta_{L+1}] side by
//                  side: forward A_{l+1} = act(A_l W_l^T + b_l) (slab_nt), residual and its sum of squares at the output,
//                  backward Delta_l = (Delta_{l+1} W_l) .* act'(A_l) (slab_nn: the same W_l read row-wise), and then all
//                  weight-gradient tiles Delta_{l+1}^T A_l at once (slab_tn_acc, accumulators in registers over the chunk's slabs)
//                  and the bias sums.  One partial per workgroup.
//   k_mlp_reduce   partials added in chunk order, + alpha W, / M; the loss.
//   k_mlp_predict  the forward half with the OUT / Yref / sumsq epilogue of k_poly_predict.
//   k_mlp_director one workgroup: L-BFGS two-loop recursion, Armijo backtracking and every accept / stop decision, with
//                  fixed-order reductions; writes the next trial weights and a status word.  The host enqueues (eval, reduce,
//                  director) ML_BATCH times and reads the status once per batch; launches after the stop exit at once.
// No floating-point atomics: the same bits on every call.
#include <cmath>
#include <cstring>

#include "rom_basis_int.h"
#include "rom_block.h"
#include "rom_slab.h"

namespace {

constexpr int ML_MAXIN = 64, ML_MAXH = 64, ML_MAXQ = 128, ML_MAXHID = 3, ML_LAYERS = ML_MAXHID + 1;
constexpr int ML_WBUDGET = 9216;       // padded weight doubles: 1 -> 64 -> 128 is the widest output (romhc.h)
constexpr int ML_LDS_MAX = 160 * 1024; // static + dynamic LDS of a workgroup
constexpr int ML_STATIC_LDS = 5120;    // upper bound of the kernels' static LDS (scalings 3072 B + reduction scratch 2048 B)
constexpr int ML_TILES = 5;            // weight-gradient tiles per wave: ML_WBUDGET / 256 = 36 tiles over 8 waves
constexpr int ML_XREG = SLAB_ROWS * ML_MAXIN / SLAB_THREADS;   // input values of a slab per thread
constexpr int ML_YREG = SLAB_ROWS * ML_MAXQ / SLAB_THREADS;    // target values of a slab per thread
constexpr int ML_BATCH = 16;           // (eval, reduce, director) sequences between two reads of the status word
constexpr int ML_MEMMAX = 64;          // L-BFGS pairs
constexpr int ML_TRIALS = 30;
constexpr int ML_DIR_THREADS = 1024;
constexpr double ML_C1 = 1e-4, ML_CURV = 1e-10;
constexpr double ML_DBL_MAX = 1.7976931348623157e308;

// scalings of a map on the device: c (64) | h (64) | y_mean (128) | y_scale (128) | bad X, bad Y (2, padded to 8)
constexpr int ML_SC_C = 0, ML_SC_H = 64, ML_SC_MEAN = 128, ML_SC_SCALE = 256, ML_SC_BAD = 384, ML_SC_SIZE = 392;

// director state: doubles and ints
enum { DS_F = 0, DS_GD, DS_T, DS_GINF, DS_GAMMA, DS_COUNT = 8 };
enum { IS_STATUS = 0, IS_PHASE, IS_K, IS_EVALS, IS_TRIAL, IS_NPAIRS, IS_HEAD, IS_STAG, IS_COUNT = 8 };

// LDS row stride (doubles) of the slab and of the weight tables (n a multiple of 16): = 2 mod 4, the stride of an NT operand
// (slab_ld_nt: lane -> row l & 15, k = l >> 4 is free of bank conflicts).  The row-wise reads of the same tables (slab_nn,
// slab_tn_acc: 16 consecutive doubles of four rows) then see consecutive rows 2 doubles apart, a two-way conflict between
// the k lanes of a half wave; the stride = 16 mod 32 that would avoid it makes the NT reads of the same table 8-way.
__host__ __device__ inline int ml_ld(int n) { return slab_ld_nt(n); }

struct MlpDesc {
  int nl, act;                      // weight layers (hidden + 1); 0 tanh, 1 logistic, 2 relu
  int n[ML_LAYERS + 1], np[ML_LAYERS + 1];   // widths m, hidden .., q and their multiples of 16
  int offA[ML_LAYERS], offD[ML_LAYERS + 1];  // slab columns of A_l (l = 0 .. nl - 1) and Delta_l (l = 1 .. nl)
  int LY, LYp;                      // slab row strides of k_mlp_eval and k_mlp_predict
  int wl[ML_LAYERS], ldw[ML_LAYERS], bo[ML_LAYERS];   // LDS offset / stride of W_l, offset of b_l among the staged biases
  int wtot, btot;                   // LDS doubles of all W_l, of all b_l
  int woff[ML_LAYERS], boff[ML_LAYERS];   // offsets in the flat parameter vector
  int pw[ML_LAYERS], pb[ML_LAYERS], ploss, pstride;   // offsets in a workgroup's partial
  int P, nW, wpad;                  // parameters, weights among them, padded weight doubles
};

// the single place of the limits (rom_mlp_layout): false outside them, with the reason in *why
bool mlp_plan(int m, int n_hidden, const int* hidden, int q, MlpDesc* D, size_t* lds_eval, size_t* lds_predict, const char** why) {
  static const char* msgs[] = {"m inputs: between 1 and 64", "hidden layers: between 1 and 3", "a hidden width: between 1 and 64",
                               "q targets: between 1 and 128", "padded weights: at most 9216 doubles", "LDS of a workgroup: at most 160 KB"};
  auto fail = [&](int i) {
    if (why) *why = msgs[i];
    return false;
  };
  if (m < 1 || m > ML_MAXIN) return fail(0);
  if (n_hidden < 1 || n_hidden > ML_MAXHID || !hidden) return fail(1);
  for (int l = 0; l < n_hidden; ++l)
    if (hidden[l] < 1 || hidden[l] > ML_MAXH) return fail(2);
  if (q < 1 || q > ML_MAXQ) return fail(3);
  MlpDesc d;
  std::memset(&d, 0, sizeof d);
  d.nl = n_hidden + 1;
  d.n[0] = m;
  for (int l = 0; l < n_hidden; ++l) d.n[l + 1] = hidden[l];
  d.n[d.nl] = q;
  for (int l = 0; l <= d.nl; ++l) d.np[l] = (d.n[l] + 15) / 16 * 16;
  int col = 0, wl = 0, bo = 0, P = 0, pp = 0;
  for (int l = 0; l < d.nl; ++l) {
    d.offA[l] = col;
    col += d.np[l];
  }
  const int colsA = col;
  for (int l = 1; l <= d.nl; ++l) {
    d.offD[l] = col;
    col += d.np[l];
  }
  d.LY = ml_ld(col);
  d.LYp = ml_ld(colsA);
  for (int l = 0; l < d.nl; ++l) {
    d.ldw[l] = ml_ld(d.np[l]);
    d.wl[l] = wl;
    wl += d.np[l + 1] * d.ldw[l];
    d.bo[l] = bo;
    bo += d.np[l + 1];
    d.woff[l] = P;
    P += d.n[l + 1] * d.n[l];
    d.pw[l] = pp;
    pp += d.np[l + 1] * d.np[l];
  }
  d.wtot = wl;
  d.btot = bo;
  d.nW = P;
  d.wpad = pp;
  if (d.wpad > ML_WBUDGET) return fail(4);
  for (int l = 0; l < d.nl; ++l) {
    d.boff[l] = P;
    P += d.n[l + 1];
    d.pb[l] = pp;
    pp += d.np[l + 1];
  }
  d.ploss = pp;
  d.pstride = pp + 1;
  d.P = P;
  const size_t le = size_t(d.wtot + d.btot + SLAB_ROWS * d.LY) * sizeof(double);
  const size_t lp = size_t(d.wtot + d.btot + SLAB_ROWS * d.LYp) * sizeof(double);
  if (le + ML_STATIC_LDS > size_t(ML_LDS_MAX)) return fail(5);
  if (D) *D = d;
  if (lds_eval) *lds_eval = le;
  if (lds_predict) *lds_predict = lp;
  return true;
}

__device__ inline double ml_act(int act, double z) {
  if (act == 0) return tanh(z);
  if (act == 1) return 1.0 / (1.0 + exp(-z));
  return z > 0.0 ? z : 0.0;
}
// the derivative from the stored activation
__device__ inline double ml_dact(int act, double a) {
  if (act == 0) return 1.0 - a * a;
  if (act == 1) return a * (1.0 - a);
  return a > 0.0 ? 1.0 : 0.0;
}

// ---- scalings: fixed-order column statistics ----------------------------------------------------------------------------
// part[chunk][0 .. 4][j] = min, max, non-finite entries, sum of (v - cen_j), sum of (v - cen_j)^2 of column j over the rows of
// the chunk (cen == NULL: 0); 256 threads = 2 row lanes x 128 columns
__global__ __launch_bounds__(256) void k_mlp_stats_partial(const double* __restrict__ A, long long lda, int n, long long M,
                                                           long long rows_per_chunk, const double* __restrict__ cen,
                                                           double* __restrict__ part) {
  __shared__ double sh[5 * 128];
  const int t = threadIdx.x, j = t & 127, ry = t >> 7;
  const long long r_begin = (long long)blockIdx.x * rows_per_chunk;
  const long long r_end = min(M, r_begin + rows_per_chunk);
  double mn = ML_DBL_MAX, mx = -ML_DBL_MAX, bad = 0.0, s1 = 0.0, s2 = 0.0;
  if (j < n) {
    const double ce = cen ? cen[j] : 0.0;
    for (long long r = r_begin + ry; r < r_end; r += 2) {
      const double v = A[r * lda + j];
      if (fabs(v) <= ML_DBL_MAX) {
        mn = fmin(mn, v);
        mx = fmax(mx, v);
        const double dv = v - ce;
        s1 += dv;
        s2 += dv * dv;
      } else {
        bad += 1.0;
      }
    }
  }
  if (ry == 1) {
    sh[j] = mn;
    sh[128 + j] = mx;
    sh[256 + j] = bad;
    sh[384 + j] = s1;
    sh[512 + j] = s2;
  }
  __syncthreads();
  if (ry == 0) {
    double* p = part + size_t(blockIdx.x) * 640;
    p[j] = fmin(mn, sh[j]);
    p[128 + j] = fmax(mx, sh[128 + j]);
    p[256 + j] = bad + sh[256 + j];
    p[384 + j] = s1 + sh[384 + j];
    p[512 + j] = s2 + sh[512 + j];
  }
}

// mode 0 (inputs): c, h and the bad count of X.  mode 1 (targets, first pass): y_mean = the column mean (the value itself for a
// constant column; 0 without scale_targets), y_scale = 1, the bad count of Y.  mode 2 (second pass, centred on y_mean):
// y_scale = sqrt(sum (y - mean)^2 / M), 1 for a constant column.
__global__ __launch_bounds__(128) void k_mlp_stats_finish(const double* __restrict__ part, int chunks, int n, long long M, int mode,
                                                          int scale_targets, double* __restrict__ sc) {
  __shared__ double sbad[128];
  const int j = threadIdx.x;
  double mn = ML_DBL_MAX, mx = -ML_DBL_MAX, bad = 0.0, s1 = 0.0, s2 = 0.0;
  for (int ch = 0; ch < chunks; ++ch) {
    const double* p = part + size_t(ch) * 640;
    mn = fmin(mn, p[j]);
    mx = fmax(mx, p[128 + j]);
    bad += p[256 + j];
    s1 += p[384 + j];
    s2 += p[512 + j];
  }
  const bool some = j < n && mn <= mx;
  if (mode == 0) {
    if (j < ML_MAXIN) {
      sc[ML_SC_C + j] = some ? 0.5 * mn + 0.5 * mx : 0.0;
      sc[ML_SC_H + j] = some ? 0.5 * mx - 0.5 * mn : 0.0;
    }
  } else if (mode == 1) {
    sc[ML_SC_MEAN + j] = (some && scale_targets) ? (mn == mx ? mn : s1 / double(M)) : 0.0;
    sc[ML_SC_SCALE + j] = 1.0;
  } else {
    sc[ML_SC_SCALE + j] = (some && mn < mx) ? sqrt(s2 / double(M)) : 1.0;
  }
  sbad[j] = j < n ? bad : 0.0;
  __syncthreads();
  if (j == 0 && mode <= 1) {
    double b = 0.0;
    for (int c = 0; c < 128; ++c) b += sbad[c];   // (counts: exact in any order)
    sc[ML_SC_BAD + mode] = b;
  }
}

// ---- the slab kernels ---------------------------------------------------------------------------------------------------
// element e of a 32 x n slab block as row << 8 | column, -1 beyond it
__device__ inline int ml_rowcol(int e, int n) {
  const int r = e / n;
  return e < SLAB_ROWS * n ? (r << 8) | (e - r * n) : -1;
}

// W_l and b_l of the flat parameter vector into their padded LDS tables; the slab zeroed
__device__ inline void ml_stage_weights(const MlpDesc& D, const double* __restrict__ W, double* Ws, double* Bs, double* S, int slab_doubles) {
  const int t = threadIdx.x;
  for (int l = 0; l < D.nl; ++l) {
    const int ld = D.ldw[l], rows = D.np[l + 1], N = D.n[l + 1], K = D.n[l];
    double* dst = Ws + D.wl[l];
    for (int e = t; e < rows * ld; e += SLAB_THREADS) {
      const int j = e / ld, c = e - j * ld;
      dst[e] = (j < N && c < K) ? W[D.woff[l] + j * K + c] : 0.0;
    }
    for (int j = t; j < rows; j += SLAB_THREADS) Bs[D.bo[l] + j] = j < N ? W[D.boff[l] + j] : 0.0;
  }
  for (int e = t; e < slab_doubles; e += SLAB_THREADS) S[e] = 0.0;
}

// hidden layers of one slab: A_{l+1} = act(A_l W_l^T + b_l), l = 0 .. nl - 2, a barrier after each.  Padded columns are zero.
__device__ inline void ml_forward_hidden(const MlpDesc& D, double* S, int LY, const double* Ws, const double* Bs) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, i = lane & 15, k = lane >> 4;
  const int rt = w & 1, ct0 = w >> 1;
  for (int l = 0; l + 1 < D.nl; ++l) {
    const int nct = D.np[l + 1] >> 4;
    d4_t y[2];
    slab_nt(S + D.offA[l], LY, Ws + D.wl[l], D.ldw[l], D.np[l], nct, y);
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int ct = ct0 + 4 * jj;
      if (ct < nct) {
        const int col = ct * 16 + i;
        const bool valid = col < D.n[l + 1];
        const double b = Bs[D.bo[l] + col];
        double* out = S + (rt * 16 + k) * LY + D.offA[l + 1] + col;
#pragma unroll
        for (int g = 0; g < 4; ++g) out[4 * g * LY] = valid ? ml_act(D.act, y[jj][g] + b) : 0.0;
      }
    }
    __syncthreads();
  }
}

// Workgroup b owns slabs_per_chunk slabs.  Part[b] (D.pstride doubles): the padded tiles of sum_rows Delta_{l+1}^T A_l per
// layer, the bias sums, the sum of squared residuals.  status != NULL and *status != 0: nothing to do.
__global__ __launch_bounds__(SLAB_THREADS) void k_mlp_eval(MlpDesc D, const double* __restrict__ X, long long ldx,
                                                          const double* __restrict__ Y, long long ldy, long long M,
                                                          long long slabs_per_chunk, const double* __restrict__ sc_g,
                                                          const double* __restrict__ W, double* __restrict__ Part,
                                                          const int* __restrict__ status) {
  extern __shared__ double ml_lds[];
  __shared__ double sc[ML_SC_BAD];
  __shared__ double wred[8];
  if (status && *status != 0) return;
  const int LY = D.LY, nl = D.nl, m = D.n[0], q = D.n[nl];
  double* Ws = ml_lds;
  double* Bs = Ws + D.wtot;
  double* S = Bs + D.btot;   // 32 x LY
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, i = lane & 15, k = lane >> 4;
  const int rt = w & 1, ct0 = w >> 1;

  for (int e = t; e < ML_SC_BAD; e += SLAB_THREADS) sc[e] = sc_g[e];
  ml_stage_weights(D, W, Ws, Bs, S, SLAB_ROWS * LY);

  // this thread's inputs and targets of a slab: e = t + 512 u of the 32 x m and the 32 x q values
  int xrc[ML_XREG], yrc[ML_YREG];   // row << 8 | column, -1: none
#pragma unroll
  for (int u = 0; u < ML_XREG; ++u) xrc[u] = ml_rowcol(t + SLAB_THREADS * u, m);
#pragma unroll
  for (int u = 0; u < ML_YREG; ++u) yrc[u] = ml_rowcol(t + SLAB_THREADS * u, q);
  long long slab0, slab1;
  slab_chunk_range(M, slabs_per_chunk, &slab0, &slab1);
  double xr[ML_XREG], yr[ML_YREG];
  auto load_slab = [&](long long s) {
    const long long row0 = s * SLAB_ROWS;
#pragma unroll
    for (int u = 0; u < ML_XREG; ++u) xr[u] = (xrc[u] >= 0 && row0 + (xrc[u] >> 8) < M) ? X[(row0 + (xrc[u] >> 8)) * ldx + (xrc[u] & 255)] : 0.0;
#pragma unroll
    for (int u = 0; u < ML_YREG; ++u) yr[u] = (yrc[u] >= 0 && row0 + (yrc[u] >> 8) < M) ? Y[(row0 + (yrc[u] >> 8)) * ldy + (yrc[u] & 255)] : 0.0;
  };

  // weight-gradient tiles of this wave: w + 8 u of the list of all layers' tiles; (ca, cb) slab columns of Delta_{l+1} and A_l,
  // tpo the tile's place in the partial (stride tld)
  const int wu = __builtin_amdgcn_readfirstlane(w);   // (the tile list is wave-uniform: scalar registers)
  int tca[ML_TILES], tcb[ML_TILES], tpo[ML_TILES], tld[ML_TILES];
  d4_t acc[ML_TILES];
#pragma unroll
  for (int u = 0; u < ML_TILES; ++u) {
    int tt = wu + 8 * u;
    tca[u] = -1;
    tcb[u] = tpo[u] = tld[u] = 0;
    for (int l = 0; l < nl; ++l) {
      const int tn = D.np[l + 1] >> 4, tk = D.np[l] >> 4;
      if (tt >= 0 && tt < tn * tk) {
        const int ti = tt / tk, tj = tt - ti * tk;
        tca[u] = D.offD[l + 1] + ti * 16;
        tcb[u] = D.offA[l] + tj * 16;
        tpo[u] = D.pw[l] + ti * 16 * D.np[l] + tj * 16;
        tld[u] = D.np[l];
        tt = -1;
      } else if (tt >= 0) {
        tt -= tn * tk;
      }
    }
    acc[u] = d4_t{0.0, 0.0, 0.0, 0.0};
  }
  // bias sum of this thread: slab column of Delta_{l+1}[:, j], its place in the partial
  int bcol = -1, bpo = 0;
  if (t < D.btot)
    for (int l = 0; l < nl; ++l)
      if (t >= D.bo[l] && t < D.bo[l] + D.np[l + 1]) {
        bcol = D.offD[l + 1] + t - D.bo[l];
        bpo = D.pb[l] + t - D.bo[l];
      }
  double bsum = 0.0, lsum = 0.0;

  if (slab0 < slab1) load_slab(slab0);
  __syncthreads();
  for (long long s = slab0; s < slab1; ++s) {
    const long long rows_valid = M - s * SLAB_ROWS;
    // the scaled inputs into A_0, the scaled targets into the place of Delta_nl (rows at and beyond M: zeros)
#pragma unroll
    for (int u = 0; u < ML_XREG; ++u)
      if (xrc[u] >= 0) {
        const int r = xrc[u] >> 8, j = xrc[u] & 255;
        const double h = sc[ML_SC_H + j];
        S[r * LY + j] = (r < rows_valid && h > 0.0) ? (xr[u] - sc[ML_SC_C + j]) / h : 0.0;
      }
#pragma unroll
    for (int u = 0; u < ML_YREG; ++u)
      if (yrc[u] >= 0) {
        const int r = yrc[u] >> 8, j = yrc[u] & 255;
        S[r * LY + D.offD[nl] + j] = r < rows_valid ? (yr[u] - sc[ML_SC_MEAN + j]) / sc[ML_SC_SCALE + j] : 0.0;
      }
    if (s + 1 < slab1) load_slab(s + 1);
    __syncthreads();
    ml_forward_hidden(D, S, LY, Ws, Bs);
    {
      // the output layer: residual r = net - y_scaled = Delta_nl (M and 1 / M enter in k_mlp_reduce)
      const int l = nl - 1, nct = D.np[nl] >> 4;
      d4_t y[2];
      slab_nt(S + D.offA[l], LY, Ws + D.wl[l], D.ldw[l], D.np[l], nct, y);
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const int ct = ct0 + 4 * jj;
        if (ct < nct) {
          const int col = ct * 16 + i;
          const double b = Bs[D.bo[l] + col];
          double* io = S + (rt * 16 + k) * LY + D.offD[nl] + col;
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const bool valid = col < q && rt * 16 + k + 4 * g < rows_valid;
            const double r = valid ? (y[jj][g] + b) - io[4 * g * LY] : 0.0;
            io[4 * g * LY] = r;
            lsum += r * r;
          }
        }
      }
      __syncthreads();
    }
    // backward: Delta_l = (Delta_{l+1} W_l) .* act'(A_l), l = nl - 1 .. 1
    for (int l = nl - 1; l >= 1; --l) {
      const int nct = D.np[l] >> 4;
      d4_t y[2];
      slab_nn(S + D.offD[l + 1], LY, Ws + D.wl[l], D.ldw[l], D.np[l + 1], nct, y);
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const int ct = ct0 + 4 * jj;
        if (ct < nct) {
          const int col = ct * 16 + i;
          const double* a = S + (rt * 16 + k) * LY + D.offA[l] + col;
          double* out = S + (rt * 16 + k) * LY + D.offD[l] + col;
#pragma unroll
          for (int g = 0; g < 4; ++g) out[4 * g * LY] = y[jj][g] * ml_dact(D.act, a[4 * g * LY]);
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < ML_TILES; ++u)
      if (tca[u] >= 0) slab_tn_acc(S, LY, tca[u], tcb[u], acc[u]);   // acc += Delta_{l+1}^T A_l
    if (bcol >= 0)
      for (int r = 0; r < SLAB_ROWS; ++r) bsum += S[r * LY + bcol];
    __syncthreads();   // (the next slab overwrites A_0 and the targets)
  }

  double* Pb = Part + size_t(blockIdx.x) * D.pstride;
#pragma unroll
  for (int u = 0; u < ML_TILES; ++u)
    if (tca[u] >= 0) {
#pragma unroll
      for (int g = 0; g < 4; ++g) Pb[tpo[u] + (k + 4 * g) * tld[u] + i] = acc[u][g];
    }
  if (bcol >= 0) Pb[bpo] = bsum;
  // the chunk's sum of squared residuals: lanes, then waves, in a fixed order
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) lsum += __shfl_xor(lsum, o, 64);
  if (lane == 0) wred[w] = lsum;
  __syncthreads();
  if (t == 0) {
    double v = 0.0;
    for (int c = 0; c < 8; ++c) v += wred[c];
    Pb[D.ploss] = v;
  }
}

// out[0] = loss, out[1 + p] = gradient entry p.  Blocks 0 .. gridDim.x - 2: the entries, partials added in chunk order, + alpha
// W for a weight, / M.  The last block: the loss, 1/(2M) (sum of the chunks' squared residuals + alpha |W|^2), |W|^2 by a fixed
// tree.
__global__ __launch_bounds__(256) void k_mlp_reduce(const double* __restrict__ Part, int chunks, int pstride, int ploss,
                                                    const int* __restrict__ pmap, int P, int nW, const double* __restrict__ W,
                                                    double alpha, double Md, double* __restrict__ out, const int* __restrict__ status) {
  __shared__ double red[256];
  if (status && *status != 0) return;
  const int t = threadIdx.x;
  if (blockIdx.x + 1 < gridDim.x) {
    const int p = blockIdx.x * 256 + t;
    if (p >= P) return;
    const int at = pmap[p];
    double s = 0.0;
    for (int ch = 0; ch < chunks; ++ch) s += Part[size_t(ch) * pstride + at];
    if (p < nW) s += alpha * W[p];
    out[1 + p] = s / Md;
    return;
  }
  double ww = 0.0;
  for (int p = t; p < nW; p += 256) ww += W[p] * W[p];
  red[t] = ww;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) red[t] += red[t + h];
    __syncthreads();
  }
  if (t == 0) {
    double rr = 0.0;
    for (int ch = 0; ch < chunks; ++ch) rr += Part[size_t(ch) * pstride + ploss];
    out[0] = (0.5 * rr + 0.5 * alpha * red[0]) / Md;
  }
}

// grid (row chunks).  The forward pass of a slab; OUT <- y_mean + y_scale net, or Yref - that.  SS[chunk][c] (with SS != NULL) =
// the chunk's sum of squares of what OUT receives in column c, in the order of k_poly_predict.
__global__ __launch_bounds__(SLAB_THREADS) void k_mlp_predict(MlpDesc D, const double* __restrict__ X, long long ldx, long long M,
                                                             long long slabs_per_chunk, const double* __restrict__ sc_g,
                                                             const double* __restrict__ W, double* __restrict__ OUT, long long ldo,
                                                             const double* __restrict__ Yref, long long ldr, double* __restrict__ SS) {
  extern __shared__ double ml_lds[];
  __shared__ double sc[ML_SC_BAD];
  __shared__ double red[2 * ML_MAXQ];
  const int LY = D.LYp, nl = D.nl, m = D.n[0], q = D.n[nl];
  double* Ws = ml_lds;
  double* Bs = Ws + D.wtot;
  double* S = Bs + D.btot;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, i = lane & 15, k = lane >> 4;
  const int rt = w & 1, ct0 = w >> 1;
  for (int e = t; e < ML_SC_BAD; e += SLAB_THREADS) sc[e] = sc_g[e];
  ml_stage_weights(D, W, Ws, Bs, S, SLAB_ROWS * LY);
  int xrc[ML_XREG];
#pragma unroll
  for (int u = 0; u < ML_XREG; ++u) xrc[u] = ml_rowcol(t + SLAB_THREADS * u, m);
  long long slab0, slab1;
  slab_chunk_range(M, slabs_per_chunk, &slab0, &slab1);
  double xr[ML_XREG];
  auto load_slab = [&](long long s) {
    const long long row0 = s * SLAB_ROWS;
#pragma unroll
    for (int u = 0; u < ML_XREG; ++u) xr[u] = (xrc[u] >= 0 && row0 + (xrc[u] >> 8) < M) ? X[(row0 + (xrc[u] >> 8)) * ldx + (xrc[u] & 255)] : 0.0;
  };
  double ss[2] = {0.0, 0.0};
  if (slab0 < slab1) load_slab(slab0);
  __syncthreads();
  for (long long s = slab0; s < slab1; ++s) {
    const long long rows_valid = M - s * SLAB_ROWS;
#pragma unroll
    for (int u = 0; u < ML_XREG; ++u)
      if (xrc[u] >= 0) {
        const int r = xrc[u] >> 8, j = xrc[u] & 255;
        const double h = sc[ML_SC_H + j];
        S[r * LY + j] = (r < rows_valid && h > 0.0) ? (xr[u] - sc[ML_SC_C + j]) / h : 0.0;
      }
    if (s + 1 < slab1) load_slab(s + 1);
    __syncthreads();
    ml_forward_hidden(D, S, LY, Ws, Bs);
    const int l = nl - 1, nct = D.np[nl] >> 4;
    d4_t y[2];
    slab_nt(S + D.offA[l], LY, Ws + D.wl[l], D.ldw[l], D.np[l], nct, y);
    const long long grow0 = s * SLAB_ROWS + rt * 16 + k;
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int col = (ct0 + 4 * jj) * 16 + i;
      if (col < q) {
        const double b = Bs[D.bo[l] + col], mean = sc[ML_SC_MEAN + col], scale = sc[ML_SC_SCALE + col];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const long long row = grow0 + 4 * g;
          if (row < M) {
            const double pred = mean + scale * (y[jj][g] + b);
            const double v = Yref ? Yref[row * ldr + col] - pred : pred;
            if (OUT) OUT[row * ldo + col] = v;
            ss[jj] += v * v;
          }
        }
      }
    }
    __syncthreads();   // (the next slab overwrites A_0, which a slower wave may still read when nl == 1 ... and A_{nl-1})
  }
  if (!SS) return;
#pragma unroll
  for (int jj = 0; jj < 2; ++jj) {
    ss[jj] += __shfl_xor(ss[jj], 16, 64);
    ss[jj] += __shfl_xor(ss[jj], 32, 64);
    const int col = (ct0 + 4 * jj) * 16 + i;
    if (k == 0) red[rt * ML_MAXQ + col] = ss[jj];
  }
  __syncthreads();
  if (t < q) SS[size_t(blockIdx.x) * q + t] = red[t] + red[ML_MAXQ + t];
}

// ---- the optimiser's director -------------------------------------------------------------------------------------------
// sum over p < P of term(p): per thread over p = t, t + 1024, .., then a fixed tree; every thread receives the value
template <class F>
__device__ inline double dir_sum(int P, double* red, F term) {
  const int t = threadIdx.x;
  double s = 0.0;
  for (int p = t; p < P; p += ML_DIR_THREADS) s += term(p);
  red[t] = s;
  __syncthreads();
  for (int h = ML_DIR_THREADS / 2; h > 0; h >>= 1) {
    if (t < h) red[t] += red[t + h];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// One step of the state machine after an evaluation ev = [loss, gradient] at the trial weights wt (nonlinear.mlp_fit_host is
// the specification).  phase 0: the evaluation of w0.  phase 1: a line-search trial.  Leaves the next trial weights in wt, or
// the stop reason + 1 in the status word; w, g, f then belong to the last accepted point.
__global__ __launch_bounds__(ML_DIR_THREADS) void k_mlp_director(int P, int mem, int max_iter, double tol, const double* __restrict__ ev,
                                                                 double* __restrict__ w, double* __restrict__ wt, double* __restrict__ g,
                                                                 double* __restrict__ d, double* __restrict__ Sm, double* __restrict__ Ym,
                                                                 double* __restrict__ rho, double* __restrict__ hist,
                                                                 double* __restrict__ ds, int* __restrict__ is) {
  __shared__ double red[ML_DIR_THREADS];
  __shared__ double al[ML_MEMMAX];
  const int t = threadIdx.x;
  if (is[IS_STATUS] != 0) return;
  const int phase = is[IS_PHASE];
  int k = is[IS_K], evals = is[IS_EVALS], trial = is[IS_TRIAL], npairs = is[IS_NPAIRS], head = is[IS_HEAD], stag = is[IS_STAG];
  double f = ds[DS_F], gd = ds[DS_GD], tt = ds[DS_T], gamma = ds[DS_GAMMA], ginf = ds[DS_GINF];
  const double ft = ev[0];
  const double* gt = ev + 1;
  __syncthreads();   // (every thread has read the state before anyone writes it)
  int status = 0;
  bool newdir = false;
  evals += 1;
  if (phase == 0) {
    for (int p = t; p < P; p += ML_DIR_THREADS) {
      w[p] = wt[p];
      g[p] = gt[p];
    }
    f = ft;
    if (t == 0) hist[0] = f;
    newdir = true;
  } else if (ft <= f + ML_C1 * tt * gd) {
    // accepted: the pair s = wt - w, y = gt - g is kept when s.y > 1e-10 |s| |y|
    const double sy = dir_sum(P, red, [&](int p) { return (wt[p] - w[p]) * (gt[p] - g[p]); });
    const double ss = dir_sum(P, red, [&](int p) { return (wt[p] - w[p]) * (wt[p] - w[p]); });
    const double yy = dir_sum(P, red, [&](int p) { return (gt[p] - g[p]) * (gt[p] - g[p]); });
    if (mem > 0 && sy > ML_CURV * sqrt(ss) * sqrt(yy)) {
      int slot;
      if (npairs < mem) {
        slot = (head + npairs) % mem;
        npairs += 1;
      } else {
        slot = head;
        head = (head + 1) % mem;
      }
      for (int p = t; p < P; p += ML_DIR_THREADS) {
        Sm[size_t(slot) * P + p] = wt[p] - w[p];
        Ym[size_t(slot) * P + p] = gt[p] - g[p];
      }
      if (t == 0) rho[slot] = 1.0 / sy;
      gamma = sy / yy;
    }
    for (int p = t; p < P; p += ML_DIR_THREADS) {
      w[p] = wt[p];
      g[p] = gt[p];
    }
    const double fold = f;
    f = ft;
    k += 1;
    if (t == 0) hist[k] = f;
    stag = (fold - f <= tol * 1e-2 * fmax(fabs(fold), fabs(f))) ? stag + 1 : 0;
    newdir = true;
  } else {
    trial += 1;
    if (trial >= ML_TRIALS) {
      status = 4;   // the line search is exhausted
    } else {
      tt *= 0.5;
      for (int p = t; p < P; p += ML_DIR_THREADS) wt[p] = w[p] + tt * d[p];
    }
  }
  __syncthreads();   // (rho, Sm, Ym, g of this call are visible to the whole workgroup)
  if (newdir) {
    // |g|_inf by the same tree (max is exact in any order)
    double mxv = 0.0;
    for (int p = t; p < P; p += ML_DIR_THREADS) mxv = fmax(mxv, fabs(g[p]));
    red[t] = mxv;
    __syncthreads();
    for (int h = ML_DIR_THREADS / 2; h > 0; h >>= 1) {
      if (t < h) red[t] = fmax(red[t], red[t + h]);
      __syncthreads();
    }
    ginf = red[0];
    __syncthreads();
    if (ginf <= tol) {
      status = 1;
    } else if (stag >= 2) {
      status = 2;
    } else if (k >= max_iter) {
      status = 3;
    } else {
      // two-loop recursion on q = g (in d), newest pair first
      for (int p = t; p < P; p += ML_DIR_THREADS) d[p] = g[p];
      for (int c = npairs - 1; c >= 0; --c) {
        const int slot = (head + c) % mem;
        const double* sv = Sm + size_t(slot) * P;
        const double* yv = Ym + size_t(slot) * P;
        const double a = rho[slot] * dir_sum(P, red, [&](int p) { return sv[p] * d[p]; });
        if (t == 0) al[c] = a;
        for (int p = t; p < P; p += ML_DIR_THREADS) d[p] -= a * yv[p];
      }
      __syncthreads();
      if (npairs > 0)
        for (int p = t; p < P; p += ML_DIR_THREADS) d[p] *= gamma;
      for (int c = 0; c < npairs; ++c) {
        const int slot = (head + c) % mem;
        const double* sv = Sm + size_t(slot) * P;
        const double* yv = Ym + size_t(slot) * P;
        const double b = rho[slot] * dir_sum(P, red, [&](int p) { return yv[p] * d[p]; });
        const double a = al[c];
        for (int p = t; p < P; p += ML_DIR_THREADS) d[p] += (a - b) * sv[p];
      }
      for (int p = t; p < P; p += ML_DIR_THREADS) d[p] = -d[p];
      gd = dir_sum(P, red, [&](int p) { return g[p] * d[p]; });
      const double gg = dir_sum(P, red, [&](int p) { return g[p] * g[p]; });
      if (!(gd < 0.0)) {   // not a descent direction: steepest descent, the memory cleared
        for (int p = t; p < P; p += ML_DIR_THREADS) d[p] = -g[p];
        gd = -gg;
        npairs = 0;
        head = 0;
      }
      tt = k == 0 ? fmin(1.0, 1.0 / sqrt(gg)) : 1.0;
      for (int p = t; p < P; p += ML_DIR_THREADS) wt[p] = w[p] + tt * d[p];
      trial = 0;
    }
  }
  if (t == 0) {
    ds[DS_F] = f;
    ds[DS_GD] = gd;
    ds[DS_T] = tt;
    ds[DS_GINF] = ginf;
    ds[DS_GAMMA] = gamma;
    is[IS_PHASE] = 1;
    is[IS_K] = k;
    is[IS_EVALS] = evals;
    is[IS_TRIAL] = trial;
    is[IS_NPAIRS] = npairs;
    is[IS_HEAD] = head;
    is[IS_STAG] = stag;
    is[IS_STATUS] = status;
  }
}

}  // namespace

struct rom_mlp {
  rom_ctx* ctx = nullptr;
  MlpDesc D;
  size_t lds_eval = 0, lds_predict = 0;
  int64_t M_train = 0;
  int iterations = 0;
  unsigned long long syncs = 0, launches = 0;
  rom_buf* dev = nullptr;    // scalings (ML_SC_SIZE) | w (P)
  rom_buf* pmap = nullptr;   // place of every parameter in a workgroup's partial (P ints)
  std::vector<double> hist;  // loss after every accepted iteration
};

extern "C" int rom_mlp_layout(int m, int n_hidden, const int* hidden, int q, int64_t* out8, int64_t* offsets) {
  MlpDesc D;
  size_t le = 0, lp = 0;
  const char* why = "";
  ROM_CHECK(mlp_plan(m, n_hidden, hidden, q, &D, &le, &lp, &why), "rom_mlp_layout: m = %d, %d hidden layers, q = %d: %s", m, n_hidden, q, why);
  if (out8) {
    out8[0] = D.P;
    out8[1] = D.wpad;
    out8[2] = int64_t(le) + ML_STATIC_LDS;
    out8[3] = int64_t(lp) + ML_STATIC_LDS;
    out8[4] = D.nl;
    out8[5] = D.pstride;
    out8[6] = D.nW;
    out8[7] = 0;
  }
  if (offsets)
    for (int l = 0; l < D.nl; ++l) {
      offsets[l] = D.woff[l];
      offsets[D.nl + l] = D.boff[l];
    }
  return ROM_OK;
}

extern "C" int rom_mlp_destroy(rom_mlp* h) {
  if (!h) return ROM_OK;
  if (h->dev) rom_buf_free(h->dev);
  if (h->pmap) rom_buf_free(h->pmap);
  delete h;
  return ROM_OK;
}

namespace {

// the three launches of one evaluation at the weights W: out = [loss, gradient]
int mlp_enqueue_eval(rom_mlp* h, const double* x, int64_t ldx, const double* y, int64_t ldy, int64_t M, double alpha, const double* W,
                     double* Part, double* out, const int* status) {
  rom_ctx* ctx = h->ctx;
  const MlpDesc& D = h->D;
  const SlabPlan plan = rom_slab_plan(ctx, M, 16);
  if (h->lds_eval > 64 * 1024)
    ROM_TRY(rom_lds_optin(ctx->lds_optin_mlp_eval, reinterpret_cast<const void*>(k_mlp_eval), ML_LDS_MAX - ML_STATIC_LDS));
  {
    ROM_PROF(ctx, "mlp_eval", 6.0 * double(M) * D.wpad, 8.0 * double(M) * (D.n[0] + D.n[D.nl]));
    k_mlp_eval<<<plan.chunks, SLAB_THREADS, h->lds_eval, ctx->stream>>>(D, x, ldx, y, ldy, M, plan.per_chunk, h->dev->p, W, Part, status);
  }
  ROM_HIP(hipGetLastError());
  {
    ROM_PROF(ctx, "mlp_reduce", double(plan.chunks) * D.P, 8.0 * double(plan.chunks) * D.pstride);
    k_mlp_reduce<<<blocks_for(D.P) + 1, 256, 0, ctx->stream>>>(Part, plan.chunks, D.pstride, D.ploss, reinterpret_cast<const int*>(h->pmap->p),
                                                              D.P, D.nW, W, alpha, double(M), out, status);
  }
  ROM_HIP(hipGetLastError());
  h->launches += 2;
  return ROM_OK;
}

}  // namespace

extern "C" int rom_mlp_fit(rom_ctx* ctx, rom_buf* X, size_t x_off, int64_t ldx, int m, rom_buf* Y, size_t y_off, int64_t ldy, int q,
                           int64_t M, int n_hidden, const int* hidden, int activation, double alpha, int scale_targets,
                           const double* w0_host, int max_iter, double tol, int memory, rom_mlp** out, double* info_host) {
  ROM_CHECK(ctx && X && Y && out && w0_host, "rom_mlp_fit: null argument (context, X, Y, w0 or the handle's address)");
  MlpDesc D;
  size_t le = 0, lp = 0;
  const char* why = "";
  ROM_CHECK(mlp_plan(m, n_hidden, hidden, q, &D, &le, &lp, &why), "rom_mlp_fit: m = %d, %d hidden layers, q = %d: %s", m, n_hidden, q, why);
  ROM_CHECK(activation >= 0 && activation <= 2, "rom_mlp_fit: activation = %d, one of 0 (tanh), 1 (logistic), 2 (relu)", activation);
  ROM_TRY(rom_check_rows("rom_mlp_fit", M));
  ROM_CHECK(alpha >= 0.0 && alpha <= ML_DBL_MAX, "rom_mlp_fit: alpha = %g, a finite number >= 0", alpha);
  ROM_CHECK(max_iter >= 0 && max_iter <= (1 << 20), "rom_mlp_fit: max_iter = %d, between 0 and 2^20", max_iter);
  ROM_CHECK(tol >= 0.0, "rom_mlp_fit: tol = %g, at least 0", tol);
  ROM_CHECK(memory >= 1 && memory <= ML_MEMMAX, "rom_mlp_fit: memory = %d pairs, between 1 and %d", memory, ML_MEMMAX);
  ROM_TRY(rom_check_block("rom_mlp_fit", {"X", "ldx", "m"}, X->n, x_off, ldx, m, M));
  ROM_TRY(rom_check_block("rom_mlp_fit", {"Y", "ldy", "q"}, Y->n, y_off, ldy, q, M));
  D.act = activation;
  const int P = D.P;
  for (int p = 0; p < P; ++p)
    ROM_CHECK(std::fabs(w0_host[p]) <= ML_DBL_MAX, "rom_mlp_fit: the initial weights contain NaN / Inf entries (entry %d)", p);
  ROM_HIP(hipSetDevice(ctx->device));
  const double* x = X->p + x_off;
  const double* y = Y->p + y_off;

  rom_mlp* h = new rom_mlp;
  HandleGuard<rom_mlp, rom_mlp_destroy> guard{h};
  h->ctx = ctx;
  h->D = D;
  h->lds_eval = le;
  h->lds_predict = lp;
  h->M_train = M;
  ROM_TRY(rom_buf_alloc(ctx, ML_SC_SIZE + size_t(P), &h->dev));
  ROM_TRY(rom_buf_alloc(ctx, (size_t(P) * sizeof(int) + sizeof(double) - 1) / sizeof(double), &h->pmap));
  double* sc = h->dev->p;
  double* w = sc + ML_SC_SIZE;
  const unsigned long long helper_syncs0 = ctx->host_syncs;
  int syncs = 0;

  // the place of every parameter in a workgroup's partial
  std::vector<int> pmap(P);
  for (int l = 0; l < D.nl; ++l) {
    for (int j = 0; j < D.n[l + 1]; ++j) {
      for (int c = 0; c < D.n[l]; ++c) pmap[D.woff[l] + j * D.n[l] + c] = D.pw[l] + j * D.np[l] + c;
      pmap[D.boff[l] + j] = D.pb[l] + j;
    }
  }
  ROM_HIP(hipMemcpyAsync(h->pmap->p, pmap.data(), size_t(P) * sizeof(int), hipMemcpyHostToDevice, ctx->stream));

  // scalings
  Tmp st_part;
  {
    const int chunks = int(std::min<int64_t>(1024, (M + 63) / 64));
    const long long per = (M + chunks - 1) / chunks;
    ROM_TRY(st_part.get(ctx, size_t(chunks) * 640));
    ROM_PROF(ctx, "mlp_scalings", 4.0 * M * (m + 2.0 * q), 8.0 * M * (m + 2.0 * q));
    k_mlp_stats_partial<<<chunks, 256, 0, ctx->stream>>>(x, ldx, m, M, per, nullptr, st_part);
    k_mlp_stats_finish<<<1, 128, 0, ctx->stream>>>(st_part, chunks, m, M, 0, scale_targets, sc);
    k_mlp_stats_partial<<<chunks, 256, 0, ctx->stream>>>(y, ldy, q, M, per, nullptr, st_part);
    k_mlp_stats_finish<<<1, 128, 0, ctx->stream>>>(st_part, chunks, q, M, 1, scale_targets, sc);
    h->launches += 4;
    if (scale_targets) {
      k_mlp_stats_partial<<<chunks, 256, 0, ctx->stream>>>(y, ldy, q, M, per, sc + ML_SC_MEAN, st_part);
      k_mlp_stats_finish<<<1, 128, 0, ctx->stream>>>(st_part, chunks, q, M, 2, scale_targets, sc);
      h->launches += 2;
    }
    ROM_HIP(hipGetLastError());
  }
  {
    double bad[2] = {0.0, 0.0};
    ROM_TRY(download(ctx, sc + ML_SC_BAD, bad, 2));
    syncs += 1;
    ROM_CHECK(bad[0] == 0.0, "rom_mlp_fit: the inputs contain %.0f NaN / Inf entries", bad[0]);
    ROM_CHECK(bad[1] == 0.0, "rom_mlp_fit: the targets contain %.0f NaN / Inf entries", bad[1]);
  }

  // optimiser state
  const SlabPlan plan = rom_slab_plan(ctx, M, 16);
  Tmp Part, ev, vec, pairs, state;
  ROM_TRY(Part.get(ctx, size_t(plan.chunks) * D.pstride));
  ROM_TRY(ev.get(ctx, 1 + size_t(P)));
  ROM_TRY(vec.get(ctx, 3 * size_t(P)));                       // wt | g | d
  ROM_TRY(pairs.get(ctx, 2 * size_t(memory) * P + memory));   // S | Y | rho
  ROM_TRY(state.get(ctx, size_t(max_iter) + 1 + DS_COUNT + IS_COUNT));   // loss history | doubles | ints
  double* wt = vec.p();
  double* g = wt + P;
  double* d = g + P;
  double* Sm = pairs.p();
  double* Ym = Sm + size_t(memory) * P;
  double* rho = Ym + size_t(memory) * P;
  double* hist = state.p();
  double* ds = hist + max_iter + 1;
  int* is = reinterpret_cast<int*>(ds + DS_COUNT);
  ROM_HIP(hipMemsetAsync(vec.p(), 0, 3 * size_t(P) * sizeof(double), ctx->stream));
  ROM_HIP(hipMemsetAsync(state.p(), 0, (size_t(max_iter) + 1 + DS_COUNT + IS_COUNT) * sizeof(double), ctx->stream));
  ROM_HIP(hipMemcpyAsync(w, w0_host, size_t(P) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  ROM_HIP(hipMemcpyAsync(wt, w0_host, size_t(P) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));

  // batches of (eval, reduce, director); the status word once per batch.  An iteration takes at most ML_TRIALS evaluations.
  const long long seq_cap = 1 + (long long)ML_TRIALS * max_iter;
  long long seq = 0;
  int status = 0;
  while (status == 0 && seq < seq_cap) {
    const int nb = int(std::min<long long>(ML_BATCH, seq_cap - seq));
    for (int b = 0; b < nb; ++b) {
      ROM_TRY(mlp_enqueue_eval(h, x, ldx, y, ldy, M, alpha, wt, Part, ev, is + IS_STATUS));
      k_mlp_director<<<1, ML_DIR_THREADS, 0, ctx->stream>>>(P, memory, max_iter, tol, ev, w, wt, g, d, Sm, Ym, rho, hist, ds, is);
      ROM_HIP(hipGetLastError());
      h->launches += 1;
    }
    seq += nb;
    ROM_HIP(hipMemcpyAsync(&status, is + IS_STATUS, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ROM_HIP(hipStreamSynchronize(ctx->stream));
    syncs += 1;
  }
  ROM_CHECK(status != 0, "rom_mlp_fit: the optimiser did not stop within %lld evaluations", seq_cap);
  std::vector<double> hs(size_t(max_iter) + 1 + DS_COUNT + IS_COUNT);
  ROM_TRY(download(ctx, state.p(), hs.data(), hs.size()));
  syncs += 1;
  const double* hds = hs.data() + max_iter + 1;
  int his[IS_COUNT];
  std::memcpy(his, hds + DS_COUNT, sizeof his);
  h->iterations = his[IS_K];
  h->hist.assign(hs.begin(), hs.begin() + his[IS_K] + 1);
  ROM_CHECK(std::fabs(hds[DS_F]) <= ML_DBL_MAX, "rom_mlp_fit: the loss at the initial weights is not finite (NaN / Inf in the network's values)");
  h->syncs = (unsigned long long)syncs + (ctx->host_syncs - helper_syncs0);
  if (info_host) {
    info_host[0] = his[IS_K];
    info_host[1] = his[IS_EVALS];
    info_host[2] = hds[DS_F];
    info_host[3] = hds[DS_GINF];
    info_host[4] = status - 1;
    info_host[5] = double(h->launches);
    info_host[6] = double(h->syncs);
    info_host[7] = 6.0 * double(M) * D.wpad * his[IS_EVALS];
  }
  *out = guard.release();
  return ROM_OK;
}

extern "C" int rom_mlp_loss_grad(rom_mlp* h, rom_buf* X, size_t x_off, int64_t ldx, rom_buf* Y, size_t y_off, int64_t ldy, int64_t M,
                                 double alpha, double* loss_host, double* grad_host) {
  ROM_CHECK(h && X && Y && loss_host && grad_host, "rom_mlp_loss_grad: null argument");
  rom_ctx* ctx = h->ctx;
  const MlpDesc& D = h->D;
  ROM_TRY(rom_check_rows("rom_mlp_loss_grad", M));
  ROM_CHECK(alpha >= 0.0 && alpha <= ML_DBL_MAX, "rom_mlp_loss_grad: alpha = %g, a finite number >= 0", alpha);
  ROM_TRY(rom_check_block("rom_mlp_loss_grad", {"X", "ldx", "m"}, X->n, x_off, ldx, D.n[0], M));
  ROM_TRY(rom_check_block("rom_mlp_loss_grad", {"Y", "ldy", "q"}, Y->n, y_off, ldy, D.n[D.nl], M));
  ROM_HIP(hipSetDevice(ctx->device));
  const SlabPlan plan = rom_slab_plan(ctx, M, 16);
  Tmp Part, ev;
  ROM_TRY(Part.get(ctx, size_t(plan.chunks) * D.pstride));
  ROM_TRY(ev.get(ctx, 1 + size_t(D.P)));
  ROM_TRY(mlp_enqueue_eval(h, X->p + x_off, ldx, Y->p + y_off, ldy, M, alpha, h->dev->p + ML_SC_SIZE, Part, ev, nullptr));
  std::vector<double> host(1 + size_t(D.P));
  ROM_TRY(download(ctx, ev, host.data(), host.size()));
  h->syncs += 1;
  *loss_host = host[0];
  std::copy(host.begin() + 1, host.end(), grad_host);
  return ROM_OK;
}

extern "C" int rom_mlp_predict(rom_mlp* h, rom_buf* X, size_t x_off, int64_t ldx, int64_t M, rom_buf* OUT, size_t o_off, int64_t ldo,
                               rom_buf* Yref, size_t r_off, int64_t ldr, double* sumsq_host) {
  ROM_CHECK(h && X, "rom_mlp_predict: null argument (handle or X)");
  ROM_CHECK(OUT || sumsq_host, "rom_mlp_predict: OUT == NULL requires sumsq_host");
  rom_ctx* ctx = h->ctx;
  const MlpDesc& D = h->D;
  const int m = D.n[0], q = D.n[D.nl];
  ROM_TRY(rom_check_predict_blocks("rom_mlp_predict", M, X, x_off, ldx, m, q, OUT, o_off, ldo, Yref, r_off, ldr));
  ROM_HIP(hipSetDevice(ctx->device));
  const SlabPlan plan = rom_slab_plan(ctx, M, 16);
  if (h->lds_predict > 64 * 1024)
    ROM_TRY(rom_lds_optin(ctx->lds_optin_mlp_predict, reinterpret_cast<const void*>(k_mlp_predict), ML_LDS_MAX - ML_STATIC_LDS));
  SumsqTail tail;
  if (sumsq_host) ROM_TRY(tail.get(ctx, plan.chunks, q));
  {
    ROM_PROF(ctx, "mlp_predict", 2.0 * double(M) * D.wpad, 8.0 * double(M) * (m + q * (Yref ? 2.0 : 1.0)));
    k_mlp_predict<<<plan.chunks, SLAB_THREADS, h->lds_predict, ctx->stream>>>(D, X->p + x_off, ldx, M, plan.per_chunk, h->dev->p,
                                                                             h->dev->p + ML_SC_SIZE, OUT ? OUT->p + o_off : nullptr, ldo,
                                                                             Yref ? Yref->p + r_off : nullptr, ldr,
                                                                             tail.partials());
  }
  ROM_HIP(hipGetLastError());
  h->launches += 1;   // (the column sums of the tail are not counted here)
  ROM_TRY(tail.finish(ctx, plan.chunks, q, sumsq_host));
  h->syncs += 1;
  return ROM_OK;
}

extern "C" int rom_mlp_query(rom_mlp* h, int64_t* out8) {
  ROM_CHECK(h && out8, "rom_mlp_query: null argument");
  out8[0] = h->D.n[0];
  out8[1] = h->D.n[h->D.nl];
  out8[2] = h->D.nl - 1;
  out8[3] = h->D.P;
  out8[4] = h->M_train;
  out8[5] = h->iterations;
  out8[6] = int64_t(h->launches);
  out8[7] = int64_t(h->syncs);
  return ROM_OK;
}

extern "C" int rom_mlp_download(rom_mlp* h, int what, double* host, size_t count) {
  ROM_CHECK(h && host, "rom_mlp_download: null argument");
  ROM_CHECK(what >= 0 && what <= 5, "rom_mlp_download: what = %d, one of 0 (w), 1 (c), 2 (h), 3 (y_mean), 4 (y_scale), 5 (loss history)", what);
  const int m = h->D.n[0], q = h->D.n[h->D.nl];
  const size_t need = what == 0 ? size_t(h->D.P) : what <= 2 ? size_t(m) : what <= 4 ? size_t(q) : h->hist.size();
  ROM_CHECK(count == need, "rom_mlp_download: part %d holds %zu doubles, count = %zu", what, need, count);
  if (what == 5) {
    std::copy(h->hist.begin(), h->hist.end(), host);
    return ROM_OK;
  }
  ROM_HIP(hipSetDevice(h->ctx->device));
  const int off[5] = {ML_SC_SIZE, ML_SC_C, ML_SC_H, ML_SC_MEAN, ML_SC_SCALE};
  h->syncs += 1;
  return download(h->ctx, h->dev->p + off[what], host, need);
}
