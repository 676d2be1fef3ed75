// rom_tree_fit / rom_tree_predict: multi-output CART regression trees and bagged forests between columns of a tall device
// block -- the "Tree" and "RF" models of the reference's second experiment (src/experiments/NonLinearROM.py:54-70,136-137:
// DecisionTreeRegressor(), RandomForestRegressor(n_estimators=10) from the leading PCA coordinates to the higher ones).
//
// A forest of T trees is ONE level-wise construction: for every input column f the rows of all trees lie in one array ord[f]
// of R = sum_t (rows of tree t with count > 0) positions, sorted by x_f inside every node; the nodes of all trees are segments
// [start, end) of it, the same segments for every f.  Per level (all open nodes of all trees, one launch each):
//   k_tree_scan<0>  tile sums (a tile = the 64 positions of a wave) of (count, count (y_k - c_k)) after the tile's last head
//   k_tree_scan<1>  column 0 only of ord: n and c1 = c0 + S / n per node, c0 = the parent's mean (0 at a root)
//   k_tree_scan<0>  the same tile sums with the shift c1, every input column
//   k_tree_scan<2>  S about c1, the node's mean c1 + S / n, "some target differs between two rows" per node
//   k_tree_scan<3>  the segmented prefix sums along every input column, the gain of every candidate, its maximum per node
//   k_tree_pick     lowest (input, position) among the candidates that attain the maximum
//   k_tree_decide   leaf or split, the threshold, the children (one workgroup: the children's numbers are a prefix count)
//   k_tree_part<0/1> stable partition of every ord[f] by the go-left flag (a segmented scan of the flag)
// then one read-back: the number of new nodes.  A prefix sum is the wave's segmented scan (six shuffles, always the same tree)
// plus the carry of the tiles between the segment's start and this tile, added in tile order.  The maximum of the gain and
// the minimum of (input, position) go through INTEGER atomics on totally ordered keys: the result does not depend on the order
// of arrival, and no floating-point atomic exists in this file -- the same bits on every call.
#include <cmath>
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>

#include "rom_basis_int.h"
#include "rom_block.h"

namespace {

typedef unsigned long long u64;
constexpr int TR_MMAX = 16, TR_QMAX = 128, TR_TMAX = 256;
constexpr int TR_WAVES = 4;        // tiles (waves) per workgroup of the scan kernels
constexpr int TR_PRED_ROWS = 32;   // rows per group of k_tree_predict
constexpr u64 TR_NOKEY = ~u64(0);

struct TreeDev {
  const double* X;
  long long ldx;
  const double* Y;
  long long ldy;
  long long M;
  const int* counts;   // T x M or NULL
  const int* ord;      // m x R: row of every position, per input column
  const int* nid;      // R: node of every position
  int m, q, R, ntiles, lvl0;
  // per node
  int *start, *end, *parent, *treeid, *depth, *feat, *left, *nlr, *nonconst;
  double *thr, *n, *val;
  u64 *bestgain, *bestkey;
  // per open node of the level (row nd - lvl0), per tile, per position
  double *c1, *stot, *tail;
  u64* G;
};

// Segmented inclusive scan over the 64 lanes of a wave (Hillis-Steele with head flags): bit s of the mask says that this lane
// adds its partner at distance 2^s.  covered: a head lies at or before this lane inside the wave.
__device__ inline unsigned seg_mask(bool head, int lane, bool* covered) {
  unsigned mask = 0;
  int f = head ? 1 : 0;
#pragma unroll
  for (int s = 0; s < 6; ++s) {
    const int d = 1 << s;
    const int tf = __shfl_up(f, d, 64);
    if (lane >= d && !f) {
      mask |= 1u << s;
      f = tf;
    }
  }
  *covered = f != 0;
  return mask;
}
template <typename V>
__device__ inline V seg_scan(V v, unsigned mask) {
#pragma unroll
  for (int s = 0; s < 6; ++s) {
    const V t = __shfl_up(v, 1 << s, 64);
    if ((mask >> s) & 1) v += t;
  }
  return v;
}

// number of NaN / Inf entries of the two blocks (an integer count: exact in any order)
__global__ void k_tree_finite(const double* __restrict__ X, long long ldx, int m, const double* __restrict__ Y, long long ldy, int q,
                              long long M, unsigned* __restrict__ bad) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int mq = m + q;
  if (idx >= M * mq) return;
  const long long row = idx / mq;
  const int c = int(idx - row * mq);
  const double v = c < m ? X[row * ldx + c] : Y[row * ldy + (c - m)];
  if (!(fabs(v) <= 1.7976931348623157e308)) atomicAdd(bad, 1u);
}

__global__ void k_tree_keys(const double* __restrict__ X, long long ldx, int f, long long M, double* __restrict__ keys, int* __restrict__ rows) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  keys[i] = X[i * ldx + f];
  rows[i] = int(i);
}

// ord[f][tree_start[t] + ...] = the rows of sorted[f] that tree t holds (count > 0), in that order.  grid (tiles / 4, m, T).
template <bool FINAL>
__global__ __launch_bounds__(256) void k_tree_compact(const int* __restrict__ sorted, const int* __restrict__ counts, long long M, int mt,
                                                      int m, int* __restrict__ ccnt, const int* __restrict__ tree_start,
                                                      int* __restrict__ ord, int R) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, f = blockIdx.y, t = blockIdx.z;
  const int tile = blockIdx.x * TR_WAVES + w;
  const long long i = (long long)tile * 64 + lane;
  const bool in = tile < mt && i < M;
  const int row = in ? sorted[size_t(f) * M + i] : 0;
  const bool keep = in && (!counts || counts[size_t(t) * M + row] > 0);
  const u64 bal = __ballot(keep);
  int* cc = ccnt + (size_t(t) * m + f) * mt;
  if (!FINAL) {
    if (lane == 0 && tile < mt) cc[tile] = __popcll(bal);
    return;
  }
  int c = 0;
  for (int tt = lane; tt < tile && tt < mt; tt += 64) c += cc[tt];
#pragma unroll
  for (int s = 0; s < 6; ++s) c += __shfl_xor(c, 1 << s, 64);
  if (keep) ord[size_t(f) * R + tree_start[t] + c + __popcll(bal & ((u64(1) << lane) - 1))] = row;
}

// ---- the scans of a level -------------------------------------------------------------------------------------------------
// grid (tiles / 4, input columns).  Columns of the scan: k = 0 the count, k = 1 .. q the count times the shifted target.
// MODE 0: tile sums (shift: c1 with use_c1, else the parent's mean).  MODE 1: n and c1 (shift: the parent's mean).  MODE 2:
// S, mean, constancy (shift c1).  MODE 3: gains (shift c1).
template <int MODE>
__global__ __launch_bounds__(256) void k_tree_scan(TreeDev d, int use_c1, double msl) {
  __shared__ double sc[TR_WAVES][TR_QMAX + 4];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, f = blockIdx.y;
  const int tile = blockIdx.x * TR_WAVES + w;
  const int p = tile * 64 + lane;
  const bool inr = tile < d.ntiles && p < d.R;
  const int nd = inr ? d.nid[p] : -1;
  const bool open = nd >= d.lvl0;
  const int* __restrict__ ord = d.ord + size_t(f) * d.R;
  const int r = open ? ord[p] : 0;
  const int st = open ? d.start[nd] : 0, en = open ? d.end[nd] : 0;
  const bool head = !open || p == st;
  const double wgt = !open ? 0.0 : d.counts ? double(d.counts[size_t(d.treeid[nd]) * d.M + r]) : 1.0;
  bool covered;
  const unsigned mask = seg_mask(head, lane, &covered);
  const int Q1 = d.q + 1;
  const bool any_open = __any(open) != 0;
  const int nd0 = __shfl(nd, 0, 64), st0 = __shfl(st, 0, 64), nd63 = __shfl(nd, 63, 64);
  if (MODE != 0 && any_open) {
    // carry of the segment that reaches into this tile: the tiles from its start to here, in tile order
    const int first = (nd0 >= d.lvl0 && st0 < tile * 64) ? (st0 >> 6) : tile;
    const double* __restrict__ tl = d.tail + size_t(f) * d.ntiles * Q1;
    for (int k = lane; k < Q1; k += 64) {
      double c = 0.0;
      for (int tt = first; tt < tile; ++tt) c += tl[size_t(tt) * Q1 + k];
      sc[w][k] = c;
    }
  }
  __syncthreads();
  if (!any_open) return;

  const int qi = open ? nd - d.lvl0 : 0;
  const int par = open ? d.parent[nd] : -1;
  const bool c1mode = MODE >= 2 || (MODE == 0 && use_c1);
  const bool last = open && p == en - 1;
  int rprev = __shfl_up(r, 1, 64);
  if (MODE == 2 && open && !head && lane == 0) rprev = ord[p - 1];
  const double ntot = (MODE >= 2 && open) ? d.n[nd] : 0.0;
  double nn = 1.0, nL = 1.0, nR = 1.0, gain = 0.0;
  bool diff = false;
  for (int k = 0; k < Q1; ++k) {
    double c = 0.0, v = wgt;
    if (k > 0) {
      double y = 0.0;
      if (open) {
        c = c1mode ? d.c1[size_t(qi) * d.q + (k - 1)] : (par >= 0 ? d.val[size_t(par) * d.q + (k - 1)] : 0.0);
        y = d.Y[(long long)r * d.ldy + (k - 1)];
        if (MODE == 2 && !head) diff = diff || (y != d.Y[(long long)rprev * d.ldy + (k - 1)]);
      }
      v = wgt * (y - c);
    }
    v = seg_scan(v, mask);
    if (MODE != 0 && !covered) v += sc[w][k];
    if (MODE == 0) {
      if (lane == 63) d.tail[(size_t(f) * d.ntiles + tile) * Q1 + k] = v;
    } else if (MODE == 1) {
      if (last) {
        if (k == 0) {
          nn = v;
          d.n[nd] = v;
        } else {
          d.c1[size_t(qi) * d.q + (k - 1)] = c + v / nn;
        }
      }
    } else if (MODE == 2) {
      if (last && k > 0) {
        d.stot[size_t(qi) * d.q + (k - 1)] = v;
        d.val[size_t(nd) * d.q + (k - 1)] = c + v / ntot;
      }
    } else {
      if (k == 0) {
        nL = v;
        nR = ntot - v;
      } else if (open) {
        const double sr = d.stot[size_t(qi) * d.q + (k - 1)] - v;
        gain += v * v / nL + sr * sr / nR;
      }
    }
  }
  if (MODE == 2 && open && !head && diff) d.nonconst[nd] = 1;   // (every writer writes the same value)
  if (MODE == 3) {
    bool valid = open && p + 1 < en && nL >= msl && nR >= msl;
    if (valid) valid = d.X[(long long)r * d.ldx + f] < d.X[(long long)ord[p + 1] * d.ldx + f];
    if (!(gain >= 0.0)) gain = 0.0;
    // (a gain is >= +0: its bits order as it does; + 1 so that a valid candidate of gain 0 beats "none")
    u64 key = valid ? u64(__double_as_longlong(gain)) + 1 : 0;
    if (inr) d.G[size_t(f) * d.R + p] = key;
    if (nd0 == nd63 && nd0 >= d.lvl0) {   // one node in the whole wave: one atomic
#pragma unroll
      for (int s = 0; s < 6; ++s) {
        const u64 o = __shfl_xor(key, 1 << s, 64);
        key = o > key ? o : key;
      }
      if (lane == 0 && key) atomicMax(&d.bestgain[nd0], key);
    } else if (key) {
      atomicMax(&d.bestgain[nd], key);
    }
  }
}

__global__ void k_tree_pick(TreeDev d) {
  const size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= size_t(d.m) * d.R) return;
  const int f = int(i / d.R), p = int(i - size_t(f) * d.R);
  const int nd = d.nid[p];
  if (nd < d.lvl0) return;
  const u64 key = d.G[i];
  if (key && key == d.bestgain[nd]) atomicMin(&d.bestkey[nd], (u64(f) << 32) | u64(unsigned(p)));
}

// One workgroup over the open nodes [lvl0, lvl1) in chunks of 1024: leaf or split; a splitting node gets its threshold and the
// children lvl1 + 2 (number of splitting nodes before it), + 1.  counter[0] = number of new nodes.
__global__ __launch_bounds__(1024) void k_tree_decide(TreeDev d, int lvl1, int max_depth, double mss, int* __restrict__ counter) {
  __shared__ int wsum[16];
  const int tid = threadIdx.x, wv = tid >> 6, ln = tid & 63;
  int base = 0;
  for (int i0 = d.lvl0; i0 < lvl1; i0 += 1024) {
    const int nd = i0 + tid;
    bool split = false;
    u64 key = 0;
    if (nd < lvl1) {
      key = d.bestkey[nd];
      const bool varies = d.nonconst[nd] != 0;
      split = d.n[nd] >= mss && (max_depth == 0 || d.depth[nd] < max_depth) && d.bestgain[nd] != 0 && varies;
      if (!varies) {   // every row holds the same targets: the value is that row, bit for bit
        const long long r0 = d.ord[d.start[nd]];
        for (int k = 0; k < d.q; ++k) d.val[size_t(nd) * d.q + k] = d.Y[r0 * d.ldy + k];
      }
    }
    const u64 bal = __ballot(split);
    const int inw = __popcll(bal & ((u64(1) << ln) - 1));
    if (ln == 0) wsum[wv] = __popcll(bal);
    __syncthreads();
    int off = 0, tot = 0;
    for (int j = 0; j < 16; ++j) {
      if (j < wv) off += wsum[j];
      tot += wsum[j];
    }
    if (nd < lvl1) {
      if (split) {
        const int f = int(key >> 32), pos = int(key & 0xffffffffu);
        const int* ordf = d.ord + size_t(f) * d.R;
        const double lo = d.X[(long long)ordf[pos] * d.ldx + f], hi = d.X[(long long)ordf[pos + 1] * d.ldx + f];
        double thr = lo + (hi - lo) / 2;
        if (!(thr < hi)) thr = lo;
        const int L = lvl1 + 2 * (base + off + inw);
        const int st = d.start[nd], en = d.end[nd], nl = pos - st + 1;
        d.feat[nd] = f;
        d.thr[nd] = thr;
        d.left[nd] = L;
        d.nlr[nd] = nl;
        for (int c = 0; c < 2; ++c) {
          const int ch = L + c;
          d.start[ch] = c == 0 ? st : st + nl;
          d.end[ch] = c == 0 ? st + nl : en;
          d.parent[ch] = nd;
          d.treeid[ch] = d.treeid[nd];
          d.depth[ch] = d.depth[nd] + 1;
          d.feat[ch] = -1;
          d.left[ch] = -1;
          d.nlr[ch] = 0;
          d.nonconst[ch] = 0;
          d.thr[ch] = 0.0;
          d.n[ch] = 0.0;
          d.bestgain[ch] = 0;
          d.bestkey[ch] = TR_NOKEY;
        }
      } else {
        d.feat[nd] = -1;
        d.left[nd] = -1;
        d.thr[nd] = 0.0;
        d.nlr[nd] = 0;
      }
    }
    base += tot;
    __syncthreads();
  }
  if (tid == 0) counter[0] = 2 * base;
}

// Stable partition of every ord[f] inside the splitting nodes: FINAL = false the tile counts of the go-left flag, FINAL = true
// the scatter into ord_out (positions outside a splitting node keep their place) and, by input column 0, the nodes of the
// positions after the split.
template <bool FINAL>
__global__ __launch_bounds__(256) void k_tree_part(TreeDev d, int* __restrict__ itail, int* __restrict__ ord_out, int* __restrict__ nid_out) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, f = blockIdx.y;
  const int tile = blockIdx.x * TR_WAVES + w;
  const int p = tile * 64 + lane;
  const bool inr = tile < d.ntiles && p < d.R;
  const int nd = inr ? d.nid[p] : -1;
  const int sf = nd >= d.lvl0 ? d.feat[nd] : -1;
  const bool flag = sf >= 0;
  const int r = inr ? d.ord[size_t(f) * d.R + p] : 0;
  const int st = flag ? d.start[nd] : 0;
  const bool head = !flag || p == st;
  const int gl = (flag && d.X[(long long)r * d.ldx + sf] <= d.thr[nd]) ? 1 : 0;
  bool covered;
  const unsigned mask = seg_mask(head, lane, &covered);
  int v = seg_scan(gl, mask);
  if (!FINAL) {
    if (lane == 63 && tile < d.ntiles) itail[size_t(f) * d.ntiles + tile] = v;
    return;
  }
  const int flag0 = __shfl(flag ? 1 : 0, 0, 64), st0 = __shfl(st, 0, 64);
  const int first = (flag0 && st0 < tile * 64) ? (st0 >> 6) : tile;
  int c = 0;
  for (int tt = first + lane; tt < tile; tt += 64) c += itail[size_t(f) * d.ntiles + tt];
#pragma unroll
  for (int s = 0; s < 6; ++s) c += __shfl_xor(c, 1 << s, 64);
  if (!covered) v += c;
  if (!inr) return;
  int np = p;
  if (flag) {
    const int before = v - gl, nl = d.nlr[nd];
    np = gl ? st + before : st + nl + (p - st - before);
  }
  ord_out[size_t(f) * d.R + np] = r;
  if (f == 0) nid_out[p] = flag ? (p < st + d.nlr[nd] ? d.left[nd] : d.left[nd] + 1) : nd;
}

// ---- prediction -------------------------------------------------------------------------------------------------------------
// Workgroup b owns groups_per_chunk groups of 32 rows; thread -> (row, column) of a group, the column fastest.  Each walks the
// T trees (the root of tree t is node t) and adds the leaves' values in tree order.  SS[b][k] = the chunk's sum of squares of
// what OUT receives in column k: thread k over the rows of every group, in row order.
__global__ __launch_bounds__(256) void k_tree_predict(const int* __restrict__ feat, const int* __restrict__ left,
                                                      const double* __restrict__ thr, const double* __restrict__ val, int q, int T,
                                                      const double* __restrict__ X, long long ldx, long long M, long long groups,
                                                      long long groups_per_chunk, double* __restrict__ OUT, long long ldo,
                                                      const double* __restrict__ Yref, long long ldr, double* __restrict__ SS) {
  __shared__ double sq[TR_PRED_ROWS * TR_QMAX];
  const int t = threadIdx.x;
  const long long g0 = (long long)blockIdx.x * groups_per_chunk, g1 = min(groups, g0 + groups_per_chunk);
  double acc = 0.0;
  for (long long g = g0; g < g1; ++g) {
    for (int e = t; e < TR_PRED_ROWS * q; e += 256) {
      const int rr = e / q, k = e - rr * q;
      const long long row = g * TR_PRED_ROWS + rr;
      double v2 = 0.0;
      if (row < M) {
        const double* __restrict__ x = X + row * ldx;
        double s = 0.0;
        for (int tr = 0; tr < T; ++tr) {
          int nd = tr, f;
          while ((f = feat[nd]) >= 0) nd = left[nd] + (x[f] <= thr[nd] ? 0 : 1);
          const double lv = val[size_t(nd) * q + k];
          s = tr == 0 ? lv : s + lv;
        }
        double v = s / double(T);
        if (Yref) v = Yref[row * ldr + k] - v;
        if (OUT) OUT[row * ldo + k] = v;
        v2 = v * v;
      }
      sq[e] = v2;
    }
    __syncthreads();
    if (SS && t < q)
      for (int rr = 0; rr < TR_PRED_ROWS; ++rr) acc += sq[rr * q + t];
    __syncthreads();
  }
  if (SS && t < q) SS[size_t(blockIdx.x) * q + t] = acc;
}

// carves arrays out of one block of doubles; without a block it only measures
struct Carver {
  double* base = nullptr;
  size_t at = 0;
  template <typename V>
  V* take(size_t n) {
    const size_t o = at;
    at += (n * sizeof(V) + sizeof(double) - 1) / sizeof(double);
    return base ? reinterpret_cast<V*>(base + o) : nullptr;
  }
};

// the node arrays a fitted forest keeps, N nodes: the layout of rom_tree::dev
struct TreeNodes {
  double *thr, *n, *val;
  int *feat, *left, *tree;
  size_t doubles;
  TreeNodes(double* base, size_t N, int q) {
    Carver c{base};
    thr = c.take<double>(N), n = c.take<double>(N), val = c.take<double>(N * q);
    feat = c.take<int>(N), left = c.take<int>(N), tree = c.take<int>(N);
    doubles = c.at;
  }
};

// the sizes of one fit
struct TreeShape {
  int64_t M;
  int m, q, T;
  bool counts;    // bootstrap counts given
  int R = 0, ntiles = 0, mt = 0;
  size_t nmax = 0;   // a binary tree over n rows has at most 2 n - 1 nodes
  std::vector<int> tree_start;   // T + 1: the positions of tree t are tree_start[t] .. tree_start[t + 1] - 1
};

// The workspace of a fit, one block: the one place that knows its layout.  d holds the node arrays (nmax nodes) and the scratch
// of a level; beside it the two copies of ord and nid that the levels alternate between, and the scratch of the presort.
struct TreeWorkspace {
  Tmp buf;
  size_t doubles = 0, sort_bytes = 0;
  TreeDev d;
  int *ord[2], *nid[2], *itail, *sorted, *rows, *ccnt, *tstart, *counter, *counts;
  double *keys0, *keys1;
  char* sort;
  unsigned* bad() const { return reinterpret_cast<unsigned*>(counter + 1); }   // (counter: 4 ints, the first the level's new nodes)

  void carve(double* base, const TreeShape& s) {
    Carver cv{base};
    const size_t nmax = s.nmax, R = size_t(s.R), m = size_t(s.m), M = size_t(s.M), q = size_t(s.q);
    d.start = cv.take<int>(nmax), d.end = cv.take<int>(nmax), d.parent = cv.take<int>(nmax), d.treeid = cv.take<int>(nmax);
    d.depth = cv.take<int>(nmax), d.feat = cv.take<int>(nmax), d.left = cv.take<int>(nmax), d.nlr = cv.take<int>(nmax);
    d.nonconst = cv.take<int>(nmax), d.thr = cv.take<double>(nmax), d.n = cv.take<double>(nmax);
    d.bestgain = cv.take<u64>(nmax), d.bestkey = cv.take<u64>(nmax), d.val = cv.take<double>(nmax * q);
    d.c1 = cv.take<double>(R * q), d.stot = cv.take<double>(R * q);
    d.tail = cv.take<double>(m * s.ntiles * (q + 1)), d.G = cv.take<u64>(m * R);
    ord[0] = cv.take<int>(m * R), ord[1] = cv.take<int>(m * R), nid[0] = cv.take<int>(R), nid[1] = cv.take<int>(R);
    itail = cv.take<int>(m * s.ntiles), sorted = cv.take<int>(m * M);
    keys0 = cv.take<double>(M), keys1 = cv.take<double>(M), rows = cv.take<int>(M);
    ccnt = cv.take<int>(size_t(s.T) * m * s.mt), tstart = cv.take<int>(s.T + 1), counter = cv.take<int>(4);
    counts = cv.take<int>(s.counts ? size_t(s.T) * M : 0);
    if (!s.counts) counts = nullptr;
    sort = cv.take<char>(sort_bytes);
    doubles = cv.at;
  }

  // the block for the sizes s, and d complete but for the level's ord, nid and lvl0: X and Y are the blocks at their offsets
  int get(rom_ctx* ctx, const TreeShape& s, const double* x, int64_t ldx, const double* y, int64_t ldy) {
    {
      double* kd = nullptr;
      int* vd = nullptr;
      ROM_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, kd, kd, vd, vd, size_t(s.M), 0u, 64u, ctx->stream));
    }
    carve(nullptr, s);
    const size_t ws_bytes = doubles * sizeof(double);
    ROM_CHECK(ws_bytes <= ctx->ws_limit, "rom_tree_fit: %zu bytes of workspace for %d rows in %d trees exceed the limit of %zu", ws_bytes, s.R,
              s.T, ctx->ws_limit);
    ROM_TRY(buf.get(ctx, doubles));
    carve(buf.p(), s);
    d.X = x, d.ldx = ldx, d.Y = y, d.ldy = ldy, d.M = s.M, d.counts = counts;
    d.m = s.m, d.q = s.q, d.R = s.R, d.ntiles = s.ntiles;
    return ROM_OK;
  }
};

}  // namespace

struct rom_tree {
  rom_ctx* ctx = nullptr;
  int m = 0, q = 0, T = 0, levels = 0;
  int64_t M_train = 0, nodes = 0;
  unsigned long long launches = 0, syncs = 0;
  rom_buf* dev = nullptr;   // thr (nodes) | n (nodes) | val (nodes x q) | feat, left, tree (ints)
  const double *thr = nullptr, *n = nullptr, *val = nullptr;
  const int *feat = nullptr, *left = nullptr, *tree = nullptr;
  // host copies in the order of rom_tree_download (filled by its first call)
  bool host_ready = false;
  std::vector<double> h_first, h_feat, h_thr, h_left, h_n, h_val;
};

extern "C" int rom_tree_destroy(rom_tree* h) {
  if (!h) return ROM_OK;
  if (h->dev) rom_buf_free(h->dev);
  delete h;
  return ROM_OK;
}

namespace {

// the rows of every tree: those with a positive count, all M without counts
int tree_rows(const int32_t* counts_host, TreeShape& s) {
  const int T = s.T;
  const int64_t M = s.M;
  s.tree_start.assign(T + 1, 0);
  for (int t = 0; t < T; ++t) {
    long long nt = M;
    if (counts_host) {
      nt = 0;
      for (int64_t i = 0; i < M; ++i) {
        const int32_t c = counts_host[size_t(t) * M + i];
        ROM_CHECK(c >= 0, "rom_tree_fit: counts[%d][%lld] = %d is negative", t, (long long)i, c);
        nt += c > 0 ? 1 : 0;
      }
      ROM_CHECK(nt > 0, "rom_tree_fit: every count of tree %d is 0: a tree without rows", t);
    }
    ROM_CHECK((long long)s.tree_start[t] + nt <= (1ll << 30), "rom_tree_fit: more than 2^30 rows in all trees together");
    s.tree_start[t + 1] = s.tree_start[t] + int(nt);
  }
  s.R = s.tree_start[T];
  s.ntiles = (s.R + 63) / 64;
  s.mt = int((M + 63) / 64);
  s.nmax = 2 * size_t(s.R) - T;
  return ROM_OK;
}

// One fit between its steps: ws.get, check_and_presort, roots, grow, handle.  The steps enqueue on ctx->stream in this order.
struct TreeFit {
  rom_ctx* ctx;
  hipStream_t st;
  const TreeShape& s;
  const int32_t* counts_host;
  TreeWorkspace ws;
  unsigned long long launches = 0, syncs = 0;
  int levels = 0, nodes = 0;
  std::vector<int> h_nid, h_int;   // what roots() uploads: the copies are asynchronous, the arrays stay until the fit ends
  std::vector<u64> h_key;

  TreeFit(rom_ctx* c, const TreeShape& shape, const int32_t* counts) : ctx(c), st(c->stream), s(shape), counts_host(counts) {}

  // NaN / Inf in the inputs or targets; then the presort: every input column once (stable radix sort of (x, row)), then the
  // rows of every tree in that order
  int check_and_presort() {
    const TreeDev& d = ws.d;
    const int64_t M = s.M;
    const int m = s.m, q = s.q, T = s.T;
    ROM_HIP(hipMemsetAsync(ws.counter, 0, 4 * sizeof(int), st));
    {
      ROM_PROF(ctx, "tree_finite", 0.0, 8.0 * M * (m + q));
      k_tree_finite<<<blocks_for(size_t(M) * (m + q)), 256, 0, st>>>(d.X, d.ldx, m, d.Y, d.ldy, q, M, ws.bad());
      ROM_HIP(hipGetLastError());
      ++launches;
    }
    unsigned bad = 0;
    ROM_HIP(hipMemcpyAsync(&bad, ws.bad(), sizeof(unsigned), hipMemcpyDeviceToHost, st));
    ROM_HIP(hipStreamSynchronize(st));
    ++syncs;
    ROM_CHECK(bad == 0, "rom_tree_fit: the inputs or targets contain %u NaN / Inf entries", bad);

    if (counts_host) ROM_HIP(hipMemcpyAsync(ws.counts, counts_host, size_t(T) * M * sizeof(int), hipMemcpyHostToDevice, st));
    ROM_HIP(hipMemcpyAsync(ws.tstart, s.tree_start.data(), (T + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    for (int f = 0; f < m; ++f) {
      ROM_PROF(ctx, "tree_sort", 0.0, 64.0 * M);
      k_tree_keys<<<blocks_for(size_t(M)), 256, 0, st>>>(d.X, d.ldx, f, M, ws.keys0, ws.rows);
      ROM_HIP(hipGetLastError());
      size_t sb = ws.sort_bytes;
      ROM_HIP(rocprim::radix_sort_pairs(reinterpret_cast<void*>(ws.sort), sb, ws.keys0, ws.keys1, ws.rows, ws.sorted + size_t(f) * M, size_t(M), 0u,
                                        64u, st));
      launches += 2;
    }
    {
      ROM_PROF(ctx, "tree_compact", 0.0, 8.0 * T * m * M);
      const dim3 grid(unsigned((s.mt + TR_WAVES - 1) / TR_WAVES), unsigned(m), unsigned(T));
      k_tree_compact<false><<<grid, 256, 0, st>>>(ws.sorted, ws.counts, M, s.mt, m, ws.ccnt, ws.tstart, ws.ord[0], s.R);
      k_tree_compact<true><<<grid, 256, 0, st>>>(ws.sorted, ws.counts, M, s.mt, m, ws.ccnt, ws.tstart, ws.ord[0], s.R);
      ROM_HIP(hipGetLastError());
      launches += 2;
    }
    return ROM_OK;
  }

  // the roots: node t is the root of tree t and owns the tree's positions
  int roots() {
    const TreeDev& d = ws.d;
    const int T = s.T, R = s.R;
    h_nid.resize(R);
    h_int.resize(T);
    h_key.assign(T, TR_NOKEY);
    for (int t = 0; t < T; ++t)
      for (int p = s.tree_start[t]; p < s.tree_start[t + 1]; ++p) h_nid[p] = t;
    ROM_HIP(hipMemcpyAsync(ws.nid[0], h_nid.data(), size_t(R) * sizeof(int), hipMemcpyHostToDevice, st));
    ROM_HIP(hipMemcpyAsync(d.start, s.tree_start.data(), T * sizeof(int), hipMemcpyHostToDevice, st));
    ROM_HIP(hipMemcpyAsync(d.end, s.tree_start.data() + 1, T * sizeof(int), hipMemcpyHostToDevice, st));
    for (int t = 0; t < T; ++t) h_int[t] = t;
    ROM_HIP(hipMemcpyAsync(d.treeid, h_int.data(), T * sizeof(int), hipMemcpyHostToDevice, st));
    ROM_HIP(hipMemsetAsync(d.parent, 0xff, T * sizeof(int), st));   // -1
    ROM_HIP(hipMemsetAsync(d.feat, 0xff, T * sizeof(int), st));
    ROM_HIP(hipMemsetAsync(d.left, 0xff, T * sizeof(int), st));
    ROM_HIP(hipMemsetAsync(d.depth, 0, T * sizeof(int), st));
    ROM_HIP(hipMemsetAsync(d.nlr, 0, T * sizeof(int), st));
    ROM_HIP(hipMemsetAsync(d.nonconst, 0, T * sizeof(int), st));
    ROM_HIP(hipMemsetAsync(d.thr, 0, T * sizeof(double), st));
    ROM_HIP(hipMemsetAsync(d.n, 0, T * sizeof(double), st));
    ROM_HIP(hipMemsetAsync(d.bestgain, 0, T * sizeof(u64), st));
    ROM_HIP(hipMemcpyAsync(d.bestkey, h_key.data(), T * sizeof(u64), hipMemcpyHostToDevice, st));
    return ROM_OK;
  }

  // the levels: all open nodes of all trees per level, one read-back (the number of new nodes) each
  int grow(int max_depth, int min_samples_split, int min_samples_leaf) {
    TreeDev& d = ws.d;
    const int m = s.m, R = s.R, Q1 = s.q + 1;
    const unsigned gx = unsigned((s.ntiles + TR_WAVES - 1) / TR_WAVES);
    const dim3 g1(gx, 1), gm(gx, unsigned(m));
    const double msl = double(min_samples_leaf), mss = double(min_samples_split);
    const double lvl_bytes = 8.0 * double(R) * (s.q + 2);
    int lvl0 = 0, lvl1 = s.T, cur = 0;
    for (;;) {
      d.lvl0 = lvl0;
      d.ord = ws.ord[cur];
      d.nid = ws.nid[cur];
      {
        ROM_PROF(ctx, "tree_stats", 4.0 * R * Q1, 4.0 * lvl_bytes);
        k_tree_scan<0><<<g1, 256, 0, st>>>(d, 0, msl);
        k_tree_scan<1><<<g1, 256, 0, st>>>(d, 0, msl);
        ROM_HIP(hipGetLastError());
      }
      {
        ROM_PROF(ctx, "tree_tiles", 1.0 * m * R * Q1, m * lvl_bytes);
        k_tree_scan<0><<<gm, 256, 0, st>>>(d, 1, msl);
        ROM_HIP(hipGetLastError());
      }
      {
        ROM_PROF(ctx, "tree_stats", 4.0 * R * Q1, 4.0 * lvl_bytes);
        k_tree_scan<2><<<g1, 256, 0, st>>>(d, 1, msl);
        ROM_HIP(hipGetLastError());
      }
      {
        ROM_PROF(ctx, "tree_gain", 6.0 * m * R * Q1, m * lvl_bytes);
        k_tree_scan<3><<<gm, 256, 0, st>>>(d, 1, msl);
        ROM_HIP(hipGetLastError());
      }
      {
        ROM_PROF(ctx, "tree_decide", 0.0, 12.0 * m * R);
        k_tree_pick<<<blocks_for(size_t(m) * R), 256, 0, st>>>(d);
        k_tree_decide<<<1, 1024, 0, st>>>(d, lvl1, max_depth, mss, ws.counter);
        ROM_HIP(hipGetLastError());
      }
      launches += 7;
      ++levels;
      int fresh = 0;
      ROM_HIP(hipMemcpyAsync(&fresh, ws.counter, sizeof(int), hipMemcpyDeviceToHost, st));
      ROM_HIP(hipStreamSynchronize(st));
      ++syncs;
      if (fresh == 0) break;
      ROM_CHECK(size_t(lvl1) + size_t(fresh) <= s.nmax, "rom_tree_fit: %d + %d nodes exceed the bound 2 R - T = %zu (internal error)", lvl1,
                fresh, s.nmax);
      {
        ROM_PROF(ctx, "tree_partition", 0.0, 24.0 * m * R);
        k_tree_part<false><<<gm, 256, 0, st>>>(d, ws.itail, ws.ord[cur ^ 1], ws.nid[cur ^ 1]);
        k_tree_part<true><<<gm, 256, 0, st>>>(d, ws.itail, ws.ord[cur ^ 1], ws.nid[cur ^ 1]);
        ROM_HIP(hipGetLastError());
      }
      launches += 2;
      cur ^= 1;
      lvl0 = lvl1;
      lvl1 += fresh;
    }
    nodes = lvl1;
    return ROM_OK;
  }

  // the handle: the node arrays at their final size, the counters and info_host
  int handle(rom_tree* h, double* info_host) {
    const TreeDev& d = ws.d;
    const size_t N = size_t(nodes), q = size_t(s.q);
    h->nodes = int64_t(N);
    h->levels = levels;
    ROM_TRY(rom_buf_alloc(ctx, TreeNodes(nullptr, N, s.q).doubles, &h->dev));
    const TreeNodes a(h->dev->p, N, s.q);
    ROM_HIP(hipMemcpyAsync(a.thr, d.thr, N * sizeof(double), hipMemcpyDeviceToDevice, st));
    ROM_HIP(hipMemcpyAsync(a.n, d.n, N * sizeof(double), hipMemcpyDeviceToDevice, st));
    ROM_HIP(hipMemcpyAsync(a.val, d.val, N * q * sizeof(double), hipMemcpyDeviceToDevice, st));
    ROM_HIP(hipMemcpyAsync(a.feat, d.feat, N * sizeof(int), hipMemcpyDeviceToDevice, st));
    ROM_HIP(hipMemcpyAsync(a.left, d.left, N * sizeof(int), hipMemcpyDeviceToDevice, st));
    ROM_HIP(hipMemcpyAsync(a.tree, d.treeid, N * sizeof(int), hipMemcpyDeviceToDevice, st));
    ROM_HIP(hipStreamSynchronize(st));   // (the workspace goes back to the allocator)
    ++syncs;
    h->thr = a.thr, h->n = a.n, h->val = a.val, h->feat = a.feat, h->left = a.left, h->tree = a.tree;
    h->launches = launches, h->syncs = syncs;
    if (info_host) {
      info_host[0] = double(N);
      info_host[1] = double((N + s.T) / 2);   // nodes = 2 leaves - 1 in every tree
      info_host[2] = double(levels - 1);
      info_host[3] = double(levels);
      info_host[4] = double(launches);
      info_host[5] = double(syncs);
      info_host[6] = double(ws.doubles * sizeof(double));
      info_host[7] = 0.0;
    }
    return ROM_OK;
  }
};

}  // namespace

extern "C" int rom_tree_fit(rom_ctx* ctx, rom_buf* X, size_t x_off, int64_t ldx, int m, rom_buf* Y, size_t y_off, int64_t ldy, int q,
                            int64_t M, int T, const int32_t* counts_host, int max_depth, int min_samples_split, int min_samples_leaf,
                            rom_tree** out, double* info_host) {
  const char* who = "rom_tree_fit";
  ROM_CHECK(ctx && X && Y && out, "rom_tree_fit: null argument (context, X, Y or the handle's address)");
  ROM_CHECK(m >= 1 && m <= TR_MMAX, "rom_tree_fit: m = %d inputs, between 1 and %d", m, TR_MMAX);
  ROM_CHECK(q >= 1 && q <= TR_QMAX, "rom_tree_fit: q = %d target columns, between 1 and %d", q, TR_QMAX);
  ROM_CHECK(T >= 1 && T <= TR_TMAX, "rom_tree_fit: T = %d trees, between 1 and %d", T, TR_TMAX);
  ROM_CHECK(M >= 1 && M <= (int64_t(1) << 30), "rom_tree_fit: M = %lld rows, between 1 and 2^30", (long long)M);
  ROM_CHECK(max_depth >= 0, "rom_tree_fit: max_depth = %d, 0 (no limit) or more", max_depth);
  ROM_CHECK(min_samples_split >= 2, "rom_tree_fit: min_samples_split = %d, at least 2", min_samples_split);
  ROM_CHECK(min_samples_leaf >= 1, "rom_tree_fit: min_samples_leaf = %d, at least 1", min_samples_leaf);
  ROM_TRY(rom_check_block(who, {"X", "ldx", "m"}, X->n, x_off, ldx, m, M));
  ROM_TRY(rom_check_block(who, {"Y", "ldy", "q"}, Y->n, y_off, ldy, q, M));
  TreeShape shape{M, m, q, T, counts_host != nullptr};
  ROM_TRY(tree_rows(counts_host, shape));
  ROM_HIP(hipSetDevice(ctx->device));

  TreeFit fit(ctx, shape, counts_host);
  ROM_TRY(fit.ws.get(ctx, shape, X->p + x_off, ldx, Y->p + y_off, ldy));
  ROM_TRY(fit.check_and_presort());
  ROM_TRY(fit.roots());
  ROM_TRY(fit.grow(max_depth, min_samples_split, min_samples_leaf));
  rom_tree* h = new rom_tree;
  HandleGuard<rom_tree, rom_tree_destroy> guard{h};
  h->ctx = ctx, h->m = m, h->q = q, h->T = T, h->M_train = M;
  ROM_TRY(fit.handle(h, info_host));
  *out = guard.release();
  return ROM_OK;
}

extern "C" int rom_tree_predict(rom_tree* h, rom_buf* X, size_t x_off, int64_t ldx, int64_t M, rom_buf* OUT, size_t o_off, int64_t ldo,
                                rom_buf* Yref, size_t r_off, int64_t ldr, double* sumsq_host) {
  ROM_CHECK(h && X, "rom_tree_predict: null argument (handle or X)");
  ROM_CHECK(OUT || sumsq_host, "rom_tree_predict: OUT == NULL requires sumsq_host");
  rom_ctx* ctx = h->ctx;
  const int m = h->m, q = h->q;
  ROM_TRY(rom_check_predict_blocks("rom_tree_predict", M, X, x_off, ldx, m, q, OUT, o_off, ldo, Yref, r_off, ldr));
  ROM_HIP(hipSetDevice(ctx->device));
  const long long groups = (M + TR_PRED_ROWS - 1) / TR_PRED_ROWS;
  const int chunks = int(std::min<long long>(groups, 4ll * std::max(ctx->n_cu, 1)));
  const long long per = (groups + chunks - 1) / chunks;
  SumsqTail tail;
  if (sumsq_host) ROM_TRY(tail.get(ctx, chunks, q));
  {
    ROM_PROF(ctx, "tree_predict", 0.0, 8.0 * M * (m + q * (Yref ? 2.0 : 1.0)));
    k_tree_predict<<<chunks, 256, 0, ctx->stream>>>(h->feat, h->left, h->thr, h->val, q, h->T, X->p + x_off, ldx, M, groups, per,
                                                    OUT ? OUT->p + o_off : nullptr, ldo, Yref ? Yref->p + r_off : nullptr, ldr,
                                                    tail.partials());
  }
  ROM_HIP(hipGetLastError());
  h->launches += sumsq_host ? 2 : 1;   // (the column sums of the tail are a launch)
  ROM_TRY(tail.finish(ctx, chunks, q, sumsq_host));
  h->syncs += 1;
  return ROM_OK;
}


extern "C" int rom_tree_query(rom_tree* h, int64_t* out8) {
  ROM_CHECK(h && out8, "rom_tree_query: null argument");
  out8[0] = h->m;
  out8[1] = h->q;
  out8[2] = h->T;
  out8[3] = h->M_train;
  out8[4] = h->nodes;
  out8[5] = h->levels - 1;
  out8[6] = int64_t(h->launches);
  out8[7] = int64_t(h->syncs);
  return ROM_OK;
}

extern "C" int rom_tree_download(rom_tree* h, int what, double* host, size_t count) {
  ROM_CHECK(h && host, "rom_tree_download: null argument");
  ROM_CHECK(what >= 0 && what <= 5,
            "rom_tree_download: what = %d, one of 0 (first nodes), 1 (input), 2 (threshold), 3 (left child), 4 (count), 5 (values)", what);
  const size_t N = size_t(h->nodes), q = size_t(h->q);
  const size_t need = what == 0 ? size_t(h->T) + 1 : what == 5 ? N * q : N;
  ROM_CHECK(count == need, "rom_tree_download: part %d holds %zu doubles, count = %zu", what, need, count);
  if (!h->host_ready) {
    // the device numbers the nodes level by level over all trees; here: tree after tree, each still breadth first
    rom_ctx* ctx = h->ctx;
    ROM_HIP(hipSetDevice(ctx->device));
    std::vector<int> feat(N), left(N), tree(N);
    std::vector<double> thr(N), n(N), val(N * q);
    ROM_HIP(hipMemcpyAsync(feat.data(), h->feat, N * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ROM_HIP(hipMemcpyAsync(left.data(), h->left, N * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ROM_HIP(hipMemcpyAsync(tree.data(), h->tree, N * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ROM_HIP(hipMemcpyAsync(thr.data(), h->thr, N * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ROM_HIP(hipMemcpyAsync(n.data(), h->n, N * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ROM_HIP(hipMemcpyAsync(val.data(), h->val, N * q * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ROM_HIP(hipStreamSynchronize(ctx->stream));
    h->syncs += 1;
    std::vector<size_t> first(h->T + 1, 0), newid(N);
    for (size_t i = 0; i < N; ++i) first[tree[i] + 1] += 1;
    for (int t = 0; t < h->T; ++t) first[t + 1] += first[t];
    std::vector<size_t> at(first.begin(), first.end() - 1);
    for (size_t i = 0; i < N; ++i) newid[i] = at[tree[i]]++;
    h->h_first.assign(first.begin(), first.end());
    h->h_feat.resize(N);
    h->h_thr.resize(N);
    h->h_left.resize(N);
    h->h_n.resize(N);
    h->h_val.resize(N * q);
    for (size_t i = 0; i < N; ++i) {
      const size_t j = newid[i];
      h->h_feat[j] = feat[i];
      h->h_thr[j] = thr[i];
      h->h_left[j] = left[i] >= 0 ? double(newid[left[i]]) : -1.0;
      h->h_n[j] = n[i];
      std::copy(val.begin() + i * q, val.begin() + (i + 1) * q, h->h_val.begin() + j * q);
    }
    h->host_ready = true;
  }
  const std::vector<double>& src = what == 0 ? h->h_first : what == 1 ? h->h_feat : what == 2 ? h->h_thr : what == 3 ? h->h_left
                                   : what == 4 ? h->h_n : h->h_val;
  std::copy(src.begin(), src.end(), host);
  return ROM_OK;
}
