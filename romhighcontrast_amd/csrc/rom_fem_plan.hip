// rom_fem_plan: geometry of the interface, closed-form edge elimination, low-rank compression of the edges, symbolic
// tile Cholesky of the reduced matrix and every parameter-independent table, built on the host in long double
// (algorithm: see the header of rom_fem_kernels.hip and DESIGN.md section 3).  Host code only: no HIP call, nothing
// from another translation unit, no environment variable -- tests/c_abi/fem_plan_check.cpp runs it under sanitizers.
#include "rom_fem_plan.h"

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <map>
#include <set>
#include <thread>
#include <tuple>

#include "rom_hostla.h"

namespace {

using hostla::ld;
using hostla::Mat;

struct Edge {
  int hv, p, q;  // hv 0: horizontal (r = pN, c in block column q); 1: vertical (c = qN, r in block row p)
  int b0, b1;    // up/dn or lf/rt block indices
};

// one parameter-independent block of the reduced matrix: coef(kind, b) * tab at (rpos, cpos)
struct Small {
  int rpos, cpos;
  Mat tab;
  int kind;
  std::array<int, 4> b;
};

// compressed representation of an active edge (shared by all edges with the same surroundings)
struct Comp {
  int r = 0;
  Mat W;               // n1 x r   orthonormal basis of the coupling range
  Mat Kt;              // r x r    (W^T K^-1 W)^-1
  Mat P;               // n1 x r   K^-1 W Kt
  std::vector<ld> gt;  // r        Kt W^T K^-1 g_f
  std::vector<ld> p0;  // n1       (K^-1 - P W^T K^-1) g_f
  Mat KiW;             // n1 x r   K^-1 W          (closed-form edges: u_e = (KiW c_e + wK) / s_e)
  std::vector<ld> wK;  // n1       K^-1 g_f
  std::vector<int> entry;  // r    rotated basis (rotate_to_echelon): first sine mode of the direction's extension-table column
};

// run fn(0) ... fn(n-1) on up to hardware_concurrency host threads (the long-double table products are
// independent of each other and dominate rom_fem_create)
template <class F>
void parallel_for(size_t n, F fn) {
  const unsigned nthr = std::max(1u, std::min<unsigned>(std::thread::hardware_concurrency(), unsigned(n)));
  std::atomic<size_t> next{0};
  auto work = [&]() {
    for (size_t i = next++; i < n; i = next++) fn(i);
  };
  std::vector<std::thread> pool;
  for (unsigned t = 1; t < nthr; ++t) pool.emplace_back(work);
  work();
  for (auto& th : pool) th.join();
}

// Closed-form tables of one unit block (N x N cells, Dirichlet 5-point Laplacian L) in long double, from the sine
// eigenbasis:  Q[j][m] = sqrt(2/N) sin(pi j m / N),  lam_m = 2 - 2 cos(pi m / N),
// rho_m(i) = sinh((N-i) phi_m) / sinh(N phi_m) with cosh phi_m = 1 + lam_m / 2.
struct UnitBlock {
  int N, n1;
  Mat Q, rho;                  // rho(m, i), i = 0..N
  std::vector<ld> lam, kappa;  // kappa_m = 1 + lam_m/2 - rho_m(1): K = tridiag(-1/2, 2, -1/2) - T_same = Q diag(kappa) Q
  Mat Wl;                      // L^-1 1
  Mat Kmat, Kinv;
  std::vector<ld> gE[2];       // interface rhs of a horizontal / vertical edge: h^2 (1 + W on the two adjacent lines)
  std::vector<double> rho_d, Wd;

  UnitBlock(int N_, bool with_edges) : N(N_), n1(N_ - 1), Q(n1, n1), rho(n1, N_ + 1), lam(n1), kappa(n1), Wl(n1, n1) {
    const ld PI = acosl(-1.0L);
    for (int j = 1; j <= n1; ++j) {
      lam[j - 1] = 2.0L - 2.0L * cosl(PI * j / N);
      for (int m = 1; m <= n1; ++m) Q(j - 1, m - 1) = sqrtl(2.0L / N) * sinl(PI * j * m / (ld)N);
    }
    for (int m = 0; m < n1; ++m) {
      const ld phi = acoshl(1.0L + lam[m] / 2.0L);
      const ld den = -expm1l(-2.0L * N * phi);  // 1 - exp(-2 N phi)
      for (int i = 0; i <= N; ++i) rho(m, i) = expl(-phi * i) * (-expm1l(-2.0L * (N - i) * phi)) / den;
      kappa[m] = 1.0L + lam[m] / 2.0L - rho(m, 1);
    }
    rho_d.resize(rho.v.size());
    for (size_t i = 0; i < rho.v.size(); ++i) rho_d[i] = double(rho.v[i]);
    {  // W = L^{-1} 1 = Q (s s^T / (lam_l + lam_m)) Q
      std::vector<ld> sv(n1, 0.0L);
      Mat Z(n1, n1);
      for (int m = 0; m < n1; ++m)
        for (int j = 0; j < n1; ++j) sv[m] += Q(j, m);
      for (int l = 0; l < n1; ++l)
        for (int m = 0; m < n1; ++m) Z(l, m) = sv[l] * sv[m] / (lam[l] + lam[m]);
      Zs = Z;
    }
    Kmat = Mat(n1, n1);
    Kinv = Mat(n1, n1);
    Mat QK(n1, n1), QKi(n1, n1);
    for (int j = 0; j < n1; ++j)
      for (int m = 0; m < n1; ++m) {
        QK(j, m) = Q(j, m) * kappa[m];
        QKi(j, m) = Q(j, m) / kappa[m];
      }
    // (four n1^3 products, one after the other with their rows spread over the host threads: two of them depend on
    // each other, so one thread per product would leave the critical path at two products)
    Wl = hostla::mul_par(Q, hostla::mul_nt_par(Zs, Q));
    if (with_edges) {
      Kmat = hostla::mul_nt_par(QK, Q);
      Kinv = hostla::mul_nt_par(QKi, Q);
    }
    Wd.resize(size_t(n1) * n1);
    for (size_t i = 0; i < Wd.size(); ++i) Wd[i] = double(Wl.v[i]);
    const ld h2 = 1.0L / ((ld)N * (ld)N);
    for (int hv = 0; hv < 2; ++hv) {
      gE[hv].resize(n1);
      for (int t = 0; t < n1; ++t)
        gE[hv][t] = h2 * (1.0L + (hv == 0 ? Wl(N - 2, t) + Wl(0, t) : Wl(t, N - 2) + Wl(t, 0)));
    }
  }

  // build the tables `ids` (and, if with_tk, their products with K^-1) on several threads
  void prepare(const std::vector<int>& ids, bool with_tk) {
    std::vector<int> todo;
    for (int id : ids)
      if (!(with_tk ? haveTK[id] : haveT[id]) && std::find(todo.begin(), todo.end(), id) == todo.end()) todo.push_back(id);
    parallel_for(todo.size(), [&](size_t i) { build(todo[i], with_tk); });
  }

  // Dirichlet-to-Neumann table T[sr*4+sc][t][k] = H_sc[interior vertex next to node t of side sr][k] (first use builds it)
  const Mat& Tm(int id) {
    if (!haveT[id]) build(id, false);
    return Tm_[id];
  }
  const Mat& Tm_ready(int id) const { return Tm_[id]; }  // (read-only access for the worker threads: built before)
  // ... and its product with K^-1
  const Mat& TK(int id) {
    if (!haveTK[id]) build(id, true);
    return TK_[id];
  }

 private:
  void build(int id, bool with_tk) {  // (distinct ids may be built concurrently)
    if (!haveT[id]) {
      const int sr = id >> 2, sc = id & 3;
      Mat V(n1, n1);
      for (int t = 0; t < n1; ++t) {
        int i, j;
        switch (sr) {
          case 0: i = 1; j = t + 1; break;
          case 1: i = N - 1; j = t + 1; break;
          case 2: i = t + 1; j = 1; break;
          default: i = t + 1; j = N - 1; break;
        }
        const int hr = h0_row(sc, i, j, N, n1);
        const int ii = hr / n1 + 1, jj = hr % n1 + 1;
        for (int m = 0; m < n1; ++m) V(t, m) = Q(jj - 1, m) * rho(m, ii);
      }
      Tm_[id] = hostla::mul_nt(V, Q);
      haveT[id] = 1;
    }
    if (with_tk && !haveTK[id]) {
      TK_[id] = hostla::mul(Tm_[id], Kinv);
      haveTK[id] = 1;
    }
  }
  Mat Zs;
  std::array<Mat, 16> Tm_, TK_;
  std::array<char, 16> haveT{}, haveTK{};
};

// Compressed form of an edge whose couplings act through the tables `tabs` (ids sr*4+sc) and, if x0 / x1, through
// its first / last node (cross points): W = orthonormal basis of the union of their ranges.
// Step 1: the nested basis down to `keep` of the first pivot, with the pivot norms (the caller picks the rank).
void compress_basis(const UnitBlock& ub, const std::vector<int>& tabs, bool x0, bool x1, ld keep, Mat& Wb, std::vector<ld>& pivots) {
  const int n1 = ub.n1;
  const int ntab = int(tabs.size());
  Mat C(n1, ntab * n1 + 2);
  for (int t = 0; t < ntab; ++t) {
    const Mat& Tt = ub.Tm_ready(tabs[t]);
    ld mx = 0;
    for (ld v : Tt.v) mx = std::max(mx, fabsl(v));
    if (mx == 0.0L) mx = 1.0L;
    for (int i = 0; i < n1; ++i)
      for (int k = 0; k < n1; ++k) C(i, t * n1 + k) = Tt(i, k) / mx;
  }
  if (x0) C(0, ntab * n1) = 1.0L;
  if (x1) C(n1 - 1, ntab * n1 + 1) = 1.0L;
  Wb = hostla::range_basis(C, keep, &pivots);
}
// Step 2: everything that follows from the first `r` columns of that basis (r >= n1 or !compress: nodal unknowns,
// W = I).  False if the compressed self block is not SPD.
bool compress_finish(const UnitBlock& ub, const Mat& Wfull, int r, int hv, bool compress, Comp& cp) {
  const int n1 = ub.n1;
  if (!compress || r >= n1) {  // nothing to gain: nodal unknowns
    cp.r = n1;
    cp.W = hostla::identity(n1);
    cp.Kt = ub.Kmat;
    cp.P = hostla::identity(n1);
    cp.gt = ub.gE[hv];
    cp.p0.assign(n1, 0.0L);
    cp.KiW = ub.Kinv;
    cp.wK = hostla::matvec(ub.Kinv, ub.gE[hv]);
    return true;
  }
  Mat Wb(n1, r);
  for (int i = 0; i < n1; ++i)
    for (int k = 0; k < r; ++k) Wb(i, k) = Wfull(i, k);
  cp.r = r;
  cp.W = Wb;
  Mat KiW = hostla::mul(ub.Kinv, Wb);
  Mat G = hostla::mul_tn(Wb, KiW);
  for (int i = 0; i < G.r; ++i)
    for (int j = 0; j < i; ++j) G(i, j) = G(j, i) = (G(i, j) + G(j, i)) / 2;
  if (!hostla::spd_inverse(G, cp.Kt)) return false;
  cp.P = hostla::mul(KiW, cp.Kt);
  std::vector<ld> v = hostla::matvec(ub.Kinv, ub.gE[hv]);
  std::vector<ld> wv = hostla::matvec(hostla::transpose(Wb), v);
  cp.gt = hostla::matvec(cp.Kt, wv);
  std::vector<ld> pw = hostla::matvec(cp.P, wv);
  cp.p0.resize(n1);
  for (int i = 0; i < n1; ++i) cp.p0[i] = v[i] - pw[i];
  cp.KiW = KiW;
  cp.wK = v;
  return true;
}

// The basis of the reduced unknowns is ours to choose: any W E with E orthogonal spans the same space and gives the same
// solution.  Choose E so that the sine coefficients of the type's extension table, (P E)^T Q (variant 0, active edges) or
// (K^-1 W E)^T Q (variant 1, closed-form edges), are in row-echelon form in mode order: direction k then carries only modes
// >= entry[k] and dies with the distance from the side like rho_entry[k](d) -- far from the side the kernel can skip it,
// by the criterion kmax applies to the sine modes.  The directions are stored in DESCENDING entry mode: the ones that can
// be dropped come first, a tile starts its walk at a later K segment and 1/s stays last.
bool rotate_to_echelon(const UnitBlock& ub, int hv, int variant, Comp& cp) {
  const int n1 = ub.n1, r = cp.r;
  std::vector<int> entry;
  const Mat E = hostla::echelon_rotation(hostla::mul_tn(variant == 0 ? cp.P : cp.KiW, ub.Q), &entry);
  const Mat WE = hostla::mul(cp.W, E);
  Mat Wr(n1, r);
  for (int i = 0; i < n1; ++i)
    for (int k = 0; k < r; ++k) Wr(i, k) = WE(i, r - 1 - k);
  if (!compress_finish(ub, Wr, r, hv, true, cp)) return false;
  cp.entry.assign(entry.rbegin(), entry.rend());
  return true;
}

struct TermAcc {
  std::array<int, 5> key;
  std::vector<double> tab;
  int r_lo, r_hi, c_lo, c_hi;
};

// n1p x n1p fp64 table (zero padded) from a long double matrix of at most that size
void put_table(std::vector<double>& pool, size_t idx, int n1p, const Mat& A, bool transposed) {
  double* dst = pool.data() + idx * size_t(n1p) * n1p;
  for (int i = 0; i < A.r; ++i)
    for (int j = 0; j < A.c; ++j) {
      if (transposed) dst[size_t(j) * n1p + i] = double(A(i, j));
      else dst[size_t(i) * n1p + j] = double(A(i, j));
    }
}

int pad_bk(int r) { return (r + 1 + BK - 1) / BK * BK; }  // width of an edge's [z, 1/s] block: rank + 1 in whole K chunks
int segs8(int r) { return (r + 1 + 7) / 8; }              // ... in the 8-wide K segments of k_extend128

int push_vec(std::vector<double>& vecs, const std::vector<ld>& v, int padded) {  // append to the vector table
  const int off = int(vecs.size());
  for (ld x : v) vecs.push_back(double(x));
  for (int i = int(v.size()); i < padded; ++i) vecs.push_back(0.0);
  return off;
}

void add_small(std::vector<Small>& smalls, int rpos, int cpos, const Mat& tab, int kind, std::array<int, 4> b) {
  smalls.push_back(Small{rpos, cpos, tab, kind, b});
  if (rpos != cpos) smalls.push_back(Small{cpos, rpos, hostla::transpose(tab), kind, b});
}

template <class F>
void for_tiles(const Small& s, F fn) {  // the tiles (tr, tc) that a block of the reduced matrix meets
  for (int tr = s.rpos / TB; tr <= (s.rpos + s.tab.r - 1) / TB; ++tr)
    for (int tc = s.cpos / TB; tc <= (s.cpos + s.tab.c - 1) / TB; ++tc) fn(tr, tc);
}

// ---- edges, crosses, cross <-> edge-end couplings, block adjacency ---------------------------------------------
struct XCpl { int cross, edge, node; };  // node: 0-based local node on the edge
struct Topology {
  int nrb, ncb, N, n1, E = 0, ncross = 0;
  std::vector<Edge> edges;
  std::vector<std::pair<int, int>> crosses;
  std::vector<std::array<int, 4>> bside;  // block -> side -> edge id   (sides: 0 top, 1 bottom, 2 left, 3 right)
  std::vector<XCpl> xc;
  std::vector<std::set<int>> adj;  // block adjacency of the edges
  int side_of(int blk, int e) const {
    for (int s = 0; s < 4; ++s)
      if (bside[blk][s] == e) return s;
    return -1;
  }
  int shared_block(int e1, int e2) const {  // the one block two distinct edges can share, or -1
    for (int b1 : {edges[e1].b0, edges[e1].b1})
      for (int b2 : {edges[e2].b0, edges[e2].b1})
        if (b1 == b2) return b1;
    return -1;
  }
  // id sr * 4 + sc of the table T that takes the values of edge `to` (side sc of the shared block) to edge `from` (side sr)
  int table_id(int from, int to) const {
    const int blk = shared_block(from, to);
    return side_of(blk, from) * 4 + side_of(blk, to);
  }
};

Topology make_topology(int nrb, int ncb, int N) {
  Topology t;
  t.nrb = nrb; t.ncb = ncb; t.N = N; t.n1 = N - 1;
  std::map<std::pair<int, int>, int> hid, vid, xid;
  for (int p = 1; p < nrb; ++p)
    for (int q = 0; q < ncb; ++q) {
      hid[{p, q}] = int(t.edges.size());
      t.edges.push_back({0, p, q, (p - 1) * ncb + q, p * ncb + q});
    }
  for (int q = 1; q < ncb; ++q)
    for (int p = 0; p < nrb; ++p) {
      vid[{p, q}] = int(t.edges.size());
      t.edges.push_back({1, p, q, p * ncb + (q - 1), p * ncb + q});
    }
  for (int p = 1; p < nrb; ++p)
    for (int q = 1; q < ncb; ++q) {
      xid[{p, q}] = int(t.crosses.size());
      t.crosses.push_back({p, q});
    }
  t.E = int(t.edges.size());
  t.ncross = int(t.crosses.size());
  t.bside.resize(nrb * ncb);
  for (int p = 0; p < nrb; ++p)
    for (int q = 0; q < ncb; ++q) {
      auto& s = t.bside[p * ncb + q];
      s[0] = p >= 1 ? hid[{p, q}] : -1;
      s[1] = p + 1 < nrb ? hid[{p + 1, q}] : -1;
      s[2] = q >= 1 ? vid[{p, q}] : -1;
      s[3] = q + 1 < ncb ? vid[{p, q + 1}] : -1;
    }
  for (int e = 0; e < t.E; ++e) {
    const Edge& ed = t.edges[e];
    if (ed.hv == 0) {
      if (ed.q >= 1) t.xc.push_back({xid[{ed.p, ed.q}], e, 0});
      if (ed.q + 1 < ncb) t.xc.push_back({xid[{ed.p, ed.q + 1}], e, t.n1 - 1});
    } else {
      if (ed.p >= 1) t.xc.push_back({xid[{ed.p, ed.q}], e, 0});
      if (ed.p + 1 < nrb) t.xc.push_back({xid[{ed.p + 1, ed.q}], e, t.n1 - 1});
    }
  }
  t.adj.resize(t.E);
  for (auto& s : t.bside)
    for (int x = 0; x < 4; ++x)
      for (int y = 0; y < 4; ++y)
        if (x != y && s[x] >= 0 && s[y] >= 0) t.adj[s[x]].insert(s[y]);
  return t;
}

// ---- edges eliminated in closed form: a maximal set no two of which touch the same block (greedy); their
//      self-interaction is (a_b0 + a_b1) K with K parameter independent and they do not couple to each other.
//      Elimination order of the active edges: greedy minimum degree on the graph (shared block, or common neighbour
//      of a closed-form edge) ------------------------------------------------------------------------------------
struct Elimination {
  std::vector<char> is_pre;
  std::vector<int> pre_list, order, ord_of;
};

Elimination choose_elimination(const Topology& t, bool no_preelim) {
  const int E = t.E;
  Elimination el;
  el.is_pre.assign(E, 0);
  el.ord_of.assign(E, -1);
  const std::vector<char>& is_pre = el.is_pre;
  if (!no_preelim) {
    std::vector<char> busy(t.nrb * t.ncb, 0);
    for (int e = 0; e < E; ++e)
      if (!busy[t.edges[e].b0] && !busy[t.edges[e].b1]) { el.is_pre[e] = 1; busy[t.edges[e].b0] = busy[t.edges[e].b1] = 1; }
  }
  for (int e = 0; e < E; ++e)
    if (is_pre[e]) el.pre_list.push_back(e);
  const int nact = E - int(el.pre_list.size());
  std::vector<std::set<int>> g(E);
  for (int e = 0; e < E; ++e)
    if (!is_pre[e])
      for (int x : t.adj[e])
        if (!is_pre[x]) g[e].insert(x);
  for (int e : el.pre_list)
    for (int x : t.adj[e])
      for (int y : t.adj[e])
        if (x != y && !is_pre[x] && !is_pre[y]) g[x].insert(y);
  std::vector<char> done(E, 0);
  for (int step = 0; step < nact; ++step) {
    int best = -1;
    size_t bd = 0;
    for (int e = 0; e < E; ++e) {
      if (done[e] || is_pre[e]) continue;
      if (best < 0 || g[e].size() < bd) { best = e; bd = g[e].size(); }
    }
    done[best] = 1;
    el.ord_of[best] = int(el.order.size());
    el.order.push_back(best);
    std::vector<int> nb(g[best].begin(), g[best].end());
    for (int x : nb) {
      g[x].erase(best);
      for (int y : nb)
        if (x != y) g[x].insert(y);
    }
  }
  return el;
}

// ---- compression of the edges -----------------------------------------------------------------------------------
struct Compression {
  std::vector<std::vector<int>> sigs;  // edges with the same surroundings share one compressed form (an edge type)
  std::vector<int> comp_of;            // edge -> type
  std::vector<Comp> comps;
  std::vector<int> kmax, rp;           // kmax[d]: see extension_ranks; rp: padded width of a type's [z, 1/s] block
  std::vector<char> use_lr;            // the type enters the extension through its reduced unknowns
  std::vector<char> variant;           // rotated bases: 0 the type of active edges, 1 of closed-form edges (two records where
                                       // the same surroundings serve both: the two extension tables need different rotations)
  double kavg = 0;
};

void edge_types(const Topology& t, const Elimination& el, bool by_variant, Compression& c) {
  std::map<std::vector<int>, int> sig_id;
  c.comp_of.assign(t.E, -1);
  for (int e = 0; e < t.E; ++e) {
    const Edge& ed = t.edges[e];
    std::vector<int> sig{ed.hv};
    for (int blk : {ed.b0, ed.b1}) {
      const int sf = t.side_of(blk, e);
      for (int s2 = 0; s2 < 4; ++s2)
        if (s2 != sf && t.bside[blk][s2] >= 0) sig.push_back(sf * 4 + s2);
    }
    bool x0 = false, x1 = false;
    for (auto& x : t.xc)
      if (x.edge == e) (x.node == 0 ? x0 : x1) = true;
    const int variant = by_variant && el.is_pre[e] ? 1 : 0;
    sig.push_back(100 + (x0 ? 1 : 0) + (x1 ? 2 : 0) + 4 * variant);
    auto it = sig_id.find(sig);
    if (it == sig_id.end()) {
      it = sig_id.emplace(sig, int(c.sigs.size())).first;
      c.sigs.push_back(sig);
      c.variant.push_back(char(variant));
    }
    c.comp_of[e] = it->second;
  }
}

// Numerical rank of an edge's coupling tables.  Directions weaker than `ctol` = 1e-14 of the strongest are dropped
// where that removes work: the tables are rounded to fp64 on upload, and against a basis kept down to 1e-17 the
// snapshots move by <= 1.2e-14 relative over seven geometries and contrasts up to 1e8 (1e-13: 9e-14; the distance to the
// reference SuperLU solve, 1e-13..1e-12, does not change in its first three digits) while the reduced system shrinks from 347
// to 301 unknowns at C4 (6 -> 5 tile columns) and from 801 to 697 at C5 (13 -> 11): -19 % per step
// (profiles/r02_compress_tolerance.txt).  Where it removes nothing -- the weaker directions fit into the padding of the
// extension's 8-wide K segments and add no tile column to the reduced matrix (C2) -- they are kept, down to `ckeep`.
// The edge types are independent: one host thread each (the tables they read are built first).
bool compress_edges(UnitBlock& ub, const Topology& t, const Elimination& el, const FemSwitches& sw, Compression& c) {
  const int n1 = t.n1;
  const bool compress = !sw.no_compress;
  const ld ctol = sw.compress_tol, ckeep = std::min<ld>(ctol, 1e-17L);
  const size_t ntype = c.sigs.size();
  c.comps.resize(ntype);
  std::vector<int> ids, ids_tk;
  for (auto& sig : c.sigs)
    for (size_t k = 1; k + 1 < sig.size(); ++k) ids.push_back(sig[k]);
  for (int e : el.pre_list)  // the closed-form edges also need T K^-1 towards their neighbours
    for (int u : t.adj[e]) {
      ids_tk.push_back(t.table_id(u, e));
      ids.push_back(t.table_id(e, u));
    }
  ub.prepare(ids, false);
  ub.prepare(ids_tk, true);
  std::vector<char> ok(ntype, 1);
  std::vector<Mat> Wfull(ntype);
  std::vector<std::vector<ld>> pivots(ntype);
  if (compress)
    parallel_for(ntype, [&](size_t k) {
      const std::vector<int>& sig = c.sigs[k];
      const int flags = sig.back() - 100;
      compress_basis(ub, std::vector<int>(sig.begin() + 1, sig.end() - 1), flags & 1, flags & 2, ckeep, Wfull[k], pivots[k]);
    });
  // the ranks: at `ctol`, or -- if that costs neither a K segment nor a tile column -- up to the end of the last segment
  std::vector<int> r_drop(ntype, n1), r_use(ntype, n1);
  if (compress) {
    std::vector<int> r_fill(ntype, n1);
    for (size_t k = 0; k < ntype; ++k) {
      int r = 0;
      while (r < int(pivots[k].size()) && pivots[k][r] > ctol * pivots[k][0]) ++r;
      r_drop[k] = r;
      r_fill[k] = std::min<int>(int(pivots[k].size()), segs8(r) * 8 - 1);
    }
    auto tiles = [&](const std::vector<int>& rr) {
      long long nred = t.ncross;
      for (int e : el.order) nred += std::min(rr[c.comp_of[e]], n1);
      return (nred + TB - 1) / TB;
    };
    r_use = tiles(r_fill) <= tiles(r_drop) ? r_fill : r_drop;
  }
  parallel_for(ntype, [&](size_t k) {
    ok[k] = compress_finish(ub, Wfull[k], r_use[k], c.sigs[k][0], compress, c.comps[k]);
    if (ok[k] && compress && !sw.no_ext_trunc && c.comps[k].r < n1) ok[k] = rotate_to_echelon(ub, c.sigs[k][0], c.variant[k], c.comps[k]);
  });
  return std::find(ok.begin(), ok.end(), 0) == ok.end();
}

// kmax[d]: sine modes with rho_mode(d) >= 1e-18 (rounded up to the K chunk): what the extension needs at
// distance d from a side.  A compressed edge enters the extension through its reduced unknowns instead
// when rank + 1 (padded) is not much above the average mode count.
void extension_ranks(const UnitBlock& ub, int n1p, bool no_lowrank_ext, Compression& c) {
  const int N = ub.N, n1 = ub.n1;
  c.kmax.assign(N + 1, n1p);
  for (int dd = 1; dd <= N; ++dd) {
    int last = -1;
    for (int m = 0; m < n1; ++m)
      if (ub.rho_d[size_t(m) * (N + 1) + std::min(dd, N)] >= 1e-18) last = m;
    c.kmax[dd] = std::min(n1p, std::max(BK, (last + 1 + BK - 1) / BK * BK));
    if (dd <= n1) c.kavg += c.kmax[dd] / double(std::max(n1, 1));
  }
  c.kmax[0] = n1p;
  c.rp.assign(c.comps.size(), 0);
  c.use_lr.assign(c.comps.size(), 0);
  for (size_t k = 0; k < c.comps.size(); ++k) {
    c.rp[k] = pad_bk(c.comps[k].r);
    // (up to a quarter more K than the truncated modes is still a gain: flat K, wide tiles, no edge transforms)
    c.use_lr[k] = c.comps[k].r < n1 && c.rp[k] <= 1.25 * c.kavg && n1 > 0 && !no_lowrank_ext;
  }
}

// ---- layout of the interface vector: the reduced part (edge groups in elimination order, every cross point right
//      behind the adjacent active edge that is eliminated last), one nodal n1p block per edge, the cross block, the
//      [z, 1/s] blocks of the edges that enter the extension in compressed form, the scalar block -------------------
struct Layout {
  std::vector<int> zpos, rk, xred, npos, cpos;
  int nred = 0, T, nGa, xb0, nGp, spos0, nsc;
};

Layout make_layout(const Topology& t, const Elimination& el, const Compression& c, int n1p) {
  const int E = t.E, ncross = t.ncross;
  Layout L;
  L.zpos.assign(E, -1); L.rk.assign(E, 0); L.xred.assign(ncross, -1); L.npos.assign(E, -1); L.cpos.assign(E, -1);
  std::vector<int> xhost(ncross, -1);
  for (int x = 0; x < ncross; ++x)
    for (auto& k : t.xc)
      if (k.cross == x && !el.is_pre[k.edge] && (xhost[x] < 0 || el.ord_of[k.edge] > el.ord_of[xhost[x]])) xhost[x] = k.edge;
  int nred = 0;
  {
    // one tile in total: cross points first, so that their couplings are table ROWS of the upper triangle
    // (the single-tile assembly reads row segments; a cross behind its edges would cost one 8-byte read per
    // edge row instead)
    int total = ncross;
    for (int e : el.order) total += c.comps[c.comp_of[e]].r;
    if (total <= TB)
      for (int x = 0; x < ncross; ++x) L.xred[x] = nred++;
  }
  for (int e : el.order) {
    L.zpos[e] = nred;
    L.rk[e] = c.comps[c.comp_of[e]].r;
    nred += L.rk[e];
    for (int x = 0; x < ncross; ++x)
      if (xhost[x] == e && L.xred[x] < 0) L.xred[x] = nred++;
  }
  for (int x = 0; x < ncross; ++x)
    if (L.xred[x] < 0) L.xred[x] = nred++;
  L.nred = nred;
  L.T = (nred + TB - 1) / TB;
  L.nGa = L.T * TB;
  for (int e = 0; e < E; ++e) L.npos[e] = L.nGa + e * n1p;
  L.xb0 = L.nGa + E * n1p;
  L.nGp = L.xb0 + (ncross > 0 ? (ncross + TB - 1) / TB * TB : 0);
  // [z_f, 1/s_f] blocks of the active edges that enter the extension in compressed form, then [c_e / s_e, 1/s_e] of the
  // closed-form edges kept in compressed form
  for (const std::vector<int>* list : {&el.order, &el.pre_list})
    for (int e : *list)
      if (c.use_lr[c.comp_of[e]]) {
        L.cpos[e] = L.nGp;
        L.nGp += c.rp[c.comp_of[e]];
      }
  // scalar block: 1/(a_p + a_q) of every edge, then h^2/a_b of every block -- with it the expansion stage is a
  // LINEAR map of the interface vector (it never reads the parameters)
  L.spos0 = L.nGp;
  L.nsc = E + t.nrb * t.ncb;
  L.nGp += (L.nsc + BK - 1) / BK * BK;
  return L;
}

// ---- The r x n1 x n1 long-double products W_c^T T (and W_c^T T K^-1) of the next two phases depend only on (edge type c,
// table id): the edges of a regular grid ask for the same few again and again (1.2 s of the 1.7 s of a 4x4 / N=256
// setup went into recomputing them one after the other).  Collect the distinct ones, compute them on all host
// threads, look them up in the loops.
using WtCache = std::map<std::tuple<int, int, int>, Mat>;  // (edge type, table id, 0: T | 1: T K^-1) -> W^T table

WtCache wt_products(UnitBlock& ub, const Topology& t, const Elimination& el, const Compression& c, const Layout& L) {
  std::vector<std::tuple<int, int, int>> keys;
  for (int e : el.order)
    for (int e2 : t.adj[e])
      if (!el.is_pre[e2] && e2 > e) keys.emplace_back(c.comp_of[e], t.table_id(e, e2), 0);
  for (int e : el.pre_list)
    for (int u : t.adj[e]) {
      const int id = t.table_id(u, e);
      keys.emplace_back(c.comp_of[u], id, 0);
      keys.emplace_back(c.comp_of[u], id, 1);
      if (L.cpos[e] >= 0) keys.emplace_back(c.comp_of[e], t.table_id(e, u), 0);
    }
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  // the tables themselves are built lazily: make sure every one that is needed exists (distinct ids concurrently)
  std::vector<std::pair<int, int>> tabs;
  for (const auto& [k, id, which] : keys) tabs.emplace_back(id, which);
  std::sort(tabs.begin(), tabs.end());
  tabs.erase(std::unique(tabs.begin(), tabs.end()), tabs.end());
  std::vector<std::pair<int, int>> tab_ids;  // one entry per id (with K^-1 if any key wants it): a build covers both
  for (const auto& tb : tabs) {
    if (!tab_ids.empty() && tab_ids.back().first == tb.first) tab_ids.back().second |= tb.second;
    else tab_ids.push_back(tb);
  }
  parallel_for(tab_ids.size(), [&](size_t k) {
    if (tab_ids[k].second) ub.TK(tab_ids[k].first);
    ub.Tm(tab_ids[k].first);
  });
  std::vector<Mat> vals(keys.size());
  parallel_for(keys.size(), [&](size_t k) {
    const auto& [k_c, id, which] = keys[k];
    vals[k] = hostla::mul_tn(c.comps[k_c].W, which ? ub.TK(id) : ub.Tm(id));
  });
  WtCache cache;
  for (size_t k = 0; k < keys.size(); ++k) cache.emplace(keys[k], std::move(vals[k]));
  return cache;
}

// ---- blocks of the reduced matrix: active edges and cross points ---------------------------------------------------
std::vector<Small> reduced_blocks(const Topology& t, const Elimination& el, const Compression& c, const Layout& L,
                                  const WtCache& wt) {
  std::vector<Small> smalls;
  for (int e : el.order) {
    const Edge& ed = t.edges[e];
    add_small(smalls, L.zpos[e], L.zpos[e], c.comps[c.comp_of[e]].Kt, 1, {ed.b0, ed.b1, 0, 0});
    for (int e2 : t.adj[e]) {
      if (el.is_pre[e2] || e2 <= e) continue;
      const Mat& WT = wt.at({c.comp_of[e], t.table_id(e, e2), 0});
      add_small(smalls, L.zpos[e], L.zpos[e2], hostla::mul(WT, c.comps[c.comp_of[e2]].W), 0, {t.shared_block(e, e2), 0, 0, 0});
    }
  }
  for (auto& x : t.xc) {
    if (el.is_pre[x.edge]) continue;  // folded into the closed-form tables
    const Comp& ce = c.comps[c.comp_of[x.edge]];
    Mat row(1, ce.r);
    for (int k = 0; k < ce.r; ++k) row(0, k) = ce.W(x.node, k);
    add_small(smalls, L.xred[x.cross], L.zpos[x.edge], row, 2, {t.edges[x.edge].b1, t.edges[x.edge].b0, 0, 0});
  }
  for (int x = 0; x < t.ncross; ++x) {
    const int p = t.crosses[x].first, q = t.crosses[x].second, ncb = t.ncb;
    Mat one(1, 1);
    one(0, 0) = 1.0L;
    add_small(smalls, L.xred[x], L.xred[x], one, 3, {(p - 1) * ncb + (q - 1), (p - 1) * ncb + q, p * ncb + (q - 1), p * ncb + q});
  }
  return smalls;
}

// ---- closed-form edges: neighbours, reduced-matrix blocks, rhs terms, back substitution ---------------------------
struct Ent { int pos, len, blk; Mat X, Y; };  // X: len x n1 coupling to e (without its weight), Y = X K^-1
struct PreWork {
  std::vector<ld> we;              // K^-1 g_e
  std::vector<Ent> ents;           // neighbours (order of adj[e]), then the cross points on e (order of xc)
  std::vector<Mat> Mt;             // per neighbour (compressed e only): (W_e^T T P_u)^T
  std::vector<std::vector<ld>> mtv;  //                                    W_e^T T p0_u
  Mat Btx;
  bool has_x = false;
  std::vector<std::vector<ld>> rhsv;  // per entity: Y g_e
  std::vector<Mat> R;                 // Y_u X_v^T for v <= u, in the order of the loops of closed_form_records
};

// the long-double products of every closed-form edge, one host thread per edge (they read shared tables only)
std::vector<PreWork> closed_form_products(const UnitBlock& ub, const Topology& t, const Elimination& el, const Compression& c,
                                          const Layout& L, const WtCache& wt) {
  const int n1 = t.n1;
  std::vector<PreWork> prework(el.pre_list.size());
  parallel_for(prework.size(), [&](size_t i) {
    const int e = el.pre_list[i];
    const std::vector<ld>& g = ub.gE[t.edges[e].hv];
    PreWork& w = prework[i];
    w.we = hostla::matvec(ub.Kinv, g);
    for (int u : t.adj[e]) {
      const int id = t.table_id(u, e);
      const Comp& cu = c.comps[c.comp_of[u]];
      w.ents.push_back(Ent{L.zpos[u], cu.r, t.shared_block(e, u), wt.at({c.comp_of[u], id, 0}), wt.at({c.comp_of[u], id, 1})});
      if (L.cpos[e] >= 0) {
        const Mat& WT = wt.at({c.comp_of[e], t.table_id(e, u), 0});  // r_e x n1
        w.Mt.push_back(hostla::transpose(hostla::mul(WT, cu.P)));     // r_u x r_e
        w.mtv.push_back(hostla::matvec(WT, cu.p0));
      }
    }
    w.Btx = Mat(n1, std::max(t.ncross, 1));
    for (auto& x : t.xc) {
      if (x.edge != e) continue;
      Ent en{L.xred[x.cross], 1, -1, Mat(1, n1), Mat(1, n1)};
      en.X(0, x.node) = 1.0L;
      for (int k = 0; k < n1; ++k) {
        en.Y(0, k) = ub.Kinv(x.node, k);
        w.Btx(k, x.cross) = ub.Kinv(k, x.node);
      }
      w.ents.push_back(std::move(en));
      w.has_x = true;
    }
    for (size_t u = 0; u < w.ents.size(); ++u) {
      w.rhsv.push_back(hostla::matvec(w.ents[u].Y, g));
      for (size_t v = 0; v <= u; ++v) {
        Mat R = hostla::mul_nt(w.ents[u].Y, w.ents[v].X);
        if (u == v)
          for (int a = 0; a < R.r; ++a)
            for (int b = 0; b < a; ++b) R(a, b) = R(b, a) = (R(a, b) + R(b, a)) / 2;
        w.R.push_back(std::move(R));
      }
    }
  });
  return prework;
}

struct BtTables {
  std::map<int, int> of_id;                // T table id -> B^T table index
  std::vector<std::pair<int, Mat>> extra;  // cross-block tables (index, n1 x ncross)
  int n = 0;
};

// The bookkeeping: appends to the shared lists (p.vecs, p.rhs_terms, p.pre_edges, p.groups, p.cm, smalls, bt) in a fixed
// order.  Returns the flops of the back substitution, or -1 if an edge has more than 8 neighbours.
double closed_form_records(const std::vector<PreWork>& prework, const Topology& t, const Elimination& el, const Compression& c,
                           const Layout& L, FemPlan& p, std::vector<Small>& smalls, BtTables& bt) {
  const int n1p = p.n1p, ncross = t.ncross;
  double pre_flops = 0;
  for (size_t i = 0; i < prework.size(); ++i) {
    const int e = el.pre_list[i];
    const Edge& pe = t.edges[e];
    const bool lr_e = L.cpos[e] >= 0;
    const Comp& cpe = c.comps[c.comp_of[e]];
    const PreWork& pw = prework[i];
    PreEdge P;
    memset(&P, 0, sizeof(P));
    CoefGroup cg;
    memset(&cg, 0, sizeof(cg));
    cg.kind = 1; cg.cpos = L.cpos[e]; cg.r = cpe.r; cg.w = c.rp[c.comp_of[e]]; cg.b0 = pe.b0; cg.b1 = pe.b1;
    bool fits = true;  // at most 8 terms per coefficient group and 8 neighbours per back substitution
    auto add_cterm = [&](int src, int blk, const Mat& Mt, int voff, int u0, int u1) {  // Mt: len x r_e
      if (cg.nterm >= 8) { fits = false; return; }
      cg.t[cg.nterm++] = CoefTerm{src, Mt.r, blk, int(p.cm.size()), voff, u0, u1};
      for (ld v : Mt.v) p.cm.push_back(double(v));
    };
    auto add_nb = [&](PreNb nb) {
      if (P.nnb >= 8) { fits = false; return; }
      P.nb[P.nnb++] = nb;
    };
    P.pos = L.npos[e];
    P.e0 = pe.b0;
    P.e1 = pe.b1;
    P.woff = push_vec(p.vecs, pw.we, n1p);
    size_t nbi = 0;  // neighbour counter (index into pw.Mt / pw.mtv)
    for (int u : t.adj[e]) {
      const int blk = t.shared_block(e, u), id = t.table_id(u, e);
      if (lr_e) {
        // c_e += a_blk * (W_e^T T^(e,u) P_u z_u + W_e^T T^(e,u) p0_u / s_u)
        const int voff = push_vec(p.vecs, pw.mtv[nbi], cpe.r);
        add_cterm(L.zpos[u], blk, pw.Mt[nbi++], voff, t.edges[u].b0, t.edges[u].b1);
        pre_flops += 2.0 * cpe.r * double(c.comps[c.comp_of[u]].r);
      } else {
        if (!bt.of_id.count(id)) bt.of_id[id] = bt.n++;
        add_nb(PreNb{L.npos[u], blk, n1p / BK, bt.of_id[id]});
        pre_flops += 2.0 * n1p * double(n1p);
      }
    }
    for (auto& x : t.xc)
      if (x.edge == e && lr_e) {  // c_e += (s_e / 2) W_e[node, :]^T u_x
        Mat Mt(1, cpe.r);
        for (int k = 0; k < cpe.r; ++k) Mt(0, k) = cpe.W(x.node, k);
        add_cterm(L.xred[x.cross], -1, Mt, -1, 0, 0);
      }
    if (lr_e) p.groups.push_back(cg);
    if (pw.has_x && !lr_e) {
      add_nb(PreNb{L.xb0, -1, (ncross + BK - 1) / BK, bt.n});
      bt.extra.push_back({bt.n++, pw.Btx});
      pre_flops += 2.0 * n1p * double((ncross + BK - 1) / BK * BK);
    }
    if (!fits) return -1;
    size_t ri = 0;
    for (size_t u = 0; u < pw.ents.size(); ++u) {
      const Ent& eu = pw.ents[u];
      p.rhs_terms.push_back(RhsTerm{eu.pos, eu.len, push_vec(p.vecs, pw.rhsv[u], eu.len), eu.blk >= 0 ? 0 : 1,
                                    std::max(eu.blk, 0), pe.b0, pe.b1});
      for (size_t v = 0; v <= u; ++v) {
        const Ent& ev = pw.ents[v];
        const Mat& R = pw.R[ri++];
        if (eu.blk >= 0 && ev.blk >= 0)
          add_small(smalls, eu.pos, ev.pos, R, 4, {std::min(eu.blk, ev.blk), std::max(eu.blk, ev.blk), pe.b0, pe.b1});
        else if (eu.blk >= 0 || ev.blk >= 0)
          add_small(smalls, eu.pos, ev.pos, R, 5, {std::max(eu.blk, ev.blk), 0, 0, 0});
        else
          add_small(smalls, eu.pos, ev.pos, R, 6, {0, 0, pe.b0, pe.b1});
      }
    }
    if (!lr_e) p.pre_edges.push_back(P);
  }
  return pre_flops;
}

// ---- tile mask + symbolic fill: the slots (tiles of the lower triangle) in column order and the update pairs of each;
//      returns the flops of the numeric factorisation ------------------------------------------------------------
double symbolic_cholesky(const std::vector<Small>& smalls, int T, FemPlan& p, std::vector<std::pair<int, int>>& slots) {
  std::vector<char> mask(size_t(T) * T, 0);
  auto M_ = [&](int i, int j) -> char& { return mask[size_t(i) * T + j]; };
  for (int k = 0; k < T; ++k) M_(k, k) = 1;
  for (const Small& s : smalls) for_tiles(s, [&](int tr, int tc) { M_(tr, tc) = M_(tc, tr) = 1; });
  for (int k = 0; k < T; ++k)
    for (int i = k + 1; i < T; ++i)
      if (M_(i, k))
        for (int j = k + 1; j <= i; ++j)
          if (M_(j, k)) M_(i, j) = M_(j, i) = 1;
  p.slot_of.assign(size_t(T) * T, -1);
  p.colptr.assign(T + 1, 0);
  p.diag_slot.assign(T, -1);
  for (int j = 0; j < T; ++j) {
    p.diag_slot[j] = int(slots.size());
    p.slot_of[size_t(j) * T + j] = int(slots.size());
    slots.push_back({j, j});
    for (int i = j + 1; i < T; ++i)
      if (M_(i, j)) {
        p.slot_of[size_t(i) * T + j] = int(slots.size());
        p.colrow.push_back(int(slots.size()));
        p.colti.push_back(i);
        slots.push_back({i, j});
      }
    p.colptr[j + 1] = int(p.colrow.size());
  }
  p.nslots = int(slots.size());
  p.kptr.assign(p.nslots + 1, 0);
  double flops = 0;
  for (int s = 0; s < p.nslots; ++s) {
    const int i = slots[s].first, j = slots[s].second;
    for (int k = 0; k < j; ++k)
      if (M_(i, k) && M_(j, k)) {
        p.kpair.push_back(p.slot_of[size_t(i) * T + k]);
        p.kpair.push_back(p.slot_of[size_t(j) * T + k]);
        flops += 2.0 * TB * TB * TB;
      }
    p.kptr[s + 1] = int(p.kpair.size() / 2);
    flops += (i == j) ? TB * double(TB) * TB / 3.0 : 2.0 * TB * TB * TB;  // potrf | trsm-as-gemm
  }
  return flops;
}

// ---- distribute the blocks over the tiles: one 64x64 table per (tile, coefficient formula).  Takes `smalls` by value:
//      they and the per-slot accumulators (large at 4x4 / N = 256) are gone as soon as the pool is built -------------
bool tile_terms(std::vector<Small> smalls, const std::vector<std::pair<int, int>>& slots, FemPlan& p) {
  std::vector<std::vector<TermAcc>> slot_terms(p.nslots);
  bool inside = true;
  for (const Small& s : smalls)
    for_tiles(s, [&](int tr, int tc) {
      if (tc > tr) return;
      const int slot = p.slot_of[size_t(tr) * p.T + tc];
      if (slot < 0) { inside = false; return; }
      const std::array<int, 5> key{s.kind, s.b[0], s.b[1], s.b[2], s.b[3]};
      TermAcc* ta = nullptr;
      for (auto& cand : slot_terms[slot])
        if (cand.key == key) ta = &cand;
      if (!ta) {
        slot_terms[slot].push_back(TermAcc{key, std::vector<double>(4096, 0.0), TB, 0, TB, 0});
        ta = &slot_terms[slot].back();
      }
      const int i0 = std::max(s.rpos, tr * TB), i1 = std::min(s.rpos + s.tab.r, (tr + 1) * TB);
      const int j0 = std::max(s.cpos, tc * TB), j1 = std::min(s.cpos + s.tab.c, (tc + 1) * TB);
      for (int i = i0; i < i1; ++i)
        for (int j = j0; j < j1; ++j) ta->tab[size_t(i - tr * TB) * TB + (j - tc * TB)] += double(s.tab(i - s.rpos, j - s.cpos));
      ta->r_lo = std::min(ta->r_lo, i0 - tr * TB);
      ta->r_hi = std::max(ta->r_hi, i1 - tr * TB);
      ta->c_lo = std::min(ta->c_lo, j0 - tc * TB);
      ta->c_hi = std::max(ta->c_hi, j1 - tc * TB);
    });
  if (!inside) return false;
  p.desc.resize(p.nslots);
  for (int s = 0; s < p.nslots; ++s) {
    TileDesc d;
    memset(&d, 0, sizeof(d));
    d.ti = slots[s].first;
    d.tj = slots[s].second;
    d.diag = d.ti == d.tj;
    d.ndr = std::max(0, std::min(TB, p.nred - d.ti * TB));
    d.t0 = int(p.terms.size());
    for (auto& ta : slot_terms[s]) {
      GenTerm g;
      g.tab = int(p.pool.size() / 4096);
      g.r_lo = short(ta.r_lo); g.r_hi = short(ta.r_hi); g.c_lo = short(ta.c_lo); g.c_hi = short(ta.c_hi);
      g.kind = ta.key[0];
      for (int q = 0; q < 4; ++q) g.b[q] = ta.key[1 + q];
      p.terms.push_back(g);
      p.pool.insert(p.pool.end(), ta.tab.begin(), ta.tab.end());
    }
    d.t1 = int(p.terms.size());
    p.desc[s] = d;
  }
  return true;
}

// ---- three encodings of the tile assembly ----------------------------------------------------------------------------
// The assembly of a tile as a stream of kilobytes (s_tile_to_lds): wave w of a workgroup owns rows 16 w .. 16 w + 15 as
// 2 x 4 positions of 8 rows x 16 columns; per tile slot and wave, the (position x, term) pieces that meet the term's
// rectangle, sorted by position, the terms of a position in their order; padded to whole rings with no-ops, 128 no-ops behind the end.
void stream_assembly(FemPlan& p) {
  const int RING = 8;
  std::vector<int>& alist = p.alist;
  for (const TileDesc& d : p.desc)
    for (int w = 0; w < 4; ++w) {
      p.aoff.push_back(int(alist.size() / 2));
      if (d.t1 - d.t0 > 128) continue;  // (such a tile takes the register path)
      for (int x = 0; x < 8; ++x) {  // position x = 4 pr + cs: rows 16 w + 8 pr .. + 7, columns 16 cs .. + 15
        const int r0 = 16 * w + 8 * (x >> 2), c0 = 16 * (x & 3);
        const size_t first = alist.size();
        for (int t = d.t0; t < d.t1; ++t) {
          const GenTerm& g = p.terms[t];
          if (!(r0 + 8 > g.r_lo && r0 < g.r_hi && c0 + 16 > g.c_lo && c0 < g.c_hi)) continue;
          alist.push_back(int(size_t(g.tab) * 4096 + size_t(r0) * TB + c0));
          alist.push_back(x | (t - d.t0) << 8);
        }
        if (alist.size() > first) alist.back() |= 1 << 16;  // last piece of this position
      }
      while ((alist.size() / 2 - size_t(p.aoff.back())) % RING) { alist.push_back(0); alist.push_back(1 << 17); }
    }
  p.aoff.push_back(int(alist.size() / 2));
  for (int i = 0; i < 128; ++i) { alist.push_back(0); alist.push_back(1 << 17); }
}

// the whole reduced solve in one wave (k_solve1) if the reduced matrix is a single tile; its assembly walks
// the (term, 16x16 block) pairs whose rectangle and block intersect
void single_tile_pairs(FemPlan& p) {
  const TileDesc& d0 = p.desc[0];
  std::vector<int>& pairs = p.pairs;
  int q = 0;
  for (int ib = 0; ib < 4; ++ib)
    for (int jb = 0; jb <= ib; ++jb, ++q) {  // sorted by block: the kernel keeps a block's sum in registers
      const size_t first = pairs.size();
      for (int t = d0.t0; t < d0.t1; ++t) {
        const GenTerm& g = p.terms[t];
        bool any = false;  // (skip blocks where the table is all zero inside the rectangle, too)
        for (int r = std::max<int>(g.r_lo, 16 * ib); r < std::min<int>(g.r_hi, 16 * ib + 16) && !any; ++r)
          for (int c = std::max<int>(g.c_lo, 16 * jb); c < std::min<int>(g.c_hi, 16 * jb + 16); ++c)
            if (p.pool[size_t(g.tab) * 4096 + size_t(r) * TB + c] != 0.0) { any = true; break; }
        if (!any) continue;
        pairs.push_back(int(size_t(g.tab) * 4096 + size_t(16 * ib) * TB + 16 * jb));
        pairs.push_back((t - d0.t0) | (q << 8));
      }
      if (pairs.size() > first) pairs.back() |= 1 << 16;  // last pair of this block
    }
}

// k_solve1 runs four systems per workgroup and deals the BLOCKS to its four waves (largest first, to the wave with the
// fewest pairs so far); wave w walks pairs wp0[w] .. wp0[w + 1] - 1 of `wmeta`, whose table pieces lie in the same order in
// `pool_acc`: piece = the 16 x 16 block of the pair's table in the accumulator layout of its consumer,
// [g pair h][lane][e] = table(16 ib + 4 (2 h + e) + (lane >> 4), 16 jb + (lane & 15))
void wave_walks(FemPlan& p) {
  const std::vector<int>& pairs = p.pairs;
  const int npr = int(pairs.size() / 2);
  std::vector<std::vector<int>> of_block(10), blocks_of(4);
  for (int i = 0; i < npr; ++i) of_block[(pairs[2 * i + 1] >> 8) & 0xff].push_back(i);
  std::vector<int> by_size(10), load(4, 0);
  for (int q = 0; q < 10; ++q) by_size[q] = q;
  std::stable_sort(by_size.begin(), by_size.end(), [&](int x, int y) { return of_block[x].size() > of_block[y].size(); });
  for (int q : by_size) {
    const int w = int(std::min_element(load.begin(), load.end()) - load.begin());
    blocks_of[w].push_back(q);
    load[w] += int(of_block[q].size());
  }
  for (int w = 0; w < 4; ++w) {
    std::sort(blocks_of[w].begin(), blocks_of[w].end());
    p.wp0[w] = int(p.wmeta.size());
    for (int q : blocks_of[w])
      for (int i : of_block[q]) {
        p.wmeta.push_back(pairs[2 * i + 1]);
        const size_t o = p.pool_acc.size();
        p.pool_acc.resize(o + 256);
        for (int h = 0; h < 2; ++h)
          for (int lane = 0; lane < 64; ++lane)
            for (int e = 0; e < 2; ++e)
              p.pool_acc[o + h * 128 + lane * 2 + e] = p.pool[size_t(pairs[2 * i]) + size_t(4 * (2 * h + e) + (lane >> 4)) * TB + (lane & 15)];
      }
    while ((int(p.wmeta.size()) - p.wp0[w]) % PAIR_RING) {  // the walk goes PAIR_RING pairs at a time: no-ops (weight 0) on zero pieces
      p.wmeta.push_back(COEF_MAX - 1);
      p.pool_acc.resize(p.pool_acc.size() + 256, 0.0);
    }
  }
  p.wp0[4] = int(p.wmeta.size());
  p.wmeta.resize(p.wmeta.size() + 128, COEF_MAX - 1);              // no-ops (the walk reads its metas 64 at a time, one group ahead)
  p.pool_acc.resize(p.pool_acc.size() + 2 * PAIR_RING * 256, 0.0);  // the fetches that run ahead of the walk
}

void single_tile_assembly(FemPlan& p) {
  p.fused1 = p.T == 1 && p.desc[0].t1 - p.desc[0].t0 < COEF_MAX && p.nGa == TB;
  if (p.fused1) {
    single_tile_pairs(p);
    wave_walks(p);
  }
  p.npairs = int((p.pairs.size() / 2 + 63) / 64 * 64);
  // no-op padding: term slot COEF_MAX - 1 is never a real term (its weight is 0), block 0 of the first table
  while (int(p.pairs.size() / 2) < p.npairs + 64) { p.pairs.push_back(0); p.pairs.push_back(COEF_MAX - 1); }
}

// ---- vmap, parameter-independent part of the reduced rhs, scalar block, positions copied without expansion ---------
void interface_maps(const Topology& t, const Elimination& el, const Compression& c, const Layout& L, FemPlan& p) {
  const int N = t.N, n1 = t.n1;
  p.vmap.assign(std::max(L.nGp, 1), -1);
  for (int e = 0; e < t.E; ++e) {
    const Edge& ed = t.edges[e];
    for (int k = 0; k < n1; ++k) {
      int r, cc;  // 1-based inner vertex coordinates
      if (ed.hv == 0) { r = ed.p * N; cc = ed.q * N + k + 1; }
      else { r = ed.p * N + k + 1; cc = ed.q * N; }
      p.vmap[L.npos[e] + k] = (r - 1) * p.nc + (cc - 1);
    }
  }
  for (int x = 0; x < t.ncross; ++x) p.vmap[L.xb0 + x] = (t.crosses[x].first * N - 1) * p.nc + (t.crosses[x].second * N - 1);
  p.g_red.assign(std::max(L.nGa, 1), 0.0);
  for (int e : el.order) {
    const Comp& ce = c.comps[c.comp_of[e]];
    for (int k = 0; k < ce.r; ++k) p.g_red[L.zpos[e] + k] = double(ce.gt[k]);
  }
  for (int x = 0; x < t.ncross; ++x) p.g_red[L.xred[x]] = 1.0 / (double(N) * double(N));
  // (b0, b1) per scalar: an edge's two blocks, or (block, -1)
  for (int e = 0; e < t.E; ++e) { p.scb.push_back(t.edges[e].b0); p.scb.push_back(t.edges[e].b1); }
  for (int b = 0; b < t.nrb * t.ncb; ++b) { p.scb.push_back(b); p.scb.push_back(-1); }
  std::vector<char> expanded(t.E, 0);
  for (int e : el.order) expanded[e] = 1;
  for (int e : el.pre_list)
    if (L.cpos[e] >= 0) expanded[e] = 1;
  for (int e = 0; e < t.E; ++e)
    if (!expanded[e])
      for (int k = 0; k < n1; ++k) p.scat.push_back(L.npos[e] + k);
  for (int x = 0; x < t.ncross; ++x) p.scat.push_back(L.xb0 + x);
}

// ---- expansion tables of the active edges and of the closed-form edges kept compressed, their coefficient groups ------
void expansion_records(const Topology& t, const Elimination& el, const Compression& c, const Layout& L, FemPlan& p) {
  // table variants of a compressed-edge type: 0 = active edge (P, p0), 1 = closed-form edge (K^-1 W, K^-1 g)
  std::map<std::pair<int, int>, int> ptab_of, p0_of;
  std::vector<std::pair<int, int>> ptab_list;
  auto variant = [&](int k, int v) {
    if (!ptab_of.count({k, v})) {
      ptab_of[{k, v}] = int(ptab_list.size());
      ptab_list.push_back({k, v});
      p0_of[{k, v}] = push_vec(p.vecs, v == 0 ? c.comps[k].p0 : c.comps[k].wK, p.n1p);
    }
    return ptab_of[{k, v}];
  };
  for (int e : el.order) {
    const int k = c.comp_of[e], pt = variant(k, 0);
    p.exps.push_back(ExpEdge{L.zpos[e], (L.rk[e] + BK - 1) / BK, L.npos[e], pt, p0_of[{k, 0}], L.spos0 + e});
    if (L.cpos[e] >= 0) {
      CoefGroup cg;
      memset(&cg, 0, sizeof(cg));
      cg.kind = 0; cg.cpos = L.cpos[e]; cg.r = L.rk[e]; cg.w = c.rp[k]; cg.b0 = t.edges[e].b0; cg.b1 = t.edges[e].b1; cg.zpos = L.zpos[e];
      p.groups.push_back(cg);
    }
  }
  for (int e : el.pre_list)
    if (L.cpos[e] >= 0) {
      const int k = c.comp_of[e], pt = variant(k, 1);
      p.exps.push_back(ExpEdge{L.cpos[e], (c.comps[k].r + BK - 1) / BK, L.npos[e], pt, p0_of[{k, 1}], L.spos0 + e});
    }
  p.Ptab.assign(std::max<size_t>(ptab_list.size() * size_t(p.n1p) * p.n1p, 1), 0.0);
  for (size_t k = 0; k < ptab_list.size(); ++k) {
    const Comp& cp = c.comps[ptab_list[k].first];
    put_table(p.Ptab, k, p.n1p, ptab_list[k].second == 0 ? cp.P : cp.KiW, false);
  }
}

// k_coef spreads the dot products of the closed-form blocks over its workgroup: tasks (group, entry k, term t) ordered by
// (group, term, k) -- neighbouring threads read neighbouring entries of a matrix row -- as flat records (rom_fem_dev.h)
void coef_tasks(FemPlan& p) {
  const std::vector<CoefGroup>& groups = p.groups;
  for (size_t g = 0; g < groups.size(); ++g)
    for (int k = 0; k < groups[g].w; ++k) { p.item_group.push_back(int(g)); p.item_k.push_back(k); }
  p.ncoef = int(p.item_group.size());
  p.item_cf.assign(p.item_group.size(), -1);
  std::vector<int> first_cf(groups.size(), -1);
  p.ncf = 0;
  for (size_t it = 0; it < p.item_group.size(); ++it) {
    const CoefGroup& cg = groups[p.item_group[it]];
    if (cg.kind == 1 && p.item_k[it] < cg.r) {
      if (first_cf[p.item_group[it]] < 0) first_cf[p.item_group[it]] = p.ncf;
      p.item_cf[it] = p.ncf++;
    }
  }
  for (size_t g = 0; g < groups.size(); ++g)
    if (groups[g].kind == 1)
      for (int t = 0; t < groups[g].nterm; ++t)
        for (int k = 0; k < groups[g].r; ++k) {
          const CoefTerm& ct = groups[g].t[t];
          const int rec[8] = {ct.moff + k, ct.src, ct.len, groups[g].r, ct.voff >= 0 ? ct.voff + k : -1, ct.u0, ct.u1, (first_cf[g] + k) * 8 + t};
          p.ctask.insert(p.ctask.end(), rec, rec + 8);
        }
  p.nctask = int(p.ctask.size() / 8);
}

// single-tile path: the coefficient blocks of the closed-form edges as one dense product (k_solve1); drops fused1
// where a limit of that kernel is exceeded
void dense_single_tile(FemPlan& p) {
  const std::vector<CoefGroup>& groups = p.groups;
  std::vector<std::pair<int, int>> dsrc;  // (group index in `groups`, first item)
  for (size_t g = 0; g < groups.size(); ++g)
    if (groups[g].kind == 1) {
      DenseGroup dg;
      memset(&dg, 0, sizeof(dg));
      dg.cpos = groups[g].cpos; dg.r = groups[g].r; dg.b0 = groups[g].b0; dg.b1 = groups[g].b1;
      dsrc.push_back({int(g), int(p.ditem_group.size())});
      for (int k = 0; k < groups[g].r; ++k) { p.ditem_group.push_back(int(p.dgroups.size())); p.ditem_k.push_back(k); }
      p.dgroups.push_back(dg);
    }
  const int ndi = int(p.ditem_group.size());
  p.dmat.assign(size_t(TB) * std::max(ndi, 1) + 128, 0.0);  // (+ 1 KB: k_solve1 copies it to LDS in whole kilobytes)
  p.dweight.assign(p.dgroups.size() * TB, -2);
  // (k_solve1: a lane per rhs term / per block coefficient)
  bool ok = p.fused1 && int(p.dgroups.size()) <= DENSE_GROUPS_MAX && p.rhs_terms.size() <= 64 && p.nrb * p.ncb <= 64 && ndi <= 64;
  for (size_t dgi = 0; dgi < p.dgroups.size() && ok; ++dgi) {
    const CoefGroup& cg = groups[dsrc[dgi].first];
    for (int t = 0; t < cg.nterm && ok; ++t) {
      const CoefTerm& ct = cg.t[t];
      for (int j = 0; j < ct.len; ++j) {
        if (ct.src + j >= TB) { ok = false; break; }
        p.dweight[dgi * TB + ct.src + j] = ct.blk >= 0 ? ct.blk : -1;
        for (int k = 0; k < cg.r; ++k) p.dmat[size_t(ct.src + j) * ndi + dsrc[dgi].second + k] = p.cm[ct.moff + size_t(j) * cg.r + k];
      }
      if (ct.voff >= 0) {
        DenseGroup& dg = p.dgroups[dgi];
        if (dg.nv >= 4) { ok = false; break; }
        dg.voff[dg.nv] = ct.voff; dg.vblk[dg.nv] = ct.blk; dg.vu0[dg.nv] = ct.u0; dg.vu1[dg.nv] = ct.u1;
        ++dg.nv;
      }
    }
  }
  if (!ok) p.fused1 = false;
  p.ndg = p.fused1 ? int(p.dgroups.size()) : 0;
  p.ndi = p.fused1 ? ndi : 0;
  // k_solve1 reads one FLAT record per item and lane (every level of indirection is a memory round trip a lone wave waits
  // out): dense item = {group, position, nv, b0, b1, voff[4] + k, vblk[4], vu0[4], vu1[4], pad} (24 ints);
  // coefficient item = {position | code << 28, source, b0, b1}, code 0 = the dense product's, 1 = 1 / (a_b0 + a_b1),
  // 2 = copy of the solution, 3 = zero
  p.s1_items.assign(size_t(std::max(ndi, 1)) * 24, 0);
  p.s1_citems.assign(size_t(std::max(p.ncoef, 1)) * 4, 0);
  if (!p.fused1) return;
  for (int it = 0; it < ndi; ++it) {
    const DenseGroup& dg = p.dgroups[p.ditem_group[it]];
    int* r = &p.s1_items[size_t(it) * 24];
    r[0] = p.ditem_group[it]; r[1] = dg.cpos + p.ditem_k[it]; r[2] = dg.nv; r[3] = dg.b0; r[4] = dg.b1;
    for (int v = 0; v < 4; ++v) {
      r[5 + v] = v < dg.nv ? dg.voff[v] + p.ditem_k[it] : 0;
      r[9 + v] = v < dg.nv ? dg.vblk[v] : 0; r[13 + v] = v < dg.nv ? dg.vu0[v] : 0; r[17 + v] = v < dg.nv ? dg.vu1[v] : 0;
    }
  }
  for (int it = 0; it < p.ncoef; ++it) {
    const CoefGroup& cg = groups[p.item_group[it]];
    const int k = p.item_k[it];
    const int code = cg.kind == 1 && k < cg.r ? 0 : k == cg.r ? 1 : k < cg.r ? 2 : 3;
    int* r = &p.s1_citems[size_t(it) * 4];
    r[0] = (cg.cpos + k) | code << 28; r[1] = cg.zpos + k; r[2] = cg.b0; r[3] = cg.b1;
  }
}

// ---- tables of the unit block: back substitution (B^T), sine matrix, rho, W = L^-1 1 ------------------------------------
void unit_block_tables(UnitBlock& ub, const BtTables& bt, FemPlan& p) {
  const int n1 = p.n1, n1p = p.n1p;
  p.Bt.assign(std::max<size_t>(size_t(bt.n) * n1p * n1p, 1), 0.0);
  for (auto& kv : bt.of_id) put_table(p.Bt, kv.second, n1p, ub.TK(kv.first), true);  // (T K^-1)^T: row = node of e
  for (auto& kv : bt.extra) put_table(p.Bt, kv.first, n1p, kv.second, false);
  p.Qp.assign(size_t(n1p) * n1p, 0.0);
  for (int j = 0; j < n1; ++j)
    for (int m = 0; m < n1; ++m) p.Qp[size_t(j) * n1p + m] = double(ub.Q(j, m));
  p.rho = ub.rho_d;
  p.Wz = ub.Wd;  // + a page of zeros: where k_extend128 points the lanes that have nothing to load
  p.Wz.resize(ub.Wd.size() + EXT_ZERO_PAGE, 0.0);
}

// ---- Representation of every block side in the extension.  A compressed edge enters through its reduced
// unknowns when that is cheaper than the distance-truncated sine modes: table G_c = H_0 [P_c, p0_c]
// = A0 (Q [P_c, p0_c]), one (n1*n1) x rp_c table per (compressed-edge type, variant) that a block side actually uses.
// Here: the sine coefficients Q^T [P_c, p0_c] of every table: long-double products, one host thread per table.
using GOffsets = std::map<std::pair<int, int>, long long>;  // (type, variant) -> offset in G

// Rotated basis: the stored coefficients below the echelon are exact zeros (in long double they are rounding residue of about
// 1e-18 of the table, far below what fp64 keeps -- but multiplied by rho ~ 1 of the low modes they would defeat the bound).
// Column k of the table at distance d from the side is bounded by sqrt(2/N) b(k, d), b(k, d) = sum_m rho_m(d) |Bh[k][m]|;
// a column is needed at d while b(k, d) reaches 1e-18 of the largest b(k, 1) -- the cut kmax applies to rho itself.
// seg0[d]: the first 8-wide segment that holds a needed column (b falls with d, so seg0 rises); the last segment, with
// 1/s, is always walked.  thr[j] = the first distance with seg0 > j.
void ext_truncation(const UnitBlock& ub, const Comp& cp, int n1p, FemPlan::GemmG& g) {
  const int n1 = ub.n1, N = ub.N, r = cp.r, nseg = segs8(r);
  g.entry = cp.entry;
  g.W = cp.W.v;
  for (int k = 0; k < r; ++k)
    for (int m = 0; m < std::min(cp.entry[k], n1); ++m) g.Bh[size_t(k) * n1p + m] = 0.0;
  auto bound = [&](int k, int d) {
    ld b = 0;
    for (int m = 0; m < n1; ++m) b += ub.rho(m, d) * fabsl(ld(g.Bh[size_t(k) * n1p + m]));
    return b;
  };
  ld top = 0;
  for (int k = 0; k < r; ++k) top = std::max(top, bound(k, 1));
  const ld cut = EXT_TRUNC_CUT * top;
  g.cut = double(cut);
  for (int d = 1; d <= n1; ++d) {
    int first = 0;
    while (first < r && bound(first, d) < cut) ++first;
    g.seg0[d] = std::min({first / 8, nseg - 1, EXT_THRESHOLDS});
  }
  g.seg0[N] = g.seg0[n1];
  for (int j = 0; j < EXT_THRESHOLDS; ++j)
    for (int d = n1; d >= 1; --d)
      if (g.seg0[d] > j) g.thr[j] = (unsigned short)d;
}
GOffsets g_tables(const UnitBlock& ub, const Topology& t, const Elimination& el, const Compression& c, const Layout& L, FemPlan& p) {
  const int n1 = t.n1, n1p = p.n1p;
  GOffsets goff;
  for (int e = 0; e < t.E; ++e)
    if (L.cpos[e] >= 0 && !goff.count({c.comp_of[e], int(el.is_pre[e])})) {
      goff[{c.comp_of[e], int(el.is_pre[e])}] = p.gtotal;
      p.gtotal += (long long)n1 * n1 * c.rp[c.comp_of[e]];
    }
  for (auto& kv : goff) p.gemm_G.push_back({{}, kv.second, c.rp[kv.first.first]});
  std::vector<std::pair<int, int>> gkeys;
  for (auto& kv : goff) gkeys.push_back(kv.first);
  parallel_for(gkeys.size(), [&](size_t gi) {
    const Comp& cp = c.comps[gkeys[gi].first];
    const Mat& Pm = gkeys[gi].second == 0 ? cp.P : cp.KiW;
    const std::vector<ld>& pv = gkeys[gi].second == 0 ? cp.p0 : cp.wK;
    Mat Bm = hostla::mul_tn(Pm, ub.Q);  // r x n1
    std::vector<double>& Bh = p.gemm_G[gi].Bh;
    Bh.assign(size_t(p.gemm_G[gi].rp) * n1p, 0.0);
    for (int k = 0; k < cp.r; ++k)
      for (int m = 0; m < n1; ++m) Bh[size_t(k) * n1p + m] = double(Bm(k, m));
    for (int m = 0; m < n1; ++m) {
      ld sacc = 0;
      for (int k = 0; k < n1; ++k) sacc += pv[k] * ub.Q(k, m);
      Bh[size_t(cp.r) * n1p + m] = double(sacc);
    }
    p.gemm_G[gi].r = cp.r;
    p.gemm_G[gi].seg0.assign(t.N + 1, 0);
    if (!cp.entry.empty()) ext_truncation(ub, cp, n1p, p.gemm_G[gi]);
  });
  return goff;
}

// the sides of every block, the segment-major copies k_extend128 reads, the edges whose sine coefficients are needed and
// the flops of the extension per system (algorithmic: no padding of K or of the vertex tiles)
void extension_sides(const Topology& t, const Elimination& el, const Compression& c, const Layout& L, const GOffsets& goff, FemPlan& p) {
  const int n1 = t.n1, N = t.N;
  const long long hrows = (long long)n1 * n1;
  p.sides.resize(t.nrb * t.ncb);
  std::map<std::tuple<int, int, int>, long long> gsoff;  // (type, variant, orientation) -> offset in Gs
  std::vector<char> need_tr(t.E, 0);
  double fl = 0;
  const int npj = (n1 + 15) / 16, npi = (n1 + 3) / 4;
  for (int b = 0; b < t.nrb * t.ncb; ++b)
    for (int sdx = 0; sdx < 4; ++sdx) {
      ExtSide& es = p.sides[b].s[sdx];
      memset(&es, 0, sizeof(es));
      const int e = t.bside[b][sdx];
      if (e < 0) continue;
      const int k = c.comp_of[e], r = c.comps[k].r;
      if (L.cpos[e] >= 0) {
        es = ExtSide{2, L.cpos[e], c.rp[k] / BK, r, int(goff.at({k, int(el.is_pre[e])})), 0, t.edges[e].b0, t.edges[e].b1, {}};
        // segment-major copy for k_extend128: rows ordered for this side's orientation (one per table and orientation)
        const auto key = std::make_tuple(k, int(el.is_pre[e]), sdx >= 2 ? 1 : 0);
        if (!gsoff.count(key)) {
          gsoff[key] = p.gstotal;
          p.gstotal += (long long)segs8(r) * hrows * 8;
        }
        es.gseg = int(gsoff[key]);
        const FemPlan::GemmG* gg = nullptr;
        for (const FemPlan::GemmG& cand : p.gemm_G)
          if (cand.off == es.gtab) gg = &cand;
        memcpy(es.thr, gg->thr, sizeof(es.thr));
        if (gg->entry.empty()) {
          fl += 2.0 * double(n1) * n1 * (r + 1);
        } else {  // the products the rows at distance d need: the columns from the first needed segment on
          for (int d = 1; d <= n1; ++d) fl += 2.0 * double(n1) * (r + 1 - 8 * gg->seg0[d]);
        }
      } else {
        es.mode = 1;
        es.off = L.npos[e];
        need_tr[e] = 1;
        for (int pi = 0; pi < npi; ++pi)
          for (int pj = 0; pj < npj; ++pj) {
            int i0 = 4 * pi + 1, j0 = 16 * pj + 1, i1 = std::min(i0 + 3, n1), j1 = std::min(j0 + 15, n1);
            int dist[4] = {i0, N - i1, j0, N - j1};
            fl += 2.0 * 64 * c.kmax[dist[sdx]];
          }
      }
    }
  for (auto& kv : gsoff) {
    const int k = std::get<0>(kv.first);
    p.repacks.push_back({goff.at({k, std::get<1>(kv.first)}), kv.second, c.rp[k], segs8(c.comps[k].r), std::get<2>(kv.first)});
  }
  for (int e = 0; e < t.E; ++e)
    if (need_tr[e]) p.epos.push_back(L.npos[e]);
  p.n_edges = int(p.epos.size());
  if (p.epos.empty()) p.epos.push_back(0);
  p.ext_flops = fl + 2.0 * p.n_edges * double(p.n1p) * p.n1p;
}

// blocks whose sides are all compressed go to k_extend128, the others to k_extend
void split_blocks(bool no_ext_lr, FemPlan& p) {
  p.lr_nch = 0;
  for (int b = 0; b < p.nrb * p.ncb; ++b) {
    int nlr = 0, nother = 0, nch = 0;
    for (const ExtSide& es : p.sides[b].s) {
      if (es.mode == 2) { ++nlr; nch += es.nch; }
      else if (es.mode != 0) ++nother;
    }
    if (nlr > 0 && nother == 0 && !no_ext_lr) {
      p.lr_blocks.push_back(b);
      p.lr_nch = std::max(p.lr_nch, nch);
    } else {
      p.gen_blocks.push_back(b);
    }
  }
}

// the per-tile records of k_extend128 (X128Tile, rom_fem_plan.h), both tilings
void x128_tiles(FemPlan& p) {
  const int n1 = p.n1, t_row = n1 * ((n1 + 127) / 128), t_flat = (n1 * n1 + 127) / 128;
  for (int b : p.lr_blocks) {
    for (int t = 0; t < t_row; ++t) p.x128_row.push_back(x128_tile_plan<false>(n1, p.N, b, t, p.sides[b]));
    for (int t = 0; t < t_flat; ++t) p.x128_flat.push_back(x128_tile_plan<true>(n1, p.N, b, t, p.sides[b]));
  }
}

// ---- every ROMHC_VERBOSE line ---------------------------------------------------------------------------------------
void report(const FemPlan& p, const Compression& c) {
  {
    size_t real = 0;
    for (size_t i = 1; i < p.alist.size(); i += 2) real += (p.alist[i] >> 17) ? 0 : 1;
    fprintf(stderr, "romhc:   tile assembly as a stream: %zu KB per system and sweep in pieces of 8 rows x 16 columns\n", real);
  }
  {  // what the assembly of the tiles reads: 128-byte strips (one thread-row x 16 columns) that meet a term's rectangle
    double strips = 0, tiles_diag = 0, tiles_sub = 0, nterm = 0;
    for (const TileDesc& d : p.desc) {
      (d.ti == d.tj ? tiles_diag : tiles_sub) += 1;
      for (int t = d.t0; t < d.t1; ++t) {
        const GenTerm& g = p.terms[t];
        nterm += 1;
        for (int r = g.r_lo; r < g.r_hi; ++r)
          for (int c0 = 0; c0 < 64; c0 += 16)
            if (c0 < g.c_hi && c0 + 16 > g.c_lo) strips += 1;
      }
    }
    fprintf(stderr, "romhc:   tile assembly: %.0f diagonal + %.0f sub-diagonal tiles, %.0f terms, %.1f KB of table strips per system and sweep\n",
            tiles_diag, tiles_sub, nterm, strips * 128 / 1024);
  }
  fprintf(stderr, "romhc: %dx%d blocks N=%d: %d edges (%d closed-form, %d of them compressed), reduced size %d -> %d tiles, "
                  "%d slots, %zu terms, kavg %.1f\n", p.nrb, p.ncb, p.N, p.n_all_edges, p.npre_all, p.npre_all - int(p.pre_edges.size()),
          p.nred, p.T, p.nslots, p.terms.size(), c.kavg);
  for (size_t k = 0; k < c.comps.size(); ++k)
    fprintf(stderr, "romhc:   edge type %zu: rank %d (padded %d), %d edges, extension %s\n", k, c.comps[k].r, c.rp[k],
            int(std::count(c.comp_of.begin(), c.comp_of.end(), int(k))), c.use_lr[k] ? "from the reduced unknowns" : "sine modes");
  for (size_t i = 0; i < p.gemm_G.size(); ++i) {  // K segments of k_extend128 per mesh row parallel to the side: needed against full
    const FemPlan::GemmG& g = p.gemm_G[i];
    const int full = segs8(g.r);
    long long need = 0;
    for (int d = 1; d <= p.n1; ++d) need += full - g.seg0[d];
    fprintf(stderr, "romhc:   extension table %zu: rank %d, %s basis, K segments needed %lld of %lld (%.2f)\n", i, g.r,
            g.entry.empty() ? "pivoted" : "echelon", need, (long long)full * p.n1, p.n1 > 0 ? double(need) / (double(full) * p.n1) : 1.0);
  }
  fprintf(stderr, "romhc:   blocks extended by the 128-tile kernel: %d, general kernel: %d\n", int(p.lr_blocks.size()), int(p.gen_blocks.size()));
  // how sparse the term tables are: non-zero 16 x 16 blocks, bounding rectangles
  size_t nzb = 0, rect = 0, rows16 = 0;
  for (const GenTerm& g : p.terms) {
    const double* tb = p.pool.data() + size_t(g.tab) * 4096;
    rect += size_t(g.r_hi - g.r_lo) * size_t(g.c_hi - g.c_lo);
    for (int ib = 0; ib < 4; ++ib)
      for (int jb = 0; jb < 4; ++jb) {
        bool nz = false;
        for (int i = 0; i < 16 && !nz; ++i)
          for (int j = 0; j < 16; ++j)
            if (tb[(16 * ib + i) * 64 + 16 * jb + j] != 0.0) { nz = true; break; }
        nzb += nz;
      }
    for (int r = 0; r < 64; ++r)
      for (int sg = 0; sg < 4; ++sg) {
        bool nz = false;
        for (int j = 0; j < 16; ++j) nz = nz || tb[r * 64 + 16 * sg + j] != 0.0;
        rows16 += nz;
      }
  }
  const size_t nt = p.terms.size();
  fprintf(stderr, "romhc:   term tables: %zu tables, %zu non-zero 16x16 blocks of %zu (%.2f), bounding rectangles cover %.2f, non-zero 1x16 strips %.2f\n",
          nt, nzb, nt * 16, double(nzb) / (nt * 16), double(rect) / (nt * 4096.0), double(rows16) / (nt * 256.0));
}

// ROMHC_VERBOSE: wall time of the phases of rom_fem_plan
struct PhaseTimer {
  bool on;
  const char* name = nullptr;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  void next(const char* n) {
    const auto t1 = std::chrono::steady_clock::now();
    if (on && name) fprintf(stderr, "romhc:   [%7.3f s] %s\n", std::chrono::duration<double>(t1 - t0).count(), name);
    name = n;
    t0 = t1;
  }
};

}  // namespace

int rom_fem_plan(int nrb, int ncb, int N, const FemSwitches& sw, FemPlan* out, std::string* error) {
  FemPlan& p = *out;
  p = FemPlan();
  auto fail = [&](const char* why) { *error = why; return ROM_ERR_INVALID; };
  PhaseTimer phase{sw.verbose};
  phase.next("topology");
  const Topology t = make_topology(nrb, ncb, N);
  const int n1 = N - 1, n1p = (n1 + TB - 1) / TB * TB;
  p.nrb = nrb; p.ncb = ncb; p.N = N; p.n1 = n1; p.n1p = n1p;
  p.nr = nrb * N - 1;
  p.nc = ncb * N - 1;
  p.dim = int64_t(p.nr) * p.nc;
  p.nG = t.E * n1 + t.ncross;
  p.ncross = t.ncross;
  p.n_all_edges = t.E;
  phase.next("elimination order");
  const Elimination el = choose_elimination(t, sw.no_preelim);
  p.npre_all = int(el.pre_list.size());
  phase.next("unit-block tables in long double, compression of the edges");
  UnitBlock ub(N, t.E > 0);
  Compression c;
  edge_types(t, el, !sw.no_ext_trunc && !sw.no_compress, c);
  if (!compress_edges(ub, t, el, sw, c)) return fail("internal: compressed edge block not positive definite");
  extension_ranks(ub, n1p, sw.no_lowrank_ext, c);
  p.kmax = c.kmax;
  phase.next("layout of the interface vector");
  const Layout L = make_layout(t, el, c, n1p);
  p.nred = L.nred; p.T = L.T; p.nGa = L.nGa; p.xb0 = L.xb0; p.nGp = L.nGp; p.spos0 = L.spos0; p.nsc = L.nsc;
  p.xred = L.xred;
  for (int e : el.order) p.ranks.push_back(L.rk[e]);
  std::vector<Small> smalls;
  BtTables bt;
  double pre_flops;
  {
    phase.next("W^T T products");
    const WtCache wt = wt_products(ub, t, el, c, L);
    phase.next("blocks of the reduced matrix");
    smalls = reduced_blocks(t, el, c, L, wt);
    phase.next("closed-form edges");
    pre_flops = closed_form_records(closed_form_products(ub, t, el, c, L, wt), t, el, c, L, p, smalls, bt);
    if (pre_flops < 0) return fail("internal: more than 8 neighbours of an eliminated edge");
  }
  phase.next("tile mask + symbolic fill");
  std::vector<std::pair<int, int>> slots;
  const double chol_flops = symbolic_cholesky(smalls, L.T, p, slots);
  phase.next("tile terms and pool");
  if (!tile_terms(std::move(smalls), slots, p)) return fail("internal: reduced-matrix block outside the tile mask");
  phase.next("assembly encodings");
  stream_assembly(p);
  single_tile_assembly(p);
  phase.next("interface maps, expansion, coefficient groups");
  interface_maps(t, el, c, L, p);
  expansion_records(t, el, c, L, p);
  coef_tasks(p);
  dense_single_tile(p);
  unit_block_tables(ub, bt, p);
  phase.next("extension sides");
  const GOffsets goff = g_tables(ub, t, el, c, L, p);
  extension_sides(t, el, c, L, goff, p);
  if (p.gtotal >= (1ll << 31) || p.gstotal >= (1ll << 31)) return fail("rom_fem_create: extension tables too large");
  split_blocks(sw.no_ext_lr, p);
  x128_tiles(p);
  phase.next("end");
  if (sw.verbose) report(p, c);
  // ---- work accounting of this algorithm, per snapshot solve ------------------------------------------------
  double exp_flops = 0;
  for (int e : el.order) exp_flops += 2.0 * n1p * double((L.rk[e] + BK - 1) / BK * BK);
  const double back_flops = 2.0 * 4096.0 * (p.nslots + L.T);
  p.flops_solve = chol_flops + p.ext_flops + back_flops + pre_flops + exp_flops;
  // HBM bytes: factor tiles written once + read once by the back substitution, inverse tiles w+r,
  // the snapshot row written once, the coefficients read.
  p.bytes_solve = 8.0 * (2.0 * 4096.0 * p.nslots + 2.0 * 4096.0 * L.T + double(p.dim) + nrb * ncb);
  return ROM_OK;
}
