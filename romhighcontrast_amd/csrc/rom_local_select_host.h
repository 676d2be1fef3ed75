// rom_local_select as host and device share it: the limits, the LDS carve-up of the fit kernel, the OUT row and the packing of the
// boxes.  (internal; no HIP call: compiles with a plain C++ compiler, which is how tests/c_abi/local_select_host_check.cpp checks
// it)
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#ifdef __HIPCC__
#define LS_HD __host__ __device__
#else
#define LS_HD
#endif

constexpr int LS_NMAX = 64, LS_KMAX = 16, LS_RMAX = 96, LS_KCMAX = 256;
constexpr int LS_KMAX_VECTORS = 1 << 23;     // vectors per call: the x extent of the fit kernel's grid, 256 threads each
constexpr int LS_HLD = LS_NMAX + 1;          // row stride of the factor (BV_LD of rom_bvls_sys.h)
constexpr int LS_LDS_BYTES = 64 * 1024;      // what a workgroup gets without opting in; it bounds rank
constexpr int LS_LAUNCHES = 3;               // G_j^T G_j, fit, pick: whatever K and kc are

// status of a system (OUT column n + k + 4), and the bits of a cluster's word after the Gram kernel
enum { LS_BAD_STATE = 1, LS_BAD_PARAM = 2, LS_OPEN_STATE = 4, LS_OPEN_PARAM = 8 };

// OUT row of system (i, j), in doubles: c (n) | a (k) | S | misfit | passes of the state solve | of the parameter solve | status
struct LsRow {
  int c, a, S, misfit, passes, status, total;
  LS_HD LsRow(int n, int k) { c = 0, a = n, S = n + k, misfit = S + 1, passes = S + 2, status = S + 4, total = S + 5; }
};

// The LDS map of k_local_fit, in doubles.  `mat` holds the factor of the state solve (n rows of LS_HLD) and, once that solve is
// over, the factor of the parameter solve (k rows of LS_HLD) followed by B (rank x k); the vectors serve both solves in turn.
struct LsLds {
  int nm, rm;   // max(n, k), max(r, rank)
  int mat, B, gram3, invd, c, z, v, gn, part, ps, rs, flag, c1, scal, ints, total;
  long long bytes;
  LS_HD LsLds(int n, int k, int rank, int r) {
    nm = n > k ? n : k, rm = r > rank ? r : rank;
    long long at = 0;
    auto take = [&](long long cnt) {
      const long long o = at;
      at += cnt;
      return int(o);
    };
    const long long m1 = (long long)n * LS_HLD, m3 = (long long)k * LS_HLD + (long long)rank * k;
    mat = take(m1 > m3 ? m1 : m3), B = mat + k * LS_HLD;
    gram3 = take(k * k), invd = take(nm), c = take(nm), z = take(nm), v = take(nm), gn = take(nm), part = take(256);
    ps = take(rm), rs = take(rm), flag = take(2), c1 = take(n), scal = take(2);
    ints = take((3 * nm + 8 + 1) / 2);   // st, barred, idx (nm each), ctl (4), the two status words, passes of the state solve
    total = int(at);
    bytes = at * 8;
  }
};

// 0 inside the limits, else 1 .. 5: n, k, r, rank below k, rank beyond the LDS; *rank_max: the largest rank at this (n, k, r)
inline int ls_check_shape(int n, int k, int rank, int r, int* rank_max) {
  if (rank_max) *rank_max = 0;
  if (n < 1 || n > LS_NMAX) return 1;
  if (k < 1 || k > LS_KMAX) return 2;
  if (r < n || r > LS_RMAX) return 3;
  // bytes(rank) is non-decreasing and linear beyond max(r, n LS_HLD / k): the largest rank by bisection
  int lo = 0, hi = LS_LDS_BYTES;
  while (lo < hi) {
    const int mid = lo + (hi - lo + 1) / 2;
    if (LsLds(n, k, mid, r).bytes <= LS_LDS_BYTES) lo = mid;
    else hi = mid - 1;
  }
  if (rank_max) *rank_max = lo;
  if (rank < k) return 4;
  if (rank > lo) return 5;
  return 0;
}

// The four boxes in one block for one upload: c_lo (kc n) | c_hi (kc n) | a_lo (kc k) | a_hi (kc k).  Returns -1, or the index
// of the first bad pair in that order of pairs (cluster j coordinate q of c: j n + q; of a: kc n + j k + q): lo <= hi without
// NaN, lo < +inf, hi > -inf.
inline long long ls_pack_boxes(int kc, int n, int k, const double* c_lo, const double* c_hi, const double* a_lo, const double* a_hi,
                               std::vector<double>& out) {
  const size_t nc = size_t(kc) * n, na = size_t(kc) * k;
  out.assign(2 * nc + 2 * na, 0.0);
  const double inf = __builtin_huge_val();
  for (size_t e = 0; e < nc + na; ++e) {
    const double lo = e < nc ? c_lo[e] : a_lo[e - nc], hi = e < nc ? c_hi[e] : a_hi[e - nc];
    if (!(lo <= hi && lo < inf && hi > -inf)) return (long long)e;
    if (e < nc) out[e] = lo, out[nc + e] = hi;
    else out[2 * nc + (e - nc)] = lo, out[2 * nc + na + (e - nc)] = hi;
  }
  return -1;
}
