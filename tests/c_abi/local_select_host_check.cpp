// The host side of rom_local_select on the CPU (run by tests/test_local_select_host.py under AddressSanitizer and UBSan):
// csrc/rom_local_select_host.h compiled with a plain C++ compiler.  The LDS map of k_local_fit (sub-arrays disjoint, inside the
// total, B behind the factor of the parameter solve and inside `mat`, the integers behind the doubles), the limits and the
// largest rank of ls_check_shape against a linear search, the OUT row, and ls_pack_boxes (the block it builds, the index of the
// first bad pair).  Exit status 0, an empty stderr and a last line "OK" mean that every check passed.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "rom_local_select_host.h"

static int g_failed = 0;
#define EXPECT(cond, ...)                           \
  do {                                              \
    if (!(cond)) {                                  \
      printf("FAILED %s:%d: ", __FILE__, __LINE__); \
      printf(__VA_ARGS__);                          \
      printf("\n");                                 \
      ++g_failed;                                   \
    }                                               \
  } while (0)

struct Arr {
  const char* name;
  long long off, cnt;
};

static void check_layout(int n, int k, int rank, int r) {
  const LsLds m(n, k, rank, r);
  const int nm = std::max(n, k), rm = std::max(r, rank);
  std::vector<Arr> a = {{"mat", m.mat, std::max<long long>((long long)n * LS_HLD, (long long)k * LS_HLD + (long long)rank * k)},
                        {"gram3", m.gram3, k * k}, {"invd", m.invd, nm}, {"c", m.c, nm},       {"z", m.z, nm},
                        {"v", m.v, nm},            {"gn", m.gn, nm},     {"part", m.part, 256}, {"ps", m.ps, rm},
                        {"rs", m.rs, rm},          {"flag", m.flag, 2},  {"c1", m.c1, n},       {"scal", m.scal, 2},
                        {"ints", m.ints, (3 * nm + 7 + 1) / 2}};
  std::sort(a.begin(), a.end(), [](const Arr& x, const Arr& y) { return x.off < y.off; });
  for (size_t i = 0; i < a.size(); ++i) {
    const long long end = a[i].off + a[i].cnt, next = i + 1 < a.size() ? a[i + 1].off : m.total;
    EXPECT(a[i].off >= 0 && end <= next, "(%d, %d, %d, %d): %s [%lld, %lld) runs into %s at %lld", n, k, rank, r, a[i].name, a[i].off, end,
           i + 1 < a.size() ? a[i + 1].name : "the end", next);
  }
  EXPECT(m.B == m.mat + k * LS_HLD && m.B + (long long)rank * k <= m.gram3, "(%d, %d, %d, %d): B leaves mat", n, k, rank, r);
  EXPECT(m.bytes == 8ll * m.total, "(%d, %d, %d, %d): bytes", n, k, rank, r);
}

static void check_shapes() {
  const int ns[] = {1, 3, 17, 32, 64}, ks[] = {1, 2, 9, 16}, rs[] = {1, 17, 40, 96};
  for (int n : ns)
    for (int k : ks)
      for (int r : rs) {
        if (r < n) {
          EXPECT(ls_check_shape(n, k, k, r, nullptr) == 3, "r = %d below n = %d passes", r, n);
          continue;
        }
        int top = 0;
        EXPECT(ls_check_shape(n, k, k, r, &top) == 0, "(%d, %d, rank = k, %d) refused", n, k, r);
        // the largest rank by walking up from k
        int walk = k;
        while (LsLds(n, k, walk + 1, r).bytes <= LS_LDS_BYTES) ++walk;
        EXPECT(top == walk, "(%d, %d, %d): rank_max %d, the walk gives %d", n, k, r, top, walk);
        EXPECT(ls_check_shape(n, k, top, r, nullptr) == 0 && ls_check_shape(n, k, top + 1, r, nullptr) == 5, "(%d, %d, %d): the edge at %d", n,
               k, r, top);
        if (k > 1) EXPECT(ls_check_shape(n, k, k - 1, r, nullptr) == 4, "rank below k passes");
        for (int rank : {k, (k + top) / 2, top}) check_layout(n, k, rank, r);
      }
  EXPECT(ls_check_shape(0, 1, 2, 1, nullptr) == 1 && ls_check_shape(65, 1, 2, 70, nullptr) == 1, "the limits of n");
  EXPECT(ls_check_shape(4, 0, 8, 4, nullptr) == 2 && ls_check_shape(4, 17, 40, 4, nullptr) == 2, "the limits of k");
  EXPECT(ls_check_shape(4, 2, 8, 3, nullptr) == 3 && ls_check_shape(4, 2, 8, 97, nullptr) == 3, "the limits of r");
  const LsRow o(5, 3);
  EXPECT(o.c == 0 && o.a == 5 && o.S == 8 && o.misfit == 9 && o.passes == 10 && o.status == 12 && o.total == 13, "the OUT row");
}

static void check_boxes() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
  const int kc = 3, n = 4, k = 2;
  std::vector<double> cl(kc * n), ch(kc * n), al(kc * k), ah(kc * k), out;
  for (int e = 0; e < kc * n; ++e) cl[e] = -1.0 - e, ch[e] = 1.0 + e;
  for (int e = 0; e < kc * k; ++e) al[e] = 0.5 + e, ah[e] = 0.5 + e;   // (pinned)
  cl[5] = -inf, ch[6] = inf;
  EXPECT(ls_pack_boxes(kc, n, k, cl.data(), ch.data(), al.data(), ah.data(), out) == -1, "a good box is refused");
  EXPECT(out.size() == size_t(2 * kc * n + 2 * kc * k), "the block has %zu doubles", out.size());
  bool same = true;
  for (int e = 0; e < kc * n; ++e) same = same && out[e] == cl[e] && out[kc * n + e] == ch[e];
  for (int e = 0; e < kc * k; ++e) same = same && out[2 * kc * n + e] == al[e] && out[2 * kc * n + kc * k + e] == ah[e];
  EXPECT(same, "the block is not c_lo | c_hi | a_lo | a_hi");
  auto bad_at = [&](std::vector<double>& v, int e, double x) {
    const double keep = v[e];
    v[e] = x;
    const long long at = ls_pack_boxes(kc, n, k, cl.data(), ch.data(), al.data(), ah.data(), out);
    v[e] = keep;
    return at;
  };
  EXPECT(bad_at(cl, 7, nan) == 7 && bad_at(ch, 2, nan) == 2 && bad_at(cl, 9, inf) == 9 && bad_at(ch, 11, -inf) == 11, "bad pairs of c");
  EXPECT(bad_at(cl, 3, 100.0) == 3, "lo > hi of c");
  EXPECT(bad_at(al, 4, nan) == kc * n + 4 && bad_at(ah, 0, -1.0) == kc * n + 0 && bad_at(ah, 5, -inf) == kc * n + 5, "bad pairs of a");
  // the sizes at the limits: kc = 256, n = 64, k = 16
  std::vector<double> L(256 * 64, -1.0), H(256 * 64, 1.0), A(256 * 16, 1.0), B(256 * 16, 2.0);
  EXPECT(ls_pack_boxes(256, 64, 16, L.data(), H.data(), A.data(), B.data(), out) == -1 && out.size() == size_t(2 * 256 * 80), "the largest boxes");
  EXPECT(ls_pack_boxes(1, 1, 1, L.data(), H.data(), A.data(), B.data(), out) == -1 && out.size() == 4, "the smallest boxes");
}

int main() {
  check_shapes();
  check_boxes();
  const int reach[2][4] = {{64, 4, 257, 96}, {32, 9, 289, 96}};
  for (auto& s : reach) {
    int top = 0;
    EXPECT(ls_check_shape(s[0], s[1], s[2], s[3], &top) == 0, "(%d, %d, %d, %d) is out of reach", s[0], s[1], s[2], s[3]);
    printf("LAYOUT %d %d %d %d %lld %d\n", s[0], s[1], s[2], s[3], LsLds(s[0], s[1], s[2], s[3]).bytes, top);
  }
  if (g_failed) {
    printf("%d checks FAILED\n", g_failed);
    return 1;
  }
  printf("OK\n");
  return 0;
}
