// Stand-alone host program over csrc/rom_philox.h (tests/test_mcmc_host.py builds it with g++ under AddressSanitizer and UBSan):
// for a list of counters and keys it prints the four Philox4x32-10 words and the bit patterns of the two uniforms made of them,
// one line each:  c0 c1 c2 c3 k0 k1 w0 w1 w2 w3 bits(u(w0, w1)) bits(u(w2, w3)).  The test recomputes every line in NumPy.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "rom_philox.h"

static void line(const uint32_t c[4], const uint32_t k[2]) {
  uint32_t w[4];
  rom_philox4x32(c, k, w);
  const double u1 = rom_philox_uniform(w[0], w[1]), u2 = rom_philox_uniform(w[2], w[3]);
  uint64_t b1, b2;
  std::memcpy(&b1, &u1, 8);
  std::memcpy(&b2, &u2, 8);
  std::printf("%08x %08x %08x %08x %08x %08x %08x %08x %08x %08x %016" PRIx64 " %016" PRIx64 "\n", c[0], c[1], c[2], c[3], k[0], k[1], w[0],
              w[1], w[2], w[3], b1, b2);
}

int main() {
  const uint32_t known[3][6] = {{0, 0, 0, 0, 0, 0},
                                {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu},
                                {0x243f6a88u, 0x85a308d3u, 0x13198a2e, 0x03707344u, 0xa4093822u, 0x299f31d0u}};
  for (const auto& row : known) line(row, row + 4);
  uint64_t s = 0x9E3779B97F4A7C15ull;   // counters and keys from a 64-bit LCG
  for (int i = 0; i < 61; ++i) {
    uint32_t v[6];
    for (uint32_t& x : v) {
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      x = uint32_t(s >> 32);
    }
    line(v, v + 4);
  }
  // the words of a chain as the sampler draws them, and the extreme uniforms
  uint32_t w[4];
  rom_mcmc_words(0x0123456789abcdefull, 0x100000002ull, 7, ROM_PHILOX_ACCEPT, w);
  const uint32_t c[4] = {7, 2, 1, 0xffffffffu}, k[2] = {0x89abcdefu, 0x01234567u};
  uint32_t w2[4];
  rom_philox4x32(c, k, w2);
  if (std::memcmp(w, w2, sizeof w) != 0) return 2;
  const double u0 = rom_philox_uniform(0, 0), u1 = rom_philox_uniform(0xffffffffu, 0xffffffffu);
  std::printf("extremes %.17g %.17g\n", u0, u1);
  return (u0 > 0.0 && u1 < 1.0) ? 0 : 3;
}
