// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC 2011) and the draws of rom_mcmc, for
// the host and the device: plain C++, no HIP needed to include it.  romhighcontrast_amd/inverse.py::philox4x32 / mcmc_uniform /
// mcmc_draws are the same functions in NumPy; the words and the uniforms agree bit for bit (tests/c_abi/philox_host_check.cpp).
//
// The stream of one chain: key = (seed low word, seed high word), counter = (step, chain id low, chain id high, purpose).  Purpose
// j < ceil(k / 2) gives the Box-Muller pair (2 j, 2 j + 1) of the step's k standard normals, purpose 0xFFFFFFFF the uniform of the
// acceptance test.  Nothing else enters: a chain's stream does not depend on what else is in the call.  (internal)
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define ROM_PHILOX_HD __host__ __device__
#else
#define ROM_PHILOX_HD
#endif

constexpr uint32_t ROM_PHILOX_M0 = 0xD2511F53u, ROM_PHILOX_M1 = 0xCD9E8D57u;   // the multipliers
constexpr uint32_t ROM_PHILOX_W0 = 0x9E3779B9u, ROM_PHILOX_W1 = 0xBB67AE85u;   // the key increments
constexpr uint32_t ROM_PHILOX_ACCEPT = 0xFFFFFFFFu;                           // the purpose of the acceptance uniform

// out = Philox4x32-10(counter, key)
ROM_PHILOX_HD inline void rom_philox4x32(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = uint64_t(ROM_PHILOX_M0) * c0, p1 = uint64_t(ROM_PHILOX_M1) * c2;
    const uint32_t n0 = uint32_t(p1 >> 32) ^ c1 ^ k0, n1 = uint32_t(p1), n2 = uint32_t(p0 >> 32) ^ c3 ^ k1, n3 = uint32_t(p0);
    c0 = n0, c1 = n1, c2 = n2, c3 = n3;
    k0 += ROM_PHILOX_W0, k1 += ROM_PHILOX_W1;
  }
  out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

// u = ((hi >> 6) 2^26 + (lo >> 6) + 0.5) 2^-52: 52 random bits and a half, exact in fp64, never 0 and never 1.  (With 53 bits
// the half no longer fits the significand: all-ones words would round to 1.)
ROM_PHILOX_HD inline double rom_philox_uniform(uint32_t hi, uint32_t lo) {
  const uint64_t bits = (uint64_t(hi >> 6) << 26) | uint64_t(lo >> 6);
  return (double(bits) + 0.5) * 0x1p-52;
}

// the words of (step, chain, purpose) under the seed
ROM_PHILOX_HD inline void rom_mcmc_words(uint64_t seed, uint64_t chain, uint32_t step, uint32_t purpose, uint32_t out[4]) {
  const uint32_t ctr[4] = {step, uint32_t(chain), uint32_t(chain >> 32), purpose};
  const uint32_t key[2] = {uint32_t(seed), uint32_t(seed >> 32)};
  rom_philox4x32(ctr, key, out);
}

// the Box-Muller pair j of a step: words 0, 1 give u1, words 2, 3 give u2
ROM_PHILOX_HD inline void rom_mcmc_normal_pair(uint64_t seed, uint64_t chain, uint32_t step, uint32_t j, double& z0, double& z1) {
  uint32_t w[4];
  rom_mcmc_words(seed, chain, step, j, w);
  const double u1 = rom_philox_uniform(w[0], w[1]), u2 = rom_philox_uniform(w[2], w[3]);
  const double rad = sqrt(-2.0 * log(u1)), ang = 6.283185307179586 * u2;
  z0 = rad * cos(ang);
  z1 = rad * sin(ang);
}

// the uniform of the acceptance test of a step
ROM_PHILOX_HD inline double rom_mcmc_accept_uniform(uint64_t seed, uint64_t chain, uint32_t step) {
  uint32_t w[4];
  rom_mcmc_words(seed, chain, step, ROM_PHILOX_ACCEPT, w);
  return rom_philox_uniform(w[0], w[1]);
}
