// The reduced model at one theta, for one workgroup of 256 threads: what k_lm_polish (rom_lm.hip) evaluates at every trial and
// k_mcmc (rom_mcmc.hip) at every proposal -- inverse.py::_rom_state without the Jacobian (cited as `py:NN`, the line numbers of that
// file).  Written once so that the two kernels make the same operations in the same order.  (internal)
#pragma once
#include "rom_lm_small.h"

namespace {

// py:51-58: A(theta) = sum_q e^theta_q Ahat_q -> As (factored in place, 1 / d -> invd), c(theta) -> cn, rho = p - G_r c -> rhon,
// |rho|^2 -> scal[LMS_FN]; theta from sm[thx ..), p from sm[m.ps ..).  Map: an LDS map with ldn, As, invd, ea, cn, rhon, ps, scal.
// Returns whether every pivot of A(theta) was positive (otherwise cn, rhon and |rho|^2 mean nothing).  All 256 threads.
template <class Map>
__device__ bool lm_eval(double* sm, const Map& m, int n, int k, int r, const double* Ahat, const double* bhat, const double* Gr, int thx) {
  const int tid = threadIdx.x, lane = tid & 63, l16 = tid & 15;
  double* As = sm + m.As;
  if (tid < k) sm[m.ea + tid] = exp(sm[thx + tid]);   // py:53
  __syncthreads();
  for (int idx = tid; idx < n * n; idx += LMS_THREADS) {   // py:54
    const int row = idx / n, col = idx - row * n;
    double s = 0.0;
    for (int q = 0; q < k; ++q) s = fma(sm[m.ea + q], Ahat[size_t(q) * n * n + idx], s);
    As[row * m.ldn + col] = s;
  }
  __syncthreads();
  const bool ok = lm_factor(As, m.ldn, n, sm + m.invd, sm + m.scal + LMS_OKA);
  if (tid < 64) {   // py:55
    double b[1] = {lane < n ? bhat[lane] : 0.0};
    lm_solve<1>(As, m.ldn, n, sm + m.invd, b, lane);
    if (lane < n) sm[m.cn + lane] = b[0];
  }
  __syncthreads();
  for (int i0 = 0; i0 < r; i0 += 16) {   // py:56: 16 lanes per row of G_r
    const int i = i0 + (tid >> 4);
    double s = 0.0;
    if (i < r)
      for (int j = l16; j < n; j += 16) s = fma(Gr[size_t(i) * n + j], sm[m.cn + j], s);
    s = group16_sum(s);
    if (i < r && l16 == 0) sm[m.rhon + i] = sm[m.ps + i] - s;
  }
  __syncthreads();
  if (tid < 64) {
    const double v = lane < r ? sm[m.rhon + lane] : 0.0;
    const double f = wave_sum(v * v);
    if (lane == 0) sm[m.scal + LMS_FN] = f;
  }
  __syncthreads();
  return ok;
}

}  // namespace
