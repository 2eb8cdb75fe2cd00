// The Gaussian mixture density at a point and the 53-bit Philox draws of the sampler: the single definition of
// both.  mixture.hip's kernels, mode.hip's start selection and sample.hip's generator all call these; a kernel that
// needs a density or a draw at a point calls them too, so that a change of the arithmetic is made once.
// (The 32-bit draws of the entropy kernels are philox.h's own and stay apart.)
#pragma once
#include <cfloat>
#include <cmath>

#include "common.h"
#include "fastmath.h"
#include "philox.h"

// ---- density ----------------------------------------------------------------------------------------------------

// The Gaussian term's exponent, bounded below: a squared distance that overflows (a coordinate near 1e308, or
// 1e200 squared) makes it -inf, where exp2_fast's rint(x) - x is NaN; the reference's exp(-inf) is 0, and so is
// exp2_fast of anything below -1075.  A NaN exponent (a NaN coordinate) fails the comparison and stays NaN.
__device__ __forceinline__ double exp2_arg(double e) { return e < -2048.0 ? -2048.0 : e; }

// x / lambda for the density.  With the gradient, a finite x whose quotient overflows is held at +-DBL_MAX:
// its term c (x / lambda - mu_k / lambda) then has c = 0 and is 0, as the reference's nn (x - mu_k) / ... is,
// while an infinite x keeps 0 * inf = NaN, as there.
template <bool GRAD>
__device__ __forceinline__ double scaled_coord(double x, double ilam) {
  const double s = x * ilam;
  if (GRAD && isinf(s) && isfinite(x)) return copysign(DBL_MAX, s);
  return s;
}

// The parts of a mixture pack that the Gaussian terms read.  A kernel takes this view first, before it loads its
// point: with the address arithmetic after the loads the compiler schedules the thread-per-point kernel differently
// (one more VGPR at DP = 8 with the gradient; profiles/mixture_dev_resources.md).
struct MixGauss {
  const double* mup;  // K x D, mu / lambda
  const double* is2;  // K, 1 / sigma^2
  const double* wc;   // K, w / ((2 pi)^(D/2) prod(lambda) sigma^D)
  int D, K;
};
__device__ __forceinline__ MixGauss mix_gauss(const double* mix, const MixLayout& ml) {
  return {mix + ml.o_mup, mix + ml.o_is2, mix + ml.o_wc, ml.D, ml.K};
}

// y += sum_k w_k N(x; mu_k, sigma_k^2 lambda^2) over k = k_begin, k_begin + KSTEP, ... at the lambda-scaled point
// xs, in the linear domain; with GRAD, g[d] += sum_k nn_k (xs[d] - mu_kd / lambda_d) / sigma_k^2 (the caller
// applies -1 / lambda_d).  One thread per point walks all components (k_begin 0, KSTEP 1); a wave per point gives
// each lane every 64th.
template <int DP, bool GRAD, int KSTEP>
__device__ __forceinline__ void mix_gauss_accumulate(const MixGauss& m, const double (&xs)[DP], int k_begin, double& y,
                                                     double (&g)[DP]) {
  const int D = m.D, K = m.K;
  const double *mup = m.mup, *is2 = m.is2, *wc = m.wc;
  for (int k = k_begin; k < K; k += KSTEP) {
    const double* mk = mup + k * D;
    double d2 = 0.0;
#pragma unroll
    for (int d = 0; d < DP; ++d)
      if (d < D) {
        const double u = xs[d] - mk[d];
        d2 = fma(u, u, d2);
      }
    // exp(-d2 / (2 sigma_k^2)) as exp2 with log2(e) folded into the scale (fastmath.h, <= 1 ulp)
    const double nn = wc[k] * fm::exp2_fast(exp2_arg((-0.5 * 0x1.71547652b82fep+0 * is2[k]) * d2));
    if (GRAD) {
      const double c = nn * is2[k];
#pragma unroll
      for (int d = 0; d < DP; ++d)
        if (d < D) g[d] = fma(c, xs[d] - mk[d], g[d]);
    }
    y += nn;
  }
}

// ---- draws ------------------------------------------------------------------------------------------------------

// 53 bits of two Philox words as a uniform in [0, 1), or in (0, 1] (the argument of a logarithm)
__device__ __forceinline__ double philox_u53(uint32_t hi, uint32_t lo) {
  return (double)((((uint64_t)hi << 32) | lo) >> 11) * 0x1.0p-53;
}
__device__ __forceinline__ double philox_u53_pos(uint32_t hi, uint32_t lo) {
  return (double)(((((uint64_t)hi << 32) | lo) >> 11) + 1) * 0x1.0p-53;
}

// the block of sample n: counter (n_lo, n_hi, c2, c3), key = seed (the streams c3 are listed in sample.hip)
__device__ __forceinline__ Philox4 philox_block(uint64_t n, uint32_t c2, uint32_t c3, uint64_t seed) {
  return philox4x32_10((uint32_t)n, (uint32_t)(n >> 32), c2, c3, (uint32_t)seed, (uint32_t)(seed >> 32));
}

__device__ __forceinline__ double philox_uniform(uint64_t n, uint32_t c3, uint64_t seed) {
  const Philox4 r = philox_block(n, 0u, c3, seed);
  return philox_u53(r.x[0], r.x[1]);
}

// one block -> two standard normals (Box-Muller on 53-bit uniforms)
__device__ __forceinline__ void philox_normal_pair(const Philox4& r, double& z0, double& z1) {
  const double u1 = philox_u53_pos(r.x[0], r.x[1]), u2 = philox_u53(r.x[2], r.x[3]);
  const double rad = sqrt(-2.0 * fm::log_fast(u1));
  double s, c;
  fm::sincospi_fast(2.0 * u2, s, c);
  z0 = rad * c;
  z1 = rad * s;
}

// np.random.choice(p=w)'s inverse CDF: the first k with u < cdf[k] (the last component catches the rest)
__device__ __forceinline__ int pick_component(const double* cdf, int K, double u) {
  int k = 0;
  while (k + 1 < K && u >= cdf[k]) ++k;
  return k;
}
