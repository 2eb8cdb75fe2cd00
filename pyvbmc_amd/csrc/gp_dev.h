// GP predict's finish for one point and the moments over the GP hyper-parameter samples: the single definition of
// both.  gp.hip's predict kernels, the acquisition kernels and vbmc_gp_predict's host loop call these.
#pragma once
#include <cmath>
#include <cstdint>

#include "common.h"

// what the finish of a point reads: every sample's hyper-parameters [S][P], smeta [S][3], the points [M][D]
struct PredView {
  const double* hyp_all = nullptr;
  const double* smeta = nullptr;
  const double* xs = nullptr;
  int D = 0, P = 0, mean_kind = 0, add_noise = 0;
};

inline PredView gp_pred_view(const GpState& g, const double* d_xs, int add_noise) {
  return {g.d_hyp, g.d_smeta, d_xs, g.D, g.P, g.mean_kind, add_noise};
}

// The squared-exponential ARD kernel by direct differences (no |a|^2 + |b|^2 - 2 a.b expansion):
//   k(a, b) = exp(lsf2 - 1/2 sum_d ((a_d - b_d) iell(d))^2),  lsf2 = 2 hyp[D], iell(d) = exp(-hyp[d])
// iell is a callable, so a caller that evaluates many pairs may hand over stored values instead of the exponentials.
template <class InvEll>
__device__ __forceinline__ double se_ard_direct(const double* __restrict__ a, const double* __restrict__ b, int D,
                                                InvEll iell, double lsf2) {
  double d2 = 0.0;
  for (int d = 0; d < D; ++d) {
    const double t = (a[d] - b[d]) * iell(d);
    d2 = fma(t, t, d2);
  }
  return exp(lsf2 - 0.5 * d2);
}

// the observation noise predict(add_noise=True) adds under GP sample smp: sn2 sn2_mult
__device__ __forceinline__ double predict_noise_add(const PredView& v, int smp) {
  const double* hyp = v.hyp_all + (size_t)smp * v.P;
  return exp(2.0 * hyp[v.D + 1]) * v.smeta[3 * smp + 1];
}

// predict, stage 3 for point m under GP sample smp: fmu = mean(x*) + f, fs2 = max(0, sf^2 -/+ s) (+ noise), with
// s / f the sums of the stage-2 partial row sums / the stage-1 partial means.
__device__ __forceinline__ void predict_point_moments(const PredView& v, int smp, int64_t m, double s, double f,
                                                      double& fmu, double& fs2) {
  const double* hyp = v.hyp_all + (size_t)smp * v.P;
  const int D = v.D;
  const bool chol = v.smeta[3 * smp] != 0.0;
  const double sf2 = exp(2.0 * hyp[D]);
  const double add = v.add_noise ? predict_noise_add(v, smp) : 0.0;
  fs2 = fmax(chol ? sf2 - s : sf2 + s, 0.0) + add;
  // mean function at x* (variational_optimization.py:1383-1392 layout)
  double mean = 0.0;
  const double* hm = hyp + D + 2;
  if (v.mean_kind == VBMC_MEAN_CONST) mean = hm[0];
  if (v.mean_kind == VBMC_MEAN_NEGQUAD) {
    mean = hm[0];
    for (int d = 0; d < D; ++d) {
      const double t = (v.xs[m * D + d] - hm[1 + d]) * exp(-hm[1 + D + d]);
      mean -= 0.5 * t * t;
    }
  }
  fmu = mean + f;
}

// abstract_acq_fcn.py:82-97 / gpyreg predict without separate_samples, from fmu[s * ld + m], fs2[s * ld + m]:
// f_bar = mean_s fmu, var_tot = var_s(fmu, ddof = 1) + mean_s fs2.  Sums over s ascending, then / S, q / (S - 1).
__host__ __device__ inline void gp_sample_moments(const double* fmu, const double* fs2, int S, int64_t ld, int64_t m,
                                                  double& f_bar, double& var_tot) {
  double fsum = 0.0, vsum = 0.0;
  for (int s = 0; s < S; ++s) {
    fsum += fmu[(size_t)s * ld + m];
    vsum += fs2[(size_t)s * ld + m];
  }
  f_bar = fsum / S;
  double q = 0.0;
  for (int s = 0; s < S; ++s) {
    const double t = fmu[(size_t)s * ld + m] - f_bar;
    q += t * t;
  }
  var_tot = (S > 1 ? q / (S - 1) : 0.0) + vsum / S;
}

// Inverse of one 64 x 64 diagonal block of an upper-triangular factor: the single definition, for trinv_diag_kernel
// (gp.hip, every block of an uploaded factor) and chol_dinv_kernel (gp_post.hip, block by block while the factor is
// formed).  A: the factor of one sample, row stride N; the block starts at row / column r0 and is padded with the identity
// past N (addresses are clamped, never out of bounds).  Called by the 64 threads of a workgroup, thread c = column c:
// back substitution, column-oriented so that the multiply-adds of a step are independent of each other -- with
// s_m = delta_mc to start,   for r = 63 .. 0:   x_r = s_r / u_rr;   s_m -= u_mr x_r  for all m < r.
// Everything is unrolled and lives in registers (x_r = 0 for r > c comes out by itself); the u_mr of a step are contiguous
// broadcast LDS reads that do not depend on the arithmetic.  sUT[r][m] = u_mr (64 x 64), sRinv[r] = 1 / u_rr; out: the
// block's inverse, row-major 64 x 64.
constexpr int TRI_B = 64;
__device__ __forceinline__ void tri_block_inverse(const double* __restrict__ A, int N, int r0, int c,
                                                  double (*sUT)[TRI_B], double* sRinv, double* __restrict__ out) {
  {
    // all 64 row loads in flight at once (clamped addresses, the padding is patched in afterwards)
    double u[TRI_B];
    const int gc = r0 + c, gcc = min(gc, N - 1);
#pragma unroll
    for (int r = 0; r < TRI_B; ++r) u[r] = A[(size_t)min(r0 + r, N - 1) * N + gcc];
#pragma unroll
    for (int r = 0; r < TRI_B; ++r) {
      const int gr = r0 + r;
      const double v = (gr < N && gc < N) ? (gc >= gr ? u[r] : 0.0) : (gr == gc ? 1.0 : 0.0);
      sUT[c][r] = v;  // element (r, c) of the block
      if (r == c) sRinv[c] = 1.0 / v;
    }
  }
  __syncthreads();
  double x[TRI_B];
#pragma unroll
  for (int m = 0; m < TRI_B; ++m) x[m] = (m == c) ? 1.0 : 0.0;
#pragma unroll
  for (int r = TRI_B - 1; r >= 0; --r) {
    const double xr = x[r] * sRinv[r];
    x[r] = xr;
#pragma unroll
    for (int m = 0; m < r; ++m) x[m] = fma(-sUT[r][m], xr, x[m]);
  }
#pragma unroll
  for (int r = 0; r < TRI_B; ++r) out[r * TRI_B + c] = x[r];
}
