// The candidate generator of optimize_vp's sieve: the reference's _vb_init (vbmc/variational_optimization.py:813-988)
// and the get_parameters its _sieve applies to every candidate (:776, variational_posterior.py:642-676), one workgroup
// per candidate, the raw theta row written straight into the buffer the batch evaluator's launches read.
//
// Candidate b of the set is candidate i of its type: the n1 of type 1 (the old parameters, new components spawned next to
// old ones), then the n2 of type 2 (the best training points as means), then the n3 of type 3 (random training points).
// Its draws are slots of one row, whoever made them:
//   normals   spawned component j < Kn - K:  j (D + 1) + d  the mean's (:905), j (D + 1) + D  the sigma's (:909)
//             o_s3 = (Kn - K)(D + 1):        type 3's sigma draw, Kn of them (:941-943)
//             o_mu = o_s3 + Kn:              the jitter of the means, element (d, k) at d Kn + k -- randn(D, K)'s C order (:960)
//             o_sg = o_mu + D Kn, o_lm = o_sg + Kn, o_w = o_lm + D:  the jitter of sigma, lambda, w (:962-966)
//   uniforms  o_u = o_w + Kn:                xi of spawned component j at o_u + j (:912)
//   indices   row b of I: the parent of spawned component j at j (:901); type 3: the training point of component k (:927-932)
// With host draws (Z, I) the rows are NumPy's, made in the reference's order by pyvbmc_amd/sieve.py.  Without, they are
// Philox draws under the call's seed, counter word 3 separating the streams (csrc/sample.hip lists the others):
//     c = (b_lo, b_hi, pair, 10)   normal slots 2 pair, 2 pair + 1 of candidate b (mixture_dev.h's 53-bit pair)
//     c = (b_lo, b_hi, 2 j,  11)   words 0, 1 as the 53-bit uniform u of spawned component j's parent floor(u K);
//     c = (b_lo, b_hi, 2 j + 1, 11)   ... and as its xi
//     c = (b_lo, b_hi, n,    12)   words 0, 1 as the 53-bit key of training point n: type 3 takes the min(Kn, N_star)
//                                  points of smallest key, ties by index, in that order
// tests/sieve_host.py states both in NumPy.
#include <cmath>

#include "common.h"
#include "fastmath.h"
#include "mixture_dev.h"

namespace {

constexpr double LOG2E = 0x1.71547652b82fep+0;

struct Slots {
  int o_s3, o_mu, o_sg, o_lm, o_w, o_u;
  __device__ Slots(int D, int K, int Kn) {
    o_s3 = (Kn - K) * (D + 1);
    o_mu = o_s3 + Kn;
    o_sg = o_mu + D * Kn;
    o_lm = o_sg + Kn;
    o_w = o_lm + D;
    o_u = o_w + Kn;
  }
};

__device__ __forceinline__ double draw_normal(const SieveFillDev& a, long long b, int j) {
  if (a.Z) return a.Z[(size_t)b * a.n_slot + j];
  double z0, z1;
  philox_normal_pair(philox_block((uint64_t)b, (uint32_t)(j >> 1), 10u, a.seed), z0, z1);
  return (j & 1) ? z1 : z0;
}
__device__ __forceinline__ double draw_uniform(const SieveFillDev& a, long long b, uint32_t c2) {
  const Philox4 r = philox_block((uint64_t)b, c2, 11u, a.seed);
  return philox_u53(r.x[0], r.x[1]);
}
__device__ __forceinline__ double exp_fifth(double z) { return fm::exp2_fast(LOG2E * (0.2 * z)); }  // exp(0.2 z)

// sums / maxima over f(0 .. n) by the 256 threads; every thread gets the result (red: 4 doubles, free again on return)
template <class F>
__device__ __forceinline__ double wg_sum(int n, F f, double* red) {
  double v = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) v += f(i);
  v = fm::wave_sum_dpp(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const double r = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return r;
}
template <class F>
__device__ __forceinline__ double wg_max(int n, F f, double* red) {
  double v = -INFINITY;
  for (int i = threadIdx.x; i < n; i += 256) v = fmax(v, f(i));
  v = fm::wave_max_dpp(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const double r = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(256) void sieve_fill_kernel(SieveFillDev a) {
  extern __shared__ double sm[];  // mu [Kn][D] | sigma [Kn] | lambda [D] | w [Kn] | var [D] | keys [Ns] (Philox type 3) | sel [Kn]
  __shared__ double red[4];
  const int D = a.D, K = a.K, Kn = a.Kn, tid = threadIdx.x;
  const long long b = blockIdx.x;
  const int type = b < a.n1 ? 1 : (b < a.n1 + a.n2 ? 2 : 3);
  const long long i = type == 1 ? b : (type == 2 ? b - a.n1 : b - a.n1 - a.n2);
  const ThetaMap tm(D, Kn, a.mask, a.n_theta);
  const Slots sl(D, K, Kn);
  const bool keyed = !a.Z && a.n3 > 0 && tm.o_mu();
  double* mu = sm;
  double* sg = mu + Kn * D;
  double* lm = sg + Kn;
  double* w = lm + D;
  double* var = w + Kn;
  unsigned long long* keys = (unsigned long long*)(var + D);
  int* sel = (int*)(keys + (keyed ? a.Ns : 0));
  const double* mu0 = a.base;
  const double* sg0 = mu0 + K * D;
  const double* lm0 = sg0 + K;
  const double* w0 = lm0 + D;
  const int* I = a.I ? a.I + (size_t)b * Kn : nullptr;

  // ---- the start of the candidate's type ----
  for (int d = tid; d < D; d += 256) lm[d] = (type != 1 && tm.o_lm()) ? a.lam_s[d] : lm0[d];  // (:920-921, :946-947)
  if (type == 1) {
    for (int e = tid; e < K * D; e += 256) mu[e] = mu0[e];
    for (int k = tid; k < K; k += 256) {
      sg[k] = sg0[k];
      w[k] = w0[k];
    }
    if (tid < Kn - K) {
      const int p = I ? I[tid] : (int)(draw_uniform(a, b, 2u * tid) * K);
      sel[tid] = p < 0 ? 0 : (p >= K ? K - 1 : p);
    }
    __syncthreads();
    // the spawned components (:900-914): means and sigmas come from the OLD components, so they are independent of one another
    for (int e = tid; e < (Kn - K) * D; e += 256) {
      const int j = e / D, d = e - j * D, p = sel[j];
      mu[(K + j) * D + d] = mu0[p * D + d] + 0.5 * sg0[p] * lm0[d] * draw_normal(a, b, j * (D + 1) + d);
    }
    for (int j = tid; j < Kn - K; j += 256) sg[K + j] = sg0[sel[j]] * exp_fifth(draw_normal(a, b, j * (D + 1) + D));
    // the weights are not: a parent hands on a share of what it has left
    if (tid == 0 && tm.o_w())
      for (int j = 0; j < Kn - K; ++j) {
        const double xi = 0.25 + 0.25 * (a.Z ? a.Z[(size_t)b * a.n_slot + sl.o_u + j] : draw_uniform(a, b, 2u * j + 1u));
        const int p = sel[j];
        w[K + j] = xi * w[p];
        w[p] *= 1.0 - xi;
      }
  } else if (type == 2) {
    for (int e = tid; e < Kn * D; e += 256) mu[e] = a.t2[e];
    for (int k = tid; k < Kn; k += 256) sg[k] = a.t2[Kn * D + k];
  } else {
    if (tm.o_mu()) {
      const int m = Kn < a.Ns ? Kn : a.Ns;
      if (keyed) {
        for (int n = tid; n < a.Ns; n += 256) {
          const Philox4 r = philox_block((uint64_t)b, (uint32_t)n, 12u, a.seed);
          keys[n] = (((unsigned long long)r.x[0] << 32) | r.x[1]) >> 11;
        }
        __syncthreads();
        for (int n = tid; n < a.Ns; n += 256) {
          const unsigned long long kn = keys[n];
          int rank = 0;
          for (int q = 0; q < a.Ns; ++q) rank += keys[q] < kn || (keys[q] == kn && q < n);
          if (rank < m) sel[rank] = n;
        }
      } else {
        for (int k = tid; k < m; k += 256) sel[k] = I[k] < 0 ? 0 : (I[k] >= a.Ns ? a.Ns - 1 : I[k]);
      }
      __syncthreads();
      for (int e = tid; e < Kn * D; e += 256) {
        const int k = e / D, d = e - k * D;
        mu[e] = a.Xs[(size_t)sel[k % m] * D + d];  // (np.tile: the first m indices, cycled)
      }
    } else {
      for (int e = tid; e < Kn * D; e += 256) mu[e] = mu0[e];
    }
    __syncthreads();
    // sigma = sqrt(mean_d var_k(mu_dk, ddof = 1) / Kn) exp(0.2 z)   (:937-943); K == 1: the X_star form, from the host
    double v3 = a.v3;
    if (K > 1) {
      if (tid < D) {
        double s = 0.0;
        for (int k = 0; k < Kn; ++k) s += mu[k * D + tid];
        const double mean = s / Kn;
        double q = 0.0;
        for (int k = 0; k < Kn; ++k) {
          const double t = mu[k * D + tid] - mean;
          q = fma(t, t, q);
        }
        var[tid] = q / (Kn - 1);
      }
      __syncthreads();
      v3 = wg_sum(D, [&](int d) { return var[d]; }, red) / D;
    }
    const double s3 = sqrt(v3 / Kn);
    for (int k = tid; k < Kn; k += 256) sg[k] = s3 * exp_fifth(draw_normal(a, b, sl.o_s3 + k));
  }
  if (type != 1 || !tm.o_w())
    for (int k = tid; k < Kn; k += 256) w[k] = 1.0 / Kn;  // (:923, :950, :975)
  __syncthreads();

  // ---- the jitter (:956-967): candidate 0 of types 1 and 2 stays as it is ----
  if (type == 3 || i > 0) {
    if (tm.o_mu())
      for (int e = tid; e < Kn * D; e += 256) {
        const int k = e / D, d = e - k * D;
        mu[e] += sg[k] * lm[d] * draw_normal(a, b, sl.o_mu + d * Kn + k);
      }
    __syncthreads();
    for (int k = tid; k < Kn; k += 256) sg[k] *= exp_fifth(draw_normal(a, b, sl.o_sg + k));
    if (tm.o_lm())
      for (int d = tid; d < D; d += 256) lm[d] *= exp_fifth(draw_normal(a, b, sl.o_lm + d));
    if (tm.o_w())
      for (int k = tid; k < Kn; k += 256) w[k] *= exp_fifth(draw_normal(a, b, sl.o_w + k));
    __syncthreads();
  }

  // ---- get_parameters (variational_posterior.py:642-676) and the max-shift of the eta tail (:1082-1085) ----
  const double nl = sqrt(wg_sum(D, [&](int d) { return lm[d] * lm[d]; }, red) / D);
  double* th = a.thetas + (size_t)b * a.n_theta;
  if (tm.o_mu())
    for (int e = tid; e < Kn * D; e += 256) th[e] = mu[e];
  for (int k = tid; k < Kn; k += 256) th[tm.p_sg + k] = fm::log_fast(sg[k] * nl);
  if (tm.o_lm())
    for (int d = tid; d < D; d += 256) th[tm.p_lm + d] = fm::log_fast(lm[d] / nl);
  if (tm.o_w()) {
    const double ws = wg_sum(Kn, [&](int k) { return w[k]; }, red);
    for (int k = tid; k < Kn; k += 256) w[k] = fm::log_fast(w[k] / ws);
    __syncthreads();
    const double mx = wg_max(Kn, [&](int k) { return w[k]; }, red);
    for (int k = tid; k < Kn; k += 256) th[tm.p_w + k] = w[k] - mx;
  }
}

__global__ __launch_bounds__(256) void sieve_nan_rows_kernel(const double* __restrict__ thetas, int n_theta, double* __restrict__ F,
                                                             double* __restrict__ G, double* __restrict__ H) {
  __shared__ int bad;
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  const double* th = thetas + (size_t)blockIdx.x * n_theta;
  int nf = 0;
  for (int i = threadIdx.x; i < n_theta; i += 256) nf |= !isfinite(th[i]);
  if (nf) atomicOr(&bad, 1);
  __syncthreads();
  if (threadIdx.x == 0 && bad) F[blockIdx.x] = G[blockIdx.x] = H[blockIdx.x] = NAN;
}

}  // namespace

size_t sieve_fill_lds_bytes(int D, int Kn, int n_keys) {
  return sizeof(double) * ((size_t)Kn * D + 2 * (size_t)Kn + 2 * (size_t)D + (size_t)n_keys) + sizeof(int) * (size_t)Kn;
}

int launch_sieve_fill(vbmc_ctx* ctx, const SieveFillDev& a) {
  const long long B = a.n1 + a.n2 + a.n3;
  const bool keyed = !a.Z && a.n3 > 0 && (a.mask & 1);  // (the kernel's own condition)
  hipLaunchKernelGGL(sieve_fill_kernel, dim3((unsigned)B), dim3(256), sieve_fill_lds_bytes(a.D, a.Kn, keyed ? a.Ns : 0), ctx->stream, a);
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

int launch_sieve_nan_rows(vbmc_ctx* ctx, const double* d_thetas, int64_t B, int n_theta, double* d_F, double* d_G, double* d_H) {
  hipLaunchKernelGGL(sieve_nan_rows_kernel, dim3((unsigned)B), dim3(256), 0, ctx->stream, d_thetas, n_theta, d_F, d_G, d_H);
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}
