// VariationalPosterior.mode (reference: variational_posterior/variational_posterior.py:810-919): n_opts rounds of
// "draw 1e5 samples (+ the component centres in round 0), take the one with the highest log-density, run a local
// search from it", the best round wins.  The reference's local search is SciPy's minimize (BFGS in the
// transformed space, L-BFGS-B with difference gradients in the original one), one round after the other; here
// every round runs at once and the local search is a monotone ascent with analytic derivatives.
//
//   mode_start_kernel   grid (candidate tiles, rounds): one thread = one candidate (a row of the host's array,
//                       or drawn in the kernel with the Philox streams of sample.hip and inverse-transformed for
//                       the original space), its log-density as vbmc_mixture_pdf / vbmc_mixture_pdf_orig compute
//                       it, wave then workgroup reduction to (value, index) per tile.  The highest value wins,
//                       ties go to the lowest index (np.argmin of the negated values).  A NaN value counts as
//                       -inf and never beats a number: the reference's argmin would return the first NaN, but it
//                       never produces one for samples inside the bounds, and a NaN start helps nobody.
//   mode_search_kernel  one workgroup per round: reduces the round's tiles, rebuilds the winning candidate from
//                       its index (with Philox the N x D draws are never stored) and searches from it.
//
// Search coordinates y (tests/mode_host.py restates all of this in NumPy):
//   transformed space   y = u, objective log q(u).
//   original space      y_d = x_d on an unbounded dimension, g_d(x_d) on a bounded one, inside the box
//                       [g(lb + sqrt(eps)), g(ub - sqrt(eps))] -- the reference's L-BFGS-B bounds (:888-898) through
//                       the transformer's own bounded_g.  u = ((y - mu) / delta) @ R / scale is affine in y (as
//                       xf_forward applies them), and the objective is log q(u(y)) - sum_d (const_d + lj_d(y_d)),
//                       xf_log_abs_det's per-dimension terms.  That function forms its argument as
//                       (u * scale) @ R^T: for an orthogonal R that is y again; the caller keeps a transformer
//                       whose R is not orthogonal on the host path.
// Derivatives from the responsibilities r_k (a_k = r_k / sigma_k^2, diff_k = (u - mu_k) / lambda):
//   grad_u = -sum_k a_k diff_k / lambda,   hess_u = (-diag(sum_k a_k) + sum_k a_k / sigma_k^2 diff_k diff_k^T) / (lambda
//   lambda^T) - grad_u grad_u^T,   grad_y = J grad_u - lj'(y),   hess_y = J hess_u J^T - diag(lj''(y)),  J = du/dy.
// Iteration: free set = dimensions not held at a bound by an outward gradient; Newton step on it when the negated
// Hessian has a Cholesky factor, clipped to the box, accepted when the objective does not go down; else the
// mean-shift fixed point sum_k a_k mu_k / sum_k a_k (transformed space) or a projected-gradient step with
// backtracking (original space).  "Does not go down" allows the rounding of one evaluation, kSlack max(1, |f|):
// next to the maximum a Newton step gains less than that, and a strict test would stop ~1e-8 short of it.  Stop: an
// accepted step <= tol max(1, |y|_inf), no acceptable step, or the iteration cap (status 2).
#include <climits>
#include <cmath>
#include <cstring>

#include "common.h"
#include "fastmath.h"
#include "mixture_dev.h"
#include "transform.h"

namespace {

constexpr int kThreads = 256;
constexpr int kLd = 33;                         // padded row of the D x D matrices in LDS
constexpr double kSlack = 64 * 0x1.0p-52;
constexpr double kSqrtEps = 0x1.0p-26;          // np.sqrt(np.finfo(float).eps)
constexpr int kStageMax = 2048;                 // K * D doubles of scaled means staged in LDS (16 KiB)

struct ModeArgs {
  const double* mix;
  MixLayout ml;
  XfView xf;
  int orig, philox;
  int n_opts;
  int64_t N;            // samples per round (the centres follow in round 0)
  const double* cand;   // [n_opts][N][D], the requested space (null with philox)
  const double* cdf;    // [K] cumulative weights (the selection of sample.hip without balance)
  uint64_t seed;
  int tiles;
  double* part_v;       // [n_opts][tiles]
  long long* part_i;
  int max_iter;
  double tol;
  double* rec;          // [n_opts][5]: start index, start value, final value, iterations, status
  double* pts;          // [n_opts][D]
  double* ys;           // [n_opts][D]: the final points in the search coordinates
};

// log q(u), as mixture_pdf_kernel<DP, 0, false> with log_flag computes it (mixture.hip)
template <int DP>
__device__ __forceinline__ double mix_log_density(const double* mix, const MixLayout& ml, const double (&u)[DP]) {
  const MixGauss mg = mix_gauss(mix, ml);
  const double* ilam = mix + ml.o_ilam;
  double xs[DP], g[DP], y = 0.0;
#pragma unroll
  for (int d = 0; d < DP; ++d) xs[d] = (d < ml.D) ? scaled_coord<false>(u[d], ilam[d]) : 0.0;
  mix_gauss_accumulate<DP, false, 1>(mg, xs, 0, y, g);
  return (y == 0.0) ? -INFINITY : log(y);
}

// pdf(v, orig_flag, log_flag=True) of one point; v is overwritten
template <int DP>
__device__ __forceinline__ double point_value(const ModeArgs& a, double (&v)[DP]) {
  if (!a.orig) return mix_log_density<DP>(a.mix, a.ml, v);
  if (!xf_inside<DP>(a.xf, v)) return -INFINITY;
  xf_forward<DP>(a.xf, v);
  const double y = mix_log_density<DP>(a.mix, a.ml, v);
  return y - xf_log_abs_det<DP>(a.xf, v);
}

// candidate i of round r, in the requested space
template <int DP>
__device__ __forceinline__ void candidate(const ModeArgs& a, int r, int64_t i, double (&v)[DP]) {
  const int D = a.ml.D, K = a.ml.K;
#pragma unroll
  for (int d = 0; d < DP; ++d) v[d] = 0.0;
  if (i >= a.N) {  // a component centre (:875-879)
    const double* mu = a.mix + a.ml.o_mu + (size_t)(i - a.N) * D;
#pragma unroll
    for (int d = 0; d < DP; ++d)
      if (d < D) v[d] = mu[d];
    if (a.orig) xf_inverse<DP>(a.xf, v);
    return;
  }
  if (!a.philox) {
    const double* x = a.cand + ((size_t)r * a.N + i) * D;
#pragma unroll
    for (int d = 0; d < DP; ++d)
      if (d < D) v[d] = x[d];
    return;
  }
  // sample i of vbmc_mixture_sample(N, seed + r, balance_flag = 0)
  const uint64_t seed = a.seed + (uint64_t)r, n = (uint64_t)i;
  const int k = K > 1 ? pick_component(a.cdf, K, philox_uniform(n, 3u, seed)) : 0;
  const double* mu = a.mix + a.ml.o_mu + (size_t)k * D;
  const double* lam = a.mix + a.ml.o_lam;
  const double sg = a.mix[a.ml.o_sig + k];
#pragma unroll
  for (int p = 0; p < (DP + 1) / 2; ++p)
    if (2 * p < D) {
      double z0, z1;
      philox_normal_pair(philox_block(n, (uint32_t)p, 2u, seed), z0, z1);
      v[2 * p] = mu[2 * p] + (lam[2 * p] * z0) * sg;
      if (2 * p + 1 < DP && 2 * p + 1 < D) v[2 * p + 1] = mu[2 * p + 1] + (lam[2 * p + 1] * z1) * sg;
    }
  if (a.orig) xf_inverse<DP>(a.xf, v);
}

__device__ __forceinline__ bool better(double v, long long i, double bv, long long bi) {
  return v > bv || (v == bv && i < bi);
}

// (value, index) of the best over the workgroup, in every thread; red_v / red_i: 4 slots of LDS
__device__ __forceinline__ void block_best(double& v, long long& i, double* red_v, long long* red_i) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double ov = __shfl_xor(v, off);
    const long long oi = __shfl_xor(i, off);
    if (better(ov, oi, v, i)) {
      v = ov;
      i = oi;
    }
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    red_v[threadIdx.x >> 6] = v;
    red_i[threadIdx.x >> 6] = i;
  }
  __syncthreads();
  v = red_v[0];
  i = red_i[0];
#pragma unroll
  for (int w = 1; w < kThreads / 64; ++w)
    if (better(red_v[w], red_i[w], v, i)) {
      v = red_v[w];
      i = red_i[w];
    }
}

template <int DP>
__global__ __launch_bounds__(256) void mode_start_kernel(ModeArgs a) {
  __shared__ double red_v[4];
  __shared__ long long red_i[4];
  const int r = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int64_t n_r = a.N + (r == 0 ? a.ml.K : 0);
  double val = -INFINITY;
  long long idx = LLONG_MAX;
  if (i < n_r) {
    double v[DP];
    candidate<DP>(a, r, i, v);
    val = point_value<DP>(a, v);
    if (val != val) val = -INFINITY;  // NaN never wins
    idx = i;
  }
  block_best(val, idx, red_v, red_i);
  if (threadIdx.x == 0) {
    a.part_v[(size_t)r * a.tiles + blockIdx.x] = val;
    a.part_i[(size_t)r * a.tiles + blockIdx.x] = idx;
  }
}

// ---- the local search ------------------------------------------------------------------------------------------

struct SearchLds {
  double y[32], yt[32], g[32], gt[32], ms[32], mst[32], us[32], gu[32], t[32], p[32], lo[32], hi[32], xlo[32], xhi[32];
  double H[32 * kLd], L[32 * kLd], J[32 * kLd], T[32 * kLd];
  double pk[kThreads], ak[kThreads], bk[kThreads];
  double red_v[4];
  long long red_i[4];
  double s_sum, s_a, s_f, s_max, s_const, s_step0;
  int fr[32];
};

template <bool STAGE>
__global__ __launch_bounds__(256) void mode_search_kernel(ModeArgs a) {
  __shared__ SearchLds s;
  extern __shared__ double smix[];  // STAGE: the K x D lambda-scaled means
  const int tid = threadIdx.x, r = blockIdx.x;
  const int D = a.ml.D, K = a.ml.K;
  const double* __restrict__ gmup = a.mix + a.ml.o_mup;
  const double* __restrict__ is2 = a.mix + a.ml.o_is2;
  const double* __restrict__ wc = a.mix + a.ml.o_wc;
  const double* __restrict__ lam = a.mix + a.ml.o_lam;
  const double* __restrict__ ilam = a.mix + a.ml.o_ilam;
  const double* __restrict__ P = a.xf.p;
  const bool orig = a.orig != 0;
  auto MUP = [&](int k, int d) -> double { return STAGE ? smix[k * D + d] : gmup[k * D + d]; };
  auto xrow = [&](int row, int d) -> double { return P[XfLayout::row(row, D) + d]; };

  if (STAGE)
    for (int e = tid; e < K * D; e += kThreads) smix[e] = gmup[e];

  // the round's best candidate
  double bv = -INFINITY;
  long long bi = LLONG_MAX;
  for (int t = tid; t < a.tiles; t += kThreads) {
    const double v = a.part_v[(size_t)r * a.tiles + t];
    const long long i = a.part_i[(size_t)r * a.tiles + t];
    if (better(v, i, bv, bi)) {
      bv = v;
      bi = i;
    }
  }
  block_best(bv, bi, s.red_v, s.red_i);
  if (bi == LLONG_MAX) bi = 0;

  // box, J = du/dy and the constant of the Jacobian term
  if (tid < D) {
    double lo = -INFINITY, hi = INFINITY, xlo = -INFINITY, xhi = INFINITY;
    if (orig) {
      const int type = (int)xrow(XfLayout::TYPE, tid);
      if (type != XF_UNBOUNDED) {
        const double lb = xrow(XfLayout::LB, tid), ub = xrow(XfLayout::UB, tid);
        xlo = lb + kSqrtEps;
        xhi = ub - kSqrtEps;
        lo = xf::bounded_g(type, xlo, lb, ub);
        hi = xf::bounded_g(type, xhi, lb, ub);
      }
    }
    s.lo[tid] = lo;
    s.hi[tid] = hi;
    s.xlo[tid] = xlo;
    s.xhi[tid] = xhi;
  }
  if (orig)
    for (int e = tid; e < D * D; e += kThreads) {
      const int i = e / D, j = e - i * D;
      const double rij = a.xf.has_R ? P[XfLayout::o_R(D) + e] : (i == j ? 1.0 : 0.0);
      s.J[i * kLd + j] = rij / (xrow(XfLayout::DELTA, i) * xrow(XfLayout::SCALE, j));
    }
  if (tid == 0) {
    double v[32];
    candidate<32>(a, r, bi, v);
    double c = 0.0;
    for (int d = 0; d < D; ++d) {
      double yd = v[d];
      if (orig) {
        const int type = (int)xrow(XfLayout::TYPE, d);
        c += xrow(XfLayout::LOG_DELTA, d) + xrow(XfLayout::LOG_SCALE, d);
        if (type != XF_UNBOUNDED) {
          const double lb = xrow(XfLayout::LB, d), ub = xrow(XfLayout::UB, d);
          c += xrow(XfLayout::LOG_SPAN, d);
          yd = yd < lb ? lb : (yd > ub ? ub : yd);  // (:899-902)
          yd = xf::bounded_g(type, yd, lb, ub);
        }
      }
      s.y[d] = yd;
    }
    s.s_const = c;
  }
  __syncthreads();
  if (tid < D) {
    double yd = s.y[tid];
    yd = yd < s.lo[tid] ? s.lo[tid] : (yd > s.hi[tid] ? s.hi[tid] : yd);
    s.y[tid] = yd;
  }
  __syncthreads();

  // log-term of component k at the scaled point s.us
  auto lk = [&](int k) -> double {
    double d2 = 0.0;
    for (int d = 0; d < D; ++d) {
      const double t = s.us[d] - MUP(k, d);
      d2 = fma(t, t, d2);
    }
    return log(wc[k]) - 0.5 * is2[k] * d2;
  };

  // objective, gradient (gout), mean-shift point (msout) and Hessian (s.H) at yv; every thread gets the value
  auto eval = [&](const double* yv, double* gout, double* msout) -> double {
    if (orig) {
      if (tid < D) s.t[tid] = yv[tid] - xrow(XfLayout::MU, tid);
      __syncthreads();
      if (tid < D) {
        double u = 0.0;
        for (int i = 0; i < D; ++i) u = fma(s.t[i], s.J[i * kLd + tid], u);
        s.us[tid] = u * ilam[tid];
      }
    } else if (tid < D) {
      s.us[tid] = yv[tid] * ilam[tid];
    }
    __syncthreads();
    double m = -INFINITY;
    for (int k = tid; k < K; k += kThreads) m = fmax(m, lk(k));
    m = fm::wave_max_dpp(m);
    if ((tid & 63) == 0) s.red_v[tid >> 6] = m;
    __syncthreads();
    m = fmax(fmax(s.red_v[0], s.red_v[1]), fmax(s.red_v[2], s.red_v[3]));
    double C[4] = {0.0, 0.0, 0.0, 0.0}, G = 0.0, MS = 0.0, S = 0.0, Sa = 0.0;
    for (int c0 = 0; c0 < K; c0 += kThreads) {
      __syncthreads();
      const int k = c0 + tid;
      const double p = k < K ? exp(lk(k) - m) : 0.0;
      const double i2 = k < K ? is2[k] : 0.0;
      s.pk[tid] = p;
      s.ak[tid] = p * i2;
      s.bk[tid] = p * i2 * i2;
      __syncthreads();
      const int kn = (K - c0) < kThreads ? (K - c0) : kThreads;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int e = tid + kThreads * q;
        if (e < D * D) {
          const int i = e / D, j = e - i * D;
          const double ui = s.us[i], uj = s.us[j];
          double acc = C[q];
          for (int kk = 0; kk < kn; ++kk) acc = fma(s.bk[kk] * (ui - MUP(c0 + kk, i)), uj - MUP(c0 + kk, j), acc);
          C[q] = acc;
        }
      }
      if (tid < D) {
        const double ud = s.us[tid];
        for (int kk = 0; kk < kn; ++kk) {
          const double mk = MUP(c0 + kk, tid);
          G = fma(s.ak[kk], ud - mk, G);
          MS = fma(s.ak[kk], mk, MS);
        }
      }
      if (tid == kThreads - 1)
        for (int kk = 0; kk < kn; ++kk) {
          S += s.pk[kk];
          Sa += s.ak[kk];
        }
    }
    if (tid == kThreads - 1) {
      s.s_sum = S;
      s.s_a = Sa;
    }
    __syncthreads();
    S = s.s_sum;
    Sa = s.s_a;
    if (tid < D) {
      s.gu[tid] = -(G / S) * ilam[tid];
      msout[tid] = lam[tid] * (MS / Sa);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = tid + kThreads * q;
      if (e < D * D) {
        const int i = e / D, j = e - i * D;
        double h = C[q] / S;
        if (i == j) h -= Sa / S;
        s.H[i * kLd + j] = h * ilam[i] * ilam[j] - s.gu[i] * s.gu[j];
      }
    }
    __syncthreads();
    if (orig) {
      for (int e = tid; e < D * D; e += kThreads) {  // T = J H
        const int i = e / D, j = e - i * D;
        double acc = 0.0;
        for (int q = 0; q < D; ++q) acc = fma(s.J[i * kLd + q], s.H[q * kLd + j], acc);
        s.T[i * kLd + j] = acc;
      }
      __syncthreads();
      for (int e = tid; e < D * D; e += kThreads) {  // H = T J^T - diag(lj'')
        const int i = e / D, j = e - i * D;
        double acc = 0.0;
        for (int q = 0; q < D; ++q) acc = fma(s.T[i * kLd + q], s.J[j * kLd + q], acc);
        if (i == j) {
          const int type = (int)xrow(XfLayout::TYPE, i);
          if (type != XF_UNBOUNDED) acc -= xf::bounded_lj_d2(type, yv[i]);
        }
        s.H[i * kLd + j] = acc;
      }
      if (tid < D) {
        double acc = 0.0;
        for (int q = 0; q < D; ++q) acc = fma(s.J[tid * kLd + q], s.gu[q], acc);
        const int type = (int)xrow(XfLayout::TYPE, tid);
        if (type != XF_UNBOUNDED) acc -= xf::bounded_lj_d1(type, yv[tid]);
        gout[tid] = acc;
      }
      if (tid == 0) {
        double f = m + log(S) - s.s_const;
        for (int d = 0; d < D; ++d) {
          const int type = (int)xrow(XfLayout::TYPE, d);
          if (type != XF_UNBOUNDED) f -= xf::bounded_lj(type, yv[d]);
        }
        s.s_f = f;
      }
    } else {
      if (tid < D) gout[tid] = s.gu[tid];
      if (tid == 0) s.s_f = m + log(S);
    }
    __syncthreads();
    return s.s_f;
  };

  auto clip = [&](int d, double v) -> double { return v < s.lo[d] ? s.lo[d] : (v > s.hi[d] ? s.hi[d] : v); };

  double f = eval(s.y, s.g, s.ms);
  int it = 0, status = 2;
  while (it < a.max_iter) {
    ++it;
    const double slack = kSlack * fmax(1.0, fabs(f));
    // free set; -H on it (identity rows for the held dimensions), the gradient as right-hand side
    if (tid < D) {
      const double yd = s.y[tid], gd = s.g[tid];
      s.fr[tid] = !((yd <= s.lo[tid] && gd < 0.0) || (yd >= s.hi[tid] && gd > 0.0));
    }
    __syncthreads();
    for (int e = tid; e < D * D; e += kThreads) {
      const int i = e / D, j = e - i * D;
      const bool fi = s.fr[i] && s.fr[j];
      s.L[i * kLd + j] = fi ? -s.H[i * kLd + j] : (i == j ? 1.0 : 0.0);
    }
    if (tid < D) {
      s.p[tid] = s.fr[tid] ? s.g[tid] : 0.0;
      double rs = 0.0;
      for (int j = 0; j < D; ++j) rs += fabs(s.H[tid * kLd + j]);
      s.t[tid] = rs;
    }
    __syncthreads();
    int n_free = 0;
    double hmax = 0.0;
    for (int d = 0; d < D; ++d) {
      n_free += s.fr[d];
      hmax = fmax(hmax, s.t[d]);
    }
    bool chol = n_free > 0;
    for (int j = 0; j < D && chol; ++j) {
      const double piv = s.L[j * kLd + j];
      if (!(piv > 0.0) || !(piv < INFINITY)) {
        chol = false;
        break;
      }
      const double sq = sqrt(piv);
      __syncthreads();
      if (tid == j) s.L[j * kLd + j] = sq;
      if (tid > j && tid < D) s.L[tid * kLd + j] /= sq;
      __syncthreads();
      for (int e = tid; e < D * D; e += kThreads) {
        const int i = e / D, c = e - i * D;
        if (c > j && i >= c) s.L[i * kLd + c] -= s.L[i * kLd + j] * s.L[c * kLd + j];
      }
      __syncthreads();
    }
    bool accepted = false;
    double ft = f;
    if (chol) {
      for (int j = 0; j < D; ++j) {  // L z = g
        if (tid == j) s.p[j] /= s.L[j * kLd + j];
        __syncthreads();
        if (tid > j && tid < D) s.p[tid] -= s.L[tid * kLd + j] * s.p[j];
        __syncthreads();
      }
      for (int j = D - 1; j >= 0; --j) {  // L^T p = z
        if (tid == j) s.p[j] /= s.L[j * kLd + j];
        __syncthreads();
        if (tid < j) s.p[tid] -= s.L[j * kLd + tid] * s.p[j];
        __syncthreads();
      }
      if (tid < D) s.yt[tid] = clip(tid, s.y[tid] + s.p[tid]);
      __syncthreads();
      ft = eval(s.yt, s.gt, s.mst);
      accepted = ft >= f - slack;
    }
    if (!accepted && !orig) {
      if (tid < D) s.yt[tid] = s.ms[tid];
      __syncthreads();
      ft = eval(s.yt, s.gt, s.mst);
      accepted = ft >= f - slack;
    }
    if (!accepted && orig && n_free > 0) {
      double step = 1.0 / fmax(hmax, 1e-300);
      for (int b = 0; b < 30 && !accepted; ++b) {
        __syncthreads();
        if (tid < D) s.yt[tid] = clip(tid, s.y[tid] + step * (s.fr[tid] ? s.g[tid] : 0.0));
        __syncthreads();
        bool moved = false;
        for (int d = 0; d < D; ++d) moved = moved || (s.yt[d] != s.y[d]);
        ft = eval(s.yt, s.gt, s.mst);
        accepted = moved && ft >= f;
        step *= 0.25;
      }
    }
    if (!accepted) {
      status = 0;
      break;
    }
    double step = 0.0, ymax = 0.0;
    for (int d = 0; d < D; ++d) {
      step = fmax(step, fabs(s.yt[d] - s.y[d]));
      ymax = fmax(ymax, fabs(s.yt[d]));
    }
    __syncthreads();
    if (tid < D) {
      s.y[tid] = s.yt[tid];
      s.g[tid] = s.gt[tid];
      s.ms[tid] = s.mst[tid];
    }
    f = ft;
    __syncthreads();
    if (step <= a.tol * fmax(1.0, ymax)) {
      status = 0;
      break;
    }
  }

  // y -> x, clipped as the reference's result is (inside its L-BFGS-B box), and the density there
  if (tid == 0) {
    double v[32];
    bool at_bound = false;
    for (int d = 0; d < 32; ++d) v[d] = 0.0;
    for (int d = 0; d < D; ++d) {
      double xd = s.y[d];
      at_bound = at_bound || xd <= s.lo[d] || xd >= s.hi[d];
      if (orig) {
        const int type = (int)xrow(XfLayout::TYPE, d);
        if (type != XF_UNBOUNDED) {
          const double lb = xrow(XfLayout::LB, d), ub = xrow(XfLayout::UB, d);
          xd = xf::bounded_ginv(type, xd) * (ub - lb) + lb;
          xd = xd < s.xlo[d] ? s.xlo[d] : (xd > s.xhi[d] ? s.xhi[d] : xd);
        }
      }
      v[d] = xd;
      a.pts[(size_t)r * D + d] = xd;
      a.ys[(size_t)r * D + d] = s.y[d];
    }
    if (status == 0 && at_bound) status = 1;
    const double fx = point_value<32>(a, v);
    double* rec = a.rec + (size_t)r * 5;
    rec[0] = (double)bi;
    rec[1] = bv;
    rec[2] = fx;
    rec[3] = (double)it;
    rec[4] = (double)status;
  }
}

template <int DP>
void launch_start_dp(vbmc_ctx* ctx, const ModeArgs& a) {
  hipLaunchKernelGGL((mode_start_kernel<DP>), dim3((unsigned)a.tiles, (unsigned)a.n_opts), dim3(kThreads), 0,
                     ctx->stream, a);
}

}  // namespace

extern "C" int vbmc_mixture_mode(vbmc_ctx* ctx, int n_opts, int orig_flag, int64_t n, const double* cand_RxnxD,
                                 uint64_t seed, int max_iter, double step_tol, double* x_D, double* f_out,
                                 double* rec_Rx5, double* pts_RxD, double* ys_RxD) {
  if (!ctx || !x_D) return VBMC_E_ARG;
  if (n_opts < 1 || n < 1 || max_iter < 1 || !(step_tol > 0.0))
    return vbmc_fail(ctx, VBMC_E_ARG, "mixture_mode: n_opts=%d, n=%lld, max_iter=%d, step_tol=%g", n_opts, (long long)n,
                     max_iter, step_tol);
  if (!ctx->mix_set) return vbmc_fail(ctx, VBMC_E_ARG, "mixture_mode: mixture not set");
  const int D = ctx->D, K = ctx->K;
  if (D > 32) return vbmc_fail(ctx, VBMC_E_UNSUP, "mixture_mode: D=%d > 32 not supported", D);
  ModeArgs a;
  if (orig_flag && !xf_view_slot(ctx, 0, D, a.xf))
    return vbmc_fail(ctx, VBMC_E_ARG, "mixture_mode: transformer slot 0 not set for D=%d", D);
  NEED_DEVICE(ctx);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // one launch covers all rounds: the grid's x is the tile count, and the host array is uploaded in one piece
  if (n > ((int64_t)1 << 24))
    return vbmc_fail(ctx, VBMC_E_UNSUP, "mixture_mode: n=%lld candidates per round (at most 2^24)", (long long)n);
  const int tiles = (int)((n + K + kThreads - 1) / kThreads);
  const size_t n_cand = cand_RxnxD ? (size_t)n_opts * (size_t)n * D : 0;
  const size_t n_part = (size_t)n_opts * tiles;
  Scratch sc;
  const auto p_cand = sc.add(n_cand), p_cdf = sc.add(selector_cdf_elems(K)), p_pv = sc.add(n_part);
  const auto p_pi = sc.add<long long>(n_part);
  const auto p_rec = sc.add((size_t)n_opts * 5), p_pts = sc.add((size_t)n_opts * D), p_ys = sc.add((size_t)n_opts * D);
  int rc = reserve(ctx, sc);
  if (rc) return rc;
  double *d_cand = sc.ptr(p_cand), *d_cdf = sc.ptr(p_cdf), *d_pv = sc.ptr(p_pv);
  long long* d_pi = sc.ptr(p_pi);
  double *d_rec = sc.ptr(p_rec), *d_pts = sc.ptr(p_pts), *d_ys = sc.ptr(p_ys);
  Selector sel;  // np.random.choice(p=w)'s inverse CDF: sample.hip's selector without balance
  make_selector(ctx->w.data(), K, n, 0, sel);
  HIP_TRY(ctx, hipMemcpyAsync(d_cdf, sel.cdf.data(), sizeof(double) * K, hipMemcpyHostToDevice, ctx->stream));
  if (cand_RxnxD)
    HIP_TRY(ctx, hipMemcpyAsync(d_cand, cand_RxnxD, sizeof(double) * n_cand, hipMemcpyHostToDevice, ctx->stream));
  a.mix = ctx->d_mix;
  a.ml = ctx->ml;
  a.orig = orig_flag ? 1 : 0;
  a.philox = cand_RxnxD ? 0 : 1;
  a.n_opts = n_opts;
  a.N = n;
  a.cand = cand_RxnxD ? d_cand : nullptr;
  a.cdf = d_cdf;
  a.seed = seed;
  a.tiles = tiles;
  a.part_v = d_pv;
  a.part_i = d_pi;
  a.max_iter = max_iter;
  a.tol = step_tol;
  a.rec = d_rec;
  a.pts = d_pts;
  a.ys = d_ys;
#define CALL(DP) launch_start_dp<DP>(ctx, a)
  VBMC_DISPATCH_DP(D, CALL);
#undef CALL
  HIP_TRY(ctx, hipGetLastError());
  // the K x D scaled means in LDS while they fit next to the kernel's own 43 KiB (64 KiB per workgroup)
  if (K * D <= kStageMax)
    hipLaunchKernelGGL((mode_search_kernel<true>), dim3((unsigned)n_opts), dim3(kThreads), sizeof(double) * K * D,
                       ctx->stream, a);
  else
    hipLaunchKernelGGL((mode_search_kernel<false>), dim3((unsigned)n_opts), dim3(kThreads), 0, ctx->stream, a);
  HIP_TRY(ctx, hipGetLastError());
  std::vector<double> rec((size_t)n_opts * 5), pts((size_t)n_opts * 2 * D);  // (points, then search coordinates)
  HIP_TRY(ctx, hipMemcpyAsync(rec.data(), d_rec, sizeof(double) * rec.size(), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(pts.data(), d_pts, sizeof(double) * pts.size(), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, stream_wait(ctx));
  // the best round (np.argmin of the negated values; a NaN value never wins)
  int best = 0;
  double fb = -INFINITY;
  for (int r = 0; r < n_opts; ++r) {
    const double fr = rec[(size_t)r * 5 + 2];
    if (fr > fb) {
      fb = fr;
      best = r;
    }
  }
  std::memcpy(x_D, pts.data() + (size_t)best * D, sizeof(double) * D);
  if (f_out) *f_out = rec[(size_t)best * 5 + 2];
  if (rec_Rx5) std::memcpy(rec_Rx5, rec.data(), sizeof(double) * rec.size());
  if (pts_RxD) std::memcpy(pts_RxD, pts.data(), sizeof(double) * n_opts * D);
  if (ys_RxD) std::memcpy(ys_RxD, pts.data() + (size_t)n_opts * D, sizeof(double) * n_opts * D);
  return VBMC_OK;
}
