// CMA-ES refinement of the acquisition search (vbmc/active_sample.py:355-423, search_optimizer = "cmaes"): R
// independent (mu/mu_w, lambda)-CMA-ES runs that minimise the acquisition function in a box, in lockstep.
//
// One evaluation of the acquisition is the launch sequence of api_search.hip's search_score_rows, not something one
// workgroup does in LDS, so a run is a state machine in global memory (scratch.h CmaState) that one launch of
// cmaes_advance_kernel moves on by one generation, as gp_hyp.hip moves a slice chain: workgroup = run; it consumes the
// lambda values the round before produced, ranks them, updates the mean, the paths, the covariance and the step size,
// factors the covariance, draws the next generation and writes every candidate twice -- the point the optimiser goes on
// with (the state's X) and the point that is evaluated, its integer columns rounded as AbstractAcqFcn._real2int does
// (search.hip's search_fill_kernel), straight into the rows the scoring launches read.  The host queues advance /
// scoring rounds in plain stream order (api_cmaes.hip).
//
// The optimiser is this package's own: tests/cmaes_host.py states it and pyvbmc_amd/cmaes.py is the same in product
// NumPy.  `cma` is not bit-compatible with anything here and is not part of the reference tree.  The covariance C is kept
// explicitly and its lower Cholesky factor L recomputed every generation (no eigendecomposition: L with a positive
// diagonal is unique and depends smoothly on C, so a host replay can follow the device).  Candidate i of generation g is
//   x_i = clip(m + sigma L z_i),  z_i = the D normals of Philox stream 8 (sample.hip) at counter (g lambda + i, pair)
// under the key seed + (r + 1) 0x9E3779B97F4A7C15 of run r; the update uses the repaired steps y_i = (x_i - m) / sigma and
// z'_i = L^-1 y_i (forward substitution): no penalty term, no resampling.  The reference wraps its optimiser in
// cma.NoiseHandler; the acquisition functions are deterministic, so there is no noise handling here.
//
// Every sum runs in rank order, then d ascending, one multiply and one add per term (no fma: NumPy's elementwise
// operations round the same way); what differs from the host statement is rcp_fast (1 / sigma), rsqrt_fast (the
// Cholesky's pivots, h_sigma's normalisation), exp2_fast (the step-size update) and the normals, by a few ulp each.
//
// Ranking: ascending by kde.hip's order-preserving key (NaN behind +inf, -0 as +0), the candidate index breaks ties.
// Stop reasons, checked after the update, the first that holds: 1 tolfun, 2 tolx, 3 maxfevals, 4 condition, 5 invalid
// (a generation whose best value is not finite, or a start whose value is not).  A stopped run writes nothing any more:
// its rows stay where they are, so the scoring launches go on reading valid points, and its state and outputs no
// longer change.  No atomics on global memory, no waiting on other workgroups: a run's results depend on its own start
// and key alone.
#include <cmath>

#include "common.h"
#include "fastmath.h"
#include "mixture_dev.h"
#include "transform.h"

namespace {

constexpr uint32_t CMA_STREAM = 8;
constexpr int CMA_DMAX = 32, CMA_LMAX = 64;
constexpr uint64_t CMA_KEY_STEP = 0x9E3779B97F4A7C15ull;
constexpr double kLog2e = 0x1.71547652b82fep+0;

enum { CMA_START = 0, CMA_WAIT_F0, CMA_WAIT_GEN, CMA_DONE };  // (a zeroed state is a run that has not looked at its x0)

struct CmaHead {
  int phase, reason;
  long long gen, evals, best_gen, hist_n;
  double decay;  // (1 - c_sigma)^(2 gen)
};
static_assert(sizeof(CmaHead) <= 8 * sizeof(double), "CmaState::head holds 8 doubles");

__device__ __forceinline__ uint64_t cma_sort_key(double v) {  // search.hip's sort_key
  if (v != v) return ~0ull - 1;
  if (v == 0.0) v = 0.0;
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// the evaluated copy of a point: integer columns rounded in original space, the others as they are
template <int DP>
__device__ __forceinline__ void cma_round(const CmaesArgs& a, double (&x)[DP]) {
  if (!a.int_bits) return;
  double v[DP];
#pragma unroll
  for (int d = 0; d < DP; ++d) v[d] = x[d];
  if (a.has_xf) xf_inverse<DP>(a.t, v);
#pragma unroll
  for (int d = 0; d < DP; ++d)
    if ((a.int_bits >> d) & 1u) v[d] = rint(v[d]);  // half to even, as np.around
  if (a.has_xf) xf_forward<DP>(a.t, v);
#pragma unroll
  for (int d = 0; d < DP; ++d)
    if ((a.int_bits >> d) & 1u) x[d] = v[d];
}

template <int DP>
__global__ __launch_bounds__(256) void cmaes_advance_kernel(CmaesArgs a) {
  __shared__ double sC[CMA_DMAX * CMA_DMAX], sL[CMA_DMAX * CMA_DMAX];
  __shared__ double sY[CMA_LMAX * CMA_DMAX], sZ[CMA_LMAX * CMA_DMAX];
  __shared__ double s_val[CMA_LMAX], s_m[CMA_DMAX], s_ps[CMA_DMAX], s_pc[CMA_DMAX], s_yw[CMA_DMAX], s_zw[CMA_DMAX], s_rd[CMA_DMAX];
  __shared__ int s_ord[CMA_LMAX];
  __shared__ double s_sigma, s_hs, s_nps;
  __shared__ int s_go, s_newbest, s_fail;
  __shared__ long long s_gen;  // generations consumed so far = the index of the generation drawn next

  const int r = blockIdx.x, tid = threadIdx.x;
  if (r >= a.R) return;  // (uniform per workgroup)
  const int D = a.D, lam = a.lam, mu = a.mu, DD = D * D;
  const CmaState ly(D, lam, a.hist);
  double* st = a.state + (size_t)r * ly.total;
  CmaHead& h = *(CmaHead*)(st + ly.head);
  double *g_ps = st + ly.ps, *g_pc = st + ly.pc, *g_L = st + ly.L, *g_rd = st + ly.rdiag;
  double *g_X = st + ly.X, *g_Y = st + ly.Y, *g_Z = st + ly.Z, *g_ring = st + ly.ring;
  double *g_m = a.mean + (size_t)r * D, *g_C = a.C + (size_t)r * DD, *g_xb = a.x_best + (size_t)r * D;
  long long* g_stats = a.stats + 4 * (size_t)r;
  const int phase = h.phase;
  __syncthreads();  // (lane 0 writes the phase further down)
  if (phase == CMA_DONE) return;

  if (phase == CMA_START) {
    // ---- the start: m = x0, sigma = sigma0, C = L = I, paths zero; x0 itself (rounded) is the one row of round 0
    for (int e = tid; e < DD; e += 256) {
      const double v = (e / D == e % D) ? 1.0 : 0.0;
      g_C[e] = v;
      g_L[e] = v;
    }
    if (tid < D) {
      g_m[tid] = a.x0[(size_t)r * D + tid];
      g_ps[tid] = 0.0;
      g_pc[tid] = 0.0;
      g_rd[tid] = 1.0;
    }
    if (tid == 0) {
      double x[DP];
#pragma unroll
      for (int d = 0; d < DP; ++d) x[d] = (d < D) ? a.x0[(size_t)r * D + d] : 0.0;
      cma_round<DP>(a, x);
#pragma unroll
      for (int d = 0; d < DP; ++d)
        if (d < D) {
          a.rows[(size_t)r * D + d] = x[d];
          g_xb[d] = x[d];
        }
      a.sigma[r] = a.sigma0[r];
      h.decay = 1.0;
      h.phase = CMA_WAIT_F0;
    }
    return;
  }

  // ---- the state into LDS
  for (int e = tid; e < DD; e += 256) {
    sC[e] = g_C[e];
    sL[e] = g_L[e];
  }
  for (int e = tid; e < lam * D; e += 256) {
    sY[e] = g_Y[e];
    sZ[e] = g_Z[e];
  }
  if (tid < D) {
    s_m[tid] = g_m[tid];
    s_ps[tid] = g_ps[tid];
    s_pc[tid] = g_pc[tid];
    s_rd[tid] = g_rd[tid];
  }
  if (tid == 0) {
    s_sigma = a.sigma[r];
    s_gen = h.gen;
    s_go = 1;
    s_newbest = 0;
    s_fail = 0;
  }
  __syncthreads();

  if (phase == CMA_WAIT_F0) {
    if (tid == 0) {
      const double f0 = a.val[r];
      a.f0[r] = f0;
      a.f_best[r] = f0;
      h.evals = 1;
      g_stats[1] = 1;
      if (!(fabs(f0) < INFINITY)) {
        h.reason = 5;
        h.phase = CMA_DONE;
        g_stats[2] = 5;
        s_go = 0;
      }
    }
    __syncthreads();
    if (!s_go) return;
  } else {
    // ---- 1. consume and rank the lambda values
    if (tid < lam) s_val[tid] = a.val[(size_t)r * lam + tid];
    __syncthreads();
    if (tid < lam) {
      const uint64_t k = cma_sort_key(s_val[tid]);
      int rank = 0;
      for (int j = 0; j < lam; ++j) {
        const uint64_t kj = cma_sort_key(s_val[j]);
        rank += (kj < k || (kj == k && j < tid)) ? 1 : 0;
      }
      s_ord[rank] = tid;
    }
    __syncthreads();
    const double vbest = s_val[s_ord[0]];
    if (tid == 0) {
      h.evals += lam;
      h.gen += 1;
      s_gen = h.gen;
      g_stats[0] = h.gen;
      g_stats[1] = h.evals;
      if (!(fabs(vbest) < INFINITY)) {
        h.reason = 5;
        h.phase = CMA_DONE;
        g_stats[2] = 5;
        s_go = 0;
      } else if (vbest < a.f_best[r]) {
        a.f_best[r] = vbest;
        h.best_gen = h.gen;
        g_stats[3] = h.gen;
        s_newbest = 1;
      }
    }
    __syncthreads();
    if (!s_go) return;
    if (s_newbest && tid < D) g_xb[tid] = a.rows[((size_t)r * lam + s_ord[0]) * D + tid];  // the rounded point
    // ---- 2. recombination, in rank order
    if (tid < D) {
      double yw = 0.0, zw = 0.0;
      for (int i = 0; i < mu; ++i) {
        const int c = s_ord[i];
        yw = yw + a.w[i] * sY[c * D + tid];
        zw = zw + a.w[i] * sZ[c * D + tid];
      }
      s_yw[tid] = yw;
      s_zw[tid] = zw;
      s_m[tid] = s_m[tid] + s_sigma * yw;
      s_ps[tid] = a.one_cs * s_ps[tid] + a.a_ps * zw;
    }
    __syncthreads();
    // ---- 3. the paths
    if (tid == 0) {
      double n2 = 0.0;
      for (int d = 0; d < D; ++d) n2 = n2 + s_ps[d] * s_ps[d];
      const double nps = sqrt(n2);
      h.decay = h.decay * a.q_cs;
      s_nps = nps;
      s_hs = (nps * fm::rsqrt_fast(1.0 - h.decay) < a.hs_thresh) ? 1.0 : 0.0;
    }
    __syncthreads();
    if (tid < D) s_pc[tid] = a.one_cc * s_pc[tid] + (s_hs * a.a_pc) * s_yw[tid];
    __syncthreads();
    // ---- 4. the covariance, a lane per entry; the rank-mu terms in rank order
    {
      const double keep = (1.0 - s_hs) * a.cc2;
      for (int e = tid; e < DD; e += 256) {
        const int i = e / D, j = e - i * D;
        double c = a.c_old * sC[e] + a.c1 * (s_pc[i] * s_pc[j] + keep * sC[e]);
        for (int k = 0; k < mu; ++k) {
          const int q = s_ord[k];
          c = c + (a.cmu * a.w[k]) * (sY[q * D + i] * sY[q * D + j]);
        }
        sC[e] = c;
      }
    }
    if (tid == 0) s_sigma = s_sigma * fm::exp2_fast(kLog2e * (a.cs_ds * (s_nps * a.inv_chi - 1.0)));
    __syncthreads();
    // ---- 5. L = chol(C), column by column; a pivot that is not positive ends the run (reason 4 at the latest)
    for (int e = tid; e < DD; e += 256) sL[e] = 0.0;
    __syncthreads();
    for (int j = 0; j < D; ++j) {
      if (tid == 0) {
        double s = sC[j * D + j];
        for (int k = 0; k < j; ++k) s = s - sL[j * D + k] * sL[j * D + k];
        if (!(s > 0.0) || !(s < INFINITY)) {
          s_fail = 1;
        } else {
          const double rj = fm::rsqrt_fast(s);
          sL[j * D + j] = s * rj;
          s_rd[j] = rj;
        }
      }
      __syncthreads();
      if (s_fail) break;  // (uniform: shared)
      if (tid > j && tid < D) {
        double t = sC[tid * D + j];
        for (int k = 0; k < j; ++k) t = t - sL[tid * D + k] * sL[j * D + k];
        sL[tid * D + j] = t * s_rd[j];
      }
      __syncthreads();
    }
    // ---- 6. the stop rules, then the state back to global memory
    if (tid == 0) {
      g_ring[(h.gen - 1) % a.hist] = vbest;
      if (h.hist_n < a.hist) h.hist_n += 1;
      const double tol_x = a.tol_x > 0.0 ? a.tol_x : 1e-11 * a.sigma0[r];
      int reason = 0;
      if (h.hist_n >= a.hist) {
        double lo = g_ring[0], hi = g_ring[0];
        for (int q = 1; q < a.hist; ++q) {
          lo = fmin(lo, g_ring[q]);
          hi = fmax(hi, g_ring[q]);
        }
        double vhi = vbest;
        for (int i = 0; i < lam; ++i)
          if (fabs(s_val[i]) < INFINITY) vhi = fmax(vhi, s_val[i]);
        if (hi - lo < a.tol_fun && vhi - vbest < a.tol_fun) reason = 1;
      }
      if (!reason) {
        double mx = 0.0;
        for (int d = 0; d < D; ++d) mx = fmax(mx, fmax(sqrt(sC[d * D + d]), fabs(s_pc[d])));
        if (s_sigma * mx < tol_x) reason = 2;
      }
      if (!reason && h.evals + lam > a.max_fevals) reason = 3;
      if (!reason) {
        if (s_fail) {
          reason = 4;
        } else {
          double lo = sL[0], hi = sL[0];
          for (int d = 1; d < D; ++d) {
            lo = fmin(lo, sL[d * D + d]);
            hi = fmax(hi, sL[d * D + d]);
          }
          if (hi * hi > 1e14 * (lo * lo)) reason = 4;
        }
      }
      a.sigma[r] = s_sigma;
      if (reason) {
        h.reason = reason;
        h.phase = CMA_DONE;
        g_stats[2] = reason;
        s_go = 0;
      }
    }
    for (int e = tid; e < DD; e += 256) {
      g_C[e] = sC[e];
      g_L[e] = sL[e];
    }
    if (tid < D) {
      g_m[tid] = s_m[tid];
      g_ps[tid] = s_ps[tid];
      g_pc[tid] = s_pc[tid];
      g_rd[tid] = s_rd[tid];
    }
    __syncthreads();
    if (!s_go) return;
  }

  // ---- 7. the next generation: normals, a lane per (candidate, pair)
  {
    const uint64_t key = a.seed + (uint64_t)(r + 1) * CMA_KEY_STEP;
    const uint64_t n0 = (uint64_t)s_gen * (uint64_t)lam;
    const int np = (D + 1) / 2;
    for (int t = tid; t < lam * np; t += 256) {
      const int i = t / np, p = t - i * np;
      double z0, z1;
      philox_normal_pair(philox_block(n0 + (uint64_t)i, (uint32_t)p, CMA_STREAM, key), z0, z1);
      sZ[i * D + 2 * p] = z0;
      if (2 * p + 1 < D) sZ[i * D + 2 * p + 1] = z1;
    }
  }
  __syncthreads();
  // ---- 8. candidates, a lane each: x = clip(m + sigma L z), y = (x - m) / sigma, z' = L^-1 y; both copies of the row
  if (tid < lam) {
    const int i = tid;
    const double sigma = s_sigma, inv_sigma = fm::rcp_fast(s_sigma);
    double x[DP];
#pragma unroll
    for (int d = 0; d < DP; ++d) {
      double v = 0.0;
      if (d < D) {
        double acc = 0.0;
        for (int k = 0; k <= d; ++k) acc = acc + sL[d * D + k] * sZ[i * D + k];
        v = s_m[d] + sigma * acc;
        v = (v < a.lb[d]) ? a.lb[d] : v;
        v = (v > a.ub[d]) ? a.ub[d] : v;
        sY[i * D + d] = (v - s_m[d]) * inv_sigma;
        g_X[i * D + d] = v;
      }
      x[d] = v;
    }
    for (int d = 0; d < D; ++d) {
      double acc = sY[i * D + d];
      for (int k = 0; k < d; ++k) acc = acc - sL[d * D + k] * sZ[i * D + k];
      sZ[i * D + d] = acc * s_rd[d];
    }
    cma_round<DP>(a, x);
#pragma unroll
    for (int d = 0; d < DP; ++d)
      if (d < D) a.rows[((size_t)r * lam + i) * D + d] = x[d];
  }
  __syncthreads();
  for (int e = tid; e < lam * D; e += 256) {
    g_Y[e] = sY[e];
    g_Z[e] = sZ[e];
  }
  if (tid == 0) h.phase = CMA_WAIT_GEN;
}

}  // namespace

int launch_cmaes_advance(vbmc_ctx* ctx, const CmaesArgs& a) {
  if (a.D < 2 || a.D > CMA_DMAX || a.lam < 4 || a.lam > CMA_LMAX || a.mu < 1 || a.mu > a.lam || a.hist < 1)
    return vbmc_fail(ctx, VBMC_E_ARG, "cmaes: D=%d lambda=%d outside the kernel's shapes", a.D, a.lam);
#define CALL(DP) hipLaunchKernelGGL(cmaes_advance_kernel<DP>, dim3((unsigned)a.R), dim3(256), 0, ctx->stream, a)
  VBMC_DISPATCH_DP(a.D, CALL);
#undef CALL
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

LockstepWord cmaes_done_word(const CmaState& ly) {
  return {ly.total, sizeof(double) * ly.head + offsetof(CmaHead, phase), CMA_DONE};
}
