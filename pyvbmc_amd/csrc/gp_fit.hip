// The hand-overs of vbmc_gp_fit (api_gp_fit.hip): the kernels that join candidate scoring, the lockstep optimiser, the
// lockstep slice chains and the posterior build without a host decision between them.  Every one is small and
// latency-bound (B candidates of P <= 99 parameters, B a few thousand at most); the factorisations, the optimiser and
// the chains are the existing kernels, unchanged.
//
//   design    candidate rows [0, H): hyp0 clipped into [lb, ub] (a NaN stays one); rows H + j: coordinate p is
//             clip(dlb_p + (dub_p - dlb_p) u, dlb_p, dub_p), u the 53-bit uniform of words 0, 1 of Philox block
//             (p, 0, j, 10) under the call's seed (stream 10 of sample.hip's list).  Products and sums are not contracted,
//             so NumPy reproduces the bits (pyvbmc_amd/gp.py fit_design).
//   stage     a chunk of candidates into the staged GP through gp_cand.h, as the lockstep drivers stage theirs.
//   score     score_j = lml_j + sum_p t_p (p ascending: what gp_opt.hip computes at a start); -inf where the candidate is
//             not finite, did not factorise, or the sum is not finite.  Never an error.
//   rank      one workgroup, a counting rank: order = the candidates by score descending, ties to the lower index
//             (NumPy's stable argsort of -score); the first R rows gathered as the optimiser's starts, a row without a
//             finite score as NaN (an invalid run that costs no evaluation).
//   select    the optimum by GP.fit's rule: the best candidate and its score, replaced by the first run of greatest finite
//             log posterior where that is strictly greater; tiled into the chains' starts.  No finite score at all: the
//             status word says so and the starts are NaN.
//   handover  the S samples to install (the chains' kept samples, or the optimum) into the staged GP through gp_cand.h.
//             A sample that cannot be used (status set, an invalid chain) is flagged and a placeholder (lb) built in its
//             place, so the build never reads a value that is not finite; the host then discards the build.
// Vector stores only; no atomics; a workgroup's results depend on its own inputs alone.
#include <cmath>

#include "common.h"
#include "fastmath.h"
#include "gp_cand.h"
#include "mixture_dev.h"

namespace {

constexpr uint32_t FIT_STREAM = 10;
constexpr int FIT_PMAX = 128;  // >= 32 + 2 + 65 parameters
constexpr int FIT_TILE = 1024;

__global__ __launch_bounds__(256) void gp_fit_design_kernel(GpFitArgs f) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int P = f.P;
  if (idx >= (size_t)f.B * P) return;
  const int j = (int)(idx / P), p = (int)(idx % P);
  double v;
  if (j < f.H) {
    const double v0 = f.x0[idx];
    v = v0 != v0 ? v0 : fmax(fmin(v0, f.ub[p]), f.lb[p]);
  } else {
    const Philox4 r = philox_block((uint64_t)p, (uint32_t)(j - f.H), FIT_STREAM, f.seed);
    const double lo = f.dlb[p], hi = f.dub[p];
    v = lo + (hi - lo) * philox_u53(r.x[0], r.x[1]);
    v = fmax(fmin(v, hi), lo);
  }
  f.cand[idx] = v;
}

__global__ __launch_bounds__(64) void gp_fit_stage_kernel(GpFitArgs f, int b0, int S) {
  const int tid = threadIdx.x, slot = blockIdx.x, j = b0 + slot;
  if (slot >= S || j >= f.B) return;  // (uniform per workgroup)
  const double* row = f.cand + (size_t)j * f.P;
  for (int p = tid; p < f.P; p += 64) gp_cand_coord(row, f.lb, p, slot, f.P, f.g_hyp);
  gp_cand_noise<64>(tid, slot, f.N, f.D, row, f.lb, f.s2, f.s2_min, f.g_sn2, f.g_sl, f.g_smeta);
}

__global__ __launch_bounds__(256) void gp_fit_score_kernel(GpFitArgs f) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= f.B) return;
  const double* row = f.cand + (size_t)j * f.P;
  bool fin = true;
  double lp = 0.0;
  for (int p = 0; p < f.P; ++p) {  // (p ascending, as the optimiser and the chains add it)
    const double h = row[p];
    fin = fin && fabs(h) < INFINITY;
    lp += gp_prior_term(f.pmu, f.psig, f.pdf, f.pconst, p, h);
  }
  const double lml = f.lml[j];
  double sc = lml + lp;
  if (!fin || f.flag[j] != 0 || !(fabs(lml) < INFINITY) || !(fabs(sc) < INFINITY)) sc = -INFINITY;
  f.score[j] = sc;
  f.flag[j] = 0;
}

__global__ __launch_bounds__(256) void gp_fit_rank_kernel(GpFitArgs f) {
  __shared__ double s_s[FIT_TILE];
  const int tid = threadIdx.x, B = f.B, P = f.P;
  for (int i0 = 0; i0 < B; i0 += 256) {  // (the trip counts are the workgroup's: every barrier is reached by all)
    const int i = i0 + tid;
    const double si = i < B ? f.score[i] : 0.0;
    int rank = 0;
    for (int t0 = 0; t0 < B; t0 += FIT_TILE) {
      const int nt = B - t0 < FIT_TILE ? B - t0 : FIT_TILE;
      __syncthreads();
      for (int q = tid; q < nt; q += 256) s_s[q] = f.score[t0 + q];
      __syncthreads();
      if (i < B)
        for (int q = 0; q < nt; ++q) {
          const double sj = s_s[q];
          rank += sj > si || (sj == si && t0 + q < i);
        }
    }
    if (i < B) f.order[rank] = i;  // (a permutation: scores are never NaN, so the order is total)
  }
  __syncthreads();
  for (int idx = tid; idx < f.R * P; idx += 256) {
    const int i = f.order[idx / P];
    f.opt_x0[idx] = f.score[i] > -INFINITY ? f.cand[(size_t)i * P + idx % P] : NAN;
  }
  for (int r = tid; r < f.R; r += 256) f.starts[r] = f.order[r];
}

__global__ __launch_bounds__(FIT_PMAX) void gp_fit_select_kernel(GpFitArgs f) {
  __shared__ int s_src, s_none;
  const int tid = threadIdx.x, P = f.P, i0 = f.order[0];
  if (tid == 0) {
    double bf = f.score[i0], bl = -INFINITY;
    int k = -1;
    for (int r = 0; r < f.R; ++r) {  // the first run of greatest finite log posterior
      const double lp = f.opt_logpost[r];
      if (!f.opt_invalid[r] && fabs(lp) < INFINITY && lp > bl) {
        bl = lp;
        k = r;
      }
    }
    if (k >= 0 && bl > bf) bf = bl; else k = -1;
    s_src = k;
    s_none = bf > -INFINITY ? 0 : 1;
    *f.best_logpost = bf;
    *f.status = s_none ? GP_FIT_NO_FINITE : 0;
  }
  __syncthreads();
  if (tid < P) {
    const double v = s_none ? NAN : s_src >= 0 ? f.opt_hyp[(size_t)s_src * P + tid] : f.cand[(size_t)i0 * P + tid];
    f.best[tid] = v;
    for (int c = 0; c < f.C; ++c) f.chain_x0[(size_t)c * P + tid] = v;
  }
}

__global__ __launch_bounds__(256) void gp_fit_handover_kernel(GpFitArgs f) {
  __shared__ int s_ok;
  const int tid = threadIdx.x, s = blockIdx.x, P = f.P;
  const double* src = f.C > 0 ? f.chain_hyp + (size_t)s * P : f.best;
  if (tid == 0) {
    bool ok = *f.status == 0 && (f.C == 0 || f.chain_invalid[s] == 0);
    for (int p = 0; p < P; ++p) ok = ok && fabs(src[p]) < INFINITY;
    s_ok = ok ? 1 : 0;
    f.bad[s] = ok ? 0 : 1;
  }
  __syncthreads();
  const double* row = s_ok ? src : f.lb;
  for (int p = tid; p < P; p += 256) {
    f.hyp[(size_t)s * P + p] = src[p];
    gp_cand_coord(row, f.lb, p, s, P, f.g_hyp);
  }
  const double e = gp_cand_noise<256>(tid, s, f.N, f.D, row, f.lb, f.s2, f.s2_min, f.g_sn2, f.g_sl, f.g_smeta);
  if (tid == 0) f.noise[s] = e;
}

}  // namespace

int launch_gp_fit_design(vbmc_ctx* ctx, const GpFitArgs& f) {
  if (f.P > FIT_PMAX) return vbmc_fail(ctx, VBMC_E_ARG, "gp_fit: P=%d > %d", f.P, FIT_PMAX);
  const size_t n = (size_t)f.B * f.P;
  hipLaunchKernelGGL(gp_fit_design_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, f);
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

int launch_gp_fit_stage(vbmc_ctx* ctx, const GpFitArgs& f, int b0, int S) {
  hipLaunchKernelGGL(gp_fit_stage_kernel, dim3(S), dim3(64), 0, ctx->stream, f, b0, S);
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

int launch_gp_fit_rank(vbmc_ctx* ctx, const GpFitArgs& f) {
  hipLaunchKernelGGL(gp_fit_score_kernel, dim3((f.B + 255) / 256), dim3(256), 0, ctx->stream, f);
  hipLaunchKernelGGL(gp_fit_rank_kernel, dim3(1), dim3(256), 0, ctx->stream, f);
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

int launch_gp_fit_select(vbmc_ctx* ctx, const GpFitArgs& f) {
  hipLaunchKernelGGL(gp_fit_select_kernel, dim3(1), dim3(FIT_PMAX), 0, ctx->stream, f);
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

int launch_gp_fit_handover(vbmc_ctx* ctx, const GpFitArgs& f) {
  hipLaunchKernelGGL(gp_fit_handover_kernel, dim3(f.S), dim3(256), 0, ctx->stream, f);
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}
