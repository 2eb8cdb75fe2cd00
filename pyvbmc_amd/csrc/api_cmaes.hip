// C-ABI entry point of the CMA-ES refinement of the acquisition search: vbmc_search_cmaes (vbmc/active_sample.py:355-423
// with search_optimizer = "cmaes").  R runs of cmaes.hip's optimiser in lockstep: a round is one advance launch, then the
// scoring of the R lambda rows it wrote (round 0: the R starts) by api_search.hip's search_score_rows -- the launches
// vbmc_search_eval runs on the resident search set.  The host queues opt_cmaes_rounds rounds between two reads of the
// count of runs not yet stopped (lockstep_rounds, common.h; DESIGN.md "lockstep drivers").  Plain stream order: no graph
// capture, no device-side launch, no waiting between workgroups, no atomics on global memory.  The bounds, the starts, the noise table and the weights go up
// once; all outputs come back in one copy.
//
// The candidates have a buffer of their own in this call's scratch: the resident search set of a preceding
// vbmc_search_fill / vbmc_search_put is preserved (a vbmc_search_eval after this call gives what it gave before).
// The installed GP, the mixture and the importance state are only read.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"

namespace {

// The strategy constants (Hansen, "The CMA Evolution Strategy: A Tutorial", 2016, defaults), in float64 in exactly this
// order of operations: pyvbmc_amd/cmaes.py and tests/cmaes_host.py compute the same bits.
struct CmaConsts {
  int mu = 0, hist = 0;
  std::vector<double> w;
  double mueff = 0, cs = 0, ds = 0, cc = 0, c1 = 0, cmu = 0, chi = 0;
};

CmaConsts cma_consts(int D, int lam) {
  CmaConsts c;
  const double d = (double)D;
  c.mu = lam / 2;
  c.w.resize(c.mu);
  double sw = 0.0;
  for (int i = 0; i < c.mu; ++i) {
    c.w[i] = std::log((lam + 1) / 2.0) - std::log((double)(i + 1));
    sw = sw + c.w[i];
  }
  double s2 = 0.0;
  for (int i = 0; i < c.mu; ++i) {
    c.w[i] = c.w[i] / sw;
    s2 = s2 + c.w[i] * c.w[i];
  }
  c.mueff = 1.0 / s2;
  c.cs = (c.mueff + 2.0) / (d + c.mueff + 5.0);
  c.ds = 1.0 + 2.0 * std::max(0.0, std::sqrt((c.mueff - 1.0) / (d + 1.0)) - 1.0) + c.cs;
  c.cc = (4.0 + c.mueff / d) / (d + 4.0 + 2.0 * c.mueff / d);
  c.c1 = 2.0 / ((d + 1.3) * (d + 1.3) + c.mueff);
  c.cmu = std::min(1.0 - c.c1, 2.0 * (c.mueff - 2.0 + 1.0 / c.mueff) / ((d + 2.0) * (d + 2.0) + c.mueff));
  c.chi = std::sqrt(d) * (1.0 - 1.0 / (4.0 * d) + 1.0 / (21.0 * d * d));
  c.hist = 10 + (30 * D + lam - 1) / lam;
  return c;
}

int cmaes_queue(vbmc_ctx* ctx, int kind, double y_max, double tol_gp_var, double u, int64_t n_noise,
                const double* X_rescaled_NxD, const double* sn2_new_N, const double* length_scale_D, int use_xf,
                const double* lb_eps_orig_D, const double* ub_eps_orig_D, int R, const double* x0_RxD, const double* sigma0_R,
                const double* lb_D, const double* ub_D, uint32_t int_bits, const vbmc_cmaes_opts* opts, double* x_best_RxD,
                double* f_best_R, double* f0_R, double* mean_RxD, double* sigma_R, double* C_RxDxD, int64_t* stats_Rx4) {
  if (!ctx || !x0_RxD || !sigma0_R || !lb_D || !ub_D || !opts) return VBMC_E_ARG;
  ctx->ev_valid[T_SEARCH_CMAES] = false;  // (never a stale interval after a call that launched nothing)
  SearchScore s;
  int rc = search_score_check(ctx, "search_cmaes", kind, n_noise, X_rescaled_NxD, sn2_new_N, length_scale_D, use_xf,
                              lb_eps_orig_D, ub_eps_orig_D, s);
  if (rc) return rc;
  const int D = ctx->gp.D;
  if (D == 1)
    return vbmc_fail(ctx, VBMC_E_UNSUP, "search_cmaes: D=1 is not CMA-ES's shape (the reference switches to Nelder-Mead)");
  if (D < 32 && (int_bits >> D)) return vbmc_fail(ctx, VBMC_E_ARG, "search_cmaes: integer_bits names a dimension >= D=%d", D);
  const int lam = opts->lambda > 0 ? opts->lambda : 4 + (int)std::floor(3.0 * std::log((double)D));
  if (R < 1) return vbmc_fail(ctx, VBMC_E_ARG, "search_cmaes: R=%d runs", R);
  if (lam < 4) return vbmc_fail(ctx, VBMC_E_ARG, "search_cmaes: lambda=%d < 4", lam);
  if (lam > 64) return vbmc_fail(ctx, VBMC_E_UNSUP, "search_cmaes: lambda=%d > 64 not supported", lam);
  if ((int64_t)R * lam > (int64_t)search_set_rows_cap())
    return vbmc_fail(ctx, VBMC_E_UNSUP, "search_cmaes: %d runs of lambda=%d are more rows than a search set holds", R, lam);
  if (opts->max_fevals < 1 + lam)
    return vbmc_fail(ctx, VBMC_E_ARG, "search_cmaes: max_fevals=%lld allows no generation of lambda=%d", (long long)opts->max_fevals, lam);
  if (!(opts->tol_fun == opts->tol_fun)) return vbmc_fail(ctx, VBMC_E_ARG, "search_cmaes: tol_fun is NaN");
  for (int d = 0; d < D; ++d)
    if (!std::isfinite(lb_D[d]) || !std::isfinite(ub_D[d]) || lb_D[d] > ub_D[d])
      return vbmc_fail(ctx, VBMC_E_ARG, "search_cmaes: the box of dimension %d is not finite or lb > ub", d);
  for (int r = 0; r < R; ++r) {
    if (!(sigma0_R[r] > 0.0) || !std::isfinite(sigma0_R[r]))
      return vbmc_fail(ctx, VBMC_E_ARG, "search_cmaes: sigma0 of run %d is not a positive finite number", r);
    for (int d = 0; d < D; ++d) {
      const double v = x0_RxD[(size_t)r * D + d];
      if (!(v >= lb_D[d] && v <= ub_D[d])) return vbmc_fail(ctx, VBMC_E_ARG, "search_cmaes: start %d lies outside the box", r);
    }
  }
  const CmaConsts c = cma_consts(D, lam);
  const int64_t M = (int64_t)R * lam;
  if ((rc = search_score_list(ctx, "search_cmaes", M, s))) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));

  // ---- behind the scoring's pieces, this call's own: the arguments x0 | sigma0 | lb | ub | w; the candidates' rows and
  // values; the count; the runs' state; the results in one block that comes back in one copy
  PredictPlan& p = s.p;
  const CmaState ly(D, lam, c.hist);
  const size_t Rs = (size_t)R, rd = Rs * D;
  const auto p_in = p.sc.add(rd + Rs + 2 * (size_t)D + (size_t)c.mu);
  const auto p_rows = p.sc.add((size_t)M * D), p_val = p.sc.add((size_t)M);
  const auto p_count = p.sc.add<int>(2);
  const auto p_state = p.sc.add(Rs * ly.total);
  const auto p_xb = p.sc.add(rd), p_fb = p.sc.add(Rs), p_f0 = p.sc.add(Rs), p_mean = p.sc.add(rd), p_sig = p.sc.add(Rs);
  const auto p_C = p.sc.add(rd * D);
  const auto p_stats = p.sc.add<long long>(4 * Rs);
  const size_t n_out = p.sc.total - p_xb.off;
  if ((rc = predict_reserve(ctx, p, 0))) return rc;
  if ((rc = ensure_pinned(ctx, std::max(n_out, (size_t)1)))) return rc;

  // ---- uploads, once per call
  std::vector<double> in(p_in.count);
  {
    double* q = in.data();
    memcpy(q, x0_RxD, sizeof(double) * rd); q += rd;
    memcpy(q, sigma0_R, sizeof(double) * Rs); q += Rs;
    memcpy(q, lb_D, sizeof(double) * D); q += D;
    memcpy(q, ub_D, sizeof(double) * D); q += D;
    memcpy(q, c.w.data(), sizeof(double) * c.mu);
  }
  hipStream_t st = ctx->stream;
  double* d_in = p.sc.ptr(p_in);
  HIP_TRY(ctx, hipMemcpyAsync(d_in, in.data(), sizeof(double) * in.size(), hipMemcpyHostToDevice, st));
  // rows of a run that stops at its start are never written; a zeroed state is a run at its start; zero results
  HIP_TRY(ctx, hipMemsetAsync(p.sc.ptr(p_rows), 0, sizeof(double) * (p.sc.total - p_rows.off), st));
  if ((rc = timing_begin(ctx, T_SEARCH_CMAES))) return rc;
  if ((rc = search_score_upload(ctx, s))) return rc;

  CmaesArgs a;
  a.R = R; a.D = D; a.lam = lam; a.mu = c.mu; a.hist = c.hist;
  a.max_fevals = (long long)opts->max_fevals;
  a.seed = opts->seed;
  a.tol_fun = opts->tol_fun;
  a.tol_x = opts->tol_x > 0.0 ? opts->tol_x : 0.0;
  a.one_cs = 1.0 - c.cs;
  a.a_ps = std::sqrt(c.cs * (2.0 - c.cs) * c.mueff);
  a.q_cs = a.one_cs * a.one_cs;
  a.hs_thresh = (1.4 + 2.0 / ((double)D + 1.0)) * c.chi;
  a.one_cc = 1.0 - c.cc;
  a.a_pc = std::sqrt(c.cc * (2.0 - c.cc) * c.mueff);
  a.c_old = 1.0 - c.c1 - c.cmu;
  a.c1 = c.c1;
  a.cmu = c.cmu;
  a.cc2 = c.cc * (2.0 - c.cc);
  a.cs_ds = c.cs / c.ds;
  a.inv_chi = 1.0 / c.chi;
  a.x0 = d_in; a.sigma0 = d_in + rd; a.lb = a.sigma0 + Rs; a.ub = a.lb + D; a.w = a.ub + D;
  a.int_bits = int_bits;
  a.has_xf = use_xf ? 1 : 0;
  a.t = s.t;
  a.val = p.sc.ptr(p_val);
  a.rows = p.sc.ptr(p_rows);
  a.state = p.sc.ptr(p_state);
  a.x_best = p.sc.ptr(p_xb); a.f_best = p.sc.ptr(p_fb); a.f0 = p.sc.ptr(p_f0);
  a.mean = p.sc.ptr(p_mean); a.sigma = p.sc.ptr(p_sig); a.C = p.sc.ptr(p_C);
  a.stats = p.sc.ptr(p_stats);

  // ---- rounds: the start, at most ceil(max_fevals / lambda) generations, and the advance that consumes the last values
  const long long max_rounds = 2 + (a.max_fevals + lam - 1) / lam;
  long long rounds = 0;
  int left = R;
  auto round = [&](long long q) {
    const int rq = launch_cmaes_advance(ctx, a);
    return rq ? rq : search_score_rows(ctx, s, a.rows, q == 0 ? (int64_t)R : M, y_max, tol_gp_var, u, p.sc.ptr(p_val));
  };
  if ((rc = lockstep_rounds(ctx, "search_cmaes", ctx->opt_cmaes_rounds, max_rounds, R, a.state, cmaes_done_word(ly),
                            p.sc.ptr(p_count), round, &rounds, &left)))
    return rc;
  if ((rc = timing_end(ctx, T_SEARCH_CMAES))) return rc;
  if (left > 0) return vbmc_fail(ctx, VBMC_E_HIP, "search_cmaes: %d runs not stopped after %lld rounds", left, rounds);
  return fetch_tail(ctx, p.sc, p_xb.off,
                    {{p_xb.off, x_best_RxD, sizeof(double) * rd},
                     {p_fb.off, f_best_R, sizeof(double) * Rs},
                     {p_f0.off, f0_R, sizeof(double) * Rs},
                     {p_mean.off, mean_RxD, sizeof(double) * rd},
                     {p_sig.off, sigma_R, sizeof(double) * Rs},
                     {p_C.off, C_RxDxD, sizeof(double) * rd * D},
                     {p_stats.off, stats_Rx4, sizeof(int64_t) * 4 * Rs}});
}

}  // namespace

extern "C" int vbmc_search_cmaes(vbmc_ctx* ctx, int kind, double y_max, double tol_gp_var, double u, int64_t n_noise,
                                 const double* X_rescaled_NxD, const double* sn2_new_N, const double* length_scale_D, int use_xf,
                                 const double* lb_eps_orig_D, const double* ub_eps_orig_D, int R, const double* x0_RxD,
                                 const double* sigma0_R, const double* lb_D, const double* ub_D, uint32_t integer_bits,
                                 const vbmc_cmaes_opts* opts, double* x_best_RxD, double* f_best_R, double* f0_R,
                                 double* mean_RxD, double* sigma_R, double* C_RxDxD, int64_t* stats_Rx4) {
  const int rc = cmaes_queue(ctx, kind, y_max, tol_gp_var, u, n_noise, X_rescaled_NxD, sn2_new_N, length_scale_D, use_xf,
                             lb_eps_orig_D, ub_eps_orig_D, R, x0_RxD, sigma0_R, lb_D, ub_D, integer_bits, opts, x_best_RxD,
                             f_best_R, f0_R, mean_RxD, sigma_R, C_RxDxD, stats_Rx4);
  return rc ? search_fail_wait(ctx, rc) : rc;
}
