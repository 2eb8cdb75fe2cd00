// C-ABI entry point of GP hyper-parameter sampling: vbmc_gp_hyp_sample.  C slice-sampling chains over
// f(h) = lml(h) + log p(h) in lockstep (gp_hyp.hip): a round is one advance launch, then the factorisation and the value
// kernels of vbmc_gp_lml on the candidates the chains left in ctx->gp_next.  The checks, the staging, the round and the
// fetch are the shared ones (gp_cand_host.h, api_gp_lml.hip, lockstep.hip; DESIGN.md "lockstep drivers"); what is stated
// here is the chains' own: their arguments, their pieces of the scratch and their bound on the rounds.
#include <algorithm>
#include <cmath>

#include "common.h"

extern "C" int vbmc_gp_hyp_sample(vbmc_ctx* ctx, int N, int D, int P, int mean_kind, const double* X_NxD, const double* y_N,
                                  const double* s2_N, int C, const double* x0_CxP, const double* widths_P, const double* lb_P,
                                  const double* ub_P, const double* prior_mu_P, const double* prior_sigma_P,
                                  const double* prior_df_P, int n, int thin, int burn_in, uint64_t seed, double* hyp_CxnxP,
                                  double* logpost_Cxn, double* logprior_Cxn, int64_t* stats_Cx4, int32_t* invalid_C) {
  const char* who = "gp_hyp_sample";
  if (!ctx || !X_NxD || !y_N || !x0_CxP || !widths_P || !lb_P || !ub_P || !prior_mu_P || !prior_sigma_P || !prior_df_P ||
      !hyp_CxnxP || !logpost_Cxn || !logprior_Cxn || !stats_Cx4 || !invalid_C)
    return VBMC_E_ARG;
  ctx->ev_valid[T_GP_HYP] = false;  // (never a stale interval after a call that launched nothing)
  WarpArgErr err;
  GpCandPlan pl;
  auto own = [&](WarpArgErr& e) {
    if (n < 1 || thin < 1 || burn_in < 0)
      return warp_arg_fail(e, VBMC_E_ARG, "%s: bad n=%d thin=%d burn_in=%d", who, n, thin, burn_in);
    for (int p = 0; p < P; ++p)
      if (!(widths_P[p] > 0.0) || !std::isfinite(widths_P[p]))
        return warp_arg_fail(e, VBMC_E_ARG, "%s: width of parameter %d is not a positive finite number", who, p);
    return 0;
  };
  if (gp_cand_check(err, who, 'C', N, D, C, P, mean_kind, lb_P, ub_P, prior_mu_P, prior_sigma_P, prior_df_P, s2_N,
                    ctx->opt_gp_lml_chunk, own, pl))
    return vbmc_fail(ctx, err.code, "%s", err.msg);
  int rc = gp_cand_begin(ctx, N, D, P, pl.chunk);
  if (rc) return rc;

  // ---- the call's device scratch, listed once (ctx->d_post_ws): a chunk's workspace, the chains' arguments, then what is
  // zeroed -- the count, the chains' points and state -- and the results in one block that comes back in one copy
  const size_t cp = (size_t)C * P, cn = (size_t)C * n;
  Scratch sc;
  const GpLmlWs ws = gp_lml_ws(sc, N, D, P, pl.mean_n, pl.chunk, C, 0);
  const auto p_in = sc.add(gp_cand_in_elems(C, P, 1, N, s2_N != nullptr));
  const auto p_count = sc.add<int>(2);
  const auto p_x = sc.add(cp), p_xp = sc.add(cp);
  const auto p_state = sc.add((size_t)C * gp_hyp_state_elems());
  const auto p_hyp = sc.add(cn * P), p_lpost = sc.add(cn), p_lprior = sc.add(cn);
  const auto p_stats = sc.add<long long>(4 * (size_t)C);
  const auto p_inv = sc.add<int>((size_t)C);
  if ((rc = reserve_in(ctx, &ctx->d_post_ws, &ctx->d_post_ws_cap, sc))) return rc;
  if ((rc = ensure_pinned(ctx, sc.total - p_hyp.off))) return rc;

  GpHypArgs a;
  a.N = N; a.D = D; a.P = P; a.C = C; a.n = n; a.thin = thin; a.burn_in = burn_in;
  a.seed = seed;
  a.s2_min = pl.s2_min;
  const std::vector<double> in =
      gp_cand_pack(a, sc.ptr(p_in), C, x0_CxP, {widths_P}, lb_P, ub_P, prior_mu_P, prior_sigma_P, prior_df_P, s2_N);
  a.widths = a.x0 + cp;
  a.x = sc.ptr(p_x); a.xp = sc.ptr(p_xp);
  a.state = sc.ptr(p_state);
  a.hyp_out = sc.ptr(p_hyp); a.logpost = sc.ptr(p_lpost); a.logprior = sc.ptr(p_lprior);
  a.stats = sc.ptr(p_stats);
  a.invalid = sc.ptr(p_inv);
  if ((rc = gp_cand_stage(ctx, who, sc, ws, sc.ptr(p_in), in, p_count.off, mean_kind, X_NxD, y_N, a))) return rc;

  // ---- rounds.  The largest number a chain can need: the start, one evaluation per step-out and shrink step of every
  // coordinate update, and the advance that consumes the last value.
  const long long max_rounds = 2 + ((long long)burn_in + (long long)n * thin) * P * (2 * 32 + 64);
  long long rounds = 0;
  int left = C;
  auto round = [&](long long) {
    return gp_cand_round(ctx, sc, ws, C, pl.chunk, [&](int b0, int S) { return launch_gp_hyp_advance(ctx, a, b0, S); });
  };
  rc = timing_begin(ctx, T_GP_HYP);
  if (!rc)
    rc = lockstep_rounds(ctx, who, ctx->opt_gp_hyp_rounds, max_rounds, C, a.state, gp_hyp_done_word(), sc.ptr(p_count),
                         round, &rounds, &left);
  if (!rc) rc = timing_end(ctx, T_GP_HYP);
  if (rc) {
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
  }
  if (left > 0) return vbmc_fail(ctx, VBMC_E_HIP, "%s: %d chains unfinished after %lld rounds", who, left, rounds);
  return fetch_tail(ctx, sc, p_hyp.off,
                    {{p_hyp.off, hyp_CxnxP, sizeof(double) * cn * P},
                     {p_lpost.off, logpost_Cxn, sizeof(double) * cn},
                     {p_lprior.off, logprior_Cxn, sizeof(double) * cn},
                     {p_stats.off, stats_Cx4, sizeof(int64_t) * 4 * C},
                     {p_inv.off, invalid_C, sizeof(int32_t) * C}});
}
