// C-ABI entry point of GP hyper-parameter optimisation: vbmc_gp_hyp_optimize.  R quasi-Newton runs over
// phi(h) = -(lml(h) + log p(h)) in lockstep (gp_opt.hip): a round is one advance launch, then the factorisation and the
// value and gradient kernels of vbmc_gp_lml on the trial points the runs left in ctx->gp_next.  The checks, the staging,
// the round and the fetch are the shared ones (gp_cand_host.h, api_gp_lml.hip, lockstep.hip; DESIGN.md "lockstep
// drivers"); what is stated here is the runs' own: their arguments, their pieces of the scratch and their bound on the
// rounds.
#include "common.h"

extern "C" int vbmc_gp_hyp_optimize(vbmc_ctx* ctx, int N, int D, int P, int mean_kind, const double* X_NxD,
                                    const double* y_N, const double* s2_N, int R, const double* x0_RxP, const double* lb_P,
                                    const double* ub_P, const double* prior_mu_P, const double* prior_sigma_P,
                                    const double* prior_df_P, int max_iter, int m, double tol_g, double tol_f, int trace_cap,
                                    double* hyp_RxP, double* logpost_R, double* grad_RxP, int64_t* stats_Rx4,
                                    int32_t* invalid_R, double* trace_iter, double* trace_eval) {
  const char* who = "gp_hyp_optimize";
  if (!ctx || !X_NxD || !y_N || !x0_RxP || !lb_P || !ub_P || !prior_mu_P || !prior_sigma_P || !prior_df_P || !hyp_RxP ||
      !logpost_R || !grad_RxP || !stats_Rx4 || !invalid_R)
    return VBMC_E_ARG;
  ctx->ev_valid[T_GP_OPT] = false;  // (never a stale interval after a call that launched nothing)
  WarpArgErr err;
  GpCandPlan pl;
  auto own = [&](WarpArgErr& e) {
    if (max_iter < 0 || max_iter > 1000000 || m < 1 || m > 16 || !(tol_g >= 0.0) || !(tol_f >= 0.0) || trace_cap < 0 ||
        trace_cap > max_iter + 1)
      return warp_arg_fail(e, VBMC_E_ARG, "%s: bad max_iter=%d m=%d tol_g=%g tol_f=%g trace_cap=%d", who, max_iter, m, tol_g,
                           tol_f, trace_cap);
    if (trace_cap > 0 && (!trace_iter || !trace_eval))
      return warp_arg_fail(e, VBMC_E_ARG, "%s: trace_cap > 0 without the trace arrays", who);
    return 0;
  };
  if (gp_cand_check(err, who, 'R', N, D, R, P, mean_kind, lb_P, ub_P, prior_mu_P, prior_sigma_P, prior_df_P, s2_N,
                    ctx->opt_gp_lml_chunk, own, pl))
    return vbmc_fail(ctx, err.code, "%s", err.msg);
  int rc = gp_cand_begin(ctx, N, D, P, pl.chunk);
  if (rc) return rc;

  // ---- the call's device scratch, listed once (ctx->d_post_ws): a chunk's workspace with the round's results per run,
  // the runs' arguments, then what is zeroed -- the count and the runs' state -- and the results in one block that comes
  // back in one copy
  const size_t rp = (size_t)R * P;
  const size_t n_it = (size_t)R * trace_cap * (3 * (size_t)P + 3), n_ev = trace_cap ? (size_t)R * (1 + 31 * (size_t)trace_cap) * 4 : 0;
  Scratch sc;
  const GpLmlWs ws = gp_lml_ws(sc, N, D, P, pl.mean_n, pl.chunk, R, 1);
  const auto p_in = sc.add(gp_cand_in_elems(R, P, 0, N, s2_N != nullptr));
  const auto p_count = sc.add<int>(2);
  const auto p_state = sc.add((size_t)R * gp_opt_state_elems(P, m));
  const auto p_hyp = sc.add(rp), p_lpost = sc.add((size_t)R), p_grad = sc.add(rp);
  const auto p_stats = sc.add<long long>(4 * (size_t)R);
  const auto p_inv = sc.add<int>((size_t)R);
  const auto p_tit = sc.add(n_it), p_tev = sc.add(n_ev);
  if ((rc = reserve_in(ctx, &ctx->d_post_ws, &ctx->d_post_ws_cap, sc))) return rc;
  if ((rc = ensure_pinned(ctx, sc.total - p_hyp.off))) return rc;

  GpOptArgs a;
  a.N = N; a.D = D; a.P = P; a.R = R; a.max_iter = max_iter; a.m = m; a.trace_cap = trace_cap;
  a.tol_g = tol_g; a.tol_f = tol_f;
  a.s2_min = pl.s2_min;
  const std::vector<double> in =
      gp_cand_pack(a, sc.ptr(p_in), R, x0_RxP, {}, lb_P, ub_P, prior_mu_P, prior_sigma_P, prior_df_P, s2_N);
  a.dlml = sc.ptr(ws.dlml);
  a.dsn2 = sc.ptr(ws.dsn2);
  a.state = sc.ptr(p_state);
  a.hyp_out = sc.ptr(p_hyp); a.logpost = sc.ptr(p_lpost); a.grad = sc.ptr(p_grad);
  a.stats = sc.ptr(p_stats);
  a.invalid = sc.ptr(p_inv);
  a.trace_it = sc.ptr(p_tit); a.trace_ev = sc.ptr(p_tev);
  if ((rc = gp_cand_stage(ctx, who, sc, ws, sc.ptr(p_in), in, p_count.off, mean_kind, X_NxD, y_N, a))) return rc;

  // ---- rounds.  The largest number a run can need: the round that submits the start, the start's evaluation, 31 trial
  // points (30 halvings) per iteration, and the advance that consumes the last of them.
  const long long max_rounds = 2 + (long long)max_iter * 31;
  long long rounds = 0;
  int left = R;
  auto round = [&](long long) {
    return gp_cand_round(ctx, sc, ws, R, pl.chunk, [&](int b0, int S) { return launch_gp_opt_advance(ctx, a, b0, S); });
  };
  rc = timing_begin(ctx, T_GP_OPT);
  if (!rc)
    rc = lockstep_rounds(ctx, who, ctx->opt_gp_opt_rounds, max_rounds, R, a.state, gp_opt_done_word(P, m), sc.ptr(p_count),
                         round, &rounds, &left);
  if (!rc) rc = timing_end(ctx, T_GP_OPT);
  if (rc) {
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
  }
  if (left > 0) return vbmc_fail(ctx, VBMC_E_HIP, "%s: %d runs unfinished after %lld rounds", who, left, rounds);
  return fetch_tail(ctx, sc, p_hyp.off,
                    {{p_hyp.off, hyp_RxP, sizeof(double) * rp},
                     {p_lpost.off, logpost_R, sizeof(double) * R},
                     {p_grad.off, grad_RxP, sizeof(double) * rp},
                     {p_stats.off, stats_Rx4, sizeof(int64_t) * 4 * R},
                     {p_inv.off, invalid_R, sizeof(int32_t) * R},
                     {p_tit.off, trace_iter, sizeof(double) * n_it},
                     {p_tev.off, trace_eval, sizeof(double) * n_ev}});
}
