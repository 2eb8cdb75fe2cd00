// C-ABI entry point of the GP hyper-parameter fit as one device call: vbmc_gp_fit.  Five stages on one stream -- the
// design, scoring and ranking of the candidates, the lockstep optimiser (gp_opt.hip), the lockstep slice chains
// (gp_hyp.hip) and the posterior build (gp_post.hip) -- joined by the hand-over kernels of gp_fit.hip, so that X, y, s2
// go up once, no host decision lies between the stages (the host reads the two drivers' "unfinished" counts, nothing
// else) and the results come back in one copy.  The checks, the staging, the rounds and the fetch are the shared ones
// (gp_cand_host.h, gp_fit_host.h, api_gp_lml.hip, lockstep.hip); stated here are the call's scratch, the order of the
// stages and the installation of the state it built.
#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

#include "common.h"

extern "C" int vbmc_gp_fit(vbmc_ctx* ctx, int N, int D, int P, int mean_kind, const double* X_NxD, const double* y_N,
                           const double* s2_N, int H, const double* hyp0_HxP, int init_N, const double* dlb_P,
                           const double* dub_P, const double* lb_P, const double* ub_P, const double* prior_mu_P,
                           const double* prior_sigma_P, const double* prior_df_P, int opts_N, int max_iter, int m, double tol_g,
                           double tol_f, int n_samples, const double* widths_P, int thin, int burn_in, uint64_t seed,
                           double* cand_BxP, double* score_B, int32_t* starts_R, double* opt_hyp_RxP, double* opt_logpost_R,
                           int64_t* opt_stats_Rx4, int32_t* opt_invalid_R, double* best_P, double* best_logpost,
                           double* hyp_SxP, double* logpost_S, double* logprior_S, int64_t* stats_Sx4, double* noise_S,
                           int32_t* status, double* alpha_SxN, double* L_SxNxN) {
  const char* who = "gp_fit";
  if (!ctx || !X_NxD || !y_N || !lb_P || !ub_P || !prior_mu_P || !prior_sigma_P || !prior_df_P || !best_P || !best_logpost ||
      !hyp_SxP || !noise_S || !status)
    return VBMC_E_ARG;
  ctx->ev_valid[T_GP_OPT] = ctx->ev_valid[T_GP_HYP] = false;  // (never a stale interval after a call that launched nothing)
  const GpFitShape sh = gp_fit_shape(H, init_N, opts_N, n_samples);
  const int B = sh.B, R = sh.R, Cn = sh.C, S = sh.S;
  WarpArgErr err;
  GpCandPlan pl;
  auto own = [&](WarpArgErr& e) {
    return gp_fit_check_own(e, who, P, H, hyp0_HxP, init_N, dlb_P, dub_P, lb_P, ub_P, opts_N, max_iter, m, tol_g, tol_f,
                            n_samples, widths_P, thin, burn_in);
  };
  if (gp_cand_check(err, who, 'B', N, D, sh.runs, P, mean_kind, lb_P, ub_P, prior_mu_P, prior_sigma_P, prior_df_P, s2_N,
                    ctx->opt_gp_lml_chunk, own, pl))
    return vbmc_fail(ctx, err.code, "%s", err.msg);
  int rc = gp_cand_begin(ctx, N, D, P, std::max(pl.chunk, S));
  if (rc) return rc;
  if (R == 0) m = 1;

  // ---- the call's device scratch, listed once (ctx->d_post_ws): a chunk's workspace with one slot per run of the
  // largest stage, the inverted blocks of the final build where it has more samples than a chunk, the `in` block, then
  // what is zeroed -- the count, the order, the drivers' starts and state -- and the results in one block that comes back
  // in one copy
  const size_t bp = (size_t)B * P, rp = (size_t)R * P, cp = (size_t)Cn * P, nb = ((size_t)N + 63) / 64;
  Scratch sc;
  const GpLmlWs ws = gp_lml_ws(sc, N, D, P, pl.mean_n, pl.chunk, sh.runs, R > 0 ? 1 : 0);
  const auto p_bDinv = sc.add(S > pl.chunk ? (size_t)S * nb * 64 * 64 : 0);
  const auto p_in = sc.add(gp_cand_in_elems(H, P, 3, N, s2_N != nullptr));
  const auto p_count = sc.add<int>(2);
  const auto p_order = sc.add<int>((size_t)B);
  const auto p_ox0 = sc.add(rp), p_ostate = sc.add((size_t)R * gp_opt_state_elems(P, m)), p_ograd = sc.add(rp);
  const auto p_cx0 = sc.add(cp), p_cx = sc.add(cp), p_cxp = sc.add(cp);
  const auto p_cstate = sc.add((size_t)Cn * gp_hyp_state_elems());
  const auto p_cand = sc.add(bp), p_score = sc.add((size_t)B);
  const auto p_starts = sc.add<int>((size_t)R);
  const auto p_ohyp = sc.add(rp), p_olpost = sc.add((size_t)R);
  const auto p_ostats = sc.add<long long>(4 * (size_t)R);
  const auto p_oinv = sc.add<int>((size_t)R);
  const auto p_best = sc.add((size_t)P), p_bestlp = sc.add(1);
  const auto p_chyp = sc.add(cp), p_clpost = sc.add((size_t)Cn), p_clprior = sc.add((size_t)Cn);
  const auto p_cstats = sc.add<long long>(4 * (size_t)Cn);
  const auto p_cinv = sc.add<int>((size_t)Cn);
  const auto p_hyp = sc.add((size_t)S * P), p_noise = sc.add((size_t)S);
  const auto p_bad = sc.add<int>((size_t)S);
  const auto p_status = sc.add<int>(2);
  const auto p_bflag = gp_post_flags(sc, S);
  if ((rc = reserve_in(ctx, &ctx->d_post_ws, &ctx->d_post_ws_cap, sc))) return rc;
  if ((rc = ensure_pinned(ctx, sc.total - p_cand.off))) return rc;

  GpFitArgs f;
  f.N = N; f.D = D; f.P = P; f.H = H; f.B = B; f.R = R; f.C = Cn; f.S = S;
  f.seed = seed;
  f.s2_min = pl.s2_min;
  // (an absent array still takes its P slots of the block: the stage that would read it does not run)
  const std::vector<double> in =
      gp_cand_pack(f, sc.ptr(p_in), H, H > 0 ? hyp0_HxP : lb_P, {dlb_P ? dlb_P : lb_P, dub_P ? dub_P : ub_P, widths_P ? widths_P : ub_P},
                   lb_P, ub_P, prior_mu_P, prior_sigma_P, prior_df_P, s2_N);
  f.dlb = f.x0 + (size_t)H * P;
  f.dub = f.dlb + P;
  const double* d_widths = f.dub + P;
  f.cand = sc.ptr(p_cand); f.score = sc.ptr(p_score);
  f.order = sc.ptr(p_order); f.starts = sc.ptr(p_starts);
  f.opt_x0 = sc.ptr(p_ox0); f.opt_hyp = sc.ptr(p_ohyp); f.opt_logpost = sc.ptr(p_olpost); f.opt_invalid = sc.ptr(p_oinv);
  f.best = sc.ptr(p_best); f.best_logpost = sc.ptr(p_bestlp);
  f.chain_x0 = sc.ptr(p_cx0); f.chain_hyp = sc.ptr(p_chyp); f.chain_invalid = sc.ptr(p_cinv);
  f.hyp = sc.ptr(p_hyp); f.noise = sc.ptr(p_noise);
  f.bad = sc.ptr(p_bad); f.status = sc.ptr(p_status);
  if ((rc = gp_cand_stage(ctx, who, sc, ws, sc.ptr(p_in), in, p_count.off, mean_kind, X_NxD, y_N, f))) return rc;
  GpLmlWs wv = ws;  // the same workspace, value only: the scores and the chains need no gradient
  wv.want_grad = 0;
  auto fail = [&](int code) {  // nothing is installed: ctx->gp is what it was
    (void)hipStreamSynchronize(ctx->stream);
    return code;
  };

  // ---- 1, 2: the design, then every candidate staged, factorised chunk by chunk, scored and ranked
  rc = launch_gp_fit_design(ctx, f);
  for (int b0 = 0; b0 < B && !rc; b0 += pl.chunk) {
    const int Sb = std::min(pl.chunk, B - b0);
    if (!(rc = launch_gp_fit_stage(ctx, f, b0, Sb))) rc = gp_lml_chunk(ctx, sc, wv, Sb, b0);
  }
  if (!rc) rc = launch_gp_fit_rank(ctx, f);
  if (rc) return fail(rc);

  // ---- 3: the optimiser from the gathered starts (api_gp_opt.hip's rounds), then the optimum and the chains' starts
  long long rounds = 0;
  int left = 0;
  if (R > 0) {
    GpOptArgs a;
    static_cast<GpCandArgs&>(a) = f;
    a.R = R; a.max_iter = max_iter; a.m = m; a.trace_cap = 0;
    a.tol_g = tol_g; a.tol_f = tol_f;
    a.x0 = f.opt_x0;
    a.dlml = sc.ptr(ws.dlml);
    a.dsn2 = sc.ptr(ws.dsn2);
    a.state = sc.ptr(p_ostate);
    a.hyp_out = sc.ptr(p_ohyp); a.logpost = sc.ptr(p_olpost); a.grad = sc.ptr(p_ograd);
    a.stats = sc.ptr(p_ostats);
    a.invalid = sc.ptr(p_oinv);
    auto round = [&](long long) {
      return gp_cand_round(ctx, sc, ws, R, pl.chunk, [&](int b0, int Sb) { return launch_gp_opt_advance(ctx, a, b0, Sb); });
    };
    rc = timing_begin(ctx, T_GP_OPT);
    if (!rc)
      rc = lockstep_rounds(ctx, who, ctx->opt_gp_opt_rounds, 2 + (long long)max_iter * 31, R, a.state, gp_opt_done_word(P, m),
                           sc.ptr(p_count), round, &rounds, &left);
    if (!rc) rc = timing_end(ctx, T_GP_OPT);
    if (rc) return fail(rc);
    if (left > 0) return vbmc_fail(ctx, VBMC_E_HIP, "%s: %d runs unfinished after %lld rounds", who, left, rounds);
  }
  if ((rc = launch_gp_fit_select(ctx, f))) return fail(rc);

  // ---- 4: the chains from the tiled optimum (api_gp_hyp.hip's rounds), one kept sample each
  if (Cn > 0) {
    GpHypArgs a;
    static_cast<GpCandArgs&>(a) = f;
    a.C = Cn; a.n = 1; a.thin = thin; a.burn_in = burn_in;
    a.seed = seed;
    a.x0 = f.chain_x0;
    a.widths = d_widths;
    a.x = sc.ptr(p_cx); a.xp = sc.ptr(p_cxp);
    a.state = sc.ptr(p_cstate);
    a.hyp_out = sc.ptr(p_chyp); a.logpost = sc.ptr(p_clpost); a.logprior = sc.ptr(p_clprior);
    a.stats = sc.ptr(p_cstats);
    a.invalid = sc.ptr(p_cinv);
    auto round = [&](long long) {
      return gp_cand_round(ctx, sc, wv, Cn, pl.chunk, [&](int b0, int Sb) { return launch_gp_hyp_advance(ctx, a, b0, Sb); });
    };
    const long long max_rounds = 2 + ((long long)burn_in + thin) * P * (2 * 32 + 64);
    rc = timing_begin(ctx, T_GP_HYP);
    if (!rc)
      rc = lockstep_rounds(ctx, who, ctx->opt_gp_hyp_rounds, max_rounds, Cn, a.state, gp_hyp_done_word(), sc.ptr(p_count),
                           round, &rounds, &left);
    if (!rc) rc = timing_end(ctx, T_GP_HYP);
    if (rc) return fail(rc);
    if (left > 0) return vbmc_fail(ctx, VBMC_E_HIP, "%s: %d chains unfinished after %lld rounds", who, left, rounds);
  }

  // ---- 5: the samples handed to the build on the device; the state under construction becomes ctx->gp for the build and
  // stays only when every sample is usable and factorised (as vbmc_gp_posterior installs its own)
  if ((rc = launch_gp_fit_handover(ctx, f))) return fail(rc);
  ctx->gp_next.S = S;
  std::swap(ctx->gp, ctx->gp_next);
  rc = launch_gp_post_build(ctx, S > pl.chunk ? sc.ptr(p_bDinv) : sc.ptr(ws.Dinv), sc.ptr(p_bflag));
  std::vector<int> bad(S, 0), bflag(S, 0), cinv(Cn, 0);
  if (!rc)
    rc = fetch_tail(ctx, sc, p_cand.off,
                    {{p_cand.off, cand_BxP, sizeof(double) * bp},
                     {p_score.off, score_B, sizeof(double) * B},
                     {p_starts.off, starts_R, sizeof(int32_t) * R},
                     {p_ohyp.off, opt_hyp_RxP, sizeof(double) * rp},
                     {p_olpost.off, opt_logpost_R, sizeof(double) * R},
                     {p_ostats.off, opt_stats_Rx4, sizeof(int64_t) * 4 * R},
                     {p_oinv.off, opt_invalid_R, sizeof(int32_t) * R},
                     {p_best.off, best_P, sizeof(double) * P},
                     {p_bestlp.off, best_logpost, sizeof(double)},
                     {p_hyp.off, hyp_SxP, sizeof(double) * S * P},
                     {p_clpost.off, logpost_S, sizeof(double) * Cn},
                     {p_clprior.off, logprior_S, sizeof(double) * Cn},
                     {p_cstats.off, stats_Sx4, sizeof(int64_t) * 4 * Cn},
                     {p_cinv.off, cinv.data(), sizeof(int) * Cn},
                     {p_noise.off, noise_S, sizeof(double) * S},
                     {p_bad.off, bad.data(), sizeof(int) * S},
                     {p_status.off, status, sizeof(int32_t)},
                     {p_bflag.off, bflag.data(), sizeof(int) * S}});
  if (rc) {
    (void)hipStreamSynchronize(ctx->stream);
    std::swap(ctx->gp, ctx->gp_next);  // the state installed before, untouched
    return rc;
  }
  if (Cn == 0 && logpost_S) logpost_S[0] = *best_logpost;
  int unusable = -1;
  for (int s = 0; s < S && unusable < 0; ++s)
    if (bad[s] || bflag[s]) unusable = s;
  if (*status != 0 || unusable >= 0) {
    std::swap(ctx->gp, ctx->gp_next);
    if (*status != 0) return VBMC_OK;  // "no candidate has a finite score": reported, not an error
    return vbmc_fail(ctx, VBMC_E_NOTPD, "%s: sample %d: %s", who, unusable,
                     bad[unusable] ? "its chain had no finite start" : "the matrix is not positive definite");
  }

  // ---- the host's copy of the state, from the samples that came back, and the uploads predict reads
  GpState& g = ctx->gp;
  g.hyp.assign(hyp_SxP, hyp_SxP + (size_t)S * P);
  g.h_sl.resize(S);
  g.h_sn2.resize((size_t)S * N);
  g.homo = true;
  for (int s = 0; s < S; ++s) {
    g.h_sl[s] = noise_S[s] + pl.s2_min;  // (gp_cand.h's sums, bit for bit)
    for (int n = 0; n < N; ++n) {
      const double v = s2_N ? noise_S[s] + s2_N[n] : noise_S[s];
      g.h_sn2[(size_t)s * N + n] = v;
      g.homo = g.homo && v == g.h_sl[s];
    }
  }
  std::vector<double> sW_host;
  gp_post_host_fields(g, N, D, S, P, mean_kind, sW_host);
  hipStream_t st = ctx->stream;
  hipError_t e = hipMemcpyAsync(g.d_smeta, g.h_small.data() + D, sizeof(double) * 3 * S, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(g.d_xc, g.h_small.data(), sizeof(double) * D, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(g.d_sW, sW_host.data(), sizeof(double) * S * N, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && alpha_SxN)
    e = hipMemcpyAsync(alpha_SxN, g.d_alpha, sizeof(double) * S * N, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && L_SxNxN)
    e = hipMemcpyAsync(L_SxNxN, g.d_L, sizeof(double) * S * N * N, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = stream_wait(ctx);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(st);
    std::swap(ctx->gp, ctx->gp_next);
    return vbmc_fail(ctx, VBMC_E_HIP, "%s: %s", who, hipGetErrorString(e));
  }
  g.set = true;
  g.dev_built = true;
  ctx->gp_watch_ptrs.clear();
  ctx->gp_watch_lens.clear();
  return VBMC_OK;
}
