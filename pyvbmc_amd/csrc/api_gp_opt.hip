// C-ABI entry point of GP hyper-parameter optimisation: vbmc_gp_hyp_optimize.  R quasi-Newton runs over
// phi(h) = -(lml(h) + log p(h)) in lockstep (gp_opt.hip): a round is one advance launch, then the factorisation and the
// value and gradient kernels of vbmc_gp_lml on the trial points the runs left in ctx->gp_next.  As in vbmc_gp_hyp_sample,
// the staged state is swapped in for its launches and swapped back on every path, so the installed GP is what it was.
// The host queues opt_gp_opt_rounds rounds, then reads ONE int (the runs that have not finished) and goes on while it is
// not zero; X, X^T, y, s2 and the runs' arguments go up once, the results come back once.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

#include "common.h"

namespace {

// the constant part of a parameter's prior term (gp_cand.h): everything of t_p that does not depend on h_p
double prior_const(double sigma, double df) {
  if (sigma != sigma) return 0.0;
  if (std::isinf(df)) return -0.5 * std::log(2.0 * M_PI) - std::log(sigma);
  return std::lgamma(0.5 * (df + 1.0)) - std::lgamma(0.5 * df) - 0.5 * std::log(M_PI * df) - std::log(sigma);
}

}  // namespace

extern "C" int vbmc_gp_hyp_optimize(vbmc_ctx* ctx, int N, int D, int P, int mean_kind, const double* X_NxD,
                                    const double* y_N, const double* s2_N, int R, const double* x0_RxP, const double* lb_P,
                                    const double* ub_P, const double* prior_mu_P, const double* prior_sigma_P,
                                    const double* prior_df_P, int max_iter, int m, double tol_g, double tol_f, int trace_cap,
                                    double* hyp_RxP, double* logpost_R, double* grad_RxP, int64_t* stats_Rx4,
                                    int32_t* invalid_R, double* trace_iter, double* trace_eval) {
  if (!ctx || !X_NxD || !y_N || !x0_RxP || !lb_P || !ub_P || !prior_mu_P || !prior_sigma_P || !prior_df_P || !hyp_RxP ||
      !logpost_R || !grad_RxP || !stats_Rx4 || !invalid_R)
    return VBMC_E_ARG;
  ctx->ev_valid[T_GP_OPT] = false;  // (never a stale interval after a call that launched nothing)
  if (N < 1 || D < 1 || R < 1) return vbmc_fail(ctx, VBMC_E_ARG, "gp_hyp_optimize: bad N=%d D=%d R=%d", N, D, R);
  const int mean_n = mean_kind == VBMC_MEAN_ZERO ? 0 : mean_kind == VBMC_MEAN_CONST ? 1 : 1 + 2 * D;
  if (mean_kind < 0 || mean_kind > 2 || P != D + 2 + mean_n)
    return vbmc_fail(ctx, VBMC_E_ARG, "gp_hyp_optimize: P=%d does not match D+2+mean(%d)=%d", P, mean_kind, D + 2 + mean_n);
  if (max_iter < 0 || max_iter > 1000000 || m < 1 || m > 16 || !(tol_g >= 0.0) || !(tol_f >= 0.0) || trace_cap < 0 ||
      trace_cap > max_iter + 1)
    return vbmc_fail(ctx, VBMC_E_ARG, "gp_hyp_optimize: bad max_iter=%d m=%d tol_g=%g tol_f=%g trace_cap=%d", max_iter, m,
                     tol_g, tol_f, trace_cap);
  if (trace_cap > 0 && (!trace_iter || !trace_eval))
    return vbmc_fail(ctx, VBMC_E_ARG, "gp_hyp_optimize: trace_cap > 0 without the trace arrays");
  for (int p = 0; p < P; ++p) {
    if (!std::isfinite(lb_P[p]) || !std::isfinite(ub_P[p]) || lb_P[p] > ub_P[p])
      return vbmc_fail(ctx, VBMC_E_ARG, "gp_hyp_optimize: bounds of parameter %d are not finite or lb > ub", p);
    if (prior_sigma_P[p] == prior_sigma_P[p] &&
        (!(prior_sigma_P[p] > 0.0) || !std::isfinite(prior_sigma_P[p]) || !std::isfinite(prior_mu_P[p]) || !(prior_df_P[p] > 0.0)))
      return vbmc_fail(ctx, VBMC_E_ARG, "gp_hyp_optimize: prior of parameter %d needs finite mu, sigma > 0 and df > 0 (or +inf)", p);
  }
  double s2_min = 0.0;
  if (s2_N) {
    s2_min = s2_N[0];
    for (int i = 0; i < N; ++i) {
      if (!(s2_N[i] >= 0.0) || !std::isfinite(s2_N[i]))
        return vbmc_fail(ctx, VBMC_E_ARG, "gp_hyp_optimize: s2[%d] is not a finite number >= 0", i);
      s2_min = std::min(s2_min, s2_N[i]);
    }
  }
  if (D > 32) return vbmc_fail(ctx, VBMC_E_UNSUP, "gp_hyp_optimize: D=%d > 32 not supported", D);
  if (!(std::exp(2.0 * lb_P[D + 1]) + s2_min >= 1e-6))
    return vbmc_fail(ctx, VBMC_E_UNSUP, "gp_hyp_optimize: the noise bound allows sn2_div < 1e-6: the non-Cholesky branch is computed on the host");
  const int chunk = gp_lml_plan(N, D, R, GP_LML_CAP_BYTES, ctx->opt_gp_lml_chunk);
  if (chunk < 1)
    return vbmc_fail(ctx, VBMC_E_UNSUP, "gp_hyp_optimize: the factor state of one candidate of N=%d points exceeds %zu bytes", N,
                     GP_LML_CAP_BYTES);
  NEED_DEVICE(ctx);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, stream_wait(ctx));
  GpState& w = ctx->gp_next;
  int rc = gp_state_grow(ctx, w, N, D, chunk, P, true);
  if (rc) return rc;

  // ---- the call's device scratch, listed once (ctx->d_post_ws): what the factorisation and the value and gradient
  // kernels of a chunk use, the round's results per run, the runs' arguments, their state, and the results in one block
  // that comes back in one copy
  const int nb = (N + 63) / 64;
  const size_t se = gp_opt_state_elems(P, m), rp = (size_t)R * P;
  const size_t n_it = (size_t)R * trace_cap * (3 * (size_t)P + 3), n_ev = trace_cap ? (size_t)R * (1 + 31 * (size_t)trace_cap) * 4 : 0;
  Scratch sc;
  const auto p_flag = gp_post_flags(sc, R);
  const auto p_Dinv = sc.add((size_t)chunk * nb * 64 * 64);
  const auto p_part = sc.add((size_t)chunk * gp_lml_part_elems(N, D));
  const auto p_mg = sc.add((size_t)chunk * mean_n);
  const auto p_sums = sc.add(2 * (size_t)chunk);
  const auto p_dsn2 = sc.add((size_t)chunk);
  const auto p_lml = sc.add((size_t)R);
  const auto p_dlml = sc.add(rp);
  const auto p_count = sc.add<int>(2);
  const auto p_in = sc.add(rp + 6 * (size_t)P + (s2_N ? (size_t)N : 0));  // x0 | lb ub mu sigma df const | s2
  const auto p_state = sc.add((size_t)R * se);
  const auto p_hyp = sc.add(rp), p_lpost = sc.add((size_t)R), p_grad = sc.add(rp);
  const auto p_stats = sc.add<long long>(4 * (size_t)R);
  const auto p_inv = sc.add<int>((size_t)R);
  const auto p_tit = sc.add(n_it), p_tev = sc.add(n_ev);
  const size_t n_out = sc.total - p_hyp.off;
  rc = reserve_in(ctx, &ctx->d_post_ws, &ctx->d_post_ws_cap, sc);
  if (rc) return rc;
  if ((rc = ensure_pinned(ctx, std::max(n_out, (size_t)1)))) return rc;

  // ---- uploads, once per call: X, X^T, y (the staged state's fields as vbmc_gp_lml sets them), the arguments
  w.set = false;
  w.dev_built = false;
  w.homo = false;
  w.N = N; w.D = D; w.P = P; w.mean_kind = mean_kind;
  w.h_X.assign(X_NxD, X_NxD + (size_t)N * D);
  w.h_y.assign(y_N, y_N + N);
  w.h_XT.resize((size_t)N * D);
  for (int i = 0; i < N; ++i)
    for (int d = 0; d < D; ++d) w.h_XT[(size_t)d * N + i] = X_NxD[(size_t)i * D + d];
  std::vector<double> in(p_in.count);
  {
    double* q = in.data();
    memcpy(q, x0_RxP, sizeof(double) * rp); q += rp;
    memcpy(q, lb_P, sizeof(double) * P); q += P;
    memcpy(q, ub_P, sizeof(double) * P); q += P;
    memcpy(q, prior_mu_P, sizeof(double) * P); q += P;
    memcpy(q, prior_sigma_P, sizeof(double) * P); q += P;
    memcpy(q, prior_df_P, sizeof(double) * P); q += P;
    for (int p = 0; p < P; ++p) q[p] = prior_const(prior_sigma_P[p], prior_df_P[p]);
    q += P;
    if (s2_N) memcpy(q, s2_N, sizeof(double) * N);
  }
  hipStream_t st = ctx->stream;
  double* d_in = sc.ptr(p_in);
  {
    hipError_t e = hipMemcpyAsync(w.d_X, w.h_X.data(), sizeof(double) * N * D, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(w.d_XT, w.h_XT.data(), sizeof(double) * N * D, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(w.d_y, w.h_y.data(), sizeof(double) * N, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_in, in.data(), sizeof(double) * in.size(), hipMemcpyHostToDevice, st);
    // flags cleared; value, gradient and count zero; a zeroed state = every run at its start, and zeros where an invalid
    // run writes nothing
    if (e == hipSuccess) e = hipMemsetAsync(sc.base, 0, sizeof(double) * p_Dinv.off, st);
    if (e == hipSuccess) e = hipMemsetAsync(sc.ptr(p_sums), 0, sizeof(double) * (p_in.off - p_sums.off), st);
    if (e == hipSuccess) e = hipMemsetAsync(sc.ptr(p_state), 0, sizeof(double) * (sc.total - p_state.off), st);
    if (e != hipSuccess) {
      (void)hipStreamSynchronize(st);
      return vbmc_fail(ctx, VBMC_E_HIP, "gp_hyp_optimize: %s", hipGetErrorString(e));
    }
  }

  GpOptArgs a;
  a.N = N; a.D = D; a.P = P; a.R = R; a.max_iter = max_iter; a.m = m; a.trace_cap = trace_cap;
  a.tol_g = tol_g; a.tol_f = tol_f;
  a.s2_min = s2_min;
  a.x0 = d_in;
  a.lb = d_in + rp; a.ub = a.lb + P;
  a.pmu = a.ub + P; a.psig = a.pmu + P; a.pdf = a.psig + P; a.pconst = a.pdf + P;
  a.s2 = s2_N ? a.pconst + P : nullptr;
  a.lml = sc.ptr(p_lml); a.dlml = sc.ptr(p_dlml);
  a.flag = sc.ptr(p_flag);
  a.dsn2 = sc.ptr(p_dsn2);
  a.state = sc.ptr(p_state);
  a.hyp_out = sc.ptr(p_hyp); a.logpost = sc.ptr(p_lpost); a.grad = sc.ptr(p_grad);
  a.stats = sc.ptr(p_stats);
  a.invalid = sc.ptr(p_inv);
  a.trace_it = sc.ptr(p_tit); a.trace_ev = sc.ptr(p_tev);
  a.g_hyp = w.d_hyp; a.g_sl = w.d_sl; a.g_smeta = w.d_smeta; a.g_sn2 = w.d_sn2;
  int* d_count = sc.ptr(p_count);
  int* h_count = (int*)ctx->h_pinned;

  // ---- rounds.  The largest number a run can need: the round that submits the start, the start's evaluation, 31 trial
  // points (30 halvings) per iteration, and the advance that consumes the last of them.
  const long long max_rounds = 2 + (long long)max_iter * 31;
  const int per_batch = ctx->opt_gp_opt_rounds;
  long long rounds = 0;
  int left = R;
  rc = timing_begin(ctx, T_GP_OPT);
  while (!rc && left > 0 && rounds < max_rounds) {
    for (int r = 0; r < per_batch && rounds < max_rounds && !rc; ++r, ++rounds) {
      for (int b0 = 0; b0 < R && !rc; b0 += chunk) {
        const int S = std::min(chunk, R - b0);
        rc = launch_gp_opt_advance(ctx, a, b0, S);
        if (rc) break;
        w.S = S;
        std::swap(ctx->gp, ctx->gp_next);  // the chunk becomes ctx->gp for its launches only
        rc = launch_gp_post_build(ctx, sc.ptr(p_Dinv), sc.ptr(p_flag) + b0);
        if (!rc)
          rc = launch_gp_lml(ctx, 1, sc.ptr(p_dsn2), sc.ptr(p_sums), sc.ptr(p_part), sc.ptr(p_mg), sc.ptr(p_lml) + b0,
                             sc.ptr(p_dlml) + (size_t)b0 * P);
        std::swap(ctx->gp, ctx->gp_next);  // the installed state again, whatever happened
      }
    }
    if (!rc) rc = launch_gp_opt_count(ctx, a, d_count);
    if (!rc) {
      hipError_t e = hipMemcpyAsync(h_count, d_count, sizeof(int), hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = stream_wait(ctx);
      if (e != hipSuccess) rc = vbmc_fail(ctx, VBMC_E_HIP, "gp_hyp_optimize: %s", hipGetErrorString(e));
      else left = *h_count;
    }
  }
  if (!rc) rc = timing_end(ctx, T_GP_OPT);
  if (rc) {
    (void)hipStreamSynchronize(st);
    return rc;
  }
  if (left > 0) return vbmc_fail(ctx, VBMC_E_HIP, "gp_hyp_optimize: %d runs unfinished after %lld rounds", left, rounds);

  // ---- the results, one copy (the pinned copy keeps the pieces' spacing)
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_pinned, a.hyp_out, sizeof(double) * n_out, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, stream_wait(ctx));
  const double* h = ctx->h_pinned;
  const size_t o0 = p_hyp.off;
  memcpy(hyp_RxP, h, sizeof(double) * rp);
  memcpy(logpost_R, h + (p_lpost.off - o0), sizeof(double) * R);
  memcpy(grad_RxP, h + (p_grad.off - o0), sizeof(double) * rp);
  memcpy(stats_Rx4, h + (p_stats.off - o0), sizeof(int64_t) * 4 * R);
  memcpy(invalid_R, h + (p_inv.off - o0), sizeof(int32_t) * R);
  if (trace_cap > 0) {
    memcpy(trace_iter, h + (p_tit.off - o0), sizeof(double) * n_it);
    memcpy(trace_eval, h + (p_tev.off - o0), sizeof(double) * n_ev);
  }
  return VBMC_OK;
}
