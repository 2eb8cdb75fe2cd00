// C-ABI entry point of GP hyper-parameter sampling: vbmc_gp_hyp_sample.  C slice-sampling chains over
// f(h) = lml(h) + log p(h) in lockstep (gp_hyp.hip): a round is one advance launch, then the factorisation and the value
// kernels of vbmc_gp_lml on the candidates the chains left in ctx->gp_next.  As there, the staged state is swapped in
// for its launches and swapped back on every path, so the installed GP is what it was.  The host queues
// opt_gp_hyp_rounds rounds, then reads ONE int (the chains that have not finished) and goes on while it is not zero; X,
// X^T, y, s2 and the chains' arguments go up once, the kept samples come back once.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <utility>
#include <vector>

#include "common.h"

namespace {

// the constant part of a parameter's prior term (gp_hyp.hip): everything of t_p that does not depend on h_p
double prior_const(double sigma, double df) {
  if (sigma != sigma) return 0.0;
  if (std::isinf(df)) return -0.5 * std::log(2.0 * M_PI) - std::log(sigma);
  return std::lgamma(0.5 * (df + 1.0)) - std::lgamma(0.5 * df) - 0.5 * std::log(M_PI * df) - std::log(sigma);
}

}  // namespace

extern "C" int vbmc_gp_hyp_sample(vbmc_ctx* ctx, int N, int D, int P, int mean_kind, const double* X_NxD, const double* y_N,
                                  const double* s2_N, int C, const double* x0_CxP, const double* widths_P, const double* lb_P,
                                  const double* ub_P, const double* prior_mu_P, const double* prior_sigma_P,
                                  const double* prior_df_P, int n, int thin, int burn_in, uint64_t seed, double* hyp_CxnxP,
                                  double* logpost_Cxn, double* logprior_Cxn, int64_t* stats_Cx4, int32_t* invalid_C) {
  if (!ctx || !X_NxD || !y_N || !x0_CxP || !widths_P || !lb_P || !ub_P || !prior_mu_P || !prior_sigma_P || !prior_df_P ||
      !hyp_CxnxP || !logpost_Cxn || !logprior_Cxn || !stats_Cx4 || !invalid_C)
    return VBMC_E_ARG;
  ctx->ev_valid[T_GP_HYP] = false;  // (never a stale interval after a call that launched nothing)
  if (N < 1 || D < 1 || C < 1) return vbmc_fail(ctx, VBMC_E_ARG, "gp_hyp_sample: bad N=%d D=%d C=%d", N, D, C);
  const int mean_n = mean_kind == VBMC_MEAN_ZERO ? 0 : mean_kind == VBMC_MEAN_CONST ? 1 : 1 + 2 * D;
  if (mean_kind < 0 || mean_kind > 2 || P != D + 2 + mean_n)
    return vbmc_fail(ctx, VBMC_E_ARG, "gp_hyp_sample: P=%d does not match D+2+mean(%d)=%d", P, mean_kind, D + 2 + mean_n);
  if (n < 1 || thin < 1 || burn_in < 0)
    return vbmc_fail(ctx, VBMC_E_ARG, "gp_hyp_sample: bad n=%d thin=%d burn_in=%d", n, thin, burn_in);
  for (int p = 0; p < P; ++p) {
    if (!std::isfinite(lb_P[p]) || !std::isfinite(ub_P[p]) || lb_P[p] > ub_P[p])
      return vbmc_fail(ctx, VBMC_E_ARG, "gp_hyp_sample: bounds of parameter %d are not finite or lb > ub", p);
    if (!(widths_P[p] > 0.0) || !std::isfinite(widths_P[p]))
      return vbmc_fail(ctx, VBMC_E_ARG, "gp_hyp_sample: width of parameter %d is not a positive finite number", p);
    if (prior_sigma_P[p] == prior_sigma_P[p] &&
        (!(prior_sigma_P[p] > 0.0) || !std::isfinite(prior_sigma_P[p]) || !std::isfinite(prior_mu_P[p]) || !(prior_df_P[p] > 0.0)))
      return vbmc_fail(ctx, VBMC_E_ARG, "gp_hyp_sample: prior of parameter %d needs finite mu, sigma > 0 and df > 0 (or +inf)", p);
  }
  double s2_min = 0.0;
  if (s2_N) {
    s2_min = s2_N[0];
    for (int i = 0; i < N; ++i) {
      if (!(s2_N[i] >= 0.0) || !std::isfinite(s2_N[i]))
        return vbmc_fail(ctx, VBMC_E_ARG, "gp_hyp_sample: s2[%d] is not a finite number >= 0", i);
      s2_min = std::min(s2_min, s2_N[i]);
    }
  }
  if (D > 32) return vbmc_fail(ctx, VBMC_E_UNSUP, "gp_hyp_sample: D=%d > 32 not supported", D);
  if (!(std::exp(2.0 * lb_P[D + 1]) + s2_min >= 1e-6))
    return vbmc_fail(ctx, VBMC_E_UNSUP, "gp_hyp_sample: the noise bound allows sn2_div < 1e-6: the non-Cholesky branch is computed on the host");
  const int chunk = gp_lml_plan(N, D, C, GP_LML_CAP_BYTES, ctx->opt_gp_lml_chunk);
  if (chunk < 1)
    return vbmc_fail(ctx, VBMC_E_UNSUP, "gp_hyp_sample: the factor state of one candidate of N=%d points exceeds %zu bytes", N,
                     GP_LML_CAP_BYTES);
  NEED_DEVICE(ctx);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, stream_wait(ctx));
  GpState& w = ctx->gp_next;
  int rc = gp_state_grow(ctx, w, N, D, chunk, P, true);
  if (rc) return rc;

  // ---- the call's device scratch, listed once (ctx->d_post_ws): what the factorisation and the value kernels of a chunk
  // use, the chains' arguments, their state, and the results in one block that comes back in one copy
  const int nb = (N + 63) / 64;
  const size_t se = gp_hyp_state_elems(), cp = (size_t)C * P, cn = (size_t)C * n;
  Scratch sc;
  const auto p_flag = gp_post_flags(sc, C);
  const auto p_Dinv = sc.add((size_t)chunk * nb * 64 * 64);
  const auto p_sums = sc.add(2 * (size_t)chunk);
  const auto p_dsn2 = sc.add((size_t)chunk);  // (read by the gradient's outputs only: none here)
  const auto p_lml = sc.add((size_t)C);
  const auto p_count = sc.add<int>(2);
  const auto p_in = sc.add(cp + 7 * (size_t)P + (s2_N ? (size_t)N : 0));  // x0 | widths lb ub mu sigma df const | s2
  const auto p_x = sc.add(cp), p_xp = sc.add(cp);
  const auto p_state = sc.add((size_t)C * se);
  const auto p_hyp = sc.add(cn * P), p_lpost = sc.add(cn), p_lprior = sc.add(cn);
  const auto p_stats = sc.add<long long>(4 * (size_t)C);
  const auto p_inv = sc.add<int>((size_t)C);
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
    memcpy(q, x0_CxP, sizeof(double) * cp); q += cp;
    memcpy(q, widths_P, sizeof(double) * P); q += P;
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
    // flags cleared, lml zero, a zeroed state = every chain at its start, and zeros where an invalid chain writes nothing
    if (e == hipSuccess) e = hipMemsetAsync(sc.base, 0, sizeof(double) * p_in.off, st);
    if (e == hipSuccess) e = hipMemsetAsync(sc.ptr(p_x), 0, sizeof(double) * (sc.total - p_x.off), st);
    if (e != hipSuccess) {
      (void)hipStreamSynchronize(st);
      return vbmc_fail(ctx, VBMC_E_HIP, "gp_hyp_sample: %s", hipGetErrorString(e));
    }
  }

  GpHypArgs a;
  a.N = N; a.D = D; a.P = P; a.C = C; a.n = n; a.thin = thin; a.burn_in = burn_in;
  a.seed = seed;
  a.s2_min = s2_min;
  a.x0 = d_in;
  a.widths = d_in + cp; a.lb = a.widths + P; a.ub = a.lb + P;
  a.pmu = a.ub + P; a.psig = a.pmu + P; a.pdf = a.psig + P; a.pconst = a.pdf + P;
  a.s2 = s2_N ? a.pconst + P : nullptr;
  a.lml = sc.ptr(p_lml);
  a.flag = sc.ptr(p_flag);
  a.x = sc.ptr(p_x); a.xp = sc.ptr(p_xp);
  a.state = sc.ptr(p_state);
  a.hyp_out = sc.ptr(p_hyp); a.logpost = sc.ptr(p_lpost); a.logprior = sc.ptr(p_lprior);
  a.stats = sc.ptr(p_stats);
  a.invalid = sc.ptr(p_inv);
  a.g_hyp = w.d_hyp; a.g_sl = w.d_sl; a.g_smeta = w.d_smeta; a.g_sn2 = w.d_sn2;
  int* d_count = sc.ptr(p_count);
  int* h_count = (int*)ctx->h_pinned;

  // ---- rounds.  The largest number a chain can need: the start, one evaluation per step-out and shrink step of every
  // coordinate update, and the advance that consumes the last value.
  const long long max_rounds = 2 + ((long long)burn_in + (long long)n * thin) * P * (2 * 32 + 64);
  const int per_batch = ctx->opt_gp_hyp_rounds;
  long long rounds = 0;
  int left = C;
  rc = timing_begin(ctx, T_GP_HYP);
  while (!rc && left > 0 && rounds < max_rounds) {
    for (int r = 0; r < per_batch && !rc; ++r, ++rounds) {
      for (int b0 = 0; b0 < C && !rc; b0 += chunk) {
        const int S = std::min(chunk, C - b0);
        rc = launch_gp_hyp_advance(ctx, a, b0, S);
        if (rc) break;
        w.S = S;
        std::swap(ctx->gp, ctx->gp_next);  // the chunk becomes ctx->gp for its launches only
        rc = launch_gp_post_build(ctx, sc.ptr(p_Dinv), sc.ptr(p_flag) + b0);
        if (!rc)
          rc = launch_gp_lml(ctx, 0, sc.ptr(p_dsn2), sc.ptr(p_sums), nullptr, nullptr, sc.ptr(p_lml) + b0, nullptr);
        std::swap(ctx->gp, ctx->gp_next);  // the installed state again, whatever happened
      }
    }
    if (!rc) rc = launch_gp_hyp_count(ctx, a.state, C, d_count);
    if (!rc) {
      hipError_t e = hipMemcpyAsync(h_count, d_count, sizeof(int), hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = stream_wait(ctx);
      if (e != hipSuccess) rc = vbmc_fail(ctx, VBMC_E_HIP, "gp_hyp_sample: %s", hipGetErrorString(e));
      else left = *h_count;
    }
  }
  if (!rc) rc = timing_end(ctx, T_GP_HYP);
  if (rc) {
    (void)hipStreamSynchronize(st);
    return rc;
  }
  if (left > 0) return vbmc_fail(ctx, VBMC_E_HIP, "gp_hyp_sample: %d chains unfinished after %lld rounds", left, rounds);

  // ---- the results, one copy (the pinned copy keeps the pieces' spacing)
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_pinned, a.hyp_out, sizeof(double) * n_out, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, stream_wait(ctx));
  const double* h = ctx->h_pinned;
  const size_t o0 = p_hyp.off;
  memcpy(hyp_CxnxP, h, sizeof(double) * cn * P);
  memcpy(logpost_Cxn, h + (p_lpost.off - o0), sizeof(double) * cn);
  memcpy(logprior_Cxn, h + (p_lprior.off - o0), sizeof(double) * cn);
  memcpy(stats_Cx4, h + (p_stats.off - o0), sizeof(int64_t) * 4 * C);
  memcpy(invalid_C, h + (p_inv.off - o0), sizeof(int32_t) * C);
  return VBMC_OK;
}
