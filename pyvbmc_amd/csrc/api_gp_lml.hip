// C-ABI entry point of the batched GP log marginal likelihood: vbmc_gp_lml.  The objective of hyper-parameter fitting
// (gpyreg's, which is not part of the reference tree; the textbook formula, restated by tests/gp_lml_host.py) for B
// candidates at once.  Candidates are factorised in chunks by vbmc_gp_posterior's kernels, which work on ctx->gp: a
// chunk is staged in ctx->gp_next, swapped in for its launches and swapped back on every path (gp_lml_chunk), so the
// installed GP (its buffers, `set`, `dev_built`, the watch lists) is what it was.  Also here: the launching side of
// gp_cand_host.h, which the lockstep entries over lml + log prior share with this one (api_gp_hyp.hip, api_gp_opt.hip).
#include <algorithm>
#include <cmath>
#include <limits>
#include <utility>
#include <vector>

#include "common.h"

int gp_stage_data(vbmc_ctx* ctx, GpState& w, int N, int D, int P, int mean_kind, const double* X, const double* y) {
  w.set = false;
  w.dev_built = false;
  w.homo = false;
  w.N = N; w.D = D; w.P = P; w.mean_kind = mean_kind;
  w.h_X.assign(X, X + (size_t)N * D);
  w.h_y.assign(y, y + N);
  w.h_XT.resize((size_t)N * D);
  for (int n = 0; n < N; ++n)
    for (int d = 0; d < D; ++d) w.h_XT[(size_t)d * N + n] = X[(size_t)n * D + d];
  hipStream_t st = ctx->stream;
  HIP_TRY(ctx, hipMemcpyAsync(w.d_X, w.h_X.data(), sizeof(double) * N * D, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(w.d_XT, w.h_XT.data(), sizeof(double) * N * D, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(w.d_y, w.h_y.data(), sizeof(double) * N, hipMemcpyHostToDevice, st));
  return 0;
}

int gp_cand_begin(vbmc_ctx* ctx, int N, int D, int P, int chunk) {
  NEED_DEVICE(ctx);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, stream_wait(ctx));
  return gp_state_grow(ctx, ctx->gp_next, N, D, chunk, P, true);
}

int gp_lml_chunk(vbmc_ctx* ctx, const Scratch& sc, const GpLmlWs& ws, int S, int slot0) {
  ctx->gp_next.S = S;
  std::swap(ctx->gp, ctx->gp_next);  // the chunk becomes ctx->gp for its launches only
  int rc = launch_gp_post_build(ctx, sc.ptr(ws.Dinv), sc.ptr(ws.flag) + slot0);
  if (!rc)
    rc = launch_gp_lml(ctx, ws.want_grad, sc.ptr(ws.dsn2), sc.ptr(ws.sums), sc.ptr(ws.part), sc.ptr(ws.mg),
                       sc.ptr(ws.lml) + slot0, sc.ptr(ws.dlml) + (size_t)slot0 * ws.P);
  std::swap(ctx->gp, ctx->gp_next);  // the installed state again, whatever happened
  return rc;
}

int gp_cand_stage(vbmc_ctx* ctx, const char* who, const Scratch& sc, const GpLmlWs& ws, double* d_in,
                  const std::vector<double>& in, size_t own_off, int mean_kind, const double* X, const double* y, GpCandArgs& a) {
  GpState& w = ctx->gp_next;
  hipStream_t st = ctx->stream;
  int rc = gp_stage_data(ctx, w, a.N, a.D, a.P, mean_kind, X, y);
  if (!rc) {
    hipError_t e = hipMemcpyAsync(d_in, in.data(), sizeof(double) * in.size(), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(sc.ptr(ws.flag), 0, sizeof(double) * (ws.clear_end - ws.flag.off), st);
    if (e == hipSuccess) e = hipMemsetAsync(sc.base + own_off, 0, sizeof(double) * (sc.total - own_off), st);
    if (e != hipSuccess) rc = vbmc_fail(ctx, VBMC_E_HIP, "%s: %s", who, hipGetErrorString(e));
  }
  if (rc) (void)hipStreamSynchronize(st);
  a.lml = sc.ptr(ws.lml);
  a.flag = sc.ptr(ws.flag);
  a.g_hyp = w.d_hyp; a.g_sl = w.d_sl; a.g_smeta = w.d_smeta; a.g_sn2 = w.d_sn2;
  return rc;
}

extern "C" int vbmc_gp_lml(vbmc_ctx* ctx, int N, int D, int B, int P, int mean_kind, const double* X_NxD, const double* y_N,
                           const double* sn2_BxN, const double* sn2_div_B, const double* dsn2_B, const double* hyp_BxP,
                           int want_grad, double* lml_B, double* dlml_BxP, int32_t* status_B) {
  if (!ctx || !X_NxD || !y_N || !sn2_BxN || !sn2_div_B || !dsn2_B || !hyp_BxP || !lml_B || !status_B) return VBMC_E_ARG;
  want_grad = want_grad ? 1 : 0;
  if (want_grad && !dlml_BxP) return vbmc_fail(ctx, VBMC_E_ARG, "gp_lml: want_grad without dlml_BxP");
  WarpArgErr err;
  GpCandPlan pl;
  auto own = [&](WarpArgErr&) { return 0; };
  if (gp_cand_check(err, "gp_lml", 'B', N, D, B, P, mean_kind, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                    ctx->opt_gp_lml_chunk, own, pl))
    return vbmc_fail(ctx, err.code, "%s", err.msg);
  for (int b = 0; b < B; ++b)
    if (!(sn2_div_B[b] >= 1e-6))
      return vbmc_fail(ctx, VBMC_E_UNSUP, "gp_lml: candidate %d has sn2_div < 1e-6: the non-Cholesky branch is computed on the host", b);
  const int chunk = pl.chunk;
  int rc = gp_cand_begin(ctx, N, D, P, chunk);
  if (rc) return rc;
  GpState& w = ctx->gp_next;
  Scratch sc;
  const GpLmlWs ws = gp_lml_ws(sc, N, D, P, pl.mean_n, chunk, chunk, want_grad);
  rc = reserve_in(ctx, &ctx->d_post_ws, &ctx->d_post_ws_cap, sc);
  if (rc) return rc;
  int* d_flag = sc.ptr(ws.flag);
  rc = gp_stage_data(ctx, w, N, D, P, mean_kind, X_NxD, y_N);
  if (rc) {
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
  }
  std::vector<double> smeta;
  std::vector<int> flags;
  hipStream_t st = ctx->stream;
  for (int b0 = 0; b0 < B && !rc; b0 += chunk) {
    const int S = std::min(chunk, B - b0);
    smeta.resize(3 * (size_t)S);
    for (int s = 0; s < S; ++s) {  // (L_chol, sn2_mult, 1 / sn2_eff): what trinv_strip_kernel reads is the first
      smeta[3 * s] = 1.0;
      smeta[3 * s + 1] = 1.0;
      smeta[3 * s + 2] = 1.0 / sn2_div_B[b0 + s];
    }
    flags.assign(S, 0);
    // this chunk's uploads: hyp, sl = sn2_div (sn2_mult = 1), sn2, dsn2, smeta, cleared flags
    auto up = [&](void* dst, const void* src, size_t bytes) {
      return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
    };
    hipError_t e = up(w.d_hyp, hyp_BxP + (size_t)b0 * P, sizeof(double) * S * P);
    if (e == hipSuccess) e = up(w.d_sl, sn2_div_B + b0, sizeof(double) * S);
    if (e == hipSuccess) e = up(w.d_sn2, sn2_BxN + (size_t)b0 * N, sizeof(double) * S * N);
    if (e == hipSuccess) e = up(sc.ptr(ws.dsn2), dsn2_B + b0, sizeof(double) * S);
    if (e == hipSuccess) e = up(w.d_smeta, smeta.data(), sizeof(double) * 3 * S);
    if (e == hipSuccess) e = hipMemsetAsync(d_flag, 0, sizeof(int) * S, st);
    if (e != hipSuccess) {
      (void)hipStreamSynchronize(st);
      return vbmc_fail(ctx, VBMC_E_HIP, "gp_lml: %s", hipGetErrorString(e));
    }
    rc = timing_begin(ctx, T_GP_LML);
    if (!rc) rc = gp_lml_chunk(ctx, sc, ws, S, 0);
    if (!rc) rc = timing_end(ctx, T_GP_LML);
    if (!rc) {
      e = hipMemcpyAsync(flags.data(), d_flag, sizeof(int) * S, hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipMemcpyAsync(lml_B + b0, sc.ptr(ws.lml), sizeof(double) * S, hipMemcpyDeviceToHost, st);
      if (e == hipSuccess && want_grad)
        e = hipMemcpyAsync(dlml_BxP + (size_t)b0 * P, sc.ptr(ws.dlml), sizeof(double) * S * P, hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = stream_wait(ctx);
      if (e != hipSuccess) rc = vbmc_fail(ctx, VBMC_E_HIP, "gp_lml: %s", hipGetErrorString(e));
    }
    if (rc) {
      (void)hipStreamSynchronize(st);
      return rc;
    }
    // a candidate that did not factorise, or whose results are not finite: -inf and a NaN gradient row, never an error
    for (int s = 0; s < S; ++s) {
      bool bad = flags[s] != 0 || !std::isfinite(lml_B[b0 + s]);
      for (int p = 0; want_grad && !bad && p < P; ++p) bad = !std::isfinite(dlml_BxP[(size_t)(b0 + s) * P + p]);
      status_B[b0 + s] = bad ? 1 : 0;
      if (!bad) continue;
      lml_B[b0 + s] = -std::numeric_limits<double>::infinity();
      for (int p = 0; want_grad && p < P; ++p) dlml_BxP[(size_t)(b0 + s) * P + p] = std::numeric_limits<double>::quiet_NaN();
    }
  }
  return VBMC_OK;
}
