// C-ABI entry points of the device-built GP posterior: vbmc_gp_posterior, vbmc_gp_append, vbmc_gp_append_noisy,
// vbmc_gp_fetch.
// They stand in for gp.py's GP._posterior (SURVEY Appendix A "Posterior"; gpyreg itself is not in the reference tree)
// followed by vbmc_set_gp.  The new state is built in ctx->gp_next and swapped with ctx->gp only when every sample
// factorised, so a failed call leaves the installed state as it was.
#include <cmath>
#include <cstring>
#include <utility>

#include "common.h"

// The host-side fields of a device-built state that follow from h_X, h_sl and the shapes: L_chol, sn2_eff, sn2_mult, the
// predict centre and smeta (h_small), X^T, and sW for the upload.  Stated once for the build entries here and for
// vbmc_gp_fit, which installs the state it built from device-resident samples (api_gp_fit.hip).
void gp_post_host_fields(GpState& w, int N, int D, int S, int P, int mean_kind, std::vector<double>& sW_host) {
  w.set = false;
  w.dev_built = false;
  w.N = N; w.D = D; w.S = S; w.P = P; w.mean_kind = mean_kind;
  w.L_chol.assign(S, 1);
  w.sn2_eff.resize(S);
  w.sn2_mult.assign(S, 1.0);
  sW_host.resize((size_t)S * N);
  for (int s = 0; s < S; ++s) {
    const double sw0 = 1.0 / std::sqrt(w.h_sl[s]);  // gp.py: sW = 1 / sqrt(sn2_div sn2_mult)
    w.sn2_eff[s] = 1.0 / (sw0 * sw0);               // as vbmc_set_gp derives it from sW
    for (int n = 0; n < N; ++n) sW_host[(size_t)s * N + n] = sw0;
  }
  const double* X = w.h_X.data();
  w.h_small.assign((size_t)D + 3 * (size_t)S, 0.0);
  double* xc = w.h_small.data();
  for (int n = 0; n < N; ++n)
    for (int d = 0; d < D; ++d) xc[d] += X[(size_t)n * D + d];
  for (int d = 0; d < D; ++d) xc[d] /= N;
  double* smeta = xc + D;
  for (int s = 0; s < S; ++s) {
    smeta[3 * s] = 1.0;
    smeta[3 * s + 1] = 1.0;
    smeta[3 * s + 2] = 1.0 / w.sn2_eff[s];
  }
  w.h_XT.resize((size_t)N * D);
  for (int n = 0; n < N; ++n)
    for (int d = 0; d < D; ++d) w.h_XT[(size_t)d * N + n] = X[(size_t)n * D + d];
}

namespace {

// host-side fields of the state under construction (gp_post_host_fields) and the uploads that do not depend on the
// factorisation: X, X^T, the predict centre, smeta, hyp, sW, y, sl.  h_X, h_y, hyp, h_sl of `w` are set by the caller.
int stage_state(vbmc_ctx* ctx, GpState& w, int N, int D, int S, int P, int mean_kind, std::vector<double>& sW_host) {
  gp_post_host_fields(w, N, D, S, P, mean_kind, sW_host);
  const double* X = w.h_X.data();
  const double* xc = w.h_small.data();
  const double* smeta = xc + D;
  hipStream_t st = ctx->stream;
  HIP_TRY(ctx, hipMemcpyAsync(w.d_smeta, smeta, sizeof(double) * 3 * S, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(w.d_xc, xc, sizeof(double) * D, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(w.d_X, X, sizeof(double) * N * D, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(w.d_XT, w.h_XT.data(), sizeof(double) * N * D, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(w.d_hyp, w.hyp.data(), sizeof(double) * S * P, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(w.d_sW, sW_host.data(), sizeof(double) * S * N, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(w.d_y, w.h_y.data(), sizeof(double) * N, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(w.d_sl, w.h_sl.data(), sizeof(double) * S, hipMemcpyHostToDevice, st));
  return 0;
}

// the noise variances' upload and the cleared flags, behind stage_state
int stage_tail(vbmc_ctx* ctx, double* d_sn2, const double* sn2, size_t n, int* d_flag, int S) {
  HIP_TRY(ctx, hipMemcpyAsync(d_sn2, sn2, sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(d_flag, 0, sizeof(int) * S, ctx->stream));
  return 0;
}

// wait for the build queued on ctx->gp (the state under construction, already swapped in) and read the flags
int finish_build(vbmc_ctx* ctx, const int* d_flag, int S, int rc, const char* who) {
  std::vector<int> flags(S, 0);
  if (!rc) {
    hipError_t e = hipMemcpyAsync(flags.data(), d_flag, sizeof(int) * S, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = stream_wait(ctx);
    if (e != hipSuccess) rc = vbmc_fail(ctx, VBMC_E_HIP, "%s: %s", who, hipGetErrorString(e));
  }
  for (int s = 0; s < S && !rc; ++s)
    if (flags[s])
      rc = vbmc_fail(ctx, VBMC_E_NOTPD, "%s: sample %d: the matrix is not positive definite (a pivot is not a positive finite number)",
                     who, s);
  if (rc) {
    (void)hipStreamSynchronize(ctx->stream);
    std::swap(ctx->gp, ctx->gp_next);  // the state installed before, untouched
    return rc;
  }
  ctx->gp.set = true;
  ctx->gp.dev_built = true;
  ctx->gp_watch_ptrs.clear();
  ctx->gp_watch_lens.clear();
  return VBMC_OK;
}

int fetch(vbmc_ctx* ctx, double* alpha, double* L) {
  const GpState& g = ctx->gp;
  if (alpha)
    HIP_TRY(ctx, hipMemcpyAsync(alpha, g.d_alpha, sizeof(double) * g.S * g.N, hipMemcpyDeviceToHost, ctx->stream));
  if (L)
    HIP_TRY(ctx, hipMemcpyAsync(L, g.d_L, sizeof(double) * g.S * g.N * g.N, hipMemcpyDeviceToHost, ctx->stream));
  if (alpha || L) HIP_TRY(ctx, stream_wait(ctx));
  return VBMC_OK;
}

}  // namespace

void gp_post_free(vbmc_ctx* ctx) {
  GpState& n = ctx->gp_next;
  double* bufs[] = {n.d_X, n.d_XT, n.d_alpha, n.d_L, n.d_Linv, n.d_LinvP, n.d_sW, n.d_hyp, n.d_xc, n.d_smeta,
                    n.d_y, n.d_r, n.d_sn2, n.d_sl, ctx->gp.d_y, ctx->gp.d_r, ctx->gp.d_sn2, ctx->gp.d_sl, ctx->d_post_ws};
  for (double* b : bufs)
    if (b) (void)hipFree(b);
}

extern "C" int vbmc_gp_posterior(vbmc_ctx* ctx, int N, int D, int S, int P, int mean_kind, const double* X_NxD,
                                 const double* y_N, const double* sn2_SxN, const double* sn2_div_S, const double* hyp_SxP,
                                 double* alpha_SxN, double* L_SxNxN) {
  if (!ctx || !X_NxD || !y_N || !sn2_SxN || !sn2_div_S || !hyp_SxP) return VBMC_E_ARG;
  if (N < 1 || D < 1 || S < 1) return vbmc_fail(ctx, VBMC_E_ARG, "gp_posterior: bad N=%d D=%d S=%d", N, D, S);
  const int mean_n = mean_kind == VBMC_MEAN_ZERO ? 0 : mean_kind == VBMC_MEAN_CONST ? 1 : 1 + 2 * D;
  if (mean_kind < 0 || mean_kind > 2 || P != D + 2 + mean_n)
    return vbmc_fail(ctx, VBMC_E_ARG, "gp_posterior: P=%d does not match D+2+mean(%d)=%d", P, mean_kind, D + 2 + mean_n);
  for (int s = 0; s < S; ++s)
    if (!(sn2_div_S[s] >= 1e-6))
      return vbmc_fail(ctx, VBMC_E_UNSUP, "gp_posterior: sample %d has sn2_div < 1e-6: the non-Cholesky branch is built on the host", s);
  NEED_DEVICE(ctx);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, stream_wait(ctx));
  GpState& w = ctx->gp_next;
  int rc = gp_state_grow(ctx, w, N, D, S, P, true);
  if (rc) return rc;
  const int nb = (N + 63) / 64;
  Scratch sc;
  const auto p_flag = gp_post_flags(sc, S);
  const auto p_Dinv = sc.add((size_t)S * nb * 64 * 64);
  rc = reserve_in(ctx, &ctx->d_post_ws, &ctx->d_post_ws_cap, sc);
  if (rc) return rc;
  int* d_flag = sc.ptr(p_flag);
  double* d_Dinv = sc.ptr(p_Dinv);
  w.h_X.assign(X_NxD, X_NxD + (size_t)N * D);
  w.h_y.assign(y_N, y_N + N);
  w.hyp.assign(hyp_SxP, hyp_SxP + (size_t)S * P);
  w.h_sl.assign(sn2_div_S, sn2_div_S + S);  // sn2_mult = 1
  w.h_sn2.assign(sn2_SxN, sn2_SxN + (size_t)S * N);
  w.homo = true;
  for (int s = 0; s < S && w.homo; ++s)
    for (int n = 0; n < N && w.homo; ++n) w.homo = sn2_SxN[(size_t)s * N + n] == sn2_div_S[s];
  std::vector<double> sW_host;
  rc = stage_state(ctx, w, N, D, S, P, mean_kind, sW_host);
  if (!rc) rc = stage_tail(ctx, w.d_sn2, sn2_SxN, (size_t)S * N, d_flag, S);
  if (rc) {
    (void)hipStreamSynchronize(ctx->stream);  // (copies from the caller's arrays and from sW_host may be queued)
    return rc;
  }
  std::swap(ctx->gp, ctx->gp_next);
  rc = launch_gp_post_build(ctx, d_Dinv, d_flag);
  rc = finish_build(ctx, d_flag, S, rc, "gp_posterior");
  if (rc) return rc;
  return fetch(ctx, alpha_SxN, L_SxNxN);
}

// One point appended to the device-built posterior.  sn2_new_S == nullptr: constant noise (vbmc_gp_append: the resident
// state is homo and the new entry is read from its d_sn2, as before); else the new point's noise variance per sample.
static int append_point(vbmc_ctx* ctx, const double* x_D, double y, const double* sn2_new_S, double* alpha_out, double* L_out,
                        const char* who) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, stream_wait(ctx));
  const GpState& o = ctx->gp;
  GpState& w = ctx->gp_next;
  const int N = o.N, D = o.D, S = o.S, P = o.P, N1 = N + 1;
  int rc = gp_state_grow(ctx, w, N1, D, S, P, true);
  if (rc) return rc;
  GpAppendWs ws = gp_post_append_ws(S, N);
  rc = reserve_in(ctx, &ctx->d_post_ws, &ctx->d_post_ws_cap, ws.sc);
  if (rc) return rc;
  int* d_flag = ws.sc.ptr(ws.flag);
  w.h_X = o.h_X;
  w.h_X.insert(w.h_X.end(), x_D, x_D + D);
  w.h_y = o.h_y;
  w.h_y.push_back(y);
  w.hyp = o.hyp;
  w.h_sl = o.h_sl;
  w.homo = o.homo;
  std::vector<double> sW_host;
  w.h_sn2.resize((size_t)S * N1);
  for (int s = 0; s < S; ++s) {
    for (int n = 0; n < N; ++n)  // (constant noise: sn2 = sn2_div = sl)
      w.h_sn2[(size_t)s * N1 + n] = sn2_new_S ? o.h_sn2[(size_t)s * N + n] : o.h_sl[s];
    const double v = sn2_new_S ? sn2_new_S[s] : o.h_sl[s];
    w.h_sn2[(size_t)s * N1 + N] = v;
    w.homo = w.homo && v == o.h_sl[s];
  }
  // the new point's noise as the kernel reads it: the old state's first entry per sample (constant noise), or the
  // new column of the state under construction
  const double* d_sn2_new = sn2_new_S ? w.d_sn2 + N : o.d_sn2;
  const size_t sn2_stride = sn2_new_S ? (size_t)N1 : (size_t)N;
  rc = stage_state(ctx, w, N1, D, S, P, o.mean_kind, sW_host);
  if (!rc) rc = stage_tail(ctx, w.d_sn2, w.h_sn2.data(), (size_t)S * N1, d_flag, S);
  if (rc) {
    (void)hipStreamSynchronize(ctx->stream);  // (copies from sW_host / h_sn2 may be queued)
    return rc;
  }
  std::swap(ctx->gp, ctx->gp_next);
  rc = launch_gp_post_append(ctx, ctx->gp_next, y, d_sn2_new, sn2_stride, ws);
  rc = finish_build(ctx, d_flag, S, rc, who);
  if (rc) return rc;
  return fetch(ctx, alpha_out, L_out);
}

extern "C" int vbmc_gp_append(vbmc_ctx* ctx, const double* x_D, double y, double* alpha_out, double* L_out) {
  if (!ctx || !x_D) return VBMC_E_ARG;
  NEED_DEVICE(ctx);
  if (!ctx->gp.set || !ctx->gp.dev_built)
    return vbmc_fail(ctx, VBMC_E_ARG, "gp_append: the context holds no posterior built by vbmc_gp_posterior");
  if (!ctx->gp.homo)
    return vbmc_fail(ctx, VBMC_E_UNSUP, "gp_append: the resident posterior has per-point noise: update it instead");
  return append_point(ctx, x_D, y, nullptr, alpha_out, L_out, "gp_append");
}

extern "C" int vbmc_gp_append_noisy(vbmc_ctx* ctx, const double* x_D, double y, const double* sn2_new_S, double* alpha_out,
                                    double* L_out) {
  if (!ctx || !x_D || !sn2_new_S) return VBMC_E_ARG;
  NEED_DEVICE(ctx);
  if (!ctx->gp.set || !ctx->gp.dev_built)
    return vbmc_fail(ctx, VBMC_E_ARG, "gp_append_noisy: the context holds no posterior built by vbmc_gp_posterior");
  const GpState& o = ctx->gp;
  if (o.h_sn2.size() != (size_t)o.S * o.N)
    return vbmc_fail(ctx, VBMC_E_ARG, "gp_append_noisy: the resident posterior carries no noise table");
  for (int s = 0; s < o.S; ++s)
    if (!(sn2_new_S[s] >= o.h_sl[s]) || !(sn2_new_S[s] < INFINITY))
      return vbmc_fail(ctx, VBMC_E_UNSUP, "gp_append_noisy: sample %d: the new point's noise is below sn2_div (the scale of the "
                       "factor would change): update it instead", s);
  return append_point(ctx, x_D, y, sn2_new_S, alpha_out, L_out, "gp_append_noisy");
}

extern "C" int vbmc_gp_fetch(vbmc_ctx* ctx, double* alpha_SxN, double* L_SxNxN) {
  if (!ctx) return VBMC_E_ARG;
  NEED_DEVICE(ctx);
  if (!ctx->gp.set) return vbmc_fail(ctx, VBMC_E_ARG, "gp_fetch: GP not set");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return fetch(ctx, alpha_SxN, L_SxNxN);
}
