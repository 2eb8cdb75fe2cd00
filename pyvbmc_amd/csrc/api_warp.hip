// Entry points of the input warping (whitening/whitening.py): vbmc_warp_points, vbmc_warp_unscent, vbmc_warp_gp,
// vbmc_warp_box.  Arguments are checked by warp_args.h, the scratch is listed in scratch.h (WarpWs), the kernels are
// warp.hip's.  Transformer slot 0 = the old transformer, slot 1 = the new one.
#include <cmath>
#include <vector>

#include "warp.h"
#include "warp_args.h"

namespace {

// the views of the slots the source needs, checked against D
int warp_views(vbmc_ctx* ctx, const char* who, int D, int source, XfView& t0, XfView& t1) {
  t0 = XfView();
  int rc = xf_need(ctx, 1, D, who, t1);
  if (rc) return rc;
  if (source == VBMC_WARP_FROM_OLD) rc = xf_need(ctx, 0, D, who, t0);
  return rc;
}

}  // namespace

extern "C" int vbmc_warp_points(vbmc_ctx* ctx, int D, int64_t n, int source, const double* x_NxD, double* y_NxD,
                                double* lj_new_N, double* lj_old_N) {
  if (!ctx) return VBMC_E_ARG;
  WarpArgErr e;
  if (warp_check_points(e, D, n, source, x_NxD, y_NxD, lj_new_N, lj_old_N)) return vbmc_fail(ctx, e.code, "%s", e.msg);
  if (n == 0) return VBMC_OK;
  XfView t0, t1;
  int rc = warp_views(ctx, "warp_points", D, source, t0, t1);
  if (rc) return rc;
  NEED_DEVICE(ctx);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int64_t BATCH = (int64_t)1 << 21;
  const int64_t nb = n < BATCH ? n : BATCH;
  WarpWs w = warp_points_ws((size_t)nb, (size_t)D, y_NxD != nullptr, lj_new_N != nullptr, lj_old_N != nullptr);
  rc = reserve(ctx, w.sc);
  if (rc) return rc;
  double* d_x = w.sc.ptr(w.x);
  double* d_y = y_NxD ? w.sc.ptr(w.y) : nullptr;
  double* d_new = lj_new_N ? w.sc.ptr(w.lj_new) : nullptr;
  double* d_old = lj_old_N ? w.sc.ptr(w.lj_old) : nullptr;
  for (int64_t o = 0; o < n; o += nb) {
    const int64_t m = (n - o) < nb ? (n - o) : nb;
    HIP_TRY(ctx, hipMemcpyAsync(d_x, x_NxD + o * D, sizeof(double) * m * D, hipMemcpyHostToDevice, ctx->stream));
    rc = launch_warp_points(ctx, t0, t1, m, source, d_x, WarpBox(), d_y, d_new, d_old);
    if (rc) return rc;
    if (d_y) HIP_TRY(ctx, hipMemcpyAsync(y_NxD + o * D, d_y, sizeof(double) * m * D, hipMemcpyDeviceToHost, ctx->stream));
    if (d_new) HIP_TRY(ctx, hipMemcpyAsync(lj_new_N + o, d_new, sizeof(double) * m, hipMemcpyDeviceToHost, ctx->stream));
    if (d_old) HIP_TRY(ctx, hipMemcpyAsync(lj_old_N + o, d_old, sizeof(double) * m, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, stream_wait(ctx));
  }
  return VBMC_OK;
}

extern "C" int vbmc_warp_unscent(vbmc_ctx* ctx, int D, int64_t n, const double* x_NxD, int64_t sigma_rows,
                                 const double* sigma, double* mean_NxD, double* std_NxD, double* pts_UxNxD) {
  if (!ctx) return VBMC_E_ARG;
  WarpArgErr e;
  if (warp_check_unscent(e, D, n, x_NxD, sigma_rows, sigma, mean_NxD, std_NxD)) return vbmc_fail(ctx, e.code, "%s", e.msg);
  XfView t0, t1;
  int rc = warp_views(ctx, "warp_unscent", D, VBMC_WARP_FROM_OLD, t0, t1);
  if (rc) return rc;
  NEED_DEVICE(ctx);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  WarpWs w = warp_unscent_ws((size_t)n, (size_t)D, (size_t)sigma_rows, pts_UxNxD != nullptr);
  rc = reserve(ctx, w.sc);
  if (rc) return rc;
  WarpUnscent a;
  a.n = n;
  a.S = 1;
  double *d_x = w.sc.ptr(w.x), *d_sigma = w.sc.ptr(w.sigma);
  a.x = d_x;
  a.sigma = d_sigma;
  a.sigma_row_stride = sigma_rows == 1 ? 0 : D;
  a.mean = w.sc.ptr(w.mean);
  a.sd = w.sc.ptr(w.sd);
  a.pts = pts_UxNxD ? w.sc.ptr(w.pts) : nullptr;
  HIP_TRY(ctx, hipMemcpyAsync(d_x, x_NxD, sizeof(double) * n * D, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_sigma, sigma, sizeof(double) * sigma_rows * D, hipMemcpyHostToDevice, ctx->stream));
  rc = launch_warp_unscent(ctx, t0, t1, a);
  if (rc) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(mean_NxD, a.mean, sizeof(double) * n * D, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(std_NxD, a.sd, sizeof(double) * n * D, hipMemcpyDeviceToHost, ctx->stream));
  if (a.pts)
    HIP_TRY(ctx, hipMemcpyAsync(pts_UxNxD, a.pts, sizeof(double) * w.pts.count, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, stream_wait(ctx));
  return VBMC_OK;
}

extern "C" int vbmc_warp_gp(vbmc_ctx* ctx, int D, int N, int S, int P, const double* X_NxD, const double* hyp_SxP,
                            double* logell_SxD, double* dy_mean, double* dy_old_mean) {
  if (!ctx) return VBMC_E_ARG;
  WarpArgErr e;
  if (warp_check_gp(e, D, N, S, P, X_NxD, hyp_SxP, logell_SxD)) return vbmc_fail(ctx, e.code, "%s", e.msg);
  XfView t0, t1;
  int rc = warp_views(ctx, "warp_gp", D, VBMC_WARP_FROM_OLD, t0, t1);
  if (rc) return rc;
  NEED_DEVICE(ctx);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  WarpWs w = warp_gp_ws((size_t)N, (size_t)D, (size_t)S);
  rc = reserve(ctx, w.sc);
  if (rc) return rc;
  // ell = np.exp(hyp[0:D]) (:301), by the host's libm as the reference's
  std::vector<double> ell((size_t)S * D);
  for (int s = 0; s < S; ++s)
    for (int d = 0; d < D; ++d) ell[(size_t)s * D + d] = std::exp(hyp_SxP[(size_t)s * P + d]);
  WarpUnscent a;
  a.n = N;
  a.S = S;
  double *d_x = w.sc.ptr(w.x), *d_sigma = w.sc.ptr(w.sigma), *d_out = w.sc.ptr(w.out);
  a.x = d_x;
  a.sigma = d_sigma;
  a.sigma_set_stride = D;
  a.log_sd = 1;
  a.mean = w.sc.ptr(w.mean);
  a.sd = w.sc.ptr(w.sd);
  a.dy = w.sc.ptr(w.lj_new);
  a.dy_old = w.sc.ptr(w.lj_old);
  HIP_TRY(ctx, hipMemcpyAsync(d_x, X_NxD, sizeof(double) * N * D, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_sigma, ell.data(), sizeof(double) * ell.size(), hipMemcpyHostToDevice, ctx->stream));
  rc = launch_warp_unscent(ctx, t0, t1, a);
  if (rc) return rc;
  rc = launch_warp_row_means(ctx, a.sd, S, N, D, d_out);
  if (rc) return rc;
  rc = launch_warp_row_means(ctx, a.dy, 1, N, 1, d_out + (size_t)S * D);
  if (rc) return rc;
  rc = launch_warp_row_means(ctx, a.dy_old, 1, N, 1, d_out + (size_t)S * D + 1);
  if (rc) return rc;
  std::vector<double> out((size_t)S * D + 2);
  HIP_TRY(ctx, hipMemcpyAsync(out.data(), d_out, sizeof(double) * out.size(), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, stream_wait(ctx));
  for (size_t i = 0; i < (size_t)S * D; ++i) logell_SxD[i] = out[i];
  if (dy_mean) *dy_mean = out[(size_t)S * D];
  if (dy_old_mean) *dy_old_mean = out[(size_t)S * D + 1];
  return VBMC_OK;
}

extern "C" int vbmc_warp_box(vbmc_ctx* ctx, int D, int64_t n, int source, const double* lo_D, const double* hi_D,
                             const double* u_NxD, uint64_t seed, int mode, double* out_2xD, double* sorted_Dxn) {
  if (!ctx) return VBMC_E_ARG;
  WarpArgErr e;
  if (warp_check_box(e, D, n, source, lo_D, hi_D, mode, out_2xD, sorted_Dxn)) return vbmc_fail(ctx, e.code, "%s", e.msg);
  XfView t0, t1;
  int rc = warp_views(ctx, "warp_box", D, source, t0, t1);
  if (rc) return rc;
  NEED_DEVICE(ctx);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const bool quant = mode == 0;
  WarpWs w = warp_box_ws((size_t)n, (size_t)D, u_NxD != nullptr, quant, (size_t)warp_sort_pmax(n), sorted_Dxn != nullptr);
  rc = reserve(ctx, w.sc);
  if (rc) return rc;
  double *d_u = u_NxD ? w.sc.ptr(w.x) : nullptr, *d_box = w.sc.ptr(w.box), *d_y = w.sc.ptr(w.y), *d_out = w.sc.ptr(w.out);
  double* d_sorted = sorted_Dxn ? w.sc.ptr(w.sorted) : nullptr;
  unsigned* d_nf = quant ? w.sc.ptr(w.nonfinite) : nullptr;
  std::vector<double> box(2 * (size_t)D);
  for (int d = 0; d < D; ++d) {
    box[d] = lo_D[d];
    box[(size_t)D + d] = hi_D[d];
  }
  HIP_TRY(ctx, hipMemcpyAsync(d_box, box.data(), sizeof(double) * box.size(), hipMemcpyHostToDevice, ctx->stream));
  if (d_u) HIP_TRY(ctx, hipMemcpyAsync(d_u, u_NxD, sizeof(double) * n * D, hipMemcpyHostToDevice, ctx->stream));
  WarpBox b;
  b.gen = d_u ? 1 : 2;
  b.lo = d_box;
  b.hi = d_box + D;
  b.seed = seed;
  rc = launch_warp_points(ctx, t0, t1, n, source, d_u, b, d_y, nullptr, nullptr);
  if (rc) return rc;
  rc = launch_warp_box_stats(ctx, d_y, n, D, mode, quant ? (uint64_t*)w.sc.ptr(w.keys) : nullptr, d_nf, d_out, d_sorted);
  if (rc) return rc;
  std::vector<unsigned> nf(quant ? D : 0);
  HIP_TRY(ctx, hipMemcpyAsync(out_2xD, d_out, sizeof(double) * 2 * D, hipMemcpyDeviceToHost, ctx->stream));
  if (quant) HIP_TRY(ctx, hipMemcpyAsync(nf.data(), d_nf, sizeof(unsigned) * D, hipMemcpyDeviceToHost, ctx->stream));
  if (d_sorted)
    HIP_TRY(ctx, hipMemcpyAsync(sorted_Dxn, d_sorted, sizeof(double) * (size_t)D * n, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, stream_wait(ctx));
  for (size_t d = 0; d < nf.size(); ++d)
    if (nf[d]) return vbmc_fail(ctx, VBMC_E_NONFINITE, "warp_box: dimension %d holds a non-finite mapped value", (int)d);
  return VBMC_OK;
}
