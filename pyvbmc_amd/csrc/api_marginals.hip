// vbmc_marginals: the numbers of a corner plot in one device call (the stages are marginals.hip's and kde.hip's).
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"
#include "kde.h"
#include "marginals.h"

namespace {

constexpr int kStages = 6;  // samples, sort + columns, kde, bins, pairs, levels

struct StageClock {
  hipEvent_t ev[kStages + 1] = {};
  bool on = false;
  int made = 0;
  ~StageClock() {
    for (int i = 0; i < made; ++i) (void)hipEventDestroy(ev[i]);
  }
  hipError_t start(bool want) {
    on = want;
    for (; on && made <= kStages; ++made) {
      const hipError_t e = hipEventCreate(&ev[made]);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  }
  hipError_t mark(int i, hipStream_t s) { return on ? hipEventRecord(ev[i], s) : hipSuccess; }
};

}  // namespace

extern "C" int vbmc_marginals(vbmc_ctx* ctx, int D, const vbmc_mtv_side* src, int orig_flag, int bins,
                              const double* ranges_Dx2, int nq, const double* q_nq, int nl, const double* levels_nl,
                              int kde_mesh, double* edges, int64_t* counts1, int64_t* counts2, int64_t* inside2,
                              double* quantiles, int64_t* level_counts, double* level_mass, double* kde_x,
                              double* kde_density, double* kde_bandwidth, float* stage_ms) {
  if (!ctx || !src || !ranges_Dx2 || !edges || !counts1 || nq < 0 || nl < 0 || (nq && (!q_nq || !quantiles)))
    return VBMC_E_ARG;
  if (D < 1 || D > kMargMaxD) return vbmc_fail(ctx, VBMC_E_UNSUP, "marginals: D=%d outside 1..%d", D, kMargMaxD);
  if (bins < 1 || bins > kMargMaxBins)
    return vbmc_fail(ctx, VBMC_E_UNSUP, "marginals: bins=%d outside 1..%d", bins, kMargMaxBins);
  const int64_t n = src->n;
  if (n < 1 || n > kMargMaxN)
    return vbmc_fail(ctx, VBMC_E_UNSUP, "marginals: %lld samples outside 1..%lld", (long long)n, (long long)kMargMaxN);
  const int P = D * (D - 1) / 2;
  if (P && (!counts2 || !inside2 || (nl && (!levels_nl || !level_counts || !level_mass)))) return VBMC_E_ARG;
  if (kde_mesh && (kde_mesh != 1 << 10 || !kde_x || !kde_density || !kde_bandwidth))
    return vbmc_fail(ctx, VBMC_E_ARG, "marginals: the kde mesh is 2^10 points or none");
  if (src->source != VBMC_MTV_HOST && src->source != VBMC_MTV_MIX1) return vbmc_fail(ctx, VBMC_E_ARG, "marginals: bad source");
  if (src->source == VBMC_MTV_HOST && !src->x_NxD) return vbmc_fail(ctx, VBMC_E_ARG, "marginals: no samples");
  XfView xf = {};
  if (src->source == VBMC_MTV_MIX1) {
    if (!ctx->mix_set || ctx->D != D) return vbmc_fail(ctx, VBMC_E_ARG, "marginals: mixture not set or D differs");
    if (orig_flag && !xf_view_slot(ctx, 0, D, xf))
      return vbmc_fail(ctx, VBMC_E_ARG, "marginals: transformer slot 0 not set for D=%d", D);
  }
  for (int d = 0; d < D; ++d) {
    const double lo = ranges_Dx2[2 * d], hi = ranges_Dx2[2 * d + 1];
    if ((lo != lo) != (hi != hi) || (lo == lo && !(std::isfinite(lo) && std::isfinite(hi) && lo < hi)))
      return vbmc_fail(ctx, VBMC_E_ARG, "marginals: range of dimension %d is not lo < hi", d);
  }
  for (int i = 0; i < nq; ++i)
    if (!(q_nq[i] >= 0.0 && q_nq[i] <= 1.0)) return vbmc_fail(ctx, VBMC_E_ARG, "marginals: quantile %g outside [0, 1]", q_nq[i]);
  for (int i = 0; i < nl; ++i)
    if (!(levels_nl[i] >= 0.0 && levels_nl[i] <= 1.0)) return vbmc_fail(ctx, VBMC_E_ARG, "marginals: level %g outside [0, 1]", levels_nl[i]);
  NEED_DEVICE(ctx);
  HIP_TRY(ctx, hipSetDevice(ctx->device));

  const int64_t ns = (n + kMargIdxAlign - 1) / kMargIdxAlign * kMargIdxAlign;
  const int nlp = P ? nl : 0;
  Scratch sc;
  const KdeCols kc = kde_cols_plan(sc, D, kde_mesh ? kde_mesh : 2, n);
  const bool draw = src->source == VBMC_MTV_MIX1;
  const MargWs w = marginals_ws(sc, (size_t)n, (size_t)ns, (size_t)D, (size_t)bins, (size_t)P, (size_t)nq, (size_t)nlp,
                                draw ? selector_elems(ctx->K) : 0, (size_t)kde_mesh, (size_t)kc.colp_stride);
  int rc = reserve(ctx, sc);
  if (rc) return rc;
  double* base = sc.base;
  StageClock clk;
  HIP_TRY(ctx, clk.start(stage_ms != nullptr));

  // ---- the samples on the device ----
  HIP_TRY(ctx, clk.mark(0, ctx->stream));
  std::vector<double> par(w.par.count);
  std::memcpy(par.data(), ranges_Dx2, sizeof(double) * 2 * D);
  if (nq) std::memcpy(par.data() + 2 * D, q_nq, sizeof(double) * nq);
  if (nlp) std::memcpy(par.data() + 2 * D + nq, levels_nl, sizeof(double) * nlp);
  double* d_par = sc.ptr(w.par);
  HIP_TRY(ctx, hipMemcpyAsync(d_par, par.data(), sizeof(double) * par.size(), hipMemcpyHostToDevice, ctx->stream));
  double* d_x = sc.ptr(w.x);
  if (draw) {
    // sample(n, orig_flag, rng="philox", seed): unbalanced draws of the mixture, then its transformer's inverse
    rc = launch_sample(ctx, ctx->d_mix, ctx->ml, ctx->w.data(), n, src->seed, 0, sc.ptr(w.sel), d_x, nullptr, INFINITY);
    if (rc) return rc;
    if (orig_flag && (rc = launch_xf_apply(ctx, xf, n, 1, d_x, d_x))) return rc;
  } else {
    HIP_TRY(ctx, hipMemcpyAsync(d_x, src->x_NxD, sizeof(double) * n * D, hipMemcpyHostToDevice, ctx->stream));
  }
  HIP_TRY(ctx, clk.mark(1, ctx->stream));

  MargArgs A = {};
  A.x = d_x;
  A.n = n;
  A.ns = ns;
  A.D = D;
  A.bins = bins;
  A.P = P;
  A.nq = nq;
  A.nl = nlp;
  A.keys = (uint64_t*)(base + kc.o_keys);
  A.pmax = kc.pmax;
  A.nonfinite = (unsigned*)(base + kc.o_nf);
  A.ranges = d_par;
  A.q = d_par + 2 * D;
  A.levels = d_par + 2 * D + nq;
  A.colinfo = sc.ptr(w.colinfo);
  A.kde_lb = base + kc.o_bnd;
  A.kde_ub = base + kc.o_bnd + D;
  A.idx = sc.ptr(w.idx);
  A.edges = sc.ptr(w.edges);
  A.quant = sc.ptr(w.quant);
  A.counts1 = sc.ptr(w.counts1);
  A.counts2 = sc.ptr(w.counts2);
  A.inside2 = sc.ptr(w.inside2);
  A.level_counts = sc.ptr(w.level_counts);
  A.level_mass = sc.ptr(w.level_mass);

  // ---- sorted columns: ranges, edges, quantiles; the kde of every column on its range ----
  rc = launch_marg_sort(ctx, A);
  if (rc) return rc;
  // (the flags of this sort: the kde stages sort the columns again into the same keys and set them anew)
  HIP_TRY(ctx, hipMemcpyAsync(sc.ptr(w.nonfinite), A.nonfinite, sizeof(unsigned) * D, hipMemcpyDeviceToDevice, ctx->stream));
  A.nonfinite = sc.ptr(w.nonfinite);
  HIP_TRY(ctx, clk.mark(2, ctx->stream));
  if (kde_mesh) {
    rc = kde_cols_launch(ctx, kc, d_x, n, D, 1, base);
    if (rc) return rc;
    const size_t nm = sizeof(double) * (size_t)D * kde_mesh;
    HIP_TRY(ctx, hipMemcpyAsync(sc.ptr(w.kde_x), base + kc.o_xm, nm, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(sc.ptr(w.kde_dens), base + kc.o_dens, nm, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(sc.ptr(w.colp), base + kc.o_colp, sizeof(double) * w.colp.count, hipMemcpyDeviceToDevice,
                                ctx->stream));
  }
  HIP_TRY(ctx, clk.mark(3, ctx->stream));

  // ---- bin indices and 1-D counts, pair histograms, levels ----
  rc = launch_marg_bins(ctx, A);
  if (rc) return rc;
  HIP_TRY(ctx, clk.mark(4, ctx->stream));
  rc = launch_marg_pairs(ctx, A);
  if (rc) return rc;
  HIP_TRY(ctx, clk.mark(5, ctx->stream));
  rc = launch_marg_levels(ctx, A);
  if (rc) return rc;
  HIP_TRY(ctx, clk.mark(6, ctx->stream));

  // ---- the one download ----
  std::vector<double> res(w.res_end - w.res_begin);
  HIP_TRY(ctx, hipMemcpyAsync(res.data(), base + w.res_begin, sizeof(double) * res.size(), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, stream_wait(ctx));
  if (stage_ms)
    for (int i = 0; i < kStages; ++i) HIP_TRY(ctx, hipEventElapsedTime(&stage_ms[i], clk.ev[i], clk.ev[i + 1]));
  auto at = [&](size_t off) { return (const void*)(res.data() + (off - w.res_begin)); };
  const unsigned* nf = (const unsigned*)at(w.nonfinite.off);
  for (int d = 0; d < D; ++d)
    if (nf[d]) return vbmc_fail(ctx, VBMC_E_NONFINITE, "marginals: column %d holds a non-finite sample", d);
  std::memcpy(edges, at(w.edges.off), sizeof(double) * w.edges.count);
  if (nq) std::memcpy(quantiles, at(w.quant.off), sizeof(double) * w.quant.count);
  std::memcpy(counts1, at(w.counts1.off), sizeof(int64_t) * w.counts1.count);
  if (P) {
    std::memcpy(counts2, at(w.counts2.off), sizeof(int64_t) * w.counts2.count);
    std::memcpy(inside2, at(w.inside2.off), sizeof(int64_t) * w.inside2.count);
    if (nlp) {
      std::memcpy(level_counts, at(w.level_counts.off), sizeof(int64_t) * w.level_counts.count);
      std::memcpy(level_mass, at(w.level_mass.off), sizeof(double) * w.level_mass.count);
    }
  }
  if (kde_mesh) {
    std::memcpy(kde_x, at(w.kde_x.off), sizeof(double) * w.kde_x.count);
    std::memcpy(kde_density, at(w.kde_dens.off), sizeof(double) * w.kde_dens.count);
    const double* colp = (const double*)at(w.colp.off);
    for (int d = 0; d < D; ++d) kde_bandwidth[d] = colp[(size_t)d * kc.colp_stride + kc.colp_bw];
  }
  return VBMC_OK;
}
