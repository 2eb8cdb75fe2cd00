// the acquisition search of active_sample (vbmc/active_sample.py:310-349, 647-837) as device calls.
//
// The context keeps one resident set of search points (M x D, transformed space).  vbmc_search_fill writes it from a
// table of sources -- host rows copied or put through the transformer, balanced draws of the context's mixture by the
// sampler of sample.hip, affine-Gaussian and box-normal rows by search.hip's generator -- clamps it to the search bounds
// and rounds its integer columns; vbmc_search_eval runs the acquisition on it with the launches vbmc_acq_eval /
// vbmc_acq_is_eval use per batch (api_acq.hip launch_acq_closed, api_acq_is.hip launch_acq_is), takes the per-point noise
// from the nearest training input (gp.hip's sq_dist argmin), masks the hard bounds, sorts, and hands acq | order | sorted
// points to the host in one copy.  Between the two calls the points exist only in device memory.
#include <cmath>
#include <cstring>

#include "common.h"
#include "transform.h"

namespace {

struct SearchState {
  double* d_X = nullptr;  // M x D
  size_t cap = 0;
  int64_t M = 0;
  int D = 0;
};

SearchState* search_of(vbmc_ctx* ctx) {
  if (!ctx->search) ctx->search = new SearchState();
  return (SearchState*)ctx->search;
}

// Rows of a set: the sort carries a row as 32 bits next to its key, and the noise lookup's argmin runs over the whole set in
// one pass with two tile minima per row and 64 noise rows in scratch -- at most kMaxLookup doubles of them (2 GiB); it is
// not batched the way vbmc_sq_dist batches its rows.
constexpr int64_t kMaxRows = (int64_t)1 << 20;
constexpr int64_t kMaxLookup = (int64_t)1 << 28;

// The copies a call queues read host memory of that call (the table, the parameters, the bounds, the caller's rows): a
// call that fails after queueing some of them waits for the stream before that memory goes away.
}  // namespace
int search_fail_wait(vbmc_ctx* ctx, int rc) {
  if (ctx && ctx->device >= 0 && ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  return rc;
}
namespace {

int search_fill_queue(vbmc_ctx* ctx, const char* who, int D, int n_src, const vbmc_search_source* src, const double* lb_D,
                     const double* ub_D, uint32_t int_bits, int use_xf, double* X_out) {
  if (!ctx || D < 1 || n_src < 0 || (n_src > 0 && !src) || (lb_D == nullptr) != (ub_D == nullptr)) return VBMC_E_ARG;
  NEED_DEVICE(ctx);
  if (D > 32) return vbmc_fail(ctx, VBMC_E_UNSUP, "%s: D=%d > 32 not supported", who, D);
  if (D < 32 && (int_bits >> D)) return vbmc_fail(ctx, VBMC_E_ARG, "%s: integer_bits names a dimension >= D=%d", who, D);
  int64_t M = 0;
  size_t n_par = 0, n_in = 0;
  int n_act = 0, n_mix = 0;
  for (int i = 0; i < n_src; ++i) {
    const vbmc_search_source& s = src[i];
    if (s.rows < 0) return vbmc_fail(ctx, VBMC_E_ARG, "%s: source %d has %lld rows", who, i, (long long)s.rows);
    if (s.rows == 0) continue;
    switch (s.kind) {
      case VBMC_SRC_COPY: break;
      case VBMC_SRC_TRANSFORM: n_in += use_xf ? (size_t)s.rows * D : 0; break;
      case VBMC_SRC_MIXTURE:
        if (!ctx->mix_set || ctx->D != D) return vbmc_fail(ctx, VBMC_E_ARG, "%s: mixture not set for D=%d", who, D);
        if (s.df < 0.0 || s.df != s.df) return vbmc_fail(ctx, VBMC_E_ARG, "%s: df=%g", who, s.df);
        ++n_mix;
        break;
      case VBMC_SRC_AFFINE: n_par += (size_t)D * (D + 1); break;
      case VBMC_SRC_BOX: n_par += 2 * (size_t)D; break;
      default: return vbmc_fail(ctx, VBMC_E_ARG, "%s: source %d has unknown kind %d", who, i, s.kind);
    }
    if (s.kind != VBMC_SRC_MIXTURE && !s.data) return vbmc_fail(ctx, VBMC_E_ARG, "%s: source %d has no data", who, i);
    M += s.rows;
    ++n_act;
  }
  if (M > kMaxRows) return vbmc_fail(ctx, VBMC_E_UNSUP, "%s: %lld rows (more than 2^20) not supported", who, (long long)M);
  XfView t;
  int rc = 0;
  if (use_xf && (rc = xf_need(ctx, 0, D, who, t))) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  SearchState* st = search_of(ctx);
  st->M = 0;  // (a fill that fails half way leaves no set)
  if ((rc = ensure_dev(ctx, &st->d_X, &st->cap, (size_t)M * D))) return rc;
  st->D = D;
  if (M == 0) return VBMC_OK;
  // scratch: the table | its parameters | the search bounds | the rows that go through the transformer | one selector per
  // mixture source
  const int K = ctx->K;
  Scratch sc;
  const auto p_tab = sc.add<SearchSrcDev>((size_t)n_act);
  const auto p_par = sc.add(n_par), p_bnd = sc.add(lb_D ? 2 * (size_t)D : 0);
  const auto p_in = sc.add(n_in), p_sel = sc.add(n_mix ? (size_t)n_mix * selector_elems(K) : 0);
  if ((rc = reserve(ctx, sc))) return rc;
  SearchSrcDev* d_tab = sc.ptr(p_tab);
  double *d_par = sc.ptr(p_par), *d_bnd = sc.ptr(p_bnd), *d_in = sc.ptr(p_in), *d_sel = sc.ptr(p_sel);
  std::vector<SearchSrcDev> tab;
  std::vector<double> par(n_par), bnd;
  if ((rc = timing_begin(ctx, T_SEARCH_FILL))) return rc;
  int64_t row = 0;
  size_t o_par = 0, o_in = 0;
  int i_mix = 0;
  for (int i = 0; i < n_src; ++i) {
    const vbmc_search_source& s = src[i];
    if (s.rows == 0) continue;
    SearchSrcDev e;
    e.kind = s.kind;
    e.pad = 0;
    e.begin = row;
    e.count = s.rows;
    e.seed = s.seed;
    e.par = (long long)o_par;
    double* d_rows = st->d_X + row * D;
    const size_t n_elem = (size_t)s.rows * D;
    if (s.kind == VBMC_SRC_COPY || (s.kind == VBMC_SRC_TRANSFORM && !use_xf)) {
      HIP_TRY(ctx, hipMemcpyAsync(d_rows, s.data, sizeof(double) * n_elem, hipMemcpyHostToDevice, ctx->stream));
    } else if (s.kind == VBMC_SRC_TRANSFORM) {
      HIP_TRY(ctx, hipMemcpyAsync(d_in + o_in, s.data, sizeof(double) * n_elem, hipMemcpyHostToDevice, ctx->stream));
      if ((rc = launch_xf_apply(ctx, t, s.rows, 0, d_in + o_in, d_rows))) return rc;
      o_in += n_elem;
    } else if (s.kind == VBMC_SRC_MIXTURE) {
      const double df = s.df == 0.0 ? INFINITY : s.df;
      rc = launch_sample(ctx, ctx->d_mix, ctx->ml, ctx->w.data(), s.rows, s.seed, 1, d_sel + (size_t)i_mix * selector_elems(K),
                         d_rows, nullptr, df);
      if (rc) return rc;
      ++i_mix;
    } else {
      const size_t n = s.kind == VBMC_SRC_AFFINE ? (size_t)D * (D + 1) : 2 * (size_t)D;
      memcpy(par.data() + o_par, s.data, sizeof(double) * n);
      o_par += n;
    }
    tab.push_back(e);
    row += s.rows;
  }
  HIP_TRY(ctx, hipMemcpyAsync(d_tab, tab.data(), sizeof(SearchSrcDev) * tab.size(), hipMemcpyHostToDevice, ctx->stream));
  if (n_par) HIP_TRY(ctx, hipMemcpyAsync(d_par, par.data(), sizeof(double) * n_par, hipMemcpyHostToDevice, ctx->stream));
  if (lb_D) {
    bnd.assign(lb_D, lb_D + D);
    bnd.insert(bnd.end(), ub_D, ub_D + D);
    HIP_TRY(ctx, hipMemcpyAsync(d_bnd, bnd.data(), sizeof(double) * 2 * D, hipMemcpyHostToDevice, ctx->stream));
  }
  rc = launch_search_fill(ctx, st->d_X, M, D, d_tab, (int)tab.size(), d_par, lb_D ? d_bnd : nullptr, lb_D ? d_bnd + D : nullptr,
                          int_bits, use_xf ? &t : nullptr);
  if (rc) return rc;
  if ((rc = timing_end(ctx, T_SEARCH_FILL))) return rc;
  if (X_out) HIP_TRY(ctx, hipMemcpyAsync(X_out, st->d_X, sizeof(double) * M * D, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, stream_wait(ctx));  // (the table, the parameters and the caller's rows are host memory of this call)
  st->M = M;
  return VBMC_OK;
}

int search_fill_impl(vbmc_ctx* ctx, const char* who, int D, int n_src, const vbmc_search_source* src, const double* lb_D,
                     const double* ub_D, uint32_t int_bits, int use_xf, double* X_out) {
  const int rc = search_fill_queue(ctx, who, D, n_src, src, lb_D, ub_D, int_bits, use_xf, X_out);
  return rc ? search_fail_wait(ctx, rc) : rc;
}

}  // namespace

void search_free(vbmc_ctx* ctx) {
  SearchState* st = (SearchState*)ctx->search;
  if (!st) return;
  if (st->d_X) (void)hipFree(st->d_X);
  delete st;
  ctx->search = nullptr;
}

extern "C" int vbmc_search_fill(vbmc_ctx* ctx, int D, int n_src, const vbmc_search_source* src, const double* lb_search_D,
                                const double* ub_search_D, uint32_t integer_bits, int use_xf, double* X_out_MxD) {
  return search_fill_impl(ctx, "search_fill", D, n_src, src, lb_search_D, ub_search_D, integer_bits, use_xf, X_out_MxD);
}

extern "C" int vbmc_search_put(vbmc_ctx* ctx, int64_t M, int D, const double* X_MxD, uint32_t integer_bits, int use_xf) {
  if (M < 0 || (M > 0 && !X_MxD)) return VBMC_E_ARG;
  vbmc_search_source s;
  s.kind = VBMC_SRC_COPY;
  s.rows = M;
  s.data = X_MxD;
  s.df = INFINITY;
  s.seed = 0;
  return search_fill_impl(ctx, "search_put", D, 1, &s, nullptr, nullptr, integer_bits, use_xf, nullptr);
}

// ---- scoring a block of device rows: what vbmc_search_eval runs on the resident set and vbmc_search_cmaes
// (api_cmaes.hip) on every generation's candidates.  The four steps are a call's order: check, list (the pieces go into
// s.p.sc in front of the caller's own), upload (after predict_reserve: the hard bounds and the noise table, once per
// call), rows (any number of times).

int search_score_check(vbmc_ctx* ctx, const char* who, int kind, int64_t n_noise, const double* X_rescaled_NxD,
                       const double* sn2_new_N, const double* length_scale_D, int use_xf, const double* lb_eps_orig_D,
                       const double* ub_eps_orig_D, SearchScore& s) {
  if (!ctx || !lb_eps_orig_D || !ub_eps_orig_D) return VBMC_E_ARG;
  NEED_DEVICE(ctx);
  if (kind < VBMC_ACQ_STD || kind > VBMC_ACQ_IS) return vbmc_fail(ctx, VBMC_E_UNSUP, "%s: unknown acquisition kind %d", who, kind);
  if (!ctx->gp.set) return vbmc_fail(ctx, VBMC_E_ARG, "%s: GP not set", who);
  s.kind = kind;
  s.is_kind = kind == VBMC_ACQ_IS;
  s.noisy = s.is_kind || kind == VBMC_ACQ_NOISY;
  const int D = ctx->gp.D;
  if (!s.is_kind && !ctx->mix_set) return vbmc_fail(ctx, VBMC_E_ARG, "%s: mixture not set", who);
  if (!s.is_kind && ctx->D != D) return vbmc_fail(ctx, VBMC_E_ARG, "%s: GP/mixture D mismatch", who);
  if (D > 32) return vbmc_fail(ctx, VBMC_E_UNSUP, "%s: D=%d > 32 not supported", who, D);
  if (s.noisy && (n_noise < 1 || !X_rescaled_NxD || !sn2_new_N || !length_scale_D))
    return vbmc_fail(ctx, VBMC_E_ARG, "%s: this acquisition needs X_rescaled, sn2_new and the length scale", who);
  if (s.noisy && n_noise > ((int64_t)1 << 24)) return vbmc_fail(ctx, VBMC_E_UNSUP, "%s: more than 2^24 noise rows", who);
  s.n_noise = s.noisy ? n_noise : 0;
  s.Na = 0;
  int rc = 0;
  if (s.is_kind && (rc = acq_is_need(ctx, who, &s.Na))) return rc;
  s.use_xf = use_xf;
  if (use_xf && (rc = xf_need(ctx, 0, D, who, s.t))) return rc;
  s.X_rescaled = X_rescaled_NxD;
  s.sn2_new = sn2_new_N;
  s.length_scale = length_scale_D;
  s.lb_eps = lb_eps_orig_D;
  s.ub_eps = ub_eps_orig_D;
  return 0;
}

int search_score_list(vbmc_ctx* ctx, const char* who, int64_t M, SearchScore& s) {
  if (s.noisy && 2 * ((s.n_noise + 63) / 64) * M > kMaxLookup)
    return vbmc_fail(ctx, VBMC_E_UNSUP, "%s: %lld points against %lld noise rows: the lookup's scratch is not batched", who,
                     (long long)M, (long long)s.n_noise);
  // The batch plans of vbmc_acq_eval / vbmc_acq_is_eval, then the scoring's own pieces:
  //   dens (mb) or Kx (mb x N) | T (mb x Na) | as [S][mb];  res (3 mb);  sn2 (M);  hard bounds (2 D);
  //   noise lookup: ell (D) | set / ell (M x D) | X_rescaled (Nn x D) | sn2_new (Nn) | centre (D) | column sums of both
  //   sets | tile minima and indices (2 tiles M) | argmin (M int64)
  const GpState& g = ctx->gp;
  const int N = g.N, D = g.D, S = g.S;
  PredictPlan& p = s.p;
  if (s.is_kind) predict_plan(ctx, M, (int64_t)1 << 26, (int64_t)S * N + N + s.Na, 16384, p);
  else predict_plan(ctx, M, (int64_t)1 << 27, (int64_t)S * N, 65536, p);
  const bool is_kind = s.is_kind, noisy = s.noisy;
  const size_t mb = (size_t)p.mb, Ms = (size_t)M, Nn = (size_t)s.n_noise, nt = (Nn + 63) / 64;
  s.M = M;
  s.p_dens = p.sc.add(is_kind ? 0 : mb);
  s.p_Kx = p.sc.add(is_kind ? mb * N : 0);
  s.p_T = p.sc.add(is_kind ? mb * (size_t)s.Na : 0);
  s.p_as = p.sc.add(is_kind ? S * mb : 0);
  s.p_res = p.sc.add(3 * mb);
  s.p_sn2 = p.sc.add(noisy ? Ms : 0);
  s.p_bnd = p.sc.add(2 * (size_t)D);
  s.p_ell = p.sc.add(noisy ? (size_t)D : 0);
  s.p_xsc = p.sc.add(Nn ? Ms * D : 0);
  s.p_b = p.sc.add(Nn * D);
  s.p_tab = p.sc.add(Nn);
  s.p_cen = p.sc.add(noisy ? (size_t)D : 0);
  s.p_part = p.sc.add(noisy ? 2 * (size_t)search_sum_blocks * D : 0);
  s.p_pmin = p.sc.add(2 * nt * (noisy ? Ms : 0));
  s.p_am = p.sc.add<int64_t>(noisy ? Ms : 0);
  return 0;
}

int search_score_upload(vbmc_ctx* ctx, SearchScore& s) {
  const int D = ctx->gp.D;
  const size_t Nn = (size_t)s.n_noise;
  s.bnd.assign(s.lb_eps, s.lb_eps + D);
  s.bnd.insert(s.bnd.end(), s.ub_eps, s.ub_eps + D);
  HIP_TRY(ctx, hipMemcpyAsync(s.p.sc.ptr(s.p_bnd), s.bnd.data(), sizeof(double) * 2 * D, hipMemcpyHostToDevice, ctx->stream));
  if (s.noisy) {
    HIP_TRY(ctx, hipMemcpyAsync(s.p.sc.ptr(s.p_ell), s.length_scale, sizeof(double) * D, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(s.p.sc.ptr(s.p_b), s.X_rescaled, sizeof(double) * Nn * D, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(s.p.sc.ptr(s.p_tab), s.sn2_new, sizeof(double) * Nn, hipMemcpyHostToDevice, ctx->stream));
  }
  return 0;
}

int search_score_rows(vbmc_ctx* ctx, const SearchScore& s, const double* d_X, int64_t M, double y_max, double tol_gp_var,
                      double u, double* d_acq) {
  const PredictPlan& p = s.p;
  const int D = ctx->gp.D;
  const size_t mb = (size_t)p.mb;
  const int64_t n_noise = s.n_noise;
  double *d_res = p.sc.ptr(s.p_res), *d_sn2 = p.sc.ptr(s.p_sn2), *d_bnd = p.sc.ptr(s.p_bnd);
  int rc = 0;
  if (s.noisy) {
    // sn2_new[argmin_n |Xs / ell - X_rescaled_n|^2]   (abstract_acq_fcn.py:244-256)
    double *d_ell = p.sc.ptr(s.p_ell), *d_xsc = p.sc.ptr(s.p_xsc), *d_b = p.sc.ptr(s.p_b), *d_tab = p.sc.ptr(s.p_tab);
    double *d_cen = p.sc.ptr(s.p_cen), *d_part = p.sc.ptr(s.p_part), *d_pmin = p.sc.ptr(s.p_pmin);
    int64_t* d_am = p.sc.ptr(s.p_am);
    if ((rc = launch_search_scale(ctx, d_X, M, D, d_ell, d_xsc))) return rc;
    if ((rc = launch_search_colsum(ctx, d_xsc, M, D, d_part))) return rc;
    if ((rc = launch_search_colsum(ctx, d_b, n_noise, D, d_part + (size_t)search_sum_blocks * D))) return rc;
    if ((rc = launch_search_centre(ctx, d_part, M, d_part + (size_t)search_sum_blocks * D, n_noise, D, d_cen))) return rc;
    if ((rc = launch_sq_dist(ctx, d_xsc, M, d_b, (int)n_noise, D, d_cen, nullptr, d_pmin, d_am))) return rc;
    if ((rc = launch_search_take(ctx, d_tab, n_noise, d_am, M, d_sn2))) return rc;
  }
  for (int64_t o = 0; o < M; o += p.mb) {
    const int64_t m = (M - o) < p.mb ? (M - o) : p.mb;
    const double* d_xs = d_X + o * D;
    if (s.is_kind) {
      rc = launch_acq_is(ctx, p, m, d_xs, d_sn2 + o, u, p.sc.ptr(s.p_Kx), p.sc.ptr(s.p_T), p.sc.ptr(s.p_as), d_res);
      if (!rc) rc = launch_search_is_finish(ctx, m, tol_gp_var, d_res + mb, d_res);
    } else {
      rc = launch_acq_closed(ctx, p, m, d_xs, s.noisy ? d_sn2 + o : nullptr, s.kind, y_max, tol_gp_var, p.sc.ptr(s.p_dens), d_res);
    }
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(d_acq + o, d_res, sizeof(double) * m, hipMemcpyDeviceToDevice, ctx->stream));
  }
  return launch_search_mask(ctx, d_X, M, D, s.use_xf ? &s.t : nullptr, d_bnd, d_bnd + D, d_acq);
}

int search_set_rows_cap() { return (int)kMaxRows; }

static int search_eval_queue(vbmc_ctx* ctx, int kind, double y_max, double tol_gp_var, double u, int64_t n_noise,
                             const double* X_rescaled_NxD, const double* sn2_new_N, const double* length_scale_D, int use_xf,
                             const double* lb_eps_orig_D, const double* ub_eps_orig_D, double* acq_M, int64_t* order_M,
                             double* X_sorted_MxD) {
  SearchScore s;
  int rc = search_score_check(ctx, "search_eval", kind, n_noise, X_rescaled_NxD, sn2_new_N, length_scale_D, use_xf,
                              lb_eps_orig_D, ub_eps_orig_D, s);
  if (rc) return rc;
  const int D = ctx->gp.D;
  const SearchState* st = (const SearchState*)ctx->search;
  if (!st || st->D != D || (st->M > 0 && !st->d_X))
    return vbmc_fail(ctx, VBMC_E_ARG, "search_eval: no search set for D=%d (vbmc_search_fill / vbmc_search_put)", D);
  const int64_t M = st->M;
  if (M == 0) return VBMC_OK;
  if ((rc = search_score_list(ctx, "search_eval", M, s))) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // behind the scoring's pieces, this call's own:
  //   acq (M) | order (M int64) | sorted points (M x D): one block, copied out in one piece;
  //   keys (P uint64) | rows (P uint32)
  PredictPlan& p = s.p;
  const size_t Ms = (size_t)M, P = (size_t)search_sort_len(M);
  const auto p_acq = p.sc.add(Ms);
  const auto p_ord = p.sc.add<int64_t>(Ms);
  const auto p_Xs = p.sc.add(Ms * D);
  const auto p_keys = p.sc.add<uint64_t>(P);
  const auto p_idx = p.sc.add<uint32_t>(P);
  const size_t n_out = (2 + (size_t)D) * Ms;
  if ((rc = predict_reserve(ctx, p, 0))) return rc;
  if ((rc = ensure_pinned(ctx, n_out))) return rc;
  double *d_acq = p.sc.ptr(p_acq), *d_Xs = p.sc.ptr(p_Xs);
  int64_t* d_ord = p.sc.ptr(p_ord);
  uint64_t* d_keys = p.sc.ptr(p_keys);
  uint32_t* d_idx = p.sc.ptr(p_idx);
  if ((rc = timing_begin(ctx, T_SEARCH_EVAL))) return rc;
  if ((rc = search_score_upload(ctx, s))) return rc;
  if ((rc = search_score_rows(ctx, s, st->d_X, M, y_max, tol_gp_var, u, d_acq))) return rc;
  if ((rc = timing_end(ctx, T_SEARCH_EVAL))) return rc;
  if ((rc = timing_begin(ctx, T_SEARCH_SORT))) return rc;
  if ((rc = launch_search_sort(ctx, d_acq, M, d_keys, d_idx))) return rc;
  if ((rc = launch_search_gather(ctx, st->d_X, d_idx, M, D, d_ord, d_Xs))) return rc;
  if ((rc = timing_end(ctx, T_SEARCH_SORT))) return rc;
  // acq | order | sorted points lie one behind the other: one copy
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_pinned, d_acq, sizeof(double) * n_out, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, stream_wait(ctx));  // (also: the bounds and the caller's noise arrays are host memory of this call)
  if (acq_M) memcpy(acq_M, ctx->h_pinned, sizeof(double) * Ms);
  if (order_M) memcpy(order_M, ctx->h_pinned + Ms, sizeof(int64_t) * Ms);
  if (X_sorted_MxD) memcpy(X_sorted_MxD, ctx->h_pinned + 2 * Ms, sizeof(double) * Ms * D);
  return VBMC_OK;
}

extern "C" int vbmc_search_eval(vbmc_ctx* ctx, int kind, double y_max, double tol_gp_var, double u, int64_t n_noise,
                                const double* X_rescaled_NxD, const double* sn2_new_N, const double* length_scale_D, int use_xf,
                                const double* lb_eps_orig_D, const double* ub_eps_orig_D, double* acq_M, int64_t* order_M,
                                double* X_sorted_MxD) {
  const int rc = search_eval_queue(ctx, kind, y_max, tol_gp_var, u, n_noise, X_rescaled_NxD, sn2_new_N, length_scale_D, use_xf,
                                   lb_eps_orig_D, ub_eps_orig_D, acq_M, order_M, X_sorted_MxD);
  return rc ? search_fail_wait(ctx, rc) : rc;
}
