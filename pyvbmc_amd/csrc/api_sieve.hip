// The sieve of optimize_vp (vbmc/variational_optimization.py:660-810) as device calls.
//
// The context keeps one resident set of candidate thetas (B x n_theta, raw parameters).  vbmc_sieve_fill generates it
// (sieve.hip: _vb_init, :813-988, and get_parameters, one workgroup per candidate), vbmc_sieve_put takes a caller's rows;
// vbmc_sieve_eval queues the scoring launches of vbmc_neg_elcbo_batch (api_batch.hip batch_score_*) on it, ranks the
// values with the acquisition search's sort (search.hip) and hands F | G | H | order | the thetas in rank order to the
// host in one copy.  Between fill and eval the candidates exist only in device memory.
#include <cmath>
#include <cstring>

#include "common.h"

namespace {

struct SieveState {
  double* d_th = nullptr;  // B x n_theta
  size_t cap = 0;
  int64_t B = 0;
  int n_theta = 0;
};

SieveState* sieve_of(vbmc_ctx* ctx) {
  if (!ctx->sieve) ctx->sieve = new SieveState();
  return (SieveState*)ctx->sieve;
}

constexpr int64_t kMaxCand = (int64_t)1 << 20;  // the sort carries a row as 32 bits; one workgroup per candidate

int sieve_fill_queue(vbmc_ctx* ctx, const vbmc_sieve_fill_args* f, double* thetas_out) {
  const char* who = "sieve_fill";
  const int D = f->D, K = f->K, Kn = f->K_new, mask = f->optimize_mask;
  if (D < 1 || K < 1 || f->n1 < 0 || f->n2 < 0 || f->n3 < 0 || !f->mu0_KxD || !f->sigma0_K || !f->lambd0_D || !f->w0_K)
    return vbmc_fail(ctx, VBMC_E_ARG, "%s: bad arguments", who);
  // what the generator covers, refused before anything is queued
  if (D > 32 || Kn > 128) return vbmc_fail(ctx, VBMC_E_UNSUP, "%s: D=%d, K_new=%d beyond D <= 32, K_new <= 128", who, D, Kn);
  if (!(mask & 2)) return vbmc_fail(ctx, VBMC_E_UNSUP, "%s: optimize_sigma off is not covered", who);
  if (Kn < K) return vbmc_fail(ctx, VBMC_E_UNSUP, "%s: K_new=%d < K=%d is not covered", who, Kn, K);
  if (Kn > K && !(mask & 1)) return vbmc_fail(ctx, VBMC_E_UNSUP, "%s: K_new > K needs optimize_mu", who);
  const int64_t B = f->n1 + f->n2 + f->n3;
  if (B > kMaxCand) return vbmc_fail(ctx, VBMC_E_UNSUP, "%s: %lld candidates (more than 2^20)", who, (long long)B);
  const bool host_draws = f->Z_BxS != nullptr;
  const bool need_X = f->n3 > 0 && (mask & 1);
  if (need_X && (f->N_star < 1 || !f->X_star_NxD)) return vbmc_fail(ctx, VBMC_E_ARG, "%s: type 3 needs X_star", who);
  if (f->n2 > 0 && (!f->mu2_KnxD || !f->sigma2_Kn)) return vbmc_fail(ctx, VBMC_E_ARG, "%s: type 2 needs its start", who);
  if ((f->n2 > 0 || f->n3 > 0) && (mask & 4) && !f->lambd_s_D) return vbmc_fail(ctx, VBMC_E_ARG, "%s: lambd_s missing", who);
  if (f->N_star > ((int64_t)1 << 30)) return vbmc_fail(ctx, VBMC_E_UNSUP, "%s: N_star too large", who);
  const int n_slot = (Kn - K) * (D + 2) + 3 * Kn + D * Kn + D;
  const bool need_I = host_draws && (Kn > K || need_X);
  if (host_draws && f->n_slot != n_slot) return vbmc_fail(ctx, VBMC_E_ARG, "%s: %d draw slots, not %d", who, f->n_slot, n_slot);
  if (need_I && !f->I_BxKn) return vbmc_fail(ctx, VBMC_E_ARG, "%s: host draws without their index matrix", who);
  if (need_I)  // every index is an address: checked here, once
    for (int64_t b = 0; b < B; ++b) {
      const bool t1 = b < f->n1, t3 = b >= f->n1 + f->n2;
      const int n = t1 ? Kn - K : (t3 && need_X ? (Kn < f->N_star ? Kn : (int)f->N_star) : 0);
      const int64_t lim = t1 ? K : f->N_star;
      for (int k = 0; k < n; ++k) {
        const int32_t v = f->I_BxKn[b * Kn + k];
        if (v < 0 || v >= lim) return vbmc_fail(ctx, VBMC_E_ARG, "%s: index %d of candidate %lld out of range", who, (int)v, (long long)b);
      }
    }
  const ThetaMap tm(D, Kn, mask);
  const int n_theta = tm.n_theta();
  SieveFillDev a;
  a.D = D; a.K = K; a.Kn = Kn; a.mask = mask; a.n_theta = n_theta; a.Ns = need_X ? (int)f->N_star : 0; a.n_slot = n_slot;
  a.n1 = f->n1; a.n2 = f->n2; a.n3 = f->n3; a.seed = f->seed; a.v3 = f->v3;
  if (sieve_fill_lds_bytes(D, Kn, (!host_draws && need_X) ? a.Ns : 0) > 64 * 1024)
    return vbmc_fail(ctx, VBMC_E_UNSUP, "%s: N_star=%lld does not fit the generator's LDS", who, (long long)f->N_star);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  SieveState* st = sieve_of(ctx);
  st->B = 0;  // (a fill that fails half way leaves no set)
  int rc = 0;
  if ((rc = ensure_dev(ctx, &st->d_th, &st->cap, (size_t)B * n_theta))) return rc;
  st->n_theta = n_theta;
  if (B == 0) return VBMC_OK;
  // scratch: base (mu0 | sigma0 | lambd0 | w0) | type 2's start | lambd_s | X_star | Z | I
  const size_t n_base = (size_t)K * D + 2 * (size_t)K + D, n_t2 = f->n2 > 0 ? (size_t)Kn * D + Kn : 0;
  Scratch sc;
  const auto p_base = sc.add(n_base), p_t2 = sc.add(n_t2), p_ls = sc.add(f->lambd_s_D ? (size_t)D : 0);
  const auto p_X = sc.add(need_X ? (size_t)f->N_star * D : 0), p_Z = sc.add(host_draws ? (size_t)B * n_slot : 0);
  const auto p_I = sc.add<int>(need_I ? (size_t)B * Kn : 0);
  if ((rc = reserve(ctx, sc))) return rc;
  if ((rc = ensure_pinned(ctx, n_base + n_t2 + D))) return rc;
  hipStream_t sm = ctx->stream;
  double* hp = ctx->h_pinned;
  memcpy(hp, f->mu0_KxD, sizeof(double) * K * D);
  memcpy(hp + (size_t)K * D, f->sigma0_K, sizeof(double) * K);
  memcpy(hp + (size_t)K * D + K, f->lambd0_D, sizeof(double) * D);
  memcpy(hp + (size_t)K * D + K + D, f->w0_K, sizeof(double) * K);
  if (n_t2) {
    memcpy(hp + n_base, f->mu2_KnxD, sizeof(double) * Kn * D);
    memcpy(hp + n_base + (size_t)Kn * D, f->sigma2_Kn, sizeof(double) * Kn);
  }
  if (f->lambd_s_D) memcpy(hp + n_base + n_t2, f->lambd_s_D, sizeof(double) * D);
  // base | t2 | lambd_s lie one behind the other in the scratch as in the pinned buffer: one copy
  HIP_TRY(ctx, hipMemcpyAsync(sc.ptr(p_base), hp, sizeof(double) * (n_base + n_t2 + (f->lambd_s_D ? D : 0)), hipMemcpyHostToDevice, sm));
  if (need_X) HIP_TRY(ctx, hipMemcpyAsync(sc.ptr(p_X), f->X_star_NxD, sizeof(double) * f->N_star * D, hipMemcpyHostToDevice, sm));
  if (host_draws) HIP_TRY(ctx, hipMemcpyAsync(sc.ptr(p_Z), f->Z_BxS, sizeof(double) * B * n_slot, hipMemcpyHostToDevice, sm));
  if (need_I) HIP_TRY(ctx, hipMemcpyAsync(sc.ptr(p_I), f->I_BxKn, sizeof(int) * B * Kn, hipMemcpyHostToDevice, sm));
  a.base = sc.ptr(p_base);
  a.t2 = n_t2 ? sc.ptr(p_t2) : nullptr;
  a.lam_s = f->lambd_s_D ? sc.ptr(p_ls) : nullptr;
  a.Xs = need_X ? sc.ptr(p_X) : nullptr;
  a.Z = host_draws ? sc.ptr(p_Z) : nullptr;
  a.I = need_I ? sc.ptr(p_I) : nullptr;
  a.thetas = st->d_th;
  if ((rc = timing_begin(ctx, T_SIEVE_FILL))) return rc;
  if ((rc = launch_sieve_fill(ctx, a))) return rc;
  if ((rc = timing_end(ctx, T_SIEVE_FILL))) return rc;
  if (thetas_out) {
    if ((rc = download_chunked(ctx, st->d_th, thetas_out, (size_t)B * n_theta))) return rc;
  } else {
    HIP_TRY(ctx, stream_wait(ctx));  // (the caller's arrays are host memory of this call)
  }
  st->B = B;
  return VBMC_OK;
}

int sieve_eval_queue(vbmc_ctx* ctx, const vbmc_elbo_opts* opts, double* F_B, double* G_B, double* H_B, int64_t* order_B,
                     double* thetas_sorted) {
  const char* who = "sieve_eval";
  const SieveState* st = (const SieveState*)ctx->sieve;
  if (!st || (st->B > 0 && !st->d_th)) return vbmc_fail(ctx, VBMC_E_ARG, "%s: no candidate set (vbmc_sieve_fill / vbmc_sieve_put)", who);
  const int64_t B = st->B;
  const int n_theta = st->n_theta;
  int rc = batch_score_check(ctx, who, (int)B, n_theta, opts);
  if (rc) return rc;
  if (ctx->D > 32) return vbmc_fail(ctx, VBMC_E_UNSUP, "%s: D=%d > 32 not supported", who, ctx->D);
  if (B == 0) return VBMC_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // scratch: the scoring's pieces, then this call's own:
  //   F G H (3 B) | order (B int64) | thetas in rank order (B x n_theta): one block, copied out in one piece;
  //   keys (P uint64) | rows (P uint32)
  Scratch sc;
  BatchScore s;
  batch_score_list(ctx, (int)B, n_theta, opts, sc, s);
  const size_t Bs = (size_t)B, P = (size_t)search_sort_len(B);
  const auto p_fgh = sc.add(3 * Bs);
  const auto p_ord = sc.add<int64_t>(Bs);
  const auto p_ths = sc.add(Bs * n_theta);
  const auto p_keys = sc.add<uint64_t>(P);
  const auto p_idx = sc.add<uint32_t>(P);
  const size_t n_out = (4 + (size_t)n_theta) * Bs;
  if ((rc = reserve(ctx, sc))) return rc;
  if ((rc = ensure_pinned(ctx, n_out + batch_score_pinned(s)))) return rc;
  double *d_fgh = sc.ptr(p_fgh), *d_ths = sc.ptr(p_ths);
  int64_t* d_ord = sc.ptr(p_ord);
  if ((rc = timing_begin(ctx, T_SIEVE_SCORE))) return rc;
  if ((rc = batch_score_queue(ctx, who, sc, s, opts, st->d_th, ctx->h_pinned + n_out))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(d_fgh, sc.ptr(s.p_out), sizeof(double) * 3 * Bs, hipMemcpyDeviceToDevice, ctx->stream));
  // a candidate that is not finite scores NaN and ranks last: the sieve drops it, it does not fail the call
  if ((rc = launch_sieve_nan_rows(ctx, st->d_th, B, n_theta, d_fgh, d_fgh + Bs, d_fgh + 2 * Bs))) return rc;
  if ((rc = timing_end(ctx, T_SIEVE_SCORE))) return rc;
  if ((rc = timing_begin(ctx, T_SIEVE_RANK))) return rc;
  if ((rc = launch_search_sort(ctx, d_fgh, B, sc.ptr(p_keys), sc.ptr(p_idx)))) return rc;
  if ((rc = launch_search_gather(ctx, st->d_th, sc.ptr(p_idx), B, n_theta, d_ord, d_ths))) return rc;
  if ((rc = timing_end(ctx, T_SIEVE_RANK))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_pinned, d_fgh, sizeof(double) * n_out, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, stream_wait(ctx));
  const double* hp = ctx->h_pinned;
  if (F_B) memcpy(F_B, hp, sizeof(double) * Bs);
  if (G_B) memcpy(G_B, hp + Bs, sizeof(double) * Bs);
  if (H_B) memcpy(H_B, hp + 2 * Bs, sizeof(double) * Bs);
  if (order_B) memcpy(order_B, hp + 3 * Bs, sizeof(int64_t) * Bs);
  if (thetas_sorted) memcpy(thetas_sorted, hp + 4 * Bs, sizeof(double) * Bs * n_theta);
  return VBMC_OK;
}

}  // namespace

void sieve_free(vbmc_ctx* ctx) {
  SieveState* st = (SieveState*)ctx->sieve;
  if (!st) return;
  if (st->d_th) (void)hipFree(st->d_th);
  delete st;
  ctx->sieve = nullptr;
}

extern "C" int vbmc_sieve_fill(vbmc_ctx* ctx, const vbmc_sieve_fill_args* args, double* thetas_out_BxN) {
  if (!ctx || !args) return VBMC_E_ARG;
  NEED_DEVICE(ctx);
  const int rc = sieve_fill_queue(ctx, args, thetas_out_BxN);
  return rc ? search_fail_wait(ctx, rc) : rc;
}

extern "C" int vbmc_sieve_put(vbmc_ctx* ctx, int64_t B, int n_theta, const double* thetas_BxN) {
  if (!ctx || B < 0 || n_theta < 1 || (B > 0 && !thetas_BxN)) return VBMC_E_ARG;
  NEED_DEVICE(ctx);
  if (B > kMaxCand) return vbmc_fail(ctx, VBMC_E_UNSUP, "sieve_put: %lld candidates (more than 2^20)", (long long)B);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  SieveState* st = sieve_of(ctx);
  st->B = 0;
  int rc = ensure_dev(ctx, &st->d_th, &st->cap, (size_t)B * n_theta);
  if (rc) return rc;
  st->n_theta = n_theta;
  if (B > 0) {
    const hipError_t e = hipMemcpyAsync(st->d_th, thetas_BxN, sizeof(double) * B * n_theta, hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) return search_fail_wait(ctx, vbmc_fail(ctx, VBMC_E_HIP, "sieve_put: %s", hipGetErrorString(e)));
    HIP_TRY(ctx, stream_wait(ctx));  // (the rows are host memory of this call)
  }
  st->B = B;
  return VBMC_OK;
}

extern "C" int vbmc_sieve_eval(vbmc_ctx* ctx, const vbmc_elbo_opts* opts, double* F_B, double* G_B, double* H_B,
                               int64_t* order_B, double* thetas_sorted_BxN) {
  if (!ctx || !opts) return VBMC_E_ARG;
  NEED_DEVICE(ctx);
  const int rc = sieve_eval_queue(ctx, opts, F_B, G_B, H_B, order_B, thetas_sorted_BxN);
  return rc ? search_fail_wait(ctx, rc) : rc;
}
