// The last stage of optimize_vp as device calls: the full ELCBO (vbmc/variational_optimization.py:428-499) and the
// pruning trials (:322-378).
//
// The context owns one record of a full evaluation: I_sk (S x K0) and J_sjk (S x K0 x K0, the gram kernel's d_Q) in a
// device buffer of its own, the current mixture (K_alive components) on the host, and the alive list -- which columns of
// the record those components stand for.  A trial removes one alive component, forms the K' mixture as the reference's
// delete / get_parameters / set_parameters do, runs the value-only entropy launches on it and re-weights the record
// (elcbo_full.hip); no GP kernel is launched.  The record's layout, listed once (scratch.h):
//   I (S K0) | J (S K0 K0, with variance) | w' (K0) | part (2 S) | out (3) | alive (K0 int)
#include <cmath>
#include <cstring>

#include "common.h"

namespace {

constexpr int kMaxD = 32, kMaxK = 128;

struct Mix {  // a mixture on the host, as the context keeps its own: mu is K x D
  int K = 0;
  std::vector<double> mu, sigma, lambd, w, eta;
  std::vector<int> alive;  // the record's column of every component
};

struct ElcboRecord {
  bool valid = false, has_J = false, trial_valid = false;
  int S = 0, K0 = 0, D = 0;
  double* d_buf = nullptr;
  size_t cap = 0;
  Scratch sc;
  Piece<> p_I, p_J, p_w, p_part, p_out;
  Piece<int> p_alive;
  Mix cur, trial;
  uint64_t gp_launches0 = 0;  // ctx->gp_launches when the record was made
  uint64_t waits0 = 0;        // ctx->stream_waits then
  std::vector<double> h_w;    // host sources of the trial's small uploads (they outlive the call)
  std::vector<int> h_alive;
};

ElcboRecord* record_of(vbmc_ctx* ctx) {
  if (!ctx->elcbo) ctx->elcbo = new ElcboRecord();
  return (ElcboRecord*)ctx->elcbo;
}

int record_reserve(vbmc_ctx* ctx, ElcboRecord* r, int S, int K0, bool has_J) {
  r->valid = r->trial_valid = false;
  r->sc = Scratch();
  const size_t s = (size_t)S, k = (size_t)K0;
  r->p_I = r->sc.add(s * k);
  r->p_J = r->sc.add(has_J ? s * k * k : 0);
  r->p_w = r->sc.add(k);
  r->p_part = r->sc.add(2 * s);
  r->p_out = r->sc.add(3);
  r->p_alive = r->sc.add<int>(k);
  const int rc = reserve_in(ctx, &r->d_buf, &r->cap, r->sc);
  if (rc) return rc;
  r->S = S;
  r->K0 = K0;
  r->has_J = has_J;
  return 0;
}

void mix_from_ctx(const vbmc_ctx* ctx, Mix& m) {
  m.K = ctx->K;
  m.mu = ctx->mu;
  m.sigma = ctx->sigma;
  m.lambd = ctx->lambd;
  m.w = ctx->w;
  m.eta = ctx->eta;
  m.alive.resize(ctx->K);
  for (int k = 0; k < ctx->K; ++k) m.alive[k] = k;
}

// weights and alive list of `m` to the record's pieces, then the re-weighting launches
int reweight_queue(vbmc_ctx* ctx, ElcboRecord* r, const Mix& m) {
  r->h_w = m.w;
  r->h_alive = m.alive;
  HIP_TRY(ctx, hipMemcpyAsync(r->sc.ptr(r->p_w), r->h_w.data(), sizeof(double) * m.K, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(r->sc.ptr(r->p_alive), r->h_alive.data(), sizeof(int) * m.K, hipMemcpyHostToDevice, ctx->stream));
  return launch_elcbo_reweight(ctx, r->S, r->K0, m.K, r->sc.ptr(r->p_I), r->has_J ? r->sc.ptr(r->p_J) : nullptr,
                               r->sc.ptr(r->p_w), r->sc.ptr(r->p_alive), r->sc.ptr(r->p_part), r->sc.ptr(r->p_out));
}

// The value-only entropy of the context's mixture, queued: *H_host is set when it has a closed form (K == 1 without
// draws, entlb_vbmc.py:60-78), else the raw vector's first entry lands in ctx->d_out[0].
int entropy_check(vbmc_ctx* ctx, const char* who, int64_t ns, int eps_mode) {
  if (ns < 0 || (ns & 1)) return vbmc_fail(ctx, VBMC_E_ARG, "%s: ns_per_comp=%lld must be even and >= 0", who, (long long)ns);
  if (ctx_is_multi(ctx)) return vbmc_fail(ctx, VBMC_E_UNSUP, "%s: not covered with a communicator", who);
  if (ns == 0) return 0;
  if (eps_mode == VBMC_EPS_RESIDENT) {
    if (!ctx->d_eps || ctx->eps_K != ctx->K || ctx->eps_D != ctx->D || ctx->eps_n_half != ns / 2 || ctx->eps_row_begin != 0 ||
        ctx->eps_rows != ns / 2)
      return vbmc_fail(ctx, VBMC_E_ARG, "%s: resident eps (K=%d D=%d n_half=%lld) does not match the request (K=%d D=%d n_half=%lld); call vbmc_set_eps",
                       who, ctx->eps_K, ctx->eps_D, (long long)ctx->eps_n_half, ctx->K, ctx->D, (long long)(ns / 2));
  } else if (eps_mode != VBMC_EPS_PHILOX) {
    return vbmc_fail(ctx, VBMC_E_ARG, "%s: unknown eps_mode %d", who, eps_mode);
  }
  return 0;
}

int entropy_queue(vbmc_ctx* ctx, int64_t ns, int eps_mode, uint64_t seed, bool* on_host, double* H_host) {
  *on_host = false;
  if (ns == 0 && ctx->K == 1) {
    *on_host = true;
    return vbmc_entlb(ctx, 0, 1, H_host, nullptr);
  }
  int rc = ensure_dev(ctx, &ctx->d_out, &ctx->d_out_cap, (size_t)raw_len(ctx->D, ctx->K));
  if (rc) return rc;
  if (ns == 0) return launch_entlb(ctx, ctx->d_out);
  return launch_entmc(ctx, ns, eps_mode, seed, 0, ns / 2, 0, ctx->d_out);
}

// H (d_out[0] unless on the host) and out = G, varG, var_ss to the host: two small copies, ONE wait
int finish_out(vbmc_ctx* ctx, ElcboRecord* r, bool H_on_host, double H_host, size_t pin_off, double out[7]) {
  double* hp = ctx->h_pinned + pin_off;
  if (!H_on_host) HIP_TRY(ctx, hipMemcpyAsync(hp, ctx->d_out, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(hp + 1, r->sc.ptr(r->p_out), sizeof(double) * 3, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, stream_wait(ctx));
  const double H = H_on_host ? H_host : hp[0], G = hp[1], varG = hp[2], var_ss = hp[3], varH = 0.0;
  out[0] = -G - H;       // nelbo (:1179)
  out[1] = G;
  out[2] = H;
  out[3] = varG + varH;  // varF (:1182-1183)
  out[4] = varG;
  out[5] = varH;
  out[6] = var_ss;
  return 0;
}

int full_queue(vbmc_ctx* ctx, double* theta, int n_theta, int mask, int64_t ns, int eps_mode, uint64_t seed, int compute_var,
               double out[7], double* I_SxK, double* J_SxKxK) {
  const char* who = "elcbo_full";
  if (!ctx->mix_set) return vbmc_fail(ctx, VBMC_E_ARG, "%s: mixture (D,K) not set", who);
  if (!ctx->gp.set) return vbmc_fail(ctx, VBMC_E_ARG, "%s: GP not set", who);
  if (ctx->gp.D != ctx->D) return vbmc_fail(ctx, VBMC_E_ARG, "%s: GP D=%d != mixture D=%d", who, ctx->gp.D, ctx->D);
  const int D = ctx->D, K = ctx->K;
  if (D > kMaxD || K > kMaxK) return vbmc_fail(ctx, VBMC_E_UNSUP, "%s: D=%d, K=%d beyond D <= %d, K <= %d", who, D, K, kMaxD, kMaxK);
  if (compute_var != 0 && compute_var != 1)
    return vbmc_fail(ctx, VBMC_E_UNSUP, "Diagonal approximation of GP log-joint variance not implemented.");
  int rc = entropy_check(ctx, who, ns, eps_mode);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  rc = vbmc_theta_to_mixture(ctx, theta, n_theta, mask, nullptr, nullptr, nullptr, nullptr, nullptr);
  if (rc) return rc;
  if (mask & 8) {  // the reference shifts its caller's theta tail in place (:1082-1085)
    double* e = theta + (n_theta - K);
    double mx = e[0];
    for (int k = 1; k < K; ++k) mx = e[k] > mx ? e[k] : mx;
    for (int k = 0; k < K; ++k) e[k] -= mx;
  }
  const GpState& g = ctx->gp;
  const int S = g.S, N = g.N;
  ElcboRecord* r = record_of(ctx);
  if ((rc = record_reserve(ctx, r, S, K, compute_var != 0))) return rc;
  // scratch of the GP launches, as vbmc_gp_log_joint lists it: res | Z | V | Q
  const size_t n_res = (size_t)S * K * (1 + 2 * D), n_Z = compute_var ? (size_t)S * K * N : 0, n_Q = compute_var ? (size_t)S * K * K : 0;
  const size_t n_I = (size_t)S * K;
  Scratch sc;
  const auto p_res = sc.add(n_res), p_Z = sc.add(n_Z), p_V = sc.add(n_Z), p_Q = sc.add(n_Q);
  if ((rc = reserve(ctx, sc))) return rc;
  if ((rc = ensure_pinned(ctx, 4 + n_I + n_Q))) return rc;
  if ((rc = launch_gp_log_joint(ctx, 0, sc.ptr(p_res), compute_var ? sc.ptr(p_Z) : nullptr))) return rc;
  if ((rc = launch_elcbo_isk(ctx, sc.ptr(p_res), r->sc.ptr(r->p_I)))) return rc;
  if (compute_var) {
    if ((rc = launch_gp_var(ctx, sc.ptr(p_Z), sc.ptr(p_V), sc.ptr(p_Q)))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(r->sc.ptr(r->p_J), sc.ptr(p_Q), sizeof(double) * n_Q, hipMemcpyDeviceToDevice, ctx->stream));
  }
  // the record is complete in stream order: the entropy launches may take the scratch
  bool H_on_host = false;
  double H_host = 0.0;
  if ((rc = entropy_queue(ctx, ns, eps_mode, seed, &H_on_host, &H_host))) return rc;
  mix_from_ctx(ctx, r->cur);
  if ((rc = reweight_queue(ctx, r, r->cur))) return rc;
  double* hp = ctx->h_pinned;
  HIP_TRY(ctx, hipMemcpyAsync(hp + 4, r->sc.ptr(r->p_I), sizeof(double) * n_I, hipMemcpyDeviceToHost, ctx->stream));
  if (compute_var)
    HIP_TRY(ctx, hipMemcpyAsync(hp + 4 + n_I, r->sc.ptr(r->p_J), sizeof(double) * n_Q, hipMemcpyDeviceToHost, ctx->stream));
  if ((rc = finish_out(ctx, r, H_on_host, H_host, 0, out))) return rc;
  if (I_SxK) memcpy(I_SxK, hp + 4, sizeof(double) * n_I);
  if (J_SxKxK && compute_var) memcpy(J_SxKxK, hp + 4 + n_I, sizeof(double) * n_Q);
  r->D = D;
  r->gp_launches0 = ctx->gp_launches;
  r->waits0 = ctx->stream_waits;
  r->valid = true;
  return VBMC_OK;
}

// The K' mixture of a trial (:335-340, then get_parameters, variational_posterior.py:642-676, and set_parameters,
// :720-756, on the raw parameters): delete; w / sum(w); lambd / nl, sigma nl; through log and exp; eta = log w - max,
// w = exp(eta) / sum; lambd / nl, sigma nl once more.
void prune_mixture(const Mix& c, int drop, int D, Mix& t) {
  const int K = c.K - 1;
  t.K = K;
  t.mu.clear();
  t.sigma.clear();
  t.w.clear();
  t.alive.clear();
  for (int k = 0; k < c.K; ++k) {
    if (k == drop) continue;
    t.mu.insert(t.mu.end(), c.mu.begin() + (size_t)k * D, c.mu.begin() + (size_t)(k + 1) * D);
    t.sigma.push_back(c.sigma[k]);
    t.w.push_back(c.w[k]);
    t.alive.push_back(c.alive[k]);
  }
  t.lambd = c.lambd;
  auto renorm = [&]() {
    double q = 0.0;
    for (int d = 0; d < D; ++d) q += t.lambd[d] * t.lambd[d];
    const double nl = std::sqrt(q / D);
    for (int d = 0; d < D; ++d) t.lambd[d] /= nl;
    for (int k = 0; k < K; ++k) t.sigma[k] *= nl;
  };
  renorm();
  double ws = 0.0;
  for (int k = 0; k < K; ++k) ws += t.w[k];
  t.eta.resize(K);
  double mx = -INFINITY;
  for (int k = 0; k < K; ++k) {
    t.eta[k] = std::log(t.w[k] / ws);
    mx = t.eta[k] > mx ? t.eta[k] : mx;
  }
  for (int k = 0; k < K; ++k) t.sigma[k] = std::exp(std::log(t.sigma[k]));
  for (int d = 0; d < D; ++d) t.lambd[d] = std::exp(std::log(t.lambd[d]));
  ws = 0.0;
  for (int k = 0; k < K; ++k) {
    t.eta[k] -= mx;
    t.w[k] = std::exp(t.eta[k]);
    ws += t.w[k];
  }
  for (int k = 0; k < K; ++k) t.w[k] /= ws;
  renorm();
}

int trial_queue(vbmc_ctx* ctx, int drop, int64_t ns, int eps_mode, uint64_t seed, double out[7]) {
  const char* who = "elcbo_prune_trial";
  ElcboRecord* r = (ElcboRecord*)ctx->elcbo;
  if (!r || !r->valid) return vbmc_fail(ctx, VBMC_E_ARG, "%s: no record (vbmc_elcbo_full / vbmc_elcbo_put)", who);
  r->trial_valid = false;
  const Mix& c = r->cur;
  if (drop >= 0 && c.K < 2) return vbmc_fail(ctx, VBMC_E_ARG, "%s: one component left", who);
  if (drop < -1 || drop >= c.K) return vbmc_fail(ctx, VBMC_E_ARG, "%s: drop=%d outside [-1, %d)", who, drop, c.K);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  Mix& t = r->trial;
  if (drop < 0)
    t = c;  // the record's mixture as it is
  else
    prune_mixture(c, drop, r->D, t);
  int rc = set_mixture_host(ctx, r->D, t.K, t.mu.data(), t.sigma.data(), t.lambd.data(), t.w.data(), t.eta.data(), false);
  if (rc) return rc;
  if ((rc = entropy_check(ctx, who, ns, eps_mode))) return rc;
  if ((rc = ensure_pinned(ctx, 4))) return rc;
  bool H_on_host = false;
  double H_host = 0.0;
  if ((rc = entropy_queue(ctx, ns, eps_mode, seed, &H_on_host, &H_host))) return rc;
  if ((rc = reweight_queue(ctx, r, t))) return rc;
  if ((rc = finish_out(ctx, r, H_on_host, H_host, 0, out))) return rc;
  r->trial_valid = true;
  return VBMC_OK;
}

}  // namespace

void elcbo_free(vbmc_ctx* ctx) {
  ElcboRecord* r = (ElcboRecord*)ctx->elcbo;
  if (!r) return;
  if (r->d_buf) (void)hipFree(r->d_buf);
  delete r;
  ctx->elcbo = nullptr;
}

extern "C" int vbmc_elcbo_full(vbmc_ctx* ctx, double* theta, int n_theta, int optimize_mask, int64_t ns_per_comp, int eps_mode,
                               uint64_t seed, int compute_var, double out[7], double* I_SxK, double* J_SxKxK) {
  if (!ctx || !theta || !out) return VBMC_E_ARG;
  NEED_DEVICE(ctx);
  const int rc = full_queue(ctx, theta, n_theta, optimize_mask, ns_per_comp, eps_mode, seed, compute_var, out, I_SxK, J_SxKxK);
  return rc ? search_fail_wait(ctx, rc) : rc;
}

extern "C" int vbmc_elcbo_prune_trial(vbmc_ctx* ctx, int drop, int64_t ns_per_comp, int eps_mode, uint64_t seed, double out[7]) {
  if (!ctx || !out) return VBMC_E_ARG;
  NEED_DEVICE(ctx);
  const int rc = trial_queue(ctx, drop, ns_per_comp, eps_mode, seed, out);
  return rc ? search_fail_wait(ctx, rc) : rc;
}

extern "C" int vbmc_elcbo_prune_accept(vbmc_ctx* ctx) {
  if (!ctx) return VBMC_E_ARG;
  ElcboRecord* r = (ElcboRecord*)ctx->elcbo;
  if (!r || !r->valid || !r->trial_valid) return vbmc_fail(ctx, VBMC_E_ARG, "elcbo_prune_accept: no trial to accept");
  r->cur = r->trial;
  r->trial_valid = false;
  return VBMC_OK;
}

extern "C" int vbmc_elcbo_put(vbmc_ctx* ctx, int S, int K0, const double* I_SxK0, const double* J_SxK0xK0) {
  if (!ctx || !I_SxK0 || S < 1 || K0 < 1) return VBMC_E_ARG;
  NEED_DEVICE(ctx);
  const char* who = "elcbo_put";
  if (!ctx->mix_set || ctx->K != K0) return vbmc_fail(ctx, VBMC_E_ARG, "%s: the context's mixture must hold the K0=%d components", who, K0);
  if (ctx->D > kMaxD || K0 > kMaxK)
    return vbmc_fail(ctx, VBMC_E_UNSUP, "%s: D=%d, K=%d beyond D <= %d, K <= %d", who, ctx->D, K0, kMaxD, kMaxK);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  ElcboRecord* r = record_of(ctx);
  int rc = record_reserve(ctx, r, S, K0, J_SxK0xK0 != nullptr);
  if (rc) return rc;
  const size_t n_I = (size_t)S * K0;
  hipError_t e = hipMemcpyAsync(r->sc.ptr(r->p_I), I_SxK0, sizeof(double) * n_I, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess && J_SxK0xK0)
    e = hipMemcpyAsync(r->sc.ptr(r->p_J), J_SxK0xK0, sizeof(double) * n_I * K0, hipMemcpyHostToDevice, ctx->stream);
  if (e != hipSuccess) return search_fail_wait(ctx, vbmc_fail(ctx, VBMC_E_HIP, "%s: %s", who, hipGetErrorString(e)));
  HIP_TRY(ctx, stream_wait(ctx));  // (the arrays are host memory of this call)
  mix_from_ctx(ctx, r->cur);
  r->D = ctx->D;
  r->gp_launches0 = ctx->gp_launches;
  r->waits0 = ctx->stream_waits;
  r->valid = true;
  return VBMC_OK;
}

extern "C" int vbmc_elcbo_record_info(const vbmc_ctx* ctx, int64_t info[5], int32_t* alive_K0) {
  if (!ctx || !info) return VBMC_E_ARG;
  const ElcboRecord* r = (const ElcboRecord*)ctx->elcbo;
  if (!r || !r->valid) return VBMC_E_ARG;
  info[0] = r->S;
  info[1] = r->K0;
  info[2] = r->cur.K;
  info[3] = (int64_t)(ctx->gp_launches - r->gp_launches0);
  info[4] = (int64_t)(ctx->stream_waits - r->waits0);
  if (alive_K0)
    for (int k = 0; k < r->cur.K; ++k) alive_K0[k] = r->cur.alive[k];
  return VBMC_OK;
}
