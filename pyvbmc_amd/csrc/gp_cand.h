// What the lockstep drivers over lml + log prior share (gp_hyp.hip's slice chains, gp_opt.hip's quasi-Newton runs): a
// parameter's term of the log prior, and the write of a run's next candidate into slot `slot` of the staged GP, the
// buffers launch_gp_post_build reads (its hyp row, sl, smeta and its N noise variances).  Stated once, so that both
// drivers hand the factorisation the same bits for the same point.
#pragma once
#include <cmath>

#include "fastmath.h"

// t_p of parameter p at h: 0 without a prior (sigma NaN), else with z = (h - mu_p) / sigma_p
//   c_p - 1/2 z^2 (df = +inf) or c_p - (df + 1) / 2 log(1 + z^2 / df);  c_p is the host's (gp_cand_host.h).
// dt (optional): its derivative, -z / sigma or -(df + 1) z / (sigma (df + z^2)).
__device__ __forceinline__ double gp_prior_term(const double* pmu, const double* psig, const double* pdf, const double* pconst,
                                                int p, double h, double* dt = nullptr) {
  const double sg = psig[p];
  double t = 0.0, g = 0.0;
  if (sg == sg) {
    const double z = (h - pmu[p]) / sg, nu = pdf[p];
    t = nu == INFINITY ? pconst[p] - 0.5 * (z * z) : pconst[p] - 0.5 * (nu + 1.0) * fm::log_fast(1.0 + z * z / nu);
    if (dt) g = nu == INFINITY ? -z / sg : -(nu + 1.0) * z / (sg * (nu + z * z));
  }
  if (dt) *dt = g;
  return t;
}

// coordinate p of the candidate xp: a coordinate that is not finite (an invalid start) is replaced by its lower bound, so
// the factorisation of this slot never reads one.  Returns what it wrote.
__device__ __forceinline__ double gp_cand_coord(const double* xp, const double* lb, int p, int slot, int P, double* g_hyp) {
  double h = xp[p];
  if (!(fabs(h) < INFINITY)) h = lb[p];
  g_hyp[(size_t)slot * P + p] = h;
  return h;
}

// the candidate's noise, by a workgroup of T threads: sn2_n = exp(2 h[D + 1]) + s2_n, sl = sn2_div = min_n sn2_n
// (sn2_mult = 1).  Returns exp(2 h[D + 1]) in every thread.
template <int T>
__device__ __forceinline__ double gp_cand_noise(int tid, int slot, int N, int D, const double* xp, const double* lb,
                                                const double* s2, double s2_min, double* g_sn2, double* g_sl,
                                                double* g_smeta) {
  double hn = xp[D + 1];
  if (!(fabs(hn) < INFINITY)) hn = lb[D + 1];
  const double e = exp(2.0 * hn);
  for (int n = tid; n < N; n += T) g_sn2[(size_t)slot * N + n] = s2 ? e + s2[n] : e;
  if (tid == 0) {
    const double sl = e + s2_min;
    g_sl[slot] = sl;
    g_smeta[3 * slot] = 1.0;  // (L_chol, sn2_mult, 1 / sn2_eff)
    g_smeta[3 * slot + 1] = 1.0;
    g_smeta[3 * slot + 2] = 1.0 / sl;
  }
  return e;
}
