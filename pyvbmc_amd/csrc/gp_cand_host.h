// The host side of a batch of GP hyper-parameter candidates, stated once for vbmc_gp_lml and the two lockstep entries
// over lml + log prior (vbmc_gp_hyp_sample, vbmc_gp_hyp_optimize): the chunk plan, the argument check, the workspace of
// a chunk, and the base of the advance kernels' arguments with the packing of its `in` block.  Host C++ with no HIP in it
// (as warp_args.h, whose error record it uses), so that a stand-alone program can run it under a sanitizer
// (tools/gp_cand_check.cpp).  The parts that launch or copy are api_gp_lml.hip's (declared in common.h).
#pragma once
#include <cmath>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "scratch.h"
#include "warp_args.h"

// the per-sample flags at the head of a build's or an append's workspace (ctx->d_post_ws): S ints and a spare double
inline Piece<int> gp_post_flags(Scratch& sc, int S) {
  const Piece<int> p = sc.add<int>((size_t)S);
  sc.add(1);
  return p;
}
// The chunk plan: the candidates factorised side by side.  A candidate's factor state is L, L^-1 (N^2 each), the padded
// copy of L^-1 (ld^2), the inverted diagonal blocks (nb 64^2) and the gradient's tile partials (nb (nb + 1) / 2 tile pairs
// of D + 2 sums); the chunk is the largest whose state stays under cap_bytes, at most B, or `forced` (> 0) where that is
// smaller.  0: not even one candidate fits.
constexpr size_t GP_LML_CAP_BYTES = (size_t)1 << 30;
inline size_t gp_lml_part_elems(int N, int D) {
  const size_t nb = ((size_t)N + 63) / 64;
  return nb * (nb + 1) / 2 * ((size_t)D + 2);
}
inline int gp_lml_plan(int N, int D, int B, size_t cap_bytes, int forced) {
  const size_t nn = (size_t)N * N, ld = (size_t)(((size_t)N + 63) / 64 * 64), nb = ld / 64;
  const size_t per = sizeof(double) * (2 * nn + ld * ld + nb * 64 * 64 + gp_lml_part_elems(N, D));
  size_t chunk = cap_bytes / per;
  if (chunk > (size_t)B) chunk = (size_t)B;
  if (forced > 0 && (size_t)forced < chunk) chunk = (size_t)forced;
  return (int)chunk;
}

// The checks the three entries share, every VBMC_E_ARG one before every VBMC_E_UNSUP one: N, D and the number of runs
// (`runs_name`: the letter the entry calls it by), P against the mean kind, then `own` -- the entry's E_ARG checks of
// its other arguments, own(e) -> code -- the bounds, the prior triples, s2, D > 32, a noise bound that allows
// sn2_div < 1e-6 and the chunk plan.  lb null (vbmc_gp_lml: no box, no prior): those checks are skipped; s2 nullable.
struct GpCandPlan {
  int mean_n = 0, chunk = 0;
  double s2_min = 0.0;  // min_n s2_n (0 without user noise)
};
template <class Own>
int gp_cand_check(WarpArgErr& e, const char* who, char runs_name, int N, int D, int runs, int P, int mean_kind,
                  const double* lb, const double* ub, const double* pmu, const double* psig, const double* pdf,
                  const double* s2, int forced_chunk, Own own, GpCandPlan& o) {
  if (N < 1 || D < 1 || runs < 1) return warp_arg_fail(e, VBMC_E_ARG, "%s: bad N=%d D=%d %c=%d", who, N, D, runs_name, runs);
  o.mean_n = mean_kind == VBMC_MEAN_ZERO ? 0 : mean_kind == VBMC_MEAN_CONST ? 1 : 1 + 2 * D;
  if (mean_kind < 0 || mean_kind > 2 || P != D + 2 + o.mean_n)
    return warp_arg_fail(e, VBMC_E_ARG, "%s: P=%d does not match D+2+mean(%d)=%d", who, P, mean_kind, D + 2 + o.mean_n);
  if (own(e)) return e.code;
  for (int p = 0; lb && p < P; ++p) {
    if (!std::isfinite(lb[p]) || !std::isfinite(ub[p]) || lb[p] > ub[p])
      return warp_arg_fail(e, VBMC_E_ARG, "%s: bounds of parameter %d are not finite or lb > ub", who, p);
    if (psig[p] == psig[p] && (!(psig[p] > 0.0) || !std::isfinite(psig[p]) || !std::isfinite(pmu[p]) || !(pdf[p] > 0.0)))
      return warp_arg_fail(e, VBMC_E_ARG, "%s: prior of parameter %d needs finite mu, sigma > 0 and df > 0 (or +inf)", who, p);
  }
  o.s2_min = s2 ? s2[0] : 0.0;
  for (int i = 0; s2 && i < N; ++i) {
    if (!(s2[i] >= 0.0) || !std::isfinite(s2[i]))
      return warp_arg_fail(e, VBMC_E_ARG, "%s: s2[%d] is not a finite number >= 0", who, i);
    if (s2[i] < o.s2_min) o.s2_min = s2[i];
  }
  if (D > 32) return warp_arg_fail(e, VBMC_E_UNSUP, "%s: D=%d > 32 not supported", who, D);
  if (lb && !(std::exp(2.0 * lb[D + 1]) + o.s2_min >= 1e-6))
    return warp_arg_fail(e, VBMC_E_UNSUP, "%s: the noise bound allows sn2_div < 1e-6: the non-Cholesky branch is computed on the host", who);
  o.chunk = gp_lml_plan(N, D, runs, GP_LML_CAP_BYTES, forced_chunk);
  if (o.chunk < 1)
    return warp_arg_fail(e, VBMC_E_UNSUP, "%s: the factor state of one candidate of N=%d points exceeds %zu bytes", who, N,
                         GP_LML_CAP_BYTES);
  return 0;
}

// The workspace of a chunk, listed once: what launch_gp_post_build and launch_gp_lml use for `chunk` candidates side by
// side, and the per-run pieces (the flags, lml, dlml) for `slots` runs -- vbmc_gp_lml has chunk slots, the lockstep
// entries all their runs.  [flag.off, clear_end): what a lockstep entry zeroes before its first round -- flags | sums
// [chunk][2] | dsn2 [chunk] | lml [slots] | dlml [slots][P] -- then Dinv [chunk][nb][64 x 64] | part | mg (want_grad).
struct GpLmlWs {
  int P = 0, want_grad = 0;
  Piece<int> flag;
  Piece<> sums, dsn2, lml, dlml, Dinv, part, mg;
  size_t clear_end = 0;
};
inline GpLmlWs gp_lml_ws(Scratch& sc, int N, int D, int P, int mean_n, int chunk, int slots, int want_grad) {
  const size_t c = (size_t)chunk, g = want_grad ? 1 : 0, nb = ((size_t)N + 63) / 64;
  GpLmlWs w;
  w.P = P;
  w.want_grad = (int)g;
  w.flag = gp_post_flags(sc, slots);
  w.sums = sc.add(2 * c);
  w.dsn2 = sc.add(c);
  w.lml = sc.add((size_t)slots);
  w.dlml = sc.add(g * (size_t)slots * P);
  w.clear_end = sc.total;
  w.Dinv = sc.add(c * nb * 64 * 64);
  w.part = sc.add(g * c * gp_lml_part_elems(N, D));
  w.mg = sc.add(g * c * (size_t)mean_n);
  return w;
}

// What the advance kernels of the lockstep entries share (gp_hyp.hip, gp_opt.hip; gp_cand.h is the device side): the
// problem, the prior, the round before's results and the staged GP's buffers.  All pointers device memory.
struct GpCandArgs {
  int N = 0, D = 0, P = 0;
  double s2_min = 0.0;          // min_n s2_n (0 without user noise)
  const double* s2 = nullptr;   // [N] user-provided noise variances, or null
  const double *x0 = nullptr, *lb = nullptr, *ub = nullptr;  // [runs][P], [P], [P]
  // the prior per parameter: location, scale (NaN: none), degrees of freedom (+inf: Gaussian), the constant part of t_p
  const double *pmu = nullptr, *psig = nullptr, *pdf = nullptr, *pconst = nullptr;
  const double* lml = nullptr;  // [runs] the value the round before produced
  int* flag = nullptr;          // [runs] its factorisation flags: read, then cleared for the next build
  double* state = nullptr;      // [runs][the entry's state elements], zeroed: a zeroed state is a run at its start
  long long* stats = nullptr;   // [runs][4]
  int* invalid = nullptr;       // [runs]
  double *g_hyp = nullptr, *g_sl = nullptr, *g_smeta = nullptr, *g_sn2 = nullptr;  // the staged GP's [S][P], [S], [S][3], [S][N]
};

// the constant part of a parameter's prior term (gp_cand.h): everything of t_p that does not depend on h_p
inline double gp_prior_const(double sigma, double df) {
  if (sigma != sigma) return 0.0;
  if (std::isinf(df)) return -0.5 * std::log(2.0 * M_PI) - std::log(sigma);
  return std::lgamma(0.5 * (df + 1.0)) - std::lgamma(0.5 * df) - 0.5 * std::log(M_PI * df) - std::log(sigma);
}

// The `in` block of a lockstep entry, one upload: x0 [runs][P] | the entry's own [P] arrays (`lead`: the slice widths) |
// lb ub mu sigma df const [P] each | s2 [N] (where given).  Packs it and points a's fields at its copy at d_in; the
// first of `lead` lies at a.x0 + runs P.  a.N and a.P are set by the caller.
inline size_t gp_cand_in_elems(int runs, int P, size_t n_lead, int N, bool has_s2) {
  return ((size_t)runs + n_lead + 6) * P + (has_s2 ? (size_t)N : 0);
}
inline std::vector<double> gp_cand_pack(GpCandArgs& a, const double* d_in, int runs, const double* x0,
                                        std::initializer_list<const double*> lead, const double* lb, const double* ub,
                                        const double* pmu, const double* psig, const double* pdf, const double* s2) {
  const size_t P = (size_t)a.P;
  std::vector<double> in(gp_cand_in_elems(runs, a.P, lead.size(), a.N, s2 != nullptr));
  double* q = in.data();
  auto put = [&q](const double* src, size_t n) {
    memcpy(q, src, sizeof(double) * n);
    q += n;
  };
  put(x0, (size_t)runs * P);
  for (const double* l : lead) put(l, P);
  a.x0 = d_in;
  a.lb = d_in + (q - in.data());
  a.ub = a.lb + P; a.pmu = a.ub + P; a.psig = a.pmu + P; a.pdf = a.psig + P; a.pconst = a.pdf + P;
  a.s2 = s2 ? a.pconst + P : nullptr;
  for (const double* src : {lb, ub, pmu, psig, pdf}) put(src, P);
  for (size_t p = 0; p < P; ++p) q[p] = gp_prior_const(psig[p], pdf[p]);
  q += P;
  if (s2) put(s2, (size_t)a.N);
  return in;
}
