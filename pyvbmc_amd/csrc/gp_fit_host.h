// The host side of vbmc_gp_fit (api_gp_fit.hip, gp_fit.hip): the entry's own argument check, the sizes of its stages and
// the arguments of its kernels.  Host C++ with no HIP in it, next to gp_cand_host.h whose check, plan and packing it
// builds on, so that a stand-alone program can run it under a sanitizer (tools/gp_fit_check.cpp).
#pragma once
#include <cmath>
#include <cstdint>

#include "gp_cand_host.h"

// The stages' sizes: B candidates (H rows of hyp0, then init_N drawn), R optimiser runs from the best of them, C slice
// chains, S posterior samples installed (the chains' samples, or the optimum alone).
struct GpFitShape {
  int H = 0, init_N = 0, B = 0, R = 0, C = 0, S = 0;
  int runs = 0;  // slots of the chunk workspace: the largest batch a stage factorises
};
inline GpFitShape gp_fit_shape(int H, int init_N, int opts_N, int n_samples) {
  GpFitShape s;
  s.H = H < 0 ? 0 : H;
  s.init_N = init_N < 0 ? 0 : init_N;
  s.B = s.H + s.init_N;
  s.R = opts_N < 0 ? 0 : opts_N < s.B ? opts_N : s.B;
  s.C = n_samples < 0 ? 0 : n_samples;
  s.S = s.C > 0 ? s.C : 1;
  s.runs = s.B > s.S ? s.B : s.S;
  if (s.runs < 1) s.runs = 1;
  return s;
}

// The entry's own VBMC_E_ARG checks, run by gp_cand_check as its `own` (after N, D and P, before the bounds, the priors
// and every VBMC_E_UNSUP): the counts, the design box inside the hard box, the optimiser's and the sampler's arguments
// where their stage runs.  lb, ub are the hard box; a design box is needed only with init_N > 0.
inline int gp_fit_check_own(WarpArgErr& e, const char* who, int P, int H, const double* hyp0, int init_N, const double* dlb,
                            const double* dub, const double* lb, const double* ub, int opts_N, int max_iter, int m,
                            double tol_g, double tol_f, int n_samples, const double* widths, int thin, int burn_in) {
  if (H < 0 || init_N < 0 || (long long)H + init_N < 1 || (long long)H + init_N > (1 << 20))
    return warp_arg_fail(e, VBMC_E_ARG, "%s: bad H=%d init_N=%d (H + init_N >= 1)", who, H, init_N);
  if (H > 0 && !hyp0) return warp_arg_fail(e, VBMC_E_ARG, "%s: H=%d without hyp0", who, H);
  if (opts_N < 0 || n_samples < 0 || n_samples > (1 << 16))
    return warp_arg_fail(e, VBMC_E_ARG, "%s: bad opts_N=%d n_samples=%d", who, opts_N, n_samples);
  if (init_N > 0) {
    if (!dlb || !dub) return warp_arg_fail(e, VBMC_E_ARG, "%s: init_N=%d without a design box", who, init_N);
    for (int p = 0; p < P; ++p)
      if (!(dlb[p] >= lb[p] && dub[p] <= ub[p] && dlb[p] <= dub[p]))
        return warp_arg_fail(e, VBMC_E_ARG, "%s: design box of parameter %d is not inside [lb, ub] or dlb > dub", who, p);
  }
  if (opts_N > 0 && (max_iter < 0 || max_iter > 1000000 || m < 1 || m > 16 || !(tol_g >= 0.0) || !(tol_f >= 0.0)))
    return warp_arg_fail(e, VBMC_E_ARG, "%s: bad max_iter=%d m=%d tol_g=%g tol_f=%g", who, max_iter, m, tol_g, tol_f);
  if (n_samples > 0) {
    if (thin < 1 || burn_in < 0) return warp_arg_fail(e, VBMC_E_ARG, "%s: bad thin=%d burn_in=%d", who, thin, burn_in);
    if (!widths) return warp_arg_fail(e, VBMC_E_ARG, "%s: n_samples=%d without widths", who, n_samples);
    for (int p = 0; p < P; ++p)
      if (!(widths[p] > 0.0) || !std::isfinite(widths[p]))
        return warp_arg_fail(e, VBMC_E_ARG, "%s: width of parameter %d is not a positive finite number", who, p);
  }
  return 0;
}

// The status word's bits (VBMC_OK comes with them; the installed GP is untouched when one is set)
constexpr int GP_FIT_NO_FINITE = 1;  // no candidate has a finite score

// What gp_fit.hip's kernels read and write, on top of the problem, the box and the prior of GpCandArgs (x0: the H rows
// of hyp0 at the head of the `in` block; behind them dlb, dub, widths, then gp_cand_pack's arrays).  All pointers device
// memory.
struct GpFitArgs : GpCandArgs {
  int H = 0, B = 0, R = 0, C = 0, S = 0;
  uint64_t seed = 0;
  const double *dlb = nullptr, *dub = nullptr;  // [P] the design box
  double* cand = nullptr;                       // [B][P]
  double* score = nullptr;                      // [B]
  int* order = nullptr;                         // [B] candidate indices by score descending, ties to the lower index
  int* starts = nullptr;                        // [R] = order[0 .. R)
  double* opt_x0 = nullptr;                     // [R][P] the optimiser's starts (NaN rows: no finite score)
  const double *opt_hyp = nullptr, *opt_logpost = nullptr;  // [R][P], [R] the optimiser's results
  const int* opt_invalid = nullptr;             // [R]
  double *best = nullptr, *best_logpost = nullptr;  // [P], [1] the optimum
  double* chain_x0 = nullptr;                   // [C][P] the optimum, tiled
  const double* chain_hyp = nullptr;            // [C][P] the chains' kept samples
  const int* chain_invalid = nullptr;           // [C]
  double* hyp = nullptr;                        // [S][P] the samples installed
  double* noise = nullptr;                      // [S] exp(2 h[D + 1]) of each
  int* bad = nullptr;                           // [S] 1: the sample's source was not usable (a placeholder was built)
  int* status = nullptr;                        // [1]
};
