// Argument checks of the input-warping entry points (api_warp.hip), host C++ with no HIP in it, so that a stand-alone
// program can run them under a sanitizer (tools/warp_args_check.cpp).  Each returns 0, or the VBMC_E_* code with the
// message in `e`; nothing is dereferenced.
#pragma once
#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/vbmc_hip.h"

struct WarpArgErr {
  int code = 0;
  char msg[192] = {0};
};

inline int warp_arg_fail(WarpArgErr& e, int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(e.msg, sizeof(e.msg), fmt, ap);
  va_end(ap);
  e.code = code;
  return code;
}

inline int warp_check_dim(WarpArgErr& e, const char* who, int D) {
  if (D < 1) return warp_arg_fail(e, VBMC_E_ARG, "%s: D=%d", who, D);
  if (D > 32) return warp_arg_fail(e, VBMC_E_UNSUP, "%s: D=%d > 32 not supported", who, D);
  return 0;
}

inline int warp_check_source(WarpArgErr& e, const char* who, int source) {
  if (source < VBMC_WARP_FROM_OLD || source > VBMC_WARP_IN_NEW)
    return warp_arg_fail(e, VBMC_E_ARG, "%s: source %d (0, 1 or 2)", who, source);
  return 0;
}

inline int warp_check_points(WarpArgErr& e, int D, int64_t n, int source, const double* x, const double* y,
                             const double* lj_new, const double* lj_old) {
  if (warp_check_dim(e, "warp_points", D) || warp_check_source(e, "warp_points", source)) return e.code;
  if (n < 0) return warp_arg_fail(e, VBMC_E_ARG, "warp_points: n=%lld", (long long)n);
  if (n > 0 && !x) return warp_arg_fail(e, VBMC_E_ARG, "warp_points: null points");
  if (n > 0 && !y && !lj_new && !lj_old) return warp_arg_fail(e, VBMC_E_ARG, "warp_points: no output asked for");
  if (lj_old && source != VBMC_WARP_FROM_OLD)
    return warp_arg_fail(e, VBMC_E_ARG, "warp_points: lj_old needs points in the old inference space (source 0)");
  return 0;
}

inline int warp_check_unscent(WarpArgErr& e, int D, int64_t n, const double* x, int64_t sigma_rows, const double* sigma,
                              const double* mean, const double* sd) {
  if (warp_check_dim(e, "warp_unscent", D)) return e.code;
  if (n < 1 || n > 0x7fffffffll) return warp_arg_fail(e, VBMC_E_ARG, "warp_unscent: n=%lld", (long long)n);
  if (sigma_rows != 1 && sigma_rows != n)
    return warp_arg_fail(e, VBMC_E_ARG, "warp_unscent: sigma has %lld rows, x %lld (1 or the same)", (long long)sigma_rows,
                         (long long)n);
  if (!x || !sigma || !mean || !sd) return warp_arg_fail(e, VBMC_E_ARG, "warp_unscent: null array");
  return 0;
}

// (the state: the warped deviations and means of every sample and training point)
inline int warp_check_gp(WarpArgErr& e, int D, int N, int S, int P, const double* X, const double* hyp,
                         const double* logell) {
  if (warp_check_dim(e, "warp_gp", D)) return e.code;
  if (N < 1 || S < 1 || S > 65535 || P < D) return warp_arg_fail(e, VBMC_E_ARG, "warp_gp: N=%d S=%d P=%d (D=%d)", N, S, P, D);
  if (!X || !hyp || !logell) return warp_arg_fail(e, VBMC_E_ARG, "warp_gp: null array");
  if (2.0 * (double)S * (double)N * (double)D > (double)(1 << 27))
    return warp_arg_fail(e, VBMC_E_UNSUP, "warp_gp: S N D = %d x %d x %d: state above 2^27 doubles", S, N, D);
  return 0;
}

inline int warp_check_box(WarpArgErr& e, int D, int64_t n, int source, const double* lo, const double* hi, int mode,
                          const double* out, const double* sorted) {
  if (warp_check_dim(e, "warp_box", D) || warp_check_source(e, "warp_box", source)) return e.code;
  if (n < 1) return warp_arg_fail(e, VBMC_E_ARG, "warp_box: n=%lld", (long long)n);
  if (n > ((int64_t)1 << 30)) return warp_arg_fail(e, VBMC_E_UNSUP, "warp_box: %lld draws > 2^30", (long long)n);
  if (mode != 0 && mode != 1) return warp_arg_fail(e, VBMC_E_ARG, "warp_box: mode %d (0 quantiles, 1 min / max)", mode);
  if (!lo || !hi || !out) return warp_arg_fail(e, VBMC_E_ARG, "warp_box: null array");
  if (sorted && mode != 0) return warp_arg_fail(e, VBMC_E_ARG, "warp_box: the sorted columns exist in quantile mode only");
  return 0;
}
