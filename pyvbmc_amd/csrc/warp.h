// Launchers of warp.hip, called by the entry points of api_warp.hip.  All pointers are device memory.
#pragma once
#include "common.h"

// where a warp_points launch takes its input rows from
struct WarpBox {
  int gen = 0;                  // 0: the rows of `in`; 1: box draws from the uniforms `in`; 2: box draws from Philox stream 9
  const double* lo = nullptr;   // [D] the box (gen != 0)
  const double* hi = nullptr;
  uint64_t seed = 0;
};

// y = the rows mapped as `source` says (include/vbmc_hip.h VBMC_WARP_*); lj_new / lj_old nullable
int launch_warp_points(vbmc_ctx* ctx, const XfView& t0, const XfView& t1, int64_t n, int source, const double* in,
                       const WarpBox& box, double* y, double* lj_new, double* lj_old);

// the unscented warp of n base points for S sets of scales: sigma + s * sigma_set_stride is set s, row i of it at
// i * sigma_row_stride (0: one row for all).  mean / sd: [S][n][D] (log_sd: the logarithm of the deviation instead);
// pts [U][n][D] (S = 1), dy / dy_old [n] (written by set 0): nullable.
struct WarpUnscent {
  int64_t n = 0;
  int S = 1;
  const double* x = nullptr;
  const double* sigma = nullptr;
  int64_t sigma_row_stride = 0, sigma_set_stride = 0;
  int log_sd = 0;
  double *mean = nullptr, *sd = nullptr, *pts = nullptr, *dy = nullptr, *dy_old = nullptr;
};
int launch_warp_unscent(vbmc_ctx* ctx, const XfView& t0, const XfView& t1, const WarpUnscent& a);

// out[s][c] = (sum_i a[s][i][c]) / rows, the sum in a fixed order
int launch_warp_row_means(vbmc_ctx* ctx, const double* a, int S, int64_t rows, int cols, double* out);

// per column of y (n x D): mode 1, out[0][c] = min, out[1][c] = max; mode 0, the column sorted through `keys`
// ([D][pmax], pmax = warp_sort_pmax(n)) and out[0][c], out[1][c] = its 0.05 / 0.95 quantiles (np.quantile's linear rule);
// nonfinite [D] flags; sorted [D][n] nullable
int64_t warp_sort_pmax(int64_t n);
int launch_warp_box_stats(vbmc_ctx* ctx, const double* y, int64_t n, int D, int mode, uint64_t* keys, unsigned* nonfinite,
                          double* out, double* sorted);
