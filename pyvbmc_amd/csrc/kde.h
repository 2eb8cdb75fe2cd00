// kde.hip's per-column stages (launch_kde) for a caller in another translation unit: vbmc_marginals runs them on the
// columns of its device samples with the bounds its own column kernel left on the device.
#pragma once
#include <cstddef>
#include <cstdint>

#include "scratch.h"

struct vbmc_ctx;

// where kde.hip's plan (KdePlan: the first pieces of the call's scratch list) put what such a caller reads or writes,
// offsets in doubles
struct KdeCols {
  int ncol = 0, nm = 0;
  int64_t pmax = 0;      // keys per column: next_pow2(max(n, 8192))
  size_t o_keys = 0;     // ncol x pmax sorted 64-bit keys
  size_t o_nf = 0;       // ncol unsigned: a column held a non-finite sample
  size_t o_bnd = 0;      // ncol lower bounds, then ncol upper bounds (read by the stages)
  size_t o_dens = 0;     // ncol x nm densities
  size_t o_xm = 0;       // ncol x nm mesh points
  size_t o_colp = 0;     // ncol x colp_stride doubles per column, the bandwidth at colp_bw
  size_t o_ga = 0, o_stat = 0;  // the stages' own: DCT coefficients (ncol x nm), len(np.unique) and flags (ncol x 2 int64)
  int colp_stride = 0, colp_bw = 0;
};

// plan the pieces of kde_1d for ncol columns of n samples on a mesh of nm points (a power of two <= 2^14)
KdeCols kde_cols_plan(Scratch& sc, int ncol, int nm, int64_t n);
// kde_1d of the columns of the device matrix d_x (element (i, c) at d_x[i rs + c cs]) with the bounds at o_bnd
int kde_cols_launch(vbmc_ctx* ctx, const KdeCols& kc, const double* d_x, int64_t n, int64_t rs, int64_t cs, double* base);
