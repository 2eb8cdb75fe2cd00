// The device stages of vbmc_marginals (marginals.hip), launched by api_marginals.hip.
#pragma once
#include <cstdint>

struct vbmc_ctx;

constexpr int kMargMaxD = 32;
constexpr int kMargMaxBins = 128;              // a bin index and the code "outside" fit a byte
constexpr int64_t kMargMaxN = (int64_t)1 << 22;  // samples: the whole-column stage of the sort is one workgroup a column
constexpr int kMargOutside = 255;              // idx code of a sample outside its dimension's range
constexpr int kMargIdxAlign = 256;             // ns, the row length of idx, is a multiple of this (padding = outside)

// every pointer is device memory
struct MargArgs {
  const double* x;   // n x D samples, row-major
  int64_t n, ns;
  int D, bins, P, nq, nl;
  uint64_t* keys;    // D x pmax: the sorted columns as order-preserving keys
  int64_t pmax;
  unsigned* nonfinite;   // D: set by the sort where a column holds a non-finite sample; every later stage then does nothing
  const double* ranges;  // D x 2: (lo, hi), or (NaN, NaN) for the column's own [min, max]
  const double* q;       // nq quantile levels
  const double* levels;  // nl mass levels
  double* colinfo;       // D x 4: lo, hi, hi - lo, step
  double* kde_lb;        // D, D: the ranges again, where the kde stages read their bounds
  double* kde_ub;
  unsigned char* idx;    // D x ns
  double* edges;         // D x (bins + 1)
  double* quant;         // nq x D
  unsigned long long* counts1;  // D x bins
  unsigned long long* counts2;  // P x bins x bins
  unsigned long long* inside2;  // P
  long long* level_counts;      // P x nl
  double* level_mass;           // P x nl
};

// pairs whose histograms share one workgroup's LDS, and with it the number of pair groups ceil(P / that)
int marg_pairs_per_group(int bins, int P);
int launch_marg_sort(vbmc_ctx* ctx, const MargArgs& A);    // sorted columns -> ranges, edges, quantiles
int launch_marg_bins(vbmc_ctx* ctx, const MargArgs& A);    // idx and counts1
int launch_marg_pairs(vbmc_ctx* ctx, const MargArgs& A);   // counts2
int launch_marg_levels(vbmc_ctx* ctx, const MargArgs& A);  // inside2, level_counts, level_mass
