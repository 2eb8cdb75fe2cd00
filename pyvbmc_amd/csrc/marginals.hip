// VariationalPosterior.marginals on the device: what the reference's plot gets from corner.corner
// (variational_posterior.py:1191-1206) -- the D one-dimensional and D (D - 1) / 2 two-dimensional histograms of the
// samples -- with the order-statistic quantiles and the highest-density levels of every pair.
//
// Four stages behind the samples (api_marginals.hip draws or uploads them):
//   kde_sort_chunks_kernel  colsort.h: the exact sort's 8192-key chunks, and the non-finite check
//   marg_column_kernel      one workgroup per column: the remaining bitonic stages (colsort.h column_merge), then from
//                           the sorted column its range ([min, max], or the caller's), np.linspace's edges and
//                           np.quantile's linear rule
//   marg_bin_kernel         one pass over the (n, D) doubles: np.histogram's bin of every sample per dimension as one
//                           byte (255 = outside the range) into idx (D x ns, a row per dimension), and the 1-D counts
//                           through integer LDS atomics
//   marg_pair_kernel        the hot path: reads idx only.  A workgroup owns a tile of samples and a group of pairs, one
//                           bins x bins uint32 histogram per pair in LDS; integer LDS atomics, then one integer atomic
//                           per non-empty cell into the global uint64 counts.  No floating-point operation at all.
//   marg_levels_kernel      one workgroup per pair: the cells bitonic-sorted by count (descending) in LDS, a prefix sum
//                           in a fixed order, the count threshold and the mass of every level
// Only integer atomics: the counts do not depend on the launch geometry.  The edge and bin arithmetic is written with
// plain operations (the build uses -ffp-contract=off), so the counts are NumPy's exactly.
//
// LDS plan of the pair kernel: 128 KiB of the CU's 160 KiB hold the histograms of a group, so bins = 128 (64 KiB a
// pair) puts 2 pairs in a group, bins = 40 (6.25 KiB) 20, bins <= 32 at most 32.  A group of consecutive pairs (i, j)
// in row-major order reads row i and a run of rows j of idx: one 4-byte load per row and four samples.  The cell
// address a bins + b is data-dependent, so bank conflicts follow the posterior, not the layout; a wave's 64 lanes
// hold 256 consecutive samples.
#include <cmath>

#include "colsort.h"  // kThreads, kChunk, KdeSrc, the keys, kde_sort_chunks_kernel, column_merge
#include "common.h"
#include "marginals.h"

namespace {

constexpr int kBinThreads = 256;
constexpr int kBinRows = 256;          // samples per tile of the bin kernel (= kMargIdxAlign)
constexpr int kPairThreads = 512;
constexpr int kPairTile = 16384;       // samples per workgroup of the pair kernel
constexpr int kPairLds = 128 * 1024;   // bytes of histograms per workgroup
constexpr int kPairMaxGroup = 32;
constexpr int kLevThreads = 512;
static_assert(kBinRows == kMargIdxAlign && kPairTile % kMargIdxAlign == 0, "idx rows are whole tiles");

__device__ inline bool any_nonfinite(const unsigned* nf, int D) {
  unsigned b = 0;
  for (int d = 0; d < D; ++d) b |= nf[d];
  return b != 0;
}

// np.linspace(lo, hi, bins + 1)[i]: i * step + lo, the last point = hi; (i / bins) * delta + lo when the step underflows
__device__ inline double edge_at(int i, double lo, double hi, double delta, double step, int bins) {
  if (i == bins) return hi;
  return (step == 0.0 ? ((double)i / (double)bins) * delta : (double)i * step) + lo;
}

// np.histogram's bin of v (bins, range=(lo, hi)): the scaled position, then corrected against the neighbouring edges;
// v == hi goes into the last bin; outside (and NaN) -> kMargOutside
__device__ inline int bin_of(double v, double lo, double hi, double delta, double step, int bins) {
  if (!(v >= lo && v <= hi)) return kMargOutside;
  const double f = ((v - lo) / delta) * (double)bins;
  int i = (f >= 0.0 && f < (double)bins) ? (int)f : (f >= (double)bins ? bins - 1 : 0);
  while (i > 0 && v < edge_at(i, lo, hi, delta, step, bins)) --i;
  while (i < bins - 1 && v >= edge_at(i + 1, lo, hi, delta, step, bins)) ++i;
  return i;
}

__global__ __launch_bounds__(kThreads) void marg_column_kernel(MargArgs A) {
  __shared__ uint64_t sk[kChunk];
  const int c = blockIdx.x, tid = threadIdx.x;
  const int64_t n = A.n;
  uint64_t* gk = A.keys + (int64_t)c * A.pmax;
  if (A.nonfinite[c]) return;  // (the call fails; nothing of this column is read)
  column_merge(gk, A.pmax, sk);
  const double vmin = from_key(gk[0]), vmax = from_key(gk[n - 1]);
  double lo = A.ranges[2 * c], hi = A.ranges[2 * c + 1];
  if (lo != lo) {
    // the column's own range; np.histogram's rule for an empty one
    lo = vmin;
    hi = vmax;
    if (lo == hi) {
      lo = lo - 0.5;
      hi = hi + 0.5;
    }
  }
  const double delta = hi - lo;
  const double step = delta / (double)A.bins;
  if (tid == 0) {
    double* ci = A.colinfo + 4 * c;
    ci[0] = lo;
    ci[1] = hi;
    ci[2] = delta;
    ci[3] = step;
    A.kde_lb[c] = lo;
    A.kde_ub[c] = hi;
  }
  for (int i = tid; i <= A.bins; i += kThreads) A.edges[(int64_t)c * (A.bins + 1) + i] = edge_at(i, lo, hi, delta, step, A.bins);
  // np.quantile(method="linear"): virtual index (n - 1) q, _lerp of its neighbours
  for (int w = tid; w < A.nq; w += kThreads) {
    const double vi = (double)(n - 1) * A.q[w];
    const double pf = floor(vi);
    int64_t ip = (int64_t)pf, inx = ip + 1;
    if (vi >= (double)(n - 1)) ip = inx = n - 1;
    if (ip < 0) ip = 0;
    if (inx > n - 1) inx = n - 1;
    const double g = vi - pf;
    const double va = from_key(gk[ip]), vb = from_key(gk[inx]);
    const double d = vb - va;
    A.quant[(int64_t)w * A.D + c] = g >= 0.5 ? vb - d * (1.0 - g) : va + d * g;
  }
}

// grid: tiles of kBinRows samples, strided.  LDS: the 1-D counts (D x bins), the tile's codes (D x kBinRows bytes)
__global__ __launch_bounds__(kBinThreads) void marg_bin_kernel(MargArgs A) {
  __shared__ unsigned cnt[kMargMaxD * kMargMaxBins];
  __shared__ __attribute__((aligned(4))) unsigned char tile[kMargMaxD][kBinRows];
  __shared__ double ci[kMargMaxD * 4];
  const int tid = threadIdx.x;
  const int D = A.D, bins = A.bins;
  if (any_nonfinite(A.nonfinite, D)) return;
  for (int e = tid; e < D * bins; e += kBinThreads) cnt[e] = 0u;
  for (int e = tid; e < 4 * D; e += kBinThreads) ci[e] = A.colinfo[e];
  __syncthreads();
  const int64_t ntiles = A.ns / kBinRows;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t s0 = t * kBinRows;
    for (int e = tid; e < kBinRows * D; e += kBinThreads) {
      const int sl = e / D, d = e - sl * D;
      const int64_t s = s0 + sl;
      int code = kMargOutside;  // the padding behind sample n - 1
      if (s < A.n) {
        const double* q = ci + 4 * d;
        code = bin_of(A.x[s * D + d], q[0], q[1], q[2], q[3], bins);
        if (code != kMargOutside) atomicAdd(&cnt[d * bins + code], 1u);
      }
      tile[d][sl] = (unsigned char)code;
    }
    __syncthreads();
    for (int e = tid; e < (kBinRows / 4) * D; e += kBinThreads) {
      const int d = e / (kBinRows / 4), w = e - d * (kBinRows / 4);
      ((unsigned*)(A.idx + (int64_t)d * A.ns + s0))[w] = ((const unsigned*)tile[d])[w];
    }
    __syncthreads();
  }
  for (int e = tid; e < D * bins; e += kBinThreads)
    if (cnt[e]) atomicAdd(&A.counts1[e], (unsigned long long)cnt[e]);
}

// grid (tiles of kPairTile samples, pair groups of G); dynamic LDS: G x bins x bins uint32
__global__ __launch_bounds__(kPairThreads) void marg_pair_kernel(const unsigned char* __restrict__ idx, int64_t ns, int D,
                                                                 int bins, int P, int G,
                                                                 const unsigned* __restrict__ nonfinite,
                                                                 unsigned long long* __restrict__ counts2) {
  extern __shared__ unsigned hist[];
  const int tid = threadIdx.x;
  if (any_nonfinite(nonfinite, D)) return;
  const int p0 = blockIdx.y * G;
  const int g = P - p0 < G ? P - p0 : G;
  const int cells = bins * bins;
  for (int e = tid; e < g * cells; e += kPairThreads) hist[e] = 0u;
  // the first pair (i0, j0) of the group: pair p of row-major order i < j
  int i0 = 0, rem = p0;
  while (i0 < D - 2 && rem >= D - 1 - i0) {
    rem -= D - 1 - i0;
    ++i0;
  }
  const int j0 = i0 + 1 + rem;
  __syncthreads();
  const int64_t nw = ns / 4;
  const int64_t w0 = (int64_t)blockIdx.x * (kPairTile / 4);
  const int64_t w1 = w0 + kPairTile / 4 < nw ? w0 + kPairTile / 4 : nw;
  for (int64_t w = w0 + tid; w < w1; w += kPairThreads) {
    int i = i0, j = j0;
    unsigned wi = ((const unsigned*)(idx + (int64_t)i * ns))[w];
    for (int q = 0; q < g; ++q) {
      const unsigned wj = ((const unsigned*)(idx + (int64_t)j * ns))[w];
      unsigned* h = hist + q * cells;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const unsigned a = (wi >> (8 * b)) & 255u, c = (wj >> (8 * b)) & 255u;
        if (!((a | c) & 0x80u)) atomicAdd(&h[a * bins + c], 1u);  // (a bin index is < 128, "outside" is 255)
      }
      if (++j == D && q + 1 < g) {
        ++i;
        j = i + 1;
        wi = ((const unsigned*)(idx + (int64_t)i * ns))[w];
      }
    }
  }
  __syncthreads();
  unsigned long long* out = counts2 + (int64_t)p0 * cells;
  for (int e = tid; e < g * cells; e += kPairThreads)
    if (hist[e]) atomicAdd(&out[e], (unsigned long long)hist[e]);
}

// grid P; dynamic LDS: next_pow2(bins x bins) uint32
__global__ __launch_bounds__(kLevThreads) void marg_levels_kernel(MargArgs A) {
  extern __shared__ unsigned sc[];
  __shared__ unsigned long long part[kLevThreads];
  __shared__ unsigned long long acc;
  __shared__ int kfirst;
  const int tid = threadIdx.x, p = blockIdx.x;
  if (any_nonfinite(A.nonfinite, A.D)) return;
  const int cells = A.bins * A.bins;
  const int M = (int)next_pow2(cells < 2 ? 2 : cells);
  const unsigned long long* cnt = A.counts2 + (int64_t)p * cells;
  for (int i = tid; i < M; i += kLevThreads) sc[i] = i < cells ? (unsigned)cnt[i] : 0u;  // (a count is <= n < 2^32)
  __syncthreads();
  for (int k = 2; k <= M; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < M / 2; i += kLevThreads) {
        const int lo = (int)pair_lo(i, j);
        const unsigned a = sc[lo], b = sc[lo + j];
        if ((a < b) == ((lo & k) == 0)) {  // descending
          sc[lo] = b;
          sc[lo + j] = a;
        }
      }
      __syncthreads();
    }
  // prefix sums: thread t owns the cells [t per, (t + 1) per); the partial sums are scanned in order by one thread
  const int per = (M + kLevThreads - 1) / kLevThreads;
  const int r0 = tid * per < M ? tid * per : M, r1 = r0 + per < M ? r0 + per : M;
  unsigned long long own = 0;
  for (int i = r0; i < r1; ++i) own += sc[i];
  part[tid] = own;
  __syncthreads();
  if (tid == 0) {
    unsigned long long run = 0;
    for (int t = 0; t < kLevThreads; ++t) {
      const unsigned long long v = part[t];
      part[t] = run;  // exclusive
      run += v;
    }
    acc = run;
  }
  __syncthreads();
  const unsigned long long total = acc;
  const unsigned long long before = part[tid];
  if (tid == 0) A.inside2[p] = total;
  for (int l = 0; l < A.nl; ++l) {
    __syncthreads();
    if (tid == 0) {
      kfirst = M - 1;
      acc = 0;
    }
    __syncthreads();
    // the shortest non-empty prefix whose sum is >= level * inside
    const double target = A.levels[l] * (double)total;
    unsigned long long cum = before;
    for (int i = r0; i < r1; ++i) {
      cum += sc[i];
      if ((double)cum >= target) {
        atomicMin(&kfirst, i);
        break;
      }
    }
    __syncthreads();
    const unsigned thr = sc[kfirst];
    unsigned long long mass = 0;
    for (int i = r0; i < r1; ++i) mass += sc[i] >= thr ? sc[i] : 0u;
    if (mass) atomicAdd(&acc, mass);
    __syncthreads();
    if (tid == 0) {
      A.level_counts[(int64_t)p * A.nl + l] = (long long)thr;
      A.level_mass[(int64_t)p * A.nl + l] = total ? (double)acc / (double)total : NAN;
    }
  }
}

}  // namespace

int marg_pairs_per_group(int bins, int P) {
  int g = kPairLds / (bins * bins * (int)sizeof(unsigned));
  g = g > kPairMaxGroup ? kPairMaxGroup : g;
  g = g > P ? P : g;
  return g < 1 ? 1 : g;
}

int launch_marg_sort(vbmc_ctx* ctx, const MargArgs& A) {
  KdeSrc src = {};
  src.x[0] = src.x[1] = A.x;
  src.n[0] = src.n[1] = A.n;
  src.rs[0] = src.rs[1] = A.D;
  src.cs[0] = src.cs[1] = 1;
  src.ncol0 = A.D;
  HIP_TRY(ctx, hipMemsetAsync(A.nonfinite, 0, sizeof(unsigned) * A.D, ctx->stream));
  hipLaunchKernelGGL(kde_sort_chunks_kernel, dim3((unsigned)(A.pmax / kChunk), (unsigned)A.D), dim3(kThreads), 0,
                     ctx->stream, src, A.keys, A.pmax, A.nonfinite);
  HIP_TRY(ctx, hipGetLastError());
  hipLaunchKernelGGL(marg_column_kernel, dim3((unsigned)A.D), dim3(kThreads), 0, ctx->stream, A);
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

int launch_marg_bins(vbmc_ctx* ctx, const MargArgs& A) {
  HIP_TRY(ctx, hipMemsetAsync(A.counts1, 0, sizeof(unsigned long long) * A.D * A.bins, ctx->stream));
  const int64_t ntiles = A.ns / kBinRows;
  // several tiles a workgroup, so that the merge of its counts is paid once for them
  const int64_t grid = ntiles < 2048 ? ntiles : 2048;
  hipLaunchKernelGGL(marg_bin_kernel, dim3((unsigned)grid), dim3(kBinThreads), 0, ctx->stream, A);
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

int launch_marg_pairs(vbmc_ctx* ctx, const MargArgs& A) {
  if (A.P == 0) return 0;
  const size_t cells = (size_t)A.bins * A.bins;
  HIP_TRY(ctx, hipMemsetAsync(A.counts2, 0, sizeof(unsigned long long) * A.P * cells, ctx->stream));
  const int G = marg_pairs_per_group(A.bins, A.P);
  const size_t lds = (size_t)G * cells * sizeof(unsigned);
  HIP_TRY(ctx, hipFuncSetAttribute((const void*)marg_pair_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const dim3 grid((unsigned)((A.ns + kPairTile - 1) / kPairTile), (unsigned)((A.P + G - 1) / G));
  hipLaunchKernelGGL(marg_pair_kernel, grid, dim3(kPairThreads), lds, ctx->stream, A.idx, A.ns, A.D, A.bins, A.P, G,
                     A.nonfinite, A.counts2);
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

int launch_marg_levels(vbmc_ctx* ctx, const MargArgs& A) {
  if (A.P == 0) return 0;
  const int cells = A.bins * A.bins;
  const size_t lds = (size_t)next_pow2(cells < 2 ? 2 : cells) * sizeof(unsigned);
  HIP_TRY(ctx, hipFuncSetAttribute((const void*)marg_levels_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(marg_levels_kernel, dim3((unsigned)A.P), dim3(kLevThreads), lds, ctx->stream, A);
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}
