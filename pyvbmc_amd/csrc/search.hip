// The kernels of active_sample's acquisition search (vbmc/active_sample.py:310-349, 647-837): the resident set of
// search points is filled, rounded, scored, masked and ranked without leaving the device (api_search.hip drives them).
//
//   search_fill_kernel     one thread per row of the set.  Rows of the affine-Gaussian sources (:736-738, :782-784:
//                          np.random.multivariate_normal's  z A + mean) and of the box-normal source (:806-809) are drawn
//                          here from Philox stream 7 (the streams are listed in sample.hip): row r of a source is
//                          counter (r_lo, r_hi, pair, 7) under the source's own key, so it depends on (sub-seed, r) only.
//                          Rows of the other sources were written by the launches before (copies, the transformer, the
//                          mixture sampler) and are only read back.  Every row is then clamped to the search bounds
//                          (:836) and, with integer variables, rounded in original space (AbstractAcqFcn._real2int,
//                          abstract_acq_fcn.py:149-193).
//   search_mask_kernel     +inf where the inverse-transformed point leaves the hard bounds (abstract_acq_fcn.py:133-139)
//   search_scale / colsum / centre / take   the operands of _estimate_observation_noise's nearest-neighbour lookup
//                          (:224-256) around gp.hip's sq_dist argmin
//   search_sort_*          (key, row) pairs -- the order-preserving 64-bit key of kde.hip, NaN after +inf, -0 as +0 --
//                          bitonic-sorted: chunks of 8192 pairs in one workgroup's LDS (96 KiB), strides of 8192 and more
//                          as global passes.  The pairs are distinct, so the result is the stable order np.argsort gives.
//   search_gather_kernel   the rows of the set in that order
// No atomics anywhere: a call with a fixed seed is bit-reproducible.
#include <cmath>
#include <cstring>

#include "common.h"
#include "fastmath.h"
#include "mixture_dev.h"
#include "transform.h"

namespace {

constexpr double kRealMax = 1.7976931348623157e+308;
constexpr int kSortThreads = 512;
constexpr int kSortChunk = 8192;  // pairs per LDS chunk: 64 KiB of keys + 32 KiB of rows
constexpr uint32_t kStream = 7u;  // Philox stream of the affine-Gaussian and box-normal sources

struct FillArgs {
  double* X;
  int64_t M;
  int D, n_src;
  const SearchSrcDev* src;
  const double* par;
  const double *lb, *ub;  // null: no clamp
  uint32_t int_bits;
  int has_xf;
  XfView t;
};

template <int DP>
__global__ __launch_bounds__(256) void search_fill_kernel(FillArgs a) {
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= a.M) return;
  const int D = a.D;
  int s = 0;
  while (s + 1 < a.n_src && n >= a.src[s + 1].begin) ++s;
  const SearchSrcDev src = a.src[s];
  double x[DP];
  if (src.kind == VBMC_SRC_AFFINE || src.kind == VBMC_SRC_BOX) {
    const uint64_t r = (uint64_t)(n - src.begin);
    double z[DP];
#pragma unroll
    for (int p = 0; 2 * p < DP; ++p) {
      double z0 = 0.0, z1 = 0.0;
      if (2 * p < D) philox_normal_pair(philox_block(r, (uint32_t)p, kStream, src.seed), z0, z1);
      z[2 * p] = z0;
      if (2 * p + 1 < DP) z[2 * p + 1] = z1;
    }
    const double* par = a.par + src.par;
    if (src.kind == VBMC_SRC_AFFINE) {
      // np.dot(z, A) in row order, then += mean (numpy/random/mtrand.pyx multivariate_normal)
      const double *mean = par, *A = par + D;
#pragma unroll
      for (int j = 0; j < DP; ++j) {
        double acc = 0.0;
        if (j < D)
#pragma unroll
          for (int i = 0; i < DP; ++i)
            if (i < D) acc = acc + z[i] * A[i * D + j];
        x[j] = (j < D) ? acc + mean[j] : 0.0;
      }
    } else {
      const double *lb = par, *ub = par + D;
#pragma unroll
      for (int d = 0; d < DP; ++d) x[d] = (d < D) ? z[d] * (ub[d] - lb[d]) + lb[d] : 0.0;
    }
  } else {
#pragma unroll
    for (int d = 0; d < DP; ++d) x[d] = (d < D) ? a.X[n * D + d] : 0.0;
  }
  if (a.lb)
#pragma unroll
    for (int d = 0; d < DP; ++d)
      if (d < D) {  // np.minimum(np.maximum(x, lb), ub): NaN stays NaN
        x[d] = (x[d] < a.lb[d]) ? a.lb[d] : x[d];
        x[d] = (x[d] > a.ub[d]) ? a.ub[d] : x[d];
      }
  if (a.int_bits) {
    double v[DP];
#pragma unroll
    for (int d = 0; d < DP; ++d) v[d] = x[d];
    if (a.has_xf) xf_inverse<DP>(a.t, v);
#pragma unroll
    for (int d = 0; d < DP; ++d)
      if ((a.int_bits >> d) & 1u) v[d] = rint(v[d]);  // half to even, as np.around
    if (a.has_xf) xf_forward<DP>(a.t, v);
#pragma unroll
    for (int d = 0; d < DP; ++d)
      if ((a.int_bits >> d) & 1u) x[d] = v[d];
  }
#pragma unroll
  for (int d = 0; d < DP; ++d)
    if (d < D) a.X[n * D + d] = x[d];
}

template <int DP>
__global__ __launch_bounds__(256) void search_mask_kernel(const double* __restrict__ X, int64_t M, int D, int has_xf, XfView t,
                                                          const double* __restrict__ lb, const double* __restrict__ ub,
                                                          double* __restrict__ acq) {
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= M) return;
  double v[DP];
#pragma unroll
  for (int d = 0; d < DP; ++d) v[d] = (d < D) ? X[n * D + d] : 0.0;
  if (has_xf) xf_inverse<DP>(t, v);
  bool out = false;
#pragma unroll
  for (int d = 0; d < DP; ++d)
    if (d < D) out = out || (v[d] < lb[d]) || (v[d] > ub[d]);
  if (out) acq[n] = INFINITY;
}

__global__ __launch_bounds__(256) void search_scale_kernel(const double* __restrict__ X, int64_t n_elem, int D,
                                                           const double* __restrict__ ell, double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_elem) return;
  out[e] = X[e] / ell[e % D];
}

// part[block][d] = sum of column d over the block's rows: thread (r, d) = (tid / 32, tid % 32) walks rows r, r + 8 g, ...
// (g = blocks), the eight row lanes are added in order
__global__ __launch_bounds__(256) void search_colsum_kernel(const double* __restrict__ x, int64_t n, int D,
                                                            double* __restrict__ part) {
  __shared__ double red[8][32];
  const int r = threadIdx.x >> 5, d = threadIdx.x & 31;
  double acc = 0.0;
  if (d < D)
    for (int64_t i = (int64_t)blockIdx.x * 8 + r; i < n; i += (int64_t)gridDim.x * 8) acc += x[i * D + d];
  red[r][d] = acc;
  __syncthreads();
  if (r == 0 && d < D) {
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < 8; ++q) s += red[q][d];
    part[(size_t)blockIdx.x * D + d] = s;
  }
}

// mu = m / (n + m) mean(b) + n / (n + m) mean(a)   (abstract_acq_fcn.py:212-215)
__global__ void search_centre_kernel(const double* __restrict__ part_a, int64_t n, const double* __restrict__ part_b,
                                     int64_t m, int D, double* __restrict__ cen) {
  const int d = threadIdx.x;
  if (d >= D) return;
  double sa = 0.0, sb = 0.0;
  for (int b = 0; b < search_sum_blocks; ++b) {
    sa += part_a[(size_t)b * D + d];
    sb += part_b[(size_t)b * D + d];
  }
  const double tot = (double)(n + m);
  cen[d] = ((double)m / tot) * (sb / (double)m) + ((double)n / tot) * (sa / (double)n);
}

// out[n] = table[pos[n]]; a row whose distances are all +inf (coordinates beyond 1e154) has no argmin: NaN
__global__ __launch_bounds__(256) void search_take_kernel(const double* __restrict__ table, int64_t n_table,
                                                          const int64_t* __restrict__ pos, int64_t M, double* __restrict__ out) {
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= M) return;
  const int64_t p = pos[n];
  out[n] = (p >= 0 && p < n_table) ? table[p] : (double)NAN;
}

__global__ __launch_bounds__(256) void search_is_finish_kernel(int64_t M, double tol, const double* __restrict__ var_tot,
                                                               double* __restrict__ acq) {
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= M) return;
  double a = acq[n];
  if (tol > 0.0 && var_tot[n] < tol) a += tol / var_tot[n] - 1.0;
  acq[n] = (a < -kRealMax) ? -kRealMax : a;  // np.maximum: NaN stays NaN
}

// ---- the sort ----------------------------------------------------------------------------------------------------

__device__ inline uint64_t sort_key(double v) {
  if (v != v) return ~0ull - 1;  // NaN: behind +inf, in front of the padding
  if (v == 0.0) v = 0.0;         // -0.0 compares equal to 0.0: one key
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ inline void cas_pair(uint64_t* k, uint32_t* v, int64_t a, int64_t b, bool asc) {
  const uint64_t ka = k[a], kb = k[b];
  const uint32_t va = v[a], vb = v[b];
  const bool gt = ka > kb || (ka == kb && va > vb);
  if (gt == asc) {
    k[a] = kb;
    k[b] = ka;
    v[a] = vb;
    v[b] = va;
  }
}

// the index pair of compare-exchange number i at stride j
__device__ inline int64_t pair_lo(int64_t i, int64_t j) { return ((i & ~(j - 1)) << 1) | (i & (j - 1)); }

// bitonic passes j = jtop .. 1 of stage k on an LDS chunk of `len` pairs whose first pair has global index g0
__device__ void lds_bitonic(uint64_t* sk, uint32_t* sv, int len, int64_t g0, int64_t k, int jtop) {
  for (int j = jtop; j > 0; j >>= 1) {
    for (int i = threadIdx.x; i < len / 2; i += kSortThreads) {
      const int lo = (int)pair_lo(i, j);
      cas_pair(sk, sv, lo, lo + j, ((g0 + lo) & k) == 0);
    }
    __syncthreads();
  }
}

// chunk b of `len` pairs (len = min(P, 8192)): keys formed from acq (padding behind M sorts last), stages k = 2 .. len
__global__ __launch_bounds__(kSortThreads) void search_sort_chunks_kernel(const double* __restrict__ acq, int64_t M, int len,
                                                                          uint64_t* __restrict__ keys,
                                                                          uint32_t* __restrict__ idx) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sort_lds[];
  uint64_t* sk = (uint64_t*)sort_lds;
  uint32_t* sv = (uint32_t*)(sk + kSortChunk);
  const int64_t g0 = (int64_t)blockIdx.x * len;
  for (int i = threadIdx.x; i < len; i += kSortThreads) {
    const int64_t g = g0 + i;
    sk[i] = g < M ? sort_key(acq[g]) : ~0ull;
    sv[i] = (uint32_t)g;
  }
  __syncthreads();
  for (int64_t k = 2; k <= len; k <<= 1) lds_bitonic(sk, sv, len, g0, k, (int)(k >> 1));
  for (int i = threadIdx.x; i < len; i += kSortThreads) {
    keys[g0 + i] = sk[i];
    idx[g0 + i] = sv[i];
  }
}

// one pass of stage k at a stride j >= 8192: compare-exchange number i of P / 2
__global__ __launch_bounds__(256) void search_sort_global_kernel(uint64_t* keys, uint32_t* idx, int64_t P, int64_t k, int64_t j) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P / 2) return;
  const int64_t lo = pair_lo(i, j);
  cas_pair(keys, idx, lo, lo + j, (lo & k) == 0);
}

// the passes j = 4096 .. 1 of stage k on chunk b
__global__ __launch_bounds__(kSortThreads) void search_sort_merge_kernel(uint64_t* __restrict__ keys, uint32_t* __restrict__ idx,
                                                                         int64_t k) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sort_lds[];
  uint64_t* sk = (uint64_t*)sort_lds;
  uint32_t* sv = (uint32_t*)(sk + kSortChunk);
  const int64_t g0 = (int64_t)blockIdx.x * kSortChunk;
  for (int i = threadIdx.x; i < kSortChunk; i += kSortThreads) {
    sk[i] = keys[g0 + i];
    sv[i] = idx[g0 + i];
  }
  __syncthreads();
  lds_bitonic(sk, sv, kSortChunk, g0, k, kSortChunk / 2);
  for (int i = threadIdx.x; i < kSortChunk; i += kSortThreads) {
    keys[g0 + i] = sk[i];
    idx[g0 + i] = sv[i];
  }
}

__global__ __launch_bounds__(256) void search_gather_kernel(const double* __restrict__ X, const uint32_t* __restrict__ idx,
                                                            int64_t M, int D, int64_t* __restrict__ order,
                                                            double* __restrict__ Xs) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= M * D) return;
  const int64_t m = e / D;
  const int d = (int)(e - m * D);
  const uint32_t src = idx[m];
  if (d == 0) order[m] = (int64_t)src;
  Xs[e] = X[(int64_t)src * D + d];
}

constexpr size_t kSortLds = (size_t)kSortChunk * (sizeof(uint64_t) + sizeof(uint32_t));

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

int launch_search_fill(vbmc_ctx* ctx, double* d_X, int64_t M, int D, const SearchSrcDev* d_src, int n_src, const double* d_par,
                       const double* d_lb, const double* d_ub, uint32_t int_bits, const XfView* t) {
  FillArgs a;
  a.X = d_X;
  a.M = M;
  a.D = D;
  a.n_src = n_src;
  a.src = d_src;
  a.par = d_par;
  a.lb = d_lb;
  a.ub = d_ub;
  a.int_bits = int_bits;
  a.has_xf = t != nullptr;
  if (t) a.t = *t;
#define CALL(DP) hipLaunchKernelGGL(search_fill_kernel<DP>, dim3(blocks_for(M)), dim3(256), 0, ctx->stream, a)
  VBMC_DISPATCH_DP(D, CALL);
#undef CALL
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

int launch_search_mask(vbmc_ctx* ctx, const double* d_X, int64_t M, int D, const XfView* t, const double* d_lb,
                       const double* d_ub, double* d_acq) {
  const XfView tv = t ? *t : XfView();
  const int has_xf = t != nullptr;
#define CALL(DP) \
  hipLaunchKernelGGL(search_mask_kernel<DP>, dim3(blocks_for(M)), dim3(256), 0, ctx->stream, d_X, M, D, has_xf, tv, d_lb, d_ub, d_acq)
  VBMC_DISPATCH_DP(D, CALL);
#undef CALL
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

int launch_search_scale(vbmc_ctx* ctx, const double* d_X, int64_t M, int D, const double* d_ell, double* d_xsc) {
  hipLaunchKernelGGL(search_scale_kernel, dim3(blocks_for(M * D)), dim3(256), 0, ctx->stream, d_X, M * D, D, d_ell, d_xsc);
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

int launch_search_colsum(vbmc_ctx* ctx, const double* d_x, int64_t n, int D, double* d_part) {
  hipLaunchKernelGGL(search_colsum_kernel, dim3(search_sum_blocks), dim3(256), 0, ctx->stream, d_x, n, D, d_part);
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

int launch_search_centre(vbmc_ctx* ctx, const double* d_part_a, int64_t n, const double* d_part_b, int64_t m, int D,
                         double* d_cen) {
  hipLaunchKernelGGL(search_centre_kernel, dim3(1), dim3(64), 0, ctx->stream, d_part_a, n, d_part_b, m, D, d_cen);
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

int launch_search_take(vbmc_ctx* ctx, const double* d_table, int64_t n_table, const int64_t* d_pos, int64_t M, double* d_out) {
  hipLaunchKernelGGL(search_take_kernel, dim3(blocks_for(M)), dim3(256), 0, ctx->stream, d_table, n_table, d_pos, M, d_out);
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

int launch_search_is_finish(vbmc_ctx* ctx, int64_t M, double tol_gp_var, const double* d_var_tot, double* d_acq) {
  hipLaunchKernelGGL(search_is_finish_kernel, dim3(blocks_for(M)), dim3(256), 0, ctx->stream, M, tol_gp_var, d_var_tot, d_acq);
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

int64_t search_sort_len(int64_t M) {
  int64_t p = 2;
  while (p < M) p <<= 1;
  return p;
}

int launch_search_sort(vbmc_ctx* ctx, const double* d_acq, int64_t M, uint64_t* d_keys, uint32_t* d_idx) {
  const int64_t P = search_sort_len(M);
  const int len = (int)(P < kSortChunk ? P : kSortChunk);
  static bool lds_set[64] = {};
  if (!lds_set[ctx->device & 63]) {
    HIP_TRY(ctx, hipFuncSetAttribute((const void*)search_sort_chunks_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)kSortLds));
    HIP_TRY(ctx, hipFuncSetAttribute((const void*)search_sort_merge_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)kSortLds));
    lds_set[ctx->device & 63] = true;
  }
  hipLaunchKernelGGL(search_sort_chunks_kernel, dim3((unsigned)(P / len)), dim3(kSortThreads), kSortLds, ctx->stream, d_acq, M,
                     len, d_keys, d_idx);
  for (int64_t k = 2 * (int64_t)kSortChunk; k <= P; k <<= 1) {
    for (int64_t j = k >> 1; j >= kSortChunk; j >>= 1)
      hipLaunchKernelGGL(search_sort_global_kernel, dim3(blocks_for(P / 2)), dim3(256), 0, ctx->stream, d_keys, d_idx, P, k, j);
    hipLaunchKernelGGL(search_sort_merge_kernel, dim3((unsigned)(P / kSortChunk)), dim3(kSortThreads), kSortLds, ctx->stream,
                       d_keys, d_idx, k);
  }
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

int launch_search_gather(vbmc_ctx* ctx, const double* d_X, const uint32_t* d_idx, int64_t M, int D, int64_t* d_order,
                         double* d_Xs) {
  hipLaunchKernelGGL(search_gather_kernel, dim3(blocks_for(M * D)), dim3(256), 0, ctx->stream, d_X, d_idx, M, D, d_order,
                     d_Xs);
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}
