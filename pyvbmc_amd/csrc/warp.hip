// Input warping (rotoscaling) on the device: the kernels behind whitening/whitening.py's unscent_warp (:7-77),
// warp_input (:165-223) and warp_gp_and_vp (:276-373).
//
// Everything here applies the composed map  old inference space -> original space -> new inference space,
// y = new(old^-1(x)), with the two transformers of transform.h: slot 0 the old one, slot 1 the new one.
//
//   warp_points_kernel    one thread per point: the map (or new(x) from the original space), optionally on box draws
//                         formed in the kernel (uploaded uniforms, or Philox stream 9 of sample.hip's list), and the
//                         log-Jacobians of the new transformer at the result / of the old one at the input
//   warp_unscent_kernel   one workgroup per base point (grid n x S): thread u warps sigma point u of the U = 2 D + 1,
//                         the points meet in LDS, thread d takes the mean and the ddof = 1 standard deviation of
//                         dimension d in two passes, both summed in the order u = 0 .. U - 1 (NumPy's order for a
//                         reduction over the leading axis)
//   warp_row_means_kernel fixed-order means over the training points (warp_gp_and_vp's mean_N log ell_new, mean dy)
//   warp_minmax_kernel    per-dimension minimum / maximum of the mapped box draws
//   warp_quantile_kernel  per dimension: the remaining bitonic stages of colsort.h over the chunk-sorted column, then
//                         np.quantile's linear rule on the exact order statistics
//
// Both transformer descriptors (with their D x D rotation matrices, read D times per point) are staged into LDS once
// per workgroup; the per-point code of transform.h then reads them from there.  FP64 throughout, no floating-point
// atomics: every result is bit-reproducible.
#include "warp.h"

#include "colsort.h"
#include "mixture_dev.h"

namespace {

constexpr int kPtThreads = 256;   // warp_points_kernel, warp_row_means_kernel, warp_minmax_kernel
constexpr int kUnsThreads = 128;  // warp_unscent_kernel: U = 2 D + 1 <= 65 sigma points
constexpr uint32_t kBoxStream = 9u;

template <int DP>
constexpr int desc_elems() { return XfLayout::NROWS * DP + DP * DP; }

// the descriptor of `t` copied to LDS (by the whole workgroup; the caller synchronises) and a view of the copy
__device__ inline XfView stage_desc(const XfView& t, double* s) {
  XfView r = t;
  if (!t.p) return r;
  const int n = XfLayout::total(t.D, t.has_R != 0);
  for (int i = threadIdx.x; i < n; i += blockDim.x) s[i] = t.p[i];
  r.p = s;
  return r;
}

struct PointArgs {
  int64_t n;
  int source;
  int gen;
  const double* in;
  const double* lo;
  const double* hi;
  uint64_t seed;
  double* y;
  double* lj_new;
  double* lj_old;
};

template <int DP>
__global__ __launch_bounds__(kPtThreads) void warp_points_kernel(XfView g0, XfView g1, PointArgs a) {
  __shared__ double s0[desc_elems<DP>()], s1[desc_elems<DP>()];
  const XfView t0 = stage_desc(g0, s0), t1 = stage_desc(g1, s1);
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kPtThreads + threadIdx.x;
  if (i >= a.n) return;
  const int D = t1.D;
  double v[DP];
  if (a.gen == 2) {
    // box draw i: dimensions 2 p, 2 p + 1 from the two 53-bit uniforms of block (i, p, stream 9)
#pragma unroll
    for (int p = 0; p < DP / 2; ++p)
      if (2 * p < D) {
        const Philox4 q = philox_block((uint64_t)i, (uint32_t)p, kBoxStream, a.seed);
        v[2 * p] = philox_u53(q.x[0], q.x[1]);
        v[2 * p + 1] = philox_u53(q.x[2], q.x[3]);
      }
  } else {
#pragma unroll
    for (int d = 0; d < DP; ++d) v[d] = (d < D) ? a.in[i * D + d] : 0.0;
  }
  if (a.gen != 0)  // np.random.rand(n, D) * (hi - lo) + lo
#pragma unroll
    for (int d = 0; d < DP; ++d) v[d] = (d < D) ? v[d] * (a.hi[d] - a.lo[d]) + a.lo[d] : 0.0;
  if (a.source == VBMC_WARP_FROM_OLD) {
    if (a.lj_old) {
      double w[DP];
#pragma unroll
      for (int d = 0; d < DP; ++d) w[d] = v[d];
      a.lj_old[i] = xf_log_abs_det<DP>(t0, w);
    }
    xf_inverse<DP>(t0, v);
  }
  if (a.source != VBMC_WARP_IN_NEW) xf_forward<DP>(t1, v);
  if (a.y)
#pragma unroll
    for (int d = 0; d < DP; ++d)
      if (d < D) a.y[i * D + d] = v[d];
  if (a.lj_new) a.lj_new[i] = xf_log_abs_det<DP>(t1, v);
}

template <int DP>
__global__ __launch_bounds__(kUnsThreads) void warp_unscent_kernel(XfView g0, XfView g1, WarpUnscent a) {
  __shared__ double s0[desc_elems<DP>()], s1[desc_elems<DP>()];
  __shared__ double sp[(2 * DP + 1) * DP];
  const XfView t0 = stage_desc(g0, s0), t1 = stage_desc(g1, s1);
  __syncthreads();
  const int D = t1.D, U = 2 * D + 1;
  const int64_t i = blockIdx.x;
  const int s = blockIdx.y, u = threadIdx.x;
  const double* sig = a.sigma + (int64_t)s * a.sigma_set_stride + i * a.sigma_row_stride;
  if (u < U) {
    double v[DP];
#pragma unroll
    for (int d = 0; d < DP; ++d) v[d] = (d < D) ? a.x[i * D + d] : 0.0;
    if (u > 0) {
      // points 2 d + 1 and 2 d + 2: x_d + / - sqrt(D) sigma_d (:60-65)
      const int d0 = (u - 1) >> 1;
      const double step = sqrt((double)D) * sig[d0];
#pragma unroll
      for (int d = 0; d < DP; ++d)
        if (d == d0) v[d] = (u & 1) ? v[d] + step : v[d] - step;
    }
    if (u == 0 && s == 0 && a.dy_old) {
      double w[DP];
#pragma unroll
      for (int d = 0; d < DP; ++d) w[d] = v[d];
      a.dy_old[i] = xf_log_abs_det<DP>(t0, w);
    }
    xf_inverse<DP>(t0, v);
    xf_forward<DP>(t1, v);
#pragma unroll
    for (int d = 0; d < DP; ++d)
      if (d < D) {
        sp[u * DP + d] = v[d];
        if (a.pts) a.pts[((int64_t)u * a.n + i) * D + d] = v[d];
      }
    if (u == 0 && s == 0 && a.dy) a.dy[i] = xf_log_abs_det<DP>(t1, v);
  }
  __syncthreads();
  if (u < D) {
    // np.mean(axis=0), np.std(axis=0, ddof=1): sum / U; sum of (x - mean)^2 / (U - 1), square root
    double m = 0.0;
    for (int p = 0; p < U; ++p) m += sp[p * DP + u];
    m = m / (double)U;
    double q = 0.0;
    for (int p = 0; p < U; ++p) {
      const double c = sp[p * DP + u] - m;
      q += c * c;
    }
    const double sd = sqrt(q / (double)(U - 1));
    const int64_t o = ((int64_t)s * a.n + i) * D + u;
    if (a.mean) a.mean[o] = m;
    if (a.sd) a.sd[o] = a.log_sd ? log(sd) : sd;
  }
}

// a workgroup's sum in a fixed order: a wave butterfly, then the wave sums in order
__device__ inline double block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[w];
  return t;
}

// grid (cols, S)
__global__ __launch_bounds__(kPtThreads) void warp_row_means_kernel(const double* __restrict__ a, int64_t rows, int cols,
                                                                    double* __restrict__ out) {
  __shared__ double red[kPtThreads / 64];
  const int c = blockIdx.x, s = blockIdx.y;
  const double* p = a + (int64_t)s * rows * cols + c;
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < rows; i += kPtThreads) acc += p[i * cols];
  const double t = block_sum(acc, red);
  if (threadIdx.x == 0) out[(int64_t)s * cols + c] = t / (double)rows;
}

// grid D: np.min / np.max over the rows (a NaN wins, as there)
__global__ __launch_bounds__(kPtThreads) void warp_minmax_kernel(const double* __restrict__ y, int64_t n, int D,
                                                                 double* __restrict__ out) {
  __shared__ double rlo[kPtThreads / 64], rhi[kPtThreads / 64];
  __shared__ int rnan[kPtThreads / 64];
  const int c = blockIdx.x;
  double lo = INFINITY, hi = -INFINITY;
  int nan = 0;
  for (int64_t i = threadIdx.x; i < n; i += kPtThreads) {
    const double v = y[i * D + c];
    nan |= (v != v);
    lo = v < lo ? v : lo;
    hi = v > hi ? v : hi;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double l2 = __shfl_xor(lo, o), h2 = __shfl_xor(hi, o);
    nan |= __shfl_xor(nan, o);
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
  }
  if ((threadIdx.x & 63) == 0) {
    rlo[threadIdx.x >> 6] = lo;
    rhi[threadIdx.x >> 6] = hi;
    rnan[threadIdx.x >> 6] = nan;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 0; w < kPtThreads / 64; ++w) {
      lo = rlo[w] < lo ? rlo[w] : lo;
      hi = rhi[w] > hi ? rhi[w] : hi;
      nan |= rnan[w];
    }
    out[c] = nan ? NAN : lo;
    out[D + c] = nan ? NAN : hi;
  }
}

// np.quantile(method="linear") of a sorted column of n keys: virtual index (n - 1) q, gamma its fractional part, _lerp of
// the two neighbours (a + (b - a) gamma, or b - (b - a)(1 - gamma) from gamma = 1/2 on)
__device__ inline double sorted_quantile(const uint64_t* gk, int64_t n, double qq) {
  const double vi = (double)(n - 1) * qq;
  const double pf = floor(vi);
  const double g = vi - pf;
  int64_t ip = (int64_t)pf, inx = ip + 1;
  if (ip < 0) ip = 0;
  if (ip > n - 1) ip = n - 1;
  if (inx > n - 1) inx = n - 1;
  const double va = from_key(gk[ip]), vb = from_key(gk[inx]);
  const double d = vb - va;
  return g >= 0.5 ? vb - d * (1.0 - g) : va + d * g;
}

// grid D, after kde_sort_chunks_kernel
__global__ __launch_bounds__(kThreads) void warp_quantile_kernel(uint64_t* __restrict__ keys, int64_t pmax, int64_t n,
                                                                 int D, const unsigned* __restrict__ nonfinite,
                                                                 double* __restrict__ out, double* __restrict__ sorted) {
  extern __shared__ __attribute__((aligned(16))) double sh[];
  const int c = blockIdx.x;
  uint64_t* gk = keys + (int64_t)c * pmax;
  if (nonfinite[c] != 0) {
    if (threadIdx.x == 0) out[c] = out[D + c] = NAN;
    return;
  }
  column_merge(gk, pmax, (uint64_t*)sh);
  if (threadIdx.x == 0) {
    out[c] = sorted_quantile(gk, n, 0.05);
    out[D + c] = sorted_quantile(gk, n, 0.95);
  }
  if (sorted)
    for (int64_t i = threadIdx.x; i < n; i += kThreads) sorted[(int64_t)c * n + i] = from_key(gk[i]);
}

template <int DP>
void points_dp(vbmc_ctx* ctx, const XfView& t0, const XfView& t1, const PointArgs& a) {
  hipLaunchKernelGGL((warp_points_kernel<DP>), dim3((unsigned)((a.n + kPtThreads - 1) / kPtThreads)), dim3(kPtThreads), 0,
                     ctx->stream, t0, t1, a);
}

template <int DP>
void unscent_dp(vbmc_ctx* ctx, const XfView& t0, const XfView& t1, const WarpUnscent& a) {
  hipLaunchKernelGGL((warp_unscent_kernel<DP>), dim3((unsigned)a.n, (unsigned)a.S), dim3(kUnsThreads), 0, ctx->stream, t0,
                     t1, a);
}

}  // namespace

int launch_warp_points(vbmc_ctx* ctx, const XfView& t0, const XfView& t1, int64_t n, int source, const double* in,
                       const WarpBox& box, double* y, double* lj_new, double* lj_old) {
  PointArgs a;
  a.n = n;
  a.source = source;
  a.gen = box.gen;
  a.in = in;
  a.lo = box.lo;
  a.hi = box.hi;
  a.seed = box.seed;
  a.y = y;
  a.lj_new = lj_new;
  a.lj_old = lj_old;
#define CALL(DP) points_dp<DP>(ctx, t0, t1, a)
  VBMC_DISPATCH_DP(t1.D, CALL);
#undef CALL
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

int launch_warp_unscent(vbmc_ctx* ctx, const XfView& t0, const XfView& t1, const WarpUnscent& a) {
#define CALL(DP) unscent_dp<DP>(ctx, t0, t1, a)
  VBMC_DISPATCH_DP(t1.D, CALL);
#undef CALL
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

int launch_warp_row_means(vbmc_ctx* ctx, const double* a, int S, int64_t rows, int cols, double* out) {
  hipLaunchKernelGGL(warp_row_means_kernel, dim3((unsigned)cols, (unsigned)S), dim3(kPtThreads), 0, ctx->stream, a, rows,
                     cols, out);
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

int64_t warp_sort_pmax(int64_t n) { return next_pow2(n > kChunk ? n : kChunk); }

int launch_warp_box_stats(vbmc_ctx* ctx, const double* y, int64_t n, int D, int mode, uint64_t* keys, unsigned* nonfinite,
                          double* out, double* sorted) {
  if (mode == 1) {
    hipLaunchKernelGGL(warp_minmax_kernel, dim3((unsigned)D), dim3(kPtThreads), 0, ctx->stream, y, n, D, out);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
  }
  const int64_t pmax = warp_sort_pmax(n);
  KdeSrc src = {};
  src.x[0] = src.x[1] = y;
  src.n[0] = src.n[1] = n;
  src.rs[0] = src.rs[1] = D;
  src.cs[0] = src.cs[1] = 1;
  src.ncol0 = D;
  HIP_TRY(ctx, hipMemsetAsync(nonfinite, 0, sizeof(unsigned) * D, ctx->stream));
  hipLaunchKernelGGL(kde_sort_chunks_kernel, dim3((unsigned)(pmax / kChunk), (unsigned)D), dim3(kThreads), 0, ctx->stream,
                     src, keys, pmax, nonfinite);
  HIP_TRY(ctx, hipGetLastError());
  const size_t lds = (size_t)kChunk * sizeof(uint64_t);
  HIP_TRY(ctx, hipFuncSetAttribute((const void*)warp_quantile_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(warp_quantile_kernel, dim3((unsigned)D), dim3(kThreads), lds, ctx->stream, keys, pmax, n, D,
                     (const unsigned*)nonfinite, out, sorted);
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}
