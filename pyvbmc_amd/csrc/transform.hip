// The parameter transformer on the device: VariationalPosterior's original-space calls
// (variational_posterior/variational_posterior.py: sample :355-362, pdf :429-439 / :543-559,
// moments :791-796, kl_div's Monte-Carlo branch :1107-1122) with the reference's
// ParameterTransformer (parameter_transformer/parameter_transformer.py) restated in transform.h.
//
// A context holds two transformer descriptors: slot 0 belongs to the context's mixture, slot 1 to the
// second mixture of vbmc_kl_div_mc_orig.  This file keeps the slots, the transformer's kernels and their launchers
// (transform.h), vbmc_transform and the Monte-Carlo moments; the original-space sample, pdf and kl_div entry points
// are the transformed-space ones of sample.hip and mixture.hip with a descriptor passed in.
#include <cmath>
#include <cstring>

#include "common.h"
#include "fastmath.h"
#include "transform.h"

namespace {

struct XfSlot {
  bool set = false;
  int D = 0;
  bool has_R = false, has_scale = false;
  std::vector<double> host;  // the descriptor as uploaded (XfLayout)
  double* d = nullptr;  // device copy, sized for D = 32 with R
};

struct XfState {
  XfSlot slot[2];
};

XfState* xf_state(vbmc_ctx* ctx) {
  if (!ctx->xf) ctx->xf = new XfState();
  return (XfState*)ctx->xf;
}

XfView xf_view(const XfSlot& s) {
  XfView v;
  v.p = s.d;
  v.D = s.D;
  v.has_R = s.has_R ? 1 : 0;
  v.has_scale = s.has_scale ? 1 : 0;
  return v;
}

constexpr int kThreads = 256;

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

// dir 0: x -> u (n x D), 1: u -> x (n x D), 2: log|det J|(u) (n).  in == out is allowed for dir 0 / 1.
template <int DP, int DIR>
__global__ __launch_bounds__(256) void xf_apply_kernel(XfView t, int64_t n, const double* in, double* out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int D = t.D;
  double v[DP];
#pragma unroll
  for (int d = 0; d < DP; ++d) v[d] = (d < D) ? in[i * D + d] : 0.0;
  if (DIR == 2) {
    out[i] = xf_log_abs_det<DP>(t, v);
    return;
  }
  if (DIR == 0) xf_forward<DP>(t, v);
  else xf_inverse<DP>(t, v);
#pragma unroll
  for (int d = 0; d < DP; ++d)
    if (d < D) out[i * D + d] = v[d];
}

// The front of pdf(orig_flag=True): rows strictly inside the bounds go to u = T(x) and their log|J|(u);
// rows outside keep their original coordinates -- non-finite ones replaced by 0, as the host path does
// before its density call (variational_posterior.py pdf) -- and are flagged.  x and u may alias.
template <int DP>
__global__ __launch_bounds__(256) void xf_prep_kernel(XfView t, int64_t n, const double* x, double* u, double* lj,
                                                      double* inside) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int D = t.D;
  double v[DP];
#pragma unroll
  for (int d = 0; d < DP; ++d) v[d] = (d < D) ? x[i * D + d] : 0.0;
  const bool in = xf_inside<DP>(t, v);
  if (in) {
    xf_forward<DP>(t, v);
  } else {
#pragma unroll
    for (int d = 0; d < DP; ++d) v[d] = isfinite(v[d]) ? v[d] : 0.0;
  }
#pragma unroll
  for (int d = 0; d < DP; ++d)
    if (d < D) u[i * D + d] = v[d];
  double l = 0.0;
  if (in) l = xf_log_abs_det<DP>(t, v);
  lj[i] = l;
  inside[i] = in ? 1.0 : 0.0;
}

// The back of pdf(orig_flag=True): log q - log|J|, or q / exp(log|J|); -inf / 0 outside the bounds.
__global__ __launch_bounds__(256) void xf_finish_kernel(int64_t n, int log_flag, const double* __restrict__ lj,
                                                        const double* __restrict__ inside, double* __restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double v = y[i];
  if (inside[i] == 0.0) v = log_flag ? -INFINITY : 0.0;
  else v = log_flag ? v - lj[i] : v / exp(lj[i]);
  y[i] = v;
}

// per-block column sums of x (n x D) -> part[block][D]
template <int DP>
__global__ __launch_bounds__(256) void col_sum_kernel(const double* __restrict__ x, int64_t n, int D,
                                                      double* __restrict__ part) {
  __shared__ double red[4][DP];
  double s[DP];
#pragma unroll
  for (int d = 0; d < DP; ++d) s[d] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
#pragma unroll
    for (int d = 0; d < DP; ++d)
      if (d < D) s[d] += x[i * D + d];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 0; d < DP; ++d) {
    const double t = fm::wave_sum_dpp(s[d]);
    if (lane == 0) red[wv][d] = t;
  }
  __syncthreads();
  if ((int)threadIdx.x < D)
    part[(size_t)blockIdx.x * D + threadIdx.x] =
        (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// per-block sums of the centred products (x_i - m_i)(x_j - m_j), i <= j, over a contiguous chunk of rows
// -> part[block][P], P = D (D + 1) / 2 (pair p of row-major upper-triangle order).  Rows are staged through
// LDS 64 at a time; thread t owns pairs t, t + 256, t + 512.
constexpr int kCovRows = 64;
__global__ __launch_bounds__(256) void cov_part_kernel(const double* __restrict__ x, int64_t n, int D,
                                                       const double* __restrict__ mean, double* __restrict__ part) {
  __shared__ double tile[kCovRows][33];
  const int P = D * (D + 1) / 2;
  int pi[3], pj[3];
  double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    int p = (int)threadIdx.x + 256 * r, i = 0;
    pi[r] = -1;
    pj[r] = 0;
    if (p < P) {
      while (p >= D - i) {
        p -= D - i;
        ++i;
      }
      pi[r] = i;
      pj[r] = i + p;
    }
  }
  const int64_t chunk = (n + gridDim.x - 1) / gridDim.x;
  const int64_t r0 = (int64_t)blockIdx.x * chunk;
  const int64_t r1 = (r0 + chunk < n) ? r0 + chunk : n;
  for (int64_t b = r0; b < r1; b += kCovRows) {
    const int rows = (int)((r1 - b) < kCovRows ? (r1 - b) : kCovRows);
    __syncthreads();
    for (int e = threadIdx.x; e < kCovRows * D; e += 256) {
      const int r = e / D, d = e - r * D;
      tile[r][d] = r < rows ? x[(b + r) * D + d] - mean[d] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 3; ++q)
      if (pi[q] >= 0) {
        double a = acc[q];
        for (int r = 0; r < rows; ++r) a = fma(tile[r][pi[q]], tile[r][pj[q]], a);
        acc[q] = a;
      }
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int p = (int)threadIdx.x + 256 * q;
    if (p < P) part[(size_t)blockIdx.x * P + p] = acc[q];
  }
}

// out[j] = (sum_b part[b][j]) * scale (or / div when div != 0), one workgroup per j; fixed order, deterministic
__global__ __launch_bounds__(256) void part_reduce_kernel(const double* __restrict__ part, int nblk, int m, double scale,
                                                          double div, double* __restrict__ out) {
  __shared__ double red[4];
  const int j = blockIdx.x;
  double s = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 256) s += part[(size_t)b * m + j];
  s = fm::wave_sum_dpp(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double t = (red[0] + red[1]) + (red[2] + red[3]);
    out[j] = div != 0.0 ? t / div : t * scale;
  }
}

template <int DP>
void launch_apply_dp(vbmc_ctx* ctx, const XfView& t, int64_t n, int dir, const double* in, double* out) {
  const dim3 g(blocks_for(n)), b(kThreads);
  if (dir == 0) hipLaunchKernelGGL((xf_apply_kernel<DP, 0>), g, b, 0, ctx->stream, t, n, in, out);
  else if (dir == 1) hipLaunchKernelGGL((xf_apply_kernel<DP, 1>), g, b, 0, ctx->stream, t, n, in, out);
  else hipLaunchKernelGGL((xf_apply_kernel<DP, 2>), g, b, 0, ctx->stream, t, n, in, out);
}

template <int DP>
void launch_prep_dp(vbmc_ctx* ctx, const XfView& t, int64_t n, const double* x, double* u, double* lj, double* in) {
  hipLaunchKernelGGL((xf_prep_kernel<DP>), dim3(blocks_for(n)), dim3(kThreads), 0, ctx->stream, t, n, x, u, lj, in);
}

template <int DP>
void launch_colsum_dp(vbmc_ctx* ctx, const double* x, int64_t n, int D, int nblk, double* part) {
  hipLaunchKernelGGL((col_sum_kernel<DP>), dim3(nblk), dim3(kThreads), 0, ctx->stream, x, n, D, part);
}

bool valid_type(double t) { return t == XF_UNBOUNDED || t == XF_LOGIT || t == XF_PROBIT || t == XF_STUDENT4; }

}  // namespace

void xf_free(vbmc_ctx* ctx) {
  if (!ctx->xf) return;
  XfState* st = (XfState*)ctx->xf;
  for (XfSlot& s : st->slot)
    if (s.d) (void)hipFree(s.d);
  delete st;
  ctx->xf = nullptr;
}

bool xf_view_slot(vbmc_ctx* ctx, int slot, int D, XfView& v) {
  const XfSlot& s = xf_state(ctx)->slot[slot];
  if (!s.set || s.D != D) return false;
  v = xf_view(s);
  return true;
}

// the slot's descriptor, checked against the context's D
int xf_need(vbmc_ctx* ctx, int slot, int D, const char* who, XfView& v) {
  XfState* st = xf_state(ctx);
  const XfSlot& s = st->slot[slot];
  if (!s.set) return vbmc_fail(ctx, VBMC_E_ARG, "%s: transformer slot %d not set", who, slot);
  if (s.D != D) return vbmc_fail(ctx, VBMC_E_ARG, "%s: transformer slot %d has D=%d, the mixture D=%d", who, slot, s.D, D);
  v = xf_view(s);
  return 0;
}

int launch_xf_apply(vbmc_ctx* ctx, const XfView& t, int64_t n, int dir, const double* d_in, double* d_out) {
#define CALL(DP) launch_apply_dp<DP>(ctx, t, n, dir, d_in, d_out)
  VBMC_DISPATCH_DP(t.D, CALL);
#undef CALL
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

int launch_xf_prep(vbmc_ctx* ctx, const XfView& t, int64_t n, const double* d_x, double* d_u, double* d_lj,
                   double* d_in) {
#define CALL(DP) launch_prep_dp<DP>(ctx, t, n, d_x, d_u, d_lj, d_in)
  VBMC_DISPATCH_DP(t.D, CALL);
#undef CALL
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

int launch_xf_finish(vbmc_ctx* ctx, int64_t n, int log_flag, const double* d_lj, const double* d_in, double* d_y) {
  hipLaunchKernelGGL(xf_finish_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, ctx->stream, n, log_flag, d_lj, d_in,
                     d_y);
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

extern "C" int vbmc_set_transformer(vbmc_ctx* ctx, int slot, int D, const double* type_D, const double* lb_D,
                                    const double* ub_D, const double* mu_D, const double* delta_D,
                                    const double* R_DxD, const double* scale_D) {
  if (!ctx) return VBMC_E_ARG;
  if (slot < 0 || slot > 1) return vbmc_fail(ctx, VBMC_E_ARG, "set_transformer: slot %d (0 or 1)", slot);
  if (D < 1) return vbmc_fail(ctx, VBMC_E_ARG, "set_transformer: D=%d", D);
  if (D > 32) return vbmc_fail(ctx, VBMC_E_UNSUP, "set_transformer: D=%d > 32 not supported", D);
  if (!type_D || !lb_D || !ub_D || !mu_D || !delta_D) return vbmc_fail(ctx, VBMC_E_ARG, "set_transformer: null array");
  for (int d = 0; d < D; ++d) {
    if (!valid_type(type_D[d]))
      return vbmc_fail(ctx, VBMC_E_ARG, "set_transformer: type[%d]=%g (0, 3, 12 or 13)", d, type_D[d]);
    if (type_D[d] != XF_UNBOUNDED && !(std::isfinite(lb_D[d]) && std::isfinite(ub_D[d]) && lb_D[d] < ub_D[d]))
      return vbmc_fail(ctx, VBMC_E_ARG, "set_transformer: bounded dimension %d needs finite lb < ub", d);
  }
  const bool has_R = R_DxD != nullptr, has_scale = scale_D != nullptr;
  std::vector<double> h((size_t)XfLayout::total(D, has_R));
  for (int d = 0; d < D; ++d) {
    h[XfLayout::row(XfLayout::TYPE, D) + d] = type_D[d];
    h[XfLayout::row(XfLayout::LB, D) + d] = lb_D[d];
    h[XfLayout::row(XfLayout::UB, D) + d] = ub_D[d];
    h[XfLayout::row(XfLayout::MU, D) + d] = mu_D[d];
    h[XfLayout::row(XfLayout::DELTA, D) + d] = delta_D[d];
    h[XfLayout::row(XfLayout::LB_UP, D) + d] = std::nextafter(lb_D[d], INFINITY);
    h[XfLayout::row(XfLayout::UB_DN, D) + d] = std::nextafter(ub_D[d], -INFINITY);
    h[XfLayout::row(XfLayout::LOG_SPAN, D) + d] = std::log(ub_D[d] - lb_D[d]);
    h[XfLayout::row(XfLayout::LOG_DELTA, D) + d] = std::log(delta_D[d]);
    h[XfLayout::row(XfLayout::SCALE, D) + d] = has_scale ? scale_D[d] : 1.0;
    h[XfLayout::row(XfLayout::LOG_SCALE, D) + d] = has_scale ? std::log(scale_D[d]) : 0.0;
  }
  if (has_R) std::memcpy(h.data() + XfLayout::o_R(D), R_DxD, sizeof(double) * D * D);
  XfSlot& s = xf_state(ctx)->slot[slot];
  // the values the device already holds: nothing to do
  if (s.set && s.D == D && s.has_R == has_R && s.has_scale == has_scale && s.host.size() == h.size() &&
      std::memcmp(s.host.data(), h.data(), sizeof(double) * h.size()) == 0)
    return VBMC_OK;
  s.set = false;
  if (ctx->device >= 0) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!s.d) HIP_TRY(ctx, hipMalloc((void**)&s.d, sizeof(double) * XfLayout::total(32, true)));  // (the largest)
    // (synchronous: a kernel queued earlier may still read the old descriptor)
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(s.d, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice));
  }
  s.host.swap(h);
  s.D = D;
  s.has_R = has_R;
  s.has_scale = has_scale;
  s.set = true;
  return VBMC_OK;
}

extern "C" int vbmc_clear_transformer(vbmc_ctx* ctx, int slot) {
  if (!ctx) return VBMC_E_ARG;
  if (slot < 0 || slot > 1) return vbmc_fail(ctx, VBMC_E_ARG, "clear_transformer: slot %d (0 or 1)", slot);
  if (ctx->xf) ((XfState*)ctx->xf)->slot[slot].set = false;
  return VBMC_OK;
}

extern "C" int vbmc_transform(vbmc_ctx* ctx, int64_t n, int direction, const double* in, double* out) {
  if (!ctx || n < 0 || (n > 0 && (!in || !out))) return VBMC_E_ARG;
  if (direction < 0 || direction > 2) return vbmc_fail(ctx, VBMC_E_ARG, "transform: direction %d (0, 1 or 2)", direction);
  XfState* st = xf_state(ctx);
  if (!st->slot[0].set) return vbmc_fail(ctx, VBMC_E_ARG, "transform: transformer slot 0 not set");
  if (n == 0) return VBMC_OK;
  NEED_DEVICE(ctx);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const XfView t = xf_view(st->slot[0]);
  const int D = t.D;
  const int64_t BATCH = (int64_t)1 << 21;
  const int64_t nb = n < BATCH ? n : BATCH;
  const size_t n_out = direction == 2 ? 1 : (size_t)D;
  Scratch sc;
  const auto p_in = sc.add((size_t)nb * D), p_out = sc.add((size_t)nb * n_out);
  int rc = reserve(ctx, sc);
  if (rc) return rc;
  double *d_in = sc.ptr(p_in), *d_out = sc.ptr(p_out);
  for (int64_t o = 0; o < n; o += nb) {
    const int64_t m = (n - o) < nb ? (n - o) : nb;
    HIP_TRY(ctx, hipMemcpyAsync(d_in, in + o * D, sizeof(double) * m * D, hipMemcpyHostToDevice, ctx->stream));
    rc = launch_xf_apply(ctx, t, m, direction, d_in, d_out);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(out + o * n_out, d_out, sizeof(double) * m * n_out, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, stream_wait(ctx));
  }
  return VBMC_OK;
}

extern "C" int vbmc_mixture_moments_orig(vbmc_ctx* ctx, int64_t N, uint64_t seed, int cov_flag, double* mean_D,
                                         double* cov_DxD) {
  if (!ctx || N < 1 || !mean_D || (cov_flag && !cov_DxD)) return VBMC_E_ARG;
  if (!ctx->mix_set) return vbmc_fail(ctx, VBMC_E_ARG, "mixture_moments_orig: mixture not set");
  XfView t;
  int rc = xf_need(ctx, 0, ctx->D, "mixture_moments_orig", t);
  if (rc) return rc;
  NEED_DEVICE(ctx);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int D = ctx->D, K = ctx->K, P = D * (D + 1) / 2;
  const int nblk = 512;
  Scratch sc;
  const auto p_x = sc.add((size_t)N * D), p_sel = sc.add(selector_elems(K));
  const auto p_part = sc.add((size_t)nblk * (D > P ? D : P)), p_mean = sc.add((size_t)D), p_cov = sc.add((size_t)P);
  rc = reserve(ctx, sc);
  if (rc) return rc;
  double *d_x = sc.ptr(p_x), *d_sel = sc.ptr(p_sel), *d_part = sc.ptr(p_part), *d_mean = sc.ptr(p_mean), *d_cov = sc.ptr(p_cov);
  // the balanced samples of sample(N, orig_flag=True, balance_flag=True) (:791-796), never copied out
  rc = launch_sample(ctx, ctx->d_mix, ctx->ml, ctx->w.data(), N, seed, 1, d_sel, d_x, nullptr, INFINITY);
  if (rc) return rc;
  rc = launch_xf_apply(ctx, t, N, 1, d_x, d_x);
  if (rc) return rc;
  // np.mean(x, axis=0) = sum / N; np.cov(x.T): centred products times 1 / (N - 1)
#define CALL(DP) launch_colsum_dp<DP>(ctx, d_x, N, D, nblk, d_part)
  VBMC_DISPATCH_DP(D, CALL);
#undef CALL
  HIP_TRY(ctx, hipGetLastError());
  hipLaunchKernelGGL(part_reduce_kernel, dim3(D), dim3(kThreads), 0, ctx->stream, (const double*)d_part, nblk, D, 0.0,
                     (double)N, d_mean);
  HIP_TRY(ctx, hipGetLastError());
  if (cov_flag) {
    hipLaunchKernelGGL(cov_part_kernel, dim3(nblk), dim3(kThreads), 0, ctx->stream, (const double*)d_x, N, D,
                       (const double*)d_mean, d_part);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(part_reduce_kernel, dim3(P), dim3(kThreads), 0, ctx->stream, (const double*)d_part, nblk, P,
                       1.0 / (double)(N - 1), 0.0, d_cov);
    HIP_TRY(ctx, hipGetLastError());
  }
  std::vector<double> tri(cov_flag ? P : 0);
  HIP_TRY(ctx, hipMemcpyAsync(mean_D, d_mean, sizeof(double) * D, hipMemcpyDeviceToHost, ctx->stream));
  if (cov_flag) HIP_TRY(ctx, hipMemcpyAsync(tri.data(), d_cov, sizeof(double) * P, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, stream_wait(ctx));
  if (cov_flag)
    for (int i = 0, p = 0; i < D; ++i)
      for (int j = i; j < D; ++j, ++p) cov_DxD[i * D + j] = cov_DxD[j * D + i] = tri[p];
  return VBMC_OK;
}
