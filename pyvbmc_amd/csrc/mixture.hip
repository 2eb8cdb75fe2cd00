// Mixture density on a batch of points: VariationalPosterior.pdf / log_pdf in the
// transformed space (reference: variational_posterior/variational_posterior.py:441-541).
//
// One thread = one point (its D coordinates, lambda-scaled, live in registers); the
// K x D scaled means and per-component constants are wave-uniform reads.  Linear-
// domain accumulation over components then log with 0 -> -inf, exactly the
// reference's order of operations (:451-463, :531-541).
#include <cmath>
#include <cstring>

#include "common.h"
#include "fastmath.h"
#include "mixture_dev.h"
#include "transform.h"

namespace {

struct PdfArgs {
  const double* mix;
  MixLayout ml;
  const double* x;  // n x D
  int64_t n;
  int log_flag, grad_flag;
  int mode;     // 0 gaussian, 1 multivariate t (df>0), 2 product of univariate t (df<0)
  double df;    // |df|
  double nf;    // tail-specific normalisation replacing nconst (t variants)
  double* y;    // n
  double* dy;   // n x D or null
};

template <int DP, int MODE, bool GRAD>
__global__ __launch_bounds__(256) void mixture_pdf_kernel(PdfArgs a) {
  const int D = a.ml.D, K = a.ml.K;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const MixGauss mg = mix_gauss(a.mix, a.ml);
  const double* ilam = a.mix + a.ml.o_ilam;
  double xs[DP], g[DP];
#pragma unroll
  for (int d = 0; d < DP; ++d) {
    xs[d] = (d < D) ? scaled_coord<GRAD>(a.x[i * D + d], ilam[d]) : 0.0;
    g[d] = 0.0;
  }
  double y = 0.0;
  if (MODE == 0) {
    mix_gauss_accumulate<DP, GRAD, 1>(mg, xs, 0, y, g);
  } else {
    const double* mup = a.mix + a.ml.o_mup;
    const double* is2 = a.mix + a.ml.o_is2;
    const double* w = a.mix + a.ml.o_w;
    const double* sig = a.mix + a.ml.o_sig;
    for (int k = 0; k < K; ++k) {
      const double* mk = mup + k * D;
      double nn;
      if (MODE == 1) {
        double d2 = 0.0;
#pragma unroll
        for (int d = 0; d < DP; ++d)
          if (d < D) {
            const double u = xs[d] - mk[d];
            d2 = fma(u, u, d2);
          }
        // nf w_k / sigma_k^D (1 + d2/df)^(-(df+D)/2)   (:484-496)
        nn = a.nf * w[k] * pow(sig[k], -(double)D) * pow(1.0 + d2 * is2[k] / a.df, -0.5 * (a.df + D));
      } else {
        // prod_d (1 + z_d^2/|df|)^(-(|df|+1)/2)   (:513-524)
        double lg = 0.0;
#pragma unroll
        for (int d = 0; d < DP; ++d)
          if (d < D) {
            const double u = xs[d] - mk[d];
            lg += log1p(u * u * is2[k] / a.df);
          }
        nn = a.nf * w[k] * pow(sig[k], -(double)D) * exp(-0.5 * (a.df + 1.0) * lg);
      }
      y += nn;
    }
  }
  if (GRAD) {
    // dy = -sum_k nn (x - mu_k)/(lambda^2 sigma_k^2); log: dy / y taken before the log (:464-469,532)
    const double s = a.log_flag ? -1.0 / y : -1.0;
#pragma unroll
    for (int d = 0; d < DP; ++d)
      if (d < D) a.dy[i * D + d] = s * g[d] * ilam[d];
  }
  if (a.log_flag) y = (y == 0.0) ? -INFINITY : log(y);
  a.y[i] = y;
}

// Small batches (acquisition populations, single points): one WAVE per point, lanes over the
// components, so the K terms are evaluated side by side and summed by a shuffle tree instead of
// one thread walking K dependent load -> exp steps (24 us for one point at K = 50, against 5).
// The sum over components is a tree here and a running sum in the kernel above: results agree to
// rounding (~1e-16 relative), not bit for bit.
template <int DP, bool GRAD>
__global__ __launch_bounds__(256) void mixture_pdf_wave_kernel(PdfArgs a) {
  const int D = a.ml.D;
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= a.n) return;
  const MixGauss mg = mix_gauss(a.mix, a.ml);
  const double* ilam = a.mix + a.ml.o_ilam;
  double xs[DP], g[DP];
#pragma unroll
  for (int d = 0; d < DP; ++d) {
    xs[d] = (d < D) ? scaled_coord<GRAD>(a.x[i * D + d], ilam[d]) : 0.0;
    g[d] = 0.0;
  }
  double y = 0.0;
  mix_gauss_accumulate<DP, GRAD, 64>(mg, xs, lane, y, g);
  y = fm::wave_sum_dpp(y);
  if (GRAD) {
    const double s = a.log_flag ? -1.0 / y : -1.0;
#pragma unroll
    for (int d = 0; d < DP; ++d)
      if (d < D) {
        const double gd = fm::wave_sum_dpp(g[d]);
        if (lane == 0) a.dy[i * D + d] = s * gd * ilam[d];
      }
  }
  if (lane == 0) a.y[i] = a.log_flag ? ((y == 0.0) ? -INFINITY : log(y)) : y;
}

// below this many points the thread-per-point kernel cannot fill the GPU (256 CUs x 2048 lanes)
constexpr int64_t kWavePerPointMax = 1 << 16;

template <int DP>
void launch_dp(vbmc_ctx* ctx, const PdfArgs& a) {
  if (a.mode == 0 && a.n <= kWavePerPointMax) {
    const dim3 grid((unsigned)((a.n + 3) / 4)), block(256);
    if (a.grad_flag) hipLaunchKernelGGL((mixture_pdf_wave_kernel<DP, true>), grid, block, 0, ctx->stream, a);
    else hipLaunchKernelGGL((mixture_pdf_wave_kernel<DP, false>), grid, block, 0, ctx->stream, a);
    return;
  }
  const dim3 grid((unsigned)((a.n + 255) / 256)), block(256);
  if (a.mode == 0) {
    if (a.grad_flag) hipLaunchKernelGGL((mixture_pdf_kernel<DP, 0, true>), grid, block, 0, ctx->stream, a);
    else hipLaunchKernelGGL((mixture_pdf_kernel<DP, 0, false>), grid, block, 0, ctx->stream, a);
  } else if (a.mode == 1) {
    hipLaunchKernelGGL((mixture_pdf_kernel<DP, 1, false>), grid, block, 0, ctx->stream, a);
  } else {
    hipLaunchKernelGGL((mixture_pdf_kernel<DP, 2, false>), grid, block, 0, ctx->stream, a);
  }
}

// Fill PdfArgs and dispatch on the padded width: the one launch path of both entry points below.
int launch_pdf(vbmc_ctx* ctx, const double* d_pack, const MixLayout& ml, const double* lambd, int64_t n,
               const double* d_x, int log_flag, int grad_flag, double df, double* d_y, double* d_dy, bool timed) {
  const int D = ml.D;
  if (D > 32) return vbmc_fail(ctx, VBMC_E_UNSUP, "mixture_pdf: D=%d > 32 not supported", D);
  PdfArgs a;
  a.mix = d_pack;
  a.ml = ml;
  a.x = d_x;
  a.n = n;
  a.log_flag = log_flag;
  a.grad_flag = grad_flag;
  a.y = d_y;
  a.dy = d_dy;
  a.df = std::fabs(df);
  a.nf = 0.0;
  a.mode = 0;
  if (std::isfinite(df) && df != 0.0) {
    double prod_lam = 1.0;
    for (int d = 0; d < D; ++d) prod_lam *= lambd[d];
    if (df > 0.0) {
      a.mode = 1;
      a.nf = std::exp(std::lgamma(0.5 * (df + D)) - std::lgamma(0.5 * df)) /
             std::pow(df * M_PI, 0.5 * D) / prod_lam;
    } else {
      a.mode = 2;
      const double ad = -df;
      a.nf = std::pow(std::exp(std::lgamma(0.5 * (ad + 1.0)) - std::lgamma(0.5 * ad)) /
                          std::sqrt(ad * M_PI),
                      (double)D) /
             prod_lam;
    }
  }
  int rc = 0;
  if (timed && (rc = timing_begin(ctx, T_PDF))) return rc;
#define CALL(DP) launch_dp<DP>(ctx, a)
  VBMC_DISPATCH_DP(D, CALL);
#undef CALL
  if (timed && (rc = timing_end(ctx, T_PDF))) return rc;
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

// the argument checks that vbmc_mixture_pdf and vbmc_mixture_pdf_orig share
int pdf_check(vbmc_ctx* ctx, const char* who, int64_t n, const double* x_nxD, int grad_flag, double df,
              const double* y_n, const double* dy_nxD) {
  if (!ctx || (n > 0 && (!x_nxD || !y_n))) return VBMC_E_ARG;
  if (!ctx->mix_set) return vbmc_fail(ctx, VBMC_E_ARG, "%s: mixture not set", who);
  if (grad_flag && !dy_nxD) return vbmc_fail(ctx, VBMC_E_ARG, "%s: grad_flag without dy", who);
  if (grad_flag && std::isfinite(df) && df != 0.0)
    return vbmc_fail(ctx, VBMC_E_UNSUP, "Gradient of heavy-tailed pdf not supported yet.");
  return 0;
}

// Host points through the density, in batches.  With a transformer `t` (original space) each batch goes x -> u and
// log|J| first and has the Jacobian divided out afterwards; without one nothing of that is allocated or launched.
int mixture_pdf_impl(vbmc_ctx* ctx, int64_t n, const double* x_nxD, int log_flag, int grad_flag, double df,
                     double* y_n, double* dy_nxD, const XfView* t) {
  if (n == 0) return VBMC_OK;
  NEED_DEVICE(ctx);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int D = ctx->D;
  // batch so that scratch stays bounded (x [u in place], y, [log|J|, inside], dy)
  const int64_t BATCH = 1 << 22;
  const int64_t nb = n < BATCH ? n : BATCH;
  Scratch sc;
  const auto p_x = sc.add((size_t)nb * D), p_y = sc.add((size_t)nb);
  const auto p_lj = sc.add(t ? (size_t)nb : 0), p_in = sc.add(t ? (size_t)nb : 0), p_dy = sc.add(grad_flag ? (size_t)nb * D : 0);
  int rc = reserve(ctx, sc);
  if (rc) return rc;
  double *d_x = sc.ptr(p_x), *d_y = sc.ptr(p_y), *d_lj = sc.ptr(p_lj), *d_in = sc.ptr(p_in), *d_dy = sc.ptr(p_dy);
  for (int64_t o = 0; o < n; o += nb) {
    const int64_t m = (n - o) < nb ? (n - o) : nb;
    HIP_TRY(ctx, hipMemcpyAsync(d_x, x_nxD + o * D, sizeof(double) * m * D, hipMemcpyHostToDevice,
                                ctx->stream));
    if (t && (rc = launch_xf_prep(ctx, *t, m, d_x, d_x, d_lj, d_in))) return rc;
    rc = launch_mixture_pdf(ctx, m, d_x, log_flag, grad_flag, df, d_y, grad_flag ? d_dy : nullptr);
    if (rc) return rc;
    if (t && (rc = launch_xf_finish(ctx, m, log_flag, d_lj, d_in, d_y))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(y_n + o, d_y, sizeof(double) * m, hipMemcpyDeviceToHost, ctx->stream));
    if (grad_flag)
      HIP_TRY(ctx, hipMemcpyAsync(dy_nxD + o * D, d_dy, sizeof(double) * m * D,
                                  hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, stream_wait(ctx));
  }
  return VBMC_OK;
}

}  // namespace

int launch_mixture_pdf(vbmc_ctx* ctx, int64_t n, const double* d_x, int log_flag, int grad_flag,
                       double df, double* d_y, double* d_dy) {
  return launch_pdf(ctx, ctx->d_mix, ctx->ml, ctx->lambd.data(), n, d_x, log_flag, grad_flag, df, d_y, d_dy, true);
}

// Gaussian-mode density of an arbitrary mixture pack (not necessarily the ctx mixture) at
// device points: used by the Monte-Carlo KL divergence, which needs two mixtures at once.
int launch_mixture_pdf_on(vbmc_ctx* ctx, const double* d_pack, const MixLayout& ml, int64_t n,
                          const double* d_x, int log_flag, double* d_y) {
  return launch_pdf(ctx, d_pack, ml, nullptr, n, d_x, log_flag, 0, 0.0, d_y, nullptr, false);
}

extern "C" int vbmc_mixture_pdf(vbmc_ctx* ctx, int64_t n, const double* x_nxD, int log_flag,
                                int grad_flag, double df, double* y_n, double* dy_nxD) {
  const int rc = pdf_check(ctx, "mixture_pdf", n, x_nxD, grad_flag, df, y_n, dy_nxD);
  if (rc) return rc;
  return mixture_pdf_impl(ctx, n, x_nxD, log_flag, grad_flag, df, y_n, dy_nxD, nullptr);
}

// pdf(orig_flag=True) (:429-439 / :543-559): bound mask, transform, density, Jacobian, on device-resident points
extern "C" int vbmc_mixture_pdf_orig(vbmc_ctx* ctx, int64_t n, const double* x_nxD, int log_flag, int grad_flag,
                                     double df, double* y_n, double* dy_nxD) {
  int rc = pdf_check(ctx, "mixture_pdf_orig", n, x_nxD, grad_flag, df, y_n, dy_nxD);
  if (rc) return rc;
  if (grad_flag && log_flag)
    return vbmc_fail(ctx, VBMC_E_UNSUP,
                     "vbmc_pdf:NoOriginalGrad: Gradient computation in original space not supported yet.");
  XfView t;
  rc = xf_need(ctx, 0, ctx->D, "mixture_pdf_orig", t);
  if (rc) return rc;
  return mixture_pdf_impl(ctx, n, x_nxD, log_flag, grad_flag, df, y_n, dy_nxD, &t);
}
