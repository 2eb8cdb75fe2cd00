// Preparing the importance state of AcqFcnVIQR / AcqFcnIMIQR: the proposal weights and the box-uniform draws of
//   vbmc/active_importance_sampling.py:116-191 (step 1) and :317-390 (active_sample_proposal_pdf).
// For Na proposal points x_a and the GP of vbmc_set_gp (S hyper-parameter samples, N training points X):
//     f_mu, f_s2        = gp.predict(x_a, separate_samples=True)                        (:351)
//     t_0(a)            = log q_is(x_a) + log w_vp      q_is the smoothed posterior      (:361-366)
//     t_i(a), i = 1..N  = log((1 - w_vp) / VV / N) where |x_a - X_i| < rect_delta in every dimension, else -inf,
//                         VV = prod(2 rect_delta)                                       (:372-378)
//     l_pdf(a)          = logsumexp_i t_i(a), shifted by the row maximum               (:380-386)
//     ln_w(a, s)        = ln_y(a, s) - l_pdf(a),  ln_y = 0 (VIQR) or f_mu (IMIQR)        (:369, :386-388)
// The N box terms of a point all have the same value, so the point only counts its hits.  One wave per point: the lanes
// share the components of q_is (mixture_dev.h) and then the training points.  The predictive moments come from the predict
// launches of gp.hip.  The box-uniform proposals themselves (:164-168) have a Philox stream of their own (sample.hip
// lists the streams).
#include <cmath>
#include <cstring>

#include "common.h"
#include "fastmath.h"
#include "gp_dev.h"
#include "mixture_dev.h"

namespace {

struct PropArgs {
  const double* mix;  // pack of q_is (has_vp)
  MixLayout ml;
  const double* x;  // n x D
  int64_t n;
  const double* X;  // N x D
  int N, D, S;
  const double* rect;  // D (has_box)
  int has_vp, has_box, ln_y_fmu;
  double log_wvp, log_box;
  const double *fmu, *fs2;  // [S][ld]
  int64_t ld;
  double *lnw, *fs2_out;  // n x S
  int* invalid;
};

template <int DP>
__global__ __launch_bounds__(256) void is_proposal_kernel(PropArgs a) {
  const int D = a.D;
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= a.n) return;
  const MixGauss mg = mix_gauss(a.mix, a.ml);  // (without has_vp: addresses only, never read -- every use is guarded)
  double x[DP], xs[DP], g[DP];
#pragma unroll
  for (int d = 0; d < DP; ++d) {
    x[d] = (d < D) ? a.x[i * D + d] : 0.0;
    xs[d] = (a.has_vp && d < D) ? scaled_coord<false>(x[d], a.mix[a.ml.o_ilam + d]) : 0.0;
    g[d] = 0.0;
  }
  double t0 = -INFINITY;
  if (a.has_vp) {
    double y = 0.0;
    mix_gauss_accumulate<DP, false, 64>(mg, xs, lane, y, g);
    y = fm::wave_sum_dpp(y);
    t0 = ((y == 0.0) ? -INFINITY : log(y)) + a.log_wvp;
  }
  double l = t0;
  if (a.has_box) {
    double cnt = 0.0;
    for (int n = lane; n < a.N; n += 64) {
      bool in = true;
#pragma unroll
      for (int d = 0; d < DP; ++d)
        if (d < D) in = in && (fabs(x[d] - a.X[(size_t)n * D + d]) < a.rect[d]);
      cnt += in ? 1.0 : 0.0;
    }
    cnt = fm::wave_sum_dpp(cnt);  // (whole numbers: exact)
    const double tb = cnt > 0.0 ? a.log_box : -INFINITY;
    const double m = t0 > tb ? t0 : tb;
    if (t0 != t0) {
      l = t0;  // a NaN density stays NaN, as np.amax keeps it
    } else if (m == -INFINITY) {
      l = NAN;
      if (lane == 0) atomicOr(a.invalid, 1);
    } else {
      const double e0 = t0 > -INFINITY ? exp(t0 - m) : 0.0;
      const double eb = cnt > 0.0 ? cnt * exp(a.log_box - m) : 0.0;
      l = log(e0 + eb) + m;
    }
  }
  for (int s = lane; s < a.S; s += 64) {
    const double ln_y = a.ln_y_fmu ? a.fmu[(size_t)s * a.ld + i] : 0.0;
    a.lnw[i * a.S + s] = ln_y - l;
    a.fs2_out[i * a.S + s] = a.fs2[(size_t)s * a.ld + i];
  }
}

// box sample n: block (n, 0, 5) picks the training point, blocks (n, 1 + p, 5) give the uniforms of dimensions 2p, 2p + 1
__global__ __launch_bounds__(256) void is_box_sample_kernel(const double* __restrict__ X, int N, int D,
                                                            const double* __restrict__ rect, int64_t n_box, uint64_t seed,
                                                            double* __restrict__ out) {
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= n_box) return;
  const Philox4 r = philox_block((uint64_t)n, 0u, 5u, seed);
  int j = (int)(philox_u53(r.x[0], r.x[1]) * (double)N);
  j = j < N - 1 ? j : N - 1;
  for (int p = 0; 2 * p < D; ++p) {
    const Philox4 q = philox_block((uint64_t)n, (uint32_t)(1 + p), 5u, seed);
    const int d0 = 2 * p, d1 = 2 * p + 1;
    out[n * D + d0] = X[(size_t)j * D + d0] + (2.0 * philox_u53(q.x[0], q.x[1]) - 1.0) * rect[d0];
    if (d1 < D) out[n * D + d1] = X[(size_t)j * D + d1] + (2.0 * philox_u53(q.x[2], q.x[3]) - 1.0) * rect[d1];
  }
}

template <int DP>
void launch_proposal_dp(vbmc_ctx* ctx, const PropArgs& a) {
  hipLaunchKernelGGL((is_proposal_kernel<DP>), dim3((unsigned)((a.n + 3) / 4)), dim3(256), 0, ctx->stream, a);
}

}  // namespace

extern "C" int vbmc_is_proposal(vbmc_ctx* ctx, int64_t Na, const double* Xa_NaxD, int K2, const double* mu2_KxD,
                                const double* sigma2_K, const double* lambd2_D, const double* w2_K, double w_vp,
                                const double* rect_delta_D, int ln_y_is_fmu, double* lnw_NaxS, double* fs2_NaxS,
                                int* invalid_out) {
  if (!ctx || Na < 0 || (Na > 0 && (!Xa_NaxD || !lnw_NaxS || !fs2_NaxS))) return VBMC_E_ARG;
  NEED_DEVICE(ctx);
  if (!ctx->gp.set) return vbmc_fail(ctx, VBMC_E_ARG, "is_proposal: GP not set");
  if (!(w_vp >= 0.0 && w_vp <= 1.0)) return vbmc_fail(ctx, VBMC_E_ARG, "is_proposal: w_vp=%g outside [0, 1]", w_vp);
  const bool has_vp = w_vp > 0.0, has_box = w_vp < 1.0;
  if (has_vp && (K2 < 1 || !mu2_KxD || !sigma2_K || !lambd2_D || !w2_K))
    return vbmc_fail(ctx, VBMC_E_ARG, "is_proposal: w_vp > 0 needs the smoothed posterior");
  if (has_box && !rect_delta_D) return vbmc_fail(ctx, VBMC_E_ARG, "is_proposal: w_vp < 1 needs rect_delta");
  if (invalid_out) *invalid_out = 0;
  const GpState& g = ctx->gp;
  const int N = g.N, D = g.D, S = g.S;
  if (D > 32) return vbmc_fail(ctx, VBMC_E_UNSUP, "is_proposal: D=%d > 32 not supported", D);
  if (Na == 0) return VBMC_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  MixLayout ml2;
  // pack of q_is | rect_delta | the invalid flag: one zeroed double slot whose first four bytes the kernel uses as the int
  // it ORs into, and the host reads the same four bytes back
  std::vector<double> fixed;
  if (has_vp) {
    const int rc = make_mixture2(ctx, "is_proposal", VBMC_E_NONFINITE, D, K2, mu2_KxD, sigma2_K, lambd2_D, w2_K, ml2, fixed);
    if (rc) return rc;
  }
  const size_t o_rect = fixed.size();
  double log_box = 0.0;
  if (has_box) {
    double VV = 1.0;
    for (int d = 0; d < D; ++d) VV *= 2.0 * rect_delta_D[d];
    log_box = std::log((1.0 - w_vp) / VV / N);
    fixed.insert(fixed.end(), rect_delta_D, rect_delta_D + D);
  }
  const size_t o_flag = fixed.size();
  fixed.push_back(0.0);
  int rc = ensure_dev(ctx, &ctx->d_out, &ctx->d_out_cap, fixed.size());
  if (rc) return rc;
  PredictPlan p;
  predict_plan(ctx, Na, (int64_t)1 << 27, (int64_t)S * N, 65536, p);
  const auto p_lnw = p.sc.add((size_t)S * p.mb), p_fs2o = p.sc.add((size_t)S * p.mb);
  rc = predict_reserve(ctx, p, 2 * (size_t)S);
  if (rc) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_out, fixed.data(), sizeof(double) * fixed.size(), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, stream_wait(ctx));  // (`fixed` is a local)
  const int64_t mb = p.mb;
  PropArgs a;
  a.mix = ctx->d_out;
  a.ml = ml2;
  a.x = p.xs;
  a.X = g.d_X;
  a.N = N; a.D = D; a.S = S;
  a.rect = ctx->d_out + o_rect;
  a.has_vp = has_vp; a.has_box = has_box; a.ln_y_fmu = ln_y_is_fmu ? 1 : 0;
  a.log_wvp = has_vp ? std::log(w_vp) : 0.0;
  a.log_box = log_box;
  a.fmu = p.fmu; a.fs2 = p.fs2; a.ld = mb;
  a.lnw = p.sc.ptr(p_lnw);
  a.fs2_out = p.sc.ptr(p_fs2o);
  a.invalid = (int*)(ctx->d_out + o_flag);
  const double* const src[2] = {a.lnw, a.fs2_out};
  double* const dst[2] = {lnw_NaxS, fs2_NaxS};
  for (int64_t o = 0; o < Na; o += mb) {
    const int64_t m = (Na - o) < mb ? (Na - o) : mb;
    HIP_TRY(ctx, hipMemcpyAsync(p.xs, Xa_NaxD + o * D, sizeof(double) * m * D, hipMemcpyHostToDevice, ctx->stream));
    rc = launch_gp_predict_all(ctx, m, p.xs, p.Ks, p.part, 0, p.fmu, p.fs2, mb);
    if (rc) return rc;
    a.n = m;
#define CALL(DP) launch_proposal_dp<DP>(ctx, a)
    VBMC_DISPATCH_DP(D, CALL);
#undef CALL
    HIP_TRY(ctx, hipGetLastError());
    if ((rc = fetch_vectors(ctx, 2, src, dst, (size_t)m * S, (size_t)S * mb, (size_t)o * S))) return rc;
  }
  int flag = 0;
  HIP_TRY(ctx, hipMemcpyAsync(&flag, a.invalid, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, stream_wait(ctx));
  if (invalid_out) *invalid_out = flag;
  return VBMC_OK;
}

extern "C" int vbmc_is_box_sample(vbmc_ctx* ctx, int64_t n_box, uint64_t seed, const double* rect_delta_D,
                                  double* x_NboxxD) {
  if (!ctx || n_box < 0 || (n_box > 0 && (!rect_delta_D || !x_NboxxD))) return VBMC_E_ARG;
  NEED_DEVICE(ctx);
  if (!ctx->gp.set) return vbmc_fail(ctx, VBMC_E_ARG, "is_box_sample: GP not set");
  const GpState& g = ctx->gp;
  const int N = g.N, D = g.D;
  if (D > 32) return vbmc_fail(ctx, VBMC_E_UNSUP, "is_box_sample: D=%d > 32 not supported", D);
  if (n_box == 0) return VBMC_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  Scratch sc;
  const auto p_x = sc.add((size_t)n_box * D), p_rect = sc.add((size_t)D);
  int rc = reserve(ctx, sc);
  if (rc) return rc;
  double *d_x = sc.ptr(p_x), *d_rect = sc.ptr(p_rect);
  HIP_TRY(ctx, hipMemcpyAsync(d_rect, rect_delta_D, sizeof(double) * D, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(is_box_sample_kernel, dim3((unsigned)((n_box + 255) / 256)), dim3(256), 0, ctx->stream,
                     (const double*)g.d_X, N, D, (const double*)d_rect, n_box, seed, d_x);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(x_NboxxD, d_x, sizeof(double) * n_box * D, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, stream_wait(ctx));
  return VBMC_OK;
}
