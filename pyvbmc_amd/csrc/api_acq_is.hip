// The two importance-sampled acquisition functions for noisy targets, AcqFcnVIQR and AcqFcnIMIQR:
//   acquisition_functions/acq_fcn_viqr.py:30-160, acq_fcn_imiqr.py:29-177
// (the classes AbstractAcqFcn.__call__ dispatches to when the target's evaluations are noisy --
// BASELINE config 5).  Per GP hyper-parameter sample s, with Xa the importance points the
// reference prepared (vbmc/active_importance_sampling.py) and C_tmp[s] = (K+Sigma)^-1 K(X, Xa)
// (or L K(X, Xa) for a non-Cholesky sample) formed there once (:262-306):
//     C      = K(Xs, Xa) -/+ K(Xs, X) C_tmp[s]                 posterior cross-covariance
//     tau2   = C^2 / (f_s2(Xs) + sn2(Xs))
//     s_pred = sqrt(max(f_s2(Xa) - tau2, 0))
//     zz     = ln_w[s] + u s_pred + log1p(-exp(-2 u s_pred))     (ln_w = 0 for VIQR)
//     acq_s  = logsumexp_a zz ,     acq = logsumexp_s acq_s - log S
// The importance state (Xa, C_tmp, f_s2(Xa), ln_w) is uploaded once per active-sampling round
// (vbmc_acq_is_set) and stays in HBM while CMA-ES calls vbmc_acq_is_eval thousands of times.
// Kernels: the predictive variance at Xs through the predict launches of gp.hip; K(Xs, X) by direct
// differences; the M x N x Na product on the FP64 matrix cores; one wave per (point, sample) for
// the cross-kernel K(Xs, Xa), the integrand and its log-sum-exp.
// vbmc_acq_is_build forms the same state on the device from Xa alone (step 3 of active_importance_sampling,
// :264-308): K_Xa_X[s] by direct differences and C_tmp[s] as two panel products against the resident L^-1
// (L^-1 (K_Xa_X L^-1)^T / sn2_eff, the intermediate transposed in between) or one against L.
#include <cmath>
#include <cstring>

#include "common.h"
#include "fastmath.h"
#include "gp_dev.h"

namespace {

struct IsState {
  int64_t Na = 0;
  int S = 0, N = 0, D = 0, per_sample = 0, has_lnw = 0;
  double* d = nullptr;  // [Xa (S or 1) x Na x D | Ctmp S x N x Na | fs2a S x Na | lnw S x Na]
  size_t cap = 0;
  size_t o_C = 0, o_f = 0, o_w = 0;
};

// K[m][n] = sf2 exp(-1/2 sum_d ((a_md - b_nd)/ell_d)^2), direct differences
__global__ __launch_bounds__(256) void se_cross_kernel(const double* __restrict__ A, int64_t M,
                                                       const double* __restrict__ B, int NB, int D,
                                                       const double* __restrict__ hyp, double* __restrict__ K) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= M * NB) return;
  const int64_t m = idx / NB;
  const int n = (int)(idx - m * NB);
  K[idx] = se_ard_direct(A + m * D, B + (size_t)n * D, D, [&](int d) { return exp(-hyp[d]); }, 2.0 * hyp[D]);
}

// One wave per point m: acq_s[m] = logsumexp_a zz(m, a) for GP sample s.
__global__ __launch_bounds__(256) void is_reduce_kernel(const double* __restrict__ xs, int64_t M, int D,
                                                        const double* __restrict__ Xa, int64_t Na,
                                                        const double* __restrict__ hyp,
                                                        const double* __restrict__ T,      // M x Na
                                                        const double* __restrict__ fs2,    // M   (f_s2 at Xs, this sample)
                                                        const double* __restrict__ sn2,    // M
                                                        const double* __restrict__ fs2a,   // Na  (f_s2 at Xa, this sample)
                                                        const double* __restrict__ lnw,    // Na or null
                                                        int chol, double u, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t m = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (m >= M) return;
  const double iy = 1.0 / (fs2[m] + sn2[m]);
  const double lsf2 = 2.0 * hyp[D];
  double mx = -INFINITY, sm = 0.0;  // per-lane running log-sum-exp
  bool bad = false;
  for (int64_t a = lane; a < Na; a += 64) {
    double d2 = 0.0;
    for (int d = 0; d < D; ++d) {
      const double t = (xs[m * D + d] - Xa[a * D + d]) * exp(-hyp[d]);
      d2 = fma(t, t, d2);
    }
    const double kxa = exp(lsf2 - 0.5 * d2);
    const double t = T[(size_t)m * Na + a];
    const double c = chol ? kxa - t : kxa + t;
    const double tau2 = c * c * iy;
    const double sp = sqrt(fmax(fs2a[a] - tau2, 0.0));
    double zz = u * sp + log1p(-exp(-2.0 * u * sp));
    if (lnw) zz += lnw[a];
    bad |= zz != zz;  // a NaN integrand (NaN f_s2, C_tmp, sn2 ...) makes the reference's logsumexp NaN: so here
    if (zz > -INFINITY) {
      if (zz > mx) {
        sm = sm * exp(mx - zz) + 1.0;
        mx = zz;
      } else {
        sm += exp(zz - mx);
      }
    }
  }
  // combine the 64 lanes
  double gm = mx;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) gm = fmax(gm, __shfl_xor(gm, off, 64));
  double part = (mx > -INFINITY && gm < INFINITY) ? sm * exp(mx - gm) : 0.0;
  part = fm::wave_sum_dpp(part);
  const bool any_bad = __any(bad ? 1 : 0) != 0;
  if (lane == 0)
    out[m] = any_bad ? (double)NAN : gm == INFINITY ? (double)INFINITY : (gm > -INFINITY) ? gm + log(part) : -INFINITY;
}

// acq[m] = logsumexp_s acq_s[s][m] - log S   (acq_fcn_viqr.py:152-158)
// var_tot[m] = mean_s f_s2 + var_s(f_mu, ddof = 1) (abstract_acq_fcn.py:82-97), for the caller's
// variance regularisation
__global__ void is_combine_kernel(const double* __restrict__ acq_s, int S, int64_t M, int64_t ld,
                                  double* __restrict__ acq, const double* __restrict__ fmu,
                                  const double* __restrict__ fs2, double* __restrict__ var_tot) {
  const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  double f_bar;
  gp_sample_moments(fmu, fs2, S, ld, m, f_bar, var_tot[m]);
  if (S == 1) {
    acq[m] = acq_s[m];
    return;
  }
  double mx = -INFINITY;
  for (int s = 0; s < S; ++s) mx = fmax(mx, acq_s[(size_t)s * ld + m]);
  if (!(mx > -INFINITY)) mx = 0.0;  // avoid -inf + inf
  double sum = 0.0;
  for (int s = 0; s < S; ++s) sum += exp(acq_s[(size_t)s * ld + m] - mx);
  acq[m] = mx + log(sum / S);
}

// B[c][r] = A[r][c] / div, A (R x C) row-major: the orientation the second factor of C_tmp needs
__global__ __launch_bounds__(256) void transpose_div_kernel(const double* __restrict__ A, int64_t R, int C, double div,
                                                            double* __restrict__ B) {
  __shared__ double t[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const int64_t r0 = (int64_t)blockIdx.y * 32;
  const int c0 = blockIdx.x * 32;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t r = r0 + ty + 8 * k;
    const int c = c0 + tx;
    t[ty + 8 * k][tx] = (r < R && c < C) ? A[(size_t)r * C + c] : 0.0;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = c0 + ty + 8 * k;
    const int64_t r = r0 + tx;
    if (r < R && c < C) B[(size_t)c * R + r] = t[tx][ty + 8 * k] / div;
  }
}

IsState* is_of(vbmc_ctx* ctx) {
  if (!ctx->acq_is) ctx->acq_is = new IsState();
  return (IsState*)ctx->acq_is;
}

// the state's allocation and layout for Na importance points of the context's GP
int is_reserve(vbmc_ctx* ctx, IsState* st, int64_t Na, int per_sample_xa, bool has_lnw) {
  const GpState& g = ctx->gp;
  const int S = g.S, N = g.N, D = g.D;
  const size_t n_xa = (size_t)(per_sample_xa ? S : 1) * Na * D, n_C = (size_t)S * N * Na, n_f = (size_t)S * Na;
  const size_t need = n_xa + n_C + 2 * n_f;
  HIP_TRY(ctx, stream_wait(ctx));
  if (st->cap < need) {
    if (st->d) HIP_TRY(ctx, hipFree(st->d));
    st->d = nullptr;
    st->cap = 0;
    HIP_TRY(ctx, hipMalloc((void**)&st->d, sizeof(double) * (need + need / 8)));
    st->cap = need + need / 8;
  }
  st->Na = Na; st->S = S; st->N = N; st->D = D; st->per_sample = per_sample_xa ? 1 : 0;
  st->has_lnw = has_lnw ? 1 : 0;
  st->o_C = n_xa; st->o_f = n_xa + n_C; st->o_w = st->o_f + n_f;
  return 0;
}

// Xa, f_s2 at Xa (arrives (Na, S) as the reference stores it; kept [S][Na]) and ln_weights into the state
int is_upload_small(vbmc_ctx* ctx, IsState* st, const double* Xa, const double* fs2a_NaxS, const double* lnw_SxNa) {
  const int S = st->S;
  const int64_t Na = st->Na;
  const size_t n_f = (size_t)S * Na;
  HIP_TRY(ctx, hipMemcpyAsync(st->d, Xa, sizeof(double) * st->o_C, hipMemcpyHostToDevice, ctx->stream));
  std::vector<double> ft(n_f);
  for (int64_t a = 0; a < Na; ++a)
    for (int s = 0; s < S; ++s) ft[(size_t)s * Na + a] = fs2a_NaxS[(size_t)a * S + s];
  HIP_TRY(ctx, hipMemcpyAsync(st->d + st->o_f, ft.data(), sizeof(double) * n_f, hipMemcpyHostToDevice, ctx->stream));
  if (lnw_SxNa)
    HIP_TRY(ctx, hipMemcpyAsync(st->d + st->o_w, lnw_SxNa, sizeof(double) * n_f, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, stream_wait(ctx));  // (ft is a local; the caller's arrays are pageable)
  return 0;
}

}  // namespace

void acq_is_free(vbmc_ctx* ctx) {
  IsState* st = (IsState*)ctx->acq_is;
  if (!st) return;
  if (st->d) (void)hipFree(st->d);
  delete st;
  ctx->acq_is = nullptr;
}

extern "C" int vbmc_acq_is_set(vbmc_ctx* ctx, int64_t Na, const double* Xa, int per_sample_xa,
                               const double* Ctmp_SxNxNa, const double* fs2a_NaxS,
                               const double* lnw_SxNa) {
  if (!ctx || Na < 1 || !Xa || !Ctmp_SxNxNa || !fs2a_NaxS) return VBMC_E_ARG;
  NEED_DEVICE(ctx);
  if (!ctx->gp.set) return vbmc_fail(ctx, VBMC_E_ARG, "acq_is_set: GP not set");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  IsState* st = is_of(ctx);
  int rc = is_reserve(ctx, st, Na, per_sample_xa, lnw_SxNa != nullptr);
  if (rc) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(st->d + st->o_C, Ctmp_SxNxNa, sizeof(double) * (st->o_f - st->o_C), hipMemcpyHostToDevice,
                              ctx->stream));
  if ((rc = is_upload_small(ctx, st, Xa, fs2a_NaxS, lnw_SxNa))) return rc;
  return VBMC_OK;
}

// Step 3 of active_importance_sampling (vbmc/active_importance_sampling.py:264-308) on the device.
extern "C" int vbmc_acq_is_build(vbmc_ctx* ctx, int64_t Na, const double* Xa, int per_sample_xa,
                                 const double* fs2a_NaxS, const double* lnw_SxNa, double* K_out_SxNaxN,
                                 double* C_out_SxNxNa) {
  if (!ctx || Na < 1 || !Xa || !fs2a_NaxS) return VBMC_E_ARG;
  NEED_DEVICE(ctx);
  if (!ctx->gp.set) return vbmc_fail(ctx, VBMC_E_ARG, "acq_is_build: GP not set");
  const GpState& g = ctx->gp;
  const int S = g.S, N = g.N, D = g.D;
  if (D > 32) return vbmc_fail(ctx, VBMC_E_UNSUP, "acq_is_build: D=%d > 32 not supported", D);
  // (Na / 32 and Na / 64 are grid.y of the transpose and of the panel product: below 65536)
  if (Na > ((int64_t)1 << 20) || (int64_t)N * Na > ((int64_t)1 << 31) - 1)
    return vbmc_fail(ctx, VBMC_E_UNSUP, "acq_is_build: Na=%lld importance points with N=%d not supported", (long long)Na, N);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  IsState* st = is_of(ctx);
  int rc = is_reserve(ctx, st, Na, per_sample_xa, lnw_SxNa != nullptr);
  if (rc) return rc;
  const size_t nk = (size_t)Na * N;
  Scratch sc;
  const auto p_K = sc.add(nk), p_T = sc.add(nk), p_TT = sc.add(nk);
  if ((rc = reserve(ctx, sc))) return rc;
  if ((rc = is_upload_small(ctx, st, Xa, fs2a_NaxS, lnw_SxNa))) return rc;
  double *d_K = sc.ptr(p_K), *d_T = sc.ptr(p_T), *d_TT = sc.ptr(p_TT);
  const dim3 tgrid((unsigned)((N + 31) / 32), (unsigned)((Na + 31) / 32));
  for (int s = 0; s < S; ++s) {
    const double* hyp = g.d_hyp + (size_t)s * g.P;
    const double* d_Xa = st->d + (st->per_sample ? (size_t)s * Na * D : 0);
    double* d_C = st->d + st->o_C + (size_t)s * N * Na;
    hipLaunchKernelGGL(se_cross_kernel, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, ctx->stream, d_Xa, Na,
                       (const double*)g.d_X, N, D, hyp, d_K);
    if (g.L_chol[s]) {
      // (L'L)^-1 K(X, Xa) / sn2_eff = L^-1 (K_Xa_X L^-1)^T / sn2_eff   (:294-304)
      if ((rc = launch_gp_panel_product(ctx, d_K, g.d_Linv + (size_t)s * N * N, d_T, Na, N, N, true))) return rc;
      hipLaunchKernelGGL(transpose_div_kernel, tgrid, dim3(256), 0, ctx->stream, (const double*)d_T, Na, N, g.sn2_eff[s],
                         d_TT);
      if ((rc = launch_gp_panel_product(ctx, g.d_Linv + (size_t)s * N * N, d_TT, d_C, N, N, (int)Na))) return rc;
    } else {
      // L K(X, Xa)   (:306)
      hipLaunchKernelGGL(transpose_div_kernel, tgrid, dim3(256), 0, ctx->stream, (const double*)d_K, Na, N, 1.0, d_TT);
      if ((rc = launch_gp_panel_product(ctx, g.d_L + (size_t)s * N * N, d_TT, d_C, N, N, (int)Na))) return rc;
    }
    HIP_TRY(ctx, hipGetLastError());
    // (the copies wait for the stream: d_K is reused by the next sample, whose kernels start behind this download)
    if (K_out_SxNaxN && (rc = download_chunked(ctx, d_K, K_out_SxNaxN + (size_t)s * nk, nk))) return rc;
    if (C_out_SxNxNa && (rc = download_chunked(ctx, d_C, C_out_SxNxNa + (size_t)s * nk, nk))) return rc;
  }
  HIP_TRY(ctx, stream_wait(ctx));
  return VBMC_OK;
}

int acq_is_need(vbmc_ctx* ctx, const char* who, int64_t* Na) {
  const IsState* st = (const IsState*)ctx->acq_is;
  const GpState& g = ctx->gp;
  if (!st || !st->d || st->S != g.S || st->N != g.N || st->D != g.D)
    return vbmc_fail(ctx, VBMC_E_ARG, "%s: importance state not set for this GP (vbmc_acq_is_set)", who);
  *Na = st->Na;
  return 0;
}

int launch_acq_is(vbmc_ctx* ctx, const PredictPlan& p, int64_t m, const double* d_xs, const double* d_sn2, double u,
                  double* d_Kx, double* d_T, double* d_as, double* d_res) {
  const IsState* st = (const IsState*)ctx->acq_is;
  const GpState& g = ctx->gp;
  const int N = g.N, D = g.D, S = g.S;
  const int64_t Na = st->Na, mb = p.mb;
  int rc = launch_gp_predict_all(ctx, m, d_xs, p.Ks, p.part, 0, p.fmu, p.fs2, mb);  // f_s2 at Xs, every sample
  if (rc) return rc;
  for (int s = 0; s < S; ++s) {
    const double* hyp = g.d_hyp + (size_t)s * g.P;
    hipLaunchKernelGGL(se_cross_kernel, dim3((unsigned)((m * N + 255) / 256)), dim3(256), 0, ctx->stream, d_xs, m,
                       (const double*)g.d_X, N, D, hyp, d_Kx);
    rc = launch_gp_panel_product(ctx, d_Kx, st->d + st->o_C + (size_t)s * N * Na, d_T, m, N, (int)Na);
    if (rc) return rc;
    const double* Xa = st->d + (st->per_sample ? (size_t)s * Na * D : 0);
    hipLaunchKernelGGL(is_reduce_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, ctx->stream, d_xs, m, D, Xa, Na, hyp,
                       (const double*)d_T, (const double*)(p.fs2 + (size_t)s * mb), d_sn2,
                       (const double*)(st->d + st->o_f + (size_t)s * Na),
                       st->has_lnw ? (const double*)(st->d + st->o_w + (size_t)s * Na) : (const double*)nullptr,
                       g.L_chol[s] ? 1 : 0, u, d_as + (size_t)s * mb);
  }
  hipLaunchKernelGGL(is_combine_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, ctx->stream, (const double*)d_as, S,
                     m, mb, d_res, (const double*)p.fmu, (const double*)p.fs2, d_res + mb);
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

extern "C" int vbmc_acq_is_eval(vbmc_ctx* ctx, int64_t M, const double* xs_MxD, const double* sn2_M,
                                double u, double* acq_M, double* var_tot_M) {
  if (!ctx || (M > 0 && (!xs_MxD || !sn2_M || !acq_M))) return VBMC_E_ARG;
  NEED_DEVICE(ctx);
  if (!ctx->gp.set) return vbmc_fail(ctx, VBMC_E_ARG, "acq_is_eval: GP not set");
  int64_t Na = 0;
  int rc = acq_is_need(ctx, "acq_is_eval", &Na);
  if (rc) return rc;
  if (M == 0) return VBMC_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const GpState& g = ctx->gp;
  const int N = g.N, D = g.D, S = g.S;
  if (D > 32) return vbmc_fail(ctx, VBMC_E_UNSUP, "acq_is_eval: D=%d > 32 not supported", D);
  // its own pieces: sn2 | Kx (mb x N) | T (mb x Na) | acq_s [S] | acq, var_tot (one piece, mb apart)
  PredictPlan p;
  predict_plan(ctx, M, (int64_t)1 << 26, (int64_t)S * N + N + Na, 16384, p);
  const int64_t mb = p.mb;
  const auto p_sn2 = p.sc.add((size_t)mb), p_Kx = p.sc.add((size_t)mb * N), p_T = p.sc.add((size_t)mb * Na);
  const auto p_as = p.sc.add((size_t)S * mb), p_acq = p.sc.add(2 * (size_t)mb);
  if ((rc = predict_reserve(ctx, p, 2))) return rc;
  double* d_xs = p.xs;
  double *d_sn2 = p.sc.ptr(p_sn2), *d_Kx = p.sc.ptr(p_Kx), *d_T = p.sc.ptr(p_T), *d_as = p.sc.ptr(p_as), *d_acq = p.sc.ptr(p_acq);
  const double* const res_src[2] = {d_acq, d_acq + mb};
  double* const res_dst[2] = {acq_M, var_tot_M};
  for (int64_t o = 0; o < M; o += mb) {
    const int64_t m = (M - o) < mb ? (M - o) : mb;
    HIP_TRY(ctx, hipMemcpyAsync(d_xs, xs_MxD + o * D, sizeof(double) * m * D, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_sn2, sn2_M + o, sizeof(double) * m, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = launch_acq_is(ctx, p, m, d_xs, d_sn2, u, d_Kx, d_T, d_as, d_acq))) return rc;
    if ((rc = fetch_vectors(ctx, 2, res_src, res_dst, (size_t)m, (size_t)mb, (size_t)o))) return rc;
  }
  return VBMC_OK;
}

// Step 2 of active_importance_sampling (vbmc/active_importance_sampling.py:195-262): the S chains in one launch
// (acq_is_mcmc.hip).  Scratch: [x0 S x D | widths | lb | ub] uploaded, [X | logp | fmu | fs2 | stats | invalid] downloaded.
extern "C" int vbmc_is_mcmc(vbmc_ctx* ctx, int ln_y_fmu, double u_q, const double* x0_SxD, const double* widths_D,
                            const double* lb_D, const double* ub_D, int n, int thin, int burn_in, uint64_t seed,
                            double* X_SxnxD, double* logp_Sxn, double* fmu_nxS, double* fs2_nxS, int64_t* stats_Sx4,
                            int* invalid) {
  if (!ctx || !x0_SxD || !widths_D || !lb_D || !ub_D || !X_SxnxD || !logp_Sxn || !fmu_nxS || !fs2_nxS || !stats_Sx4 ||
      !invalid || n < 1 || thin < 1 || burn_in < 0)
    return VBMC_E_ARG;
  NEED_DEVICE(ctx);
  if (!ctx->gp.set) return vbmc_fail(ctx, VBMC_E_ARG, "is_mcmc: GP not set");
  const GpState& g = ctx->gp;
  const int S = g.S, N = g.N, D = g.D;
  if (D > 32) return vbmc_fail(ctx, VBMC_E_UNSUP, "is_mcmc: D=%d > 32 not supported", D);
  if (is_mcmc_lds_bytes(N, ctx->opt_is_mcmc_threads) > 156 * 1024)
    return vbmc_fail(ctx, VBMC_E_UNSUP, "is_mcmc: N=%d training points do not fit a chain's LDS", N);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t n_in = (size_t)S * D + 3 * (size_t)D, n_x = (size_t)S * n * D, n_sn = (size_t)S * n;
  Scratch sc;
  const auto p_in = sc.add(n_in), p_X = sc.add(n_x), p_logp = sc.add(n_sn), p_fmu = sc.add(n_sn), p_fs2 = sc.add(n_sn);
  const auto p_stats = sc.add<long long>(4 * (size_t)S);
  const auto p_inv = sc.add<int>((size_t)S);
  const size_t n_out = sc.total - p_X.off;  // everything from X on comes back in one copy
  int rc = reserve(ctx, sc);
  if (rc) return rc;
  if ((rc = ensure_pinned(ctx, n_out))) return rc;
  std::vector<double> in(n_in);
  memcpy(in.data(), x0_SxD, sizeof(double) * S * D);
  memcpy(in.data() + (size_t)S * D, widths_D, sizeof(double) * D);
  memcpy(in.data() + (size_t)S * D + D, lb_D, sizeof(double) * D);
  memcpy(in.data() + (size_t)S * D + 2 * D, ub_D, sizeof(double) * D);
  double *d_in = sc.ptr(p_in), *d_X = sc.ptr(p_X), *d_logp = sc.ptr(p_logp), *d_fmu = sc.ptr(p_fmu), *d_fs2 = sc.ptr(p_fs2);
  long long* d_stats = sc.ptr(p_stats);
  int* d_inv = sc.ptr(p_inv);
  HIP_TRY(ctx, hipMemcpyAsync(d_in, in.data(), sizeof(double) * n_in, hipMemcpyHostToDevice, ctx->stream));
  // (a chain whose start is invalid writes nothing: its rows come back as zeros)
  HIP_TRY(ctx, hipMemsetAsync(d_X, 0, sizeof(double) * n_out, ctx->stream));
  if ((rc = timing_begin(ctx, T_IS_MCMC))) return rc;
  rc = launch_is_mcmc(ctx, ln_y_fmu ? 1 : 0, u_q, d_in, d_in + (size_t)S * D, d_in + (size_t)S * D + D,
                      d_in + (size_t)S * D + 2 * D, n, thin, burn_in, seed, d_X, d_logp, d_fmu, d_fs2, d_stats, d_inv);
  if (rc) return rc;
  if ((rc = timing_end(ctx, T_IS_MCMC))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_pinned, d_X, sizeof(double) * n_out, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, stream_wait(ctx));  // (`in` is a local)
  const double* h = ctx->h_pinned;  // (the pinned copy keeps the pieces' spacing)
  const size_t o0 = p_X.off;
  memcpy(X_SxnxD, h, sizeof(double) * n_x);
  memcpy(logp_Sxn, h + (p_logp.off - o0), sizeof(double) * n_sn);
  memcpy(fmu_nxS, h + (p_fmu.off - o0), sizeof(double) * n_sn);
  memcpy(fs2_nxS, h + (p_fs2.off - o0), sizeof(double) * n_sn);
  memcpy(stats_Sx4, h + (p_stats.off - o0), sizeof(int64_t) * 4 * S);
  const int* h_inv = (const int*)(h + (p_inv.off - o0));
  *invalid = 0;
  for (int s = 0; s < S; ++s) *invalid |= h_inv[s] != 0;
  return VBMC_OK;
}
