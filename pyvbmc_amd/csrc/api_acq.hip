// acquisition-function evaluation, and row a13 (_sq_dist).
//
// AbstractAcqFcn.__call__ (acquisition_functions/abstract_acq_fcn.py:68-147) evaluates, for a
// batch of points, gp.predict(separate_samples=True), the mean / total variance over the GP
// hyper-parameter samples, vp.pdf (or log pdf) and one of the closed-form acquisition
// formulas.  Here the points are uploaded once, the per-sample predictive moments stay on the
// device, and one fused kernel turns them into the acquisition value: the only D2H traffic
// is the M results.
#include <cmath>
#include <cstring>

#include <chrono>

#include "common.h"
#include "fastmath.h"
#include "gp_dev.h"
#include "mixture_dev.h"

namespace {

constexpr double kRealMin = 2.2250738585072014e-308;   // sys.float_info.min
constexpr double kRealMax = 1.7976931348623157e+308;   // sys.float_info.max
constexpr double kLogRealMin = -708.3964185322641;     // np.log(sys.float_info.min)

// the acquisition value of one point from its mean prediction, total variance and (log) density
__device__ __forceinline__ double acq_value(int kind, double f_bar, double var_tot, double dens, double sn, double y_max,
                                            double tol_var) {
  double a;
  bool log_flag = false;
  switch (kind) {
    case VBMC_ACQ_LOG: {  // acq_fcn_log.py:43-52
      const double log_p = fmax(dens, kLogRealMin);
      a = -(log(var_tot) + f_bar - y_max + log_p);
      log_flag = true;
      break;
    }
    case VBMC_ACQ_VANILLA: {  // acq_fcn_vanilla.py:38-42
      const double p = fmax(dens, kRealMin);
      a = -var_tot * (p * p);
      break;
    }
    case VBMC_ACQ_NOISY: {  // acq_fcn_noisy.py:33-41
      const double p = fmax(dens, kRealMin);
      a = -var_tot * (1.0 - sn / (var_tot + sn)) * exp(f_bar - y_max) * p;
      break;
    }
    default: {  // VBMC_ACQ_STD, acq_fcn.py:38-45
      const double p = fmax(dens, kRealMin);
      a = -var_tot * exp(f_bar - y_max) * p;
      break;
    }
  }
  // variance regularisation (abstract_acq_fcn.py:112-128)
  if (tol_var > 0.0 && var_tot < tol_var) {
    const double pen = tol_var / var_tot - 1.0;
    if (log_flag)
      a += pen;
    else
      a *= exp(-pen);
  }
  return fmax(a, -kRealMax);  // :130-131
}

// fmu, fs2: [S][M] per-sample predictive moments; dens: pdf (or log pdf for VBMC_ACQ_LOG).
__global__ __launch_bounds__(256) void acq_combine_kernel(
    const double* __restrict__ fmu, const double* __restrict__ fs2, const double* __restrict__ dens,
    const double* __restrict__ sn2, int S, int64_t M, int64_t ld, int kind, double y_max,
    double tol_var, double* __restrict__ acq, double* __restrict__ f_bar_out,
    double* __restrict__ var_tot_out) {
  const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  double f_bar, var_tot;
  gp_sample_moments(fmu, fs2, S, ld, m, f_bar, var_tot);
  acq[m] = acq_value(kind, f_bar, var_tot, dens[m], kind == VBMC_ACQ_NOISY ? sn2[m] : 0.0, y_max, tol_var);
  if (f_bar_out) f_bar_out[m] = f_bar;
  if (var_tot_out) var_tot_out[m] = var_tot;
}

// Small batches (at most 256 points: a CMA-ES population, a single point): what follows the two predict products as ONE
// launch, wave = point -- predict's finish (gp.hip predict_finish_kernel: partial sums -> f_mu, f_s2
// per GP sample, mean function), the mixture density at the point (mixture.hip's wave-per-point form), the
// formula -- with the results stored write-through into pinned host memory, drained, counted, and a completion word published for
// the host to poll (the recipe of the ELBO step's completion word, entropy.hip): three launches, no copy call and no
// stream synchronisation per batch instead of five launches, two copies and a wait.
struct AcqTail {
  const double* part;  // predict partials [S][2][ntiles][M]
  int64_t pstride;
  int ntiles, M, S, kind, log_dens;
  PredView pv;  // (add_noise 0)
  const double *mix, *sn2;
  MixLayout ml;
  double y_max, tol_var;
  double *acq, *f_bar, *var_tot;  // pinned host memory (device addresses); f_bar / var_tot nullable
  uint64_t* flag;
  uint64_t seq;
  int* cnt;  // zero between launches: workgroups that have stored their results
};

template <int DP>
__global__ __launch_bounds__(256) void acq_tail_small_kernel(AcqTail a) {
  // wave = point: lanes over the GP samples for predict's finish, lanes over the components for the density
  __shared__ int s_last;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = blockIdx.x * 4 + wave, M = a.M, D = a.pv.D, S = a.S;
  if (m < M) {
    // ---- predict's finish, lane = GP sample ----
    double fmu = 0.0, fs2 = 0.0;
    if (lane < S) {
      const double* part = a.part + (size_t)lane * a.pstride;
      const double* fpart = part + (size_t)a.ntiles * M;
      double sv = 0.0, f = 0.0;
      for (int t = 0; t < a.ntiles; ++t) {
        sv += part[(size_t)t * M + m];
        f += fpart[(size_t)t * M + m];
      }
      predict_point_moments(a.pv, lane, m, sv, f, fmu, fs2);
    }
    // ---- abstract_acq_fcn.py:82-97 (the samples sit in lanes: wave sums, a tree, not gp_sample_moments' running sums) ----
    const double f_bar = fm::wave_sum_dpp(fmu) / S, var_bar = fm::wave_sum_dpp(fs2) / S;
    double var_f = 0.0;
    if (S > 1) {
      const double t = lane < S ? fmu - f_bar : 0.0;
      var_f = fm::wave_sum_dpp(t * t) / (S - 1);
    }
    const double var_tot = var_f + var_bar;
    // ---- the mixture density at the point (mixture.hip's wave-per-point form), lane = first component ----
    const MixGauss mg = mix_gauss(a.mix, a.ml);
    const double* ilam = a.mix + a.ml.o_ilam;
    double xs[DP], g[DP];
#pragma unroll
    for (int d = 0; d < DP; ++d) {
      xs[d] = (d < D) ? scaled_coord<false>(a.pv.xs[m * D + d], ilam[d]) : 0.0;
      g[d] = 0.0;
    }
    double y = 0.0;
    mix_gauss_accumulate<DP, false, 64>(mg, xs, lane, y, g);
    y = fm::wave_sum_dpp(y);
    if (lane == 0) {
      const double dens = a.log_dens ? ((y == 0.0) ? -INFINITY : log(y)) : y;
      const double av = acq_value(a.kind, f_bar, var_tot, dens, a.kind == VBMC_ACQ_NOISY ? a.sn2[m] : 0.0, a.y_max, a.tol_var);
      __hip_atomic_store(a.acq + m, av, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      if (a.f_bar) __hip_atomic_store(a.f_bar + m, f_bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      if (a.var_tot) __hip_atomic_store(a.var_tot + m, var_tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
  // every workgroup: results acknowledged, then ONE count; the last workgroup to count publishes the sequence number
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
  __syncthreads();
  if (threadIdx.x == 0)
    s_last = __hip_atomic_fetch_add(a.cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1;
  __syncthreads();
  if (s_last && threadIdx.x == 0) {
    __hip_atomic_store(a.cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(a.flag, a.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

}  // namespace

int launch_acq_closed(vbmc_ctx* ctx, const PredictPlan& p, int64_t m, const double* d_xs, const double* d_sn2, int kind,
                      double y_max, double tol_gp_var, double* d_dens, double* d_res) {
  int rc = launch_gp_predict_all(ctx, m, d_xs, p.Ks, p.part, 0, p.fmu, p.fs2, p.mb);
  if (rc) return rc;
  rc = launch_mixture_pdf(ctx, m, d_xs, kind == VBMC_ACQ_LOG, 0, INFINITY, d_dens, nullptr);
  if (rc) return rc;
  hipLaunchKernelGGL(acq_combine_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, ctx->stream,
                     (const double*)p.fmu, (const double*)p.fs2, (const double*)d_dens, d_sn2, ctx->gp.S, m, p.mb, kind,
                     y_max, tol_gp_var, d_res, d_res + p.mb, d_res + 2 * p.mb);
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

extern "C" int vbmc_acq_eval(vbmc_ctx* ctx, int64_t M, const double* xs_MxD, int kind, double y_max,
                             double tol_gp_var, const double* sn2_M, double* acq_M, double* f_bar_M,
                             double* var_tot_M) {
  if (!ctx || (M > 0 && (!xs_MxD || !acq_M))) return VBMC_E_ARG;
  NEED_DEVICE(ctx);
  if (!ctx->gp.set) return vbmc_fail(ctx, VBMC_E_ARG, "acq_eval: GP not set");
  if (!ctx->mix_set) return vbmc_fail(ctx, VBMC_E_ARG, "acq_eval: mixture not set");
  if (ctx->gp.D != ctx->D) return vbmc_fail(ctx, VBMC_E_ARG, "acq_eval: GP/mixture D mismatch");
  if (kind < VBMC_ACQ_STD || kind > VBMC_ACQ_NOISY)
    return vbmc_fail(ctx, VBMC_E_UNSUP, "acq_eval: unknown acquisition kind %d", kind);
  if (kind == VBMC_ACQ_NOISY && !sn2_M)
    return vbmc_fail(ctx, VBMC_E_ARG, "acq_eval: the noisy acquisition needs sn2 per point");
  if (M == 0) return VBMC_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const GpState& g = ctx->gp;
  const int N = g.N, D = g.D, S = g.S;
  if (D > 32) return vbmc_fail(ctx, VBMC_E_UNSUP, "acq_eval: D=%d > 32 not supported", D);
  // S kernel matrices of a batch under 1 GiB; its own pieces: dens | sn2 | acq, f_bar, var_tot (one piece, mb apart)
  PredictPlan p;
  predict_plan(ctx, M, (int64_t)1 << 27, (int64_t)S * N, 65536, p);
  const int64_t mb = p.mb;
  const int ntiles = p.ntiles;
  const auto p_dens = p.sc.add((size_t)mb), p_sn2 = p.sc.add((size_t)mb), p_acq = p.sc.add(3 * (size_t)mb);
  int rc = predict_reserve(ctx, p, 3);
  if (rc) return rc;
  double *d_xs = p.xs, *d_Ks = p.Ks, *d_part = p.part;
  double *d_dens = p.sc.ptr(p_dens), *d_sn2 = p.sc.ptr(p_sn2), *d_acq = p.sc.ptr(p_acq);
  const double* const res_src[3] = {d_acq, d_acq + mb, d_acq + 2 * mb};
  double* const res_dst[3] = {acq_M, f_bar_M, var_tot_M};
  // ---- small batches (a CMA-ES population, a single point): the CPU writes the points straight into host-writable
  // device memory, the last kernel writes the results into pinned host memory and publishes a completion word that the
  // CPU polls: no copy calls and no stream synchronisation around ~30 us of kernels ----
  if (M <= 256 && M <= mb && S <= 64 && ctx->opt_acq_poll && !ctx->acq_fg_failed) {
    if (!ctx->d_acq_fg) {
      int large_bar = 0;
      if (hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, ctx->device) != hipSuccess || !large_bar ||
          hipExtMallocWithFlags((void**)&ctx->d_acq_fg, sizeof(double) * 256 * 33, hipDeviceMallocFinegrained) != hipSuccess) {
        (void)hipGetLastError();
        ctx->d_acq_fg = nullptr;
        ctx->acq_fg_failed = true;
      }
    }
  }
  // (M <= mb: the scratch and the pinned result rows are laid out for batches of mb points, which S * N can push below M)
  if (M <= 256 && M <= mb && S <= 64 && ctx->opt_acq_poll && ctx->d_acq_fg) {
    if (ctx->spec.armed) spec_disarm(ctx);  // (launches waiting for a theta would sit in front of these)
    const int64_t m = M;
    memcpy(ctx->d_acq_fg, xs_MxD, sizeof(double) * m * D);
    if (kind == VBMC_ACQ_NOISY) memcpy(ctx->d_acq_fg + 256 * 32, sn2_M, sizeof(double) * m);
    __builtin_ia32_sfence();  // write-combined stores drained before the doorbell of the launches
    const double* x_dev = ctx->d_acq_fg;
    rc = launch_gp_predict_products(ctx, m, x_dev, d_Ks, d_part);  // K*, the variance product: their partial sums
    if (rc) return rc;
    const uint64_t seq = ++ctx->acq_seq;
    volatile uint64_t* flag = ctx->h_done + 7;
    AcqTail t;
    t.part = d_part;
    t.ntiles = ntiles;
    t.pstride = 2 * (int64_t)ntiles * m;
    t.M = (int)m;
    t.S = S;
    t.kind = kind;
    t.log_dens = kind == VBMC_ACQ_LOG;
    t.pv = gp_pred_view(g, x_dev, 0);
    t.mix = ctx->d_mix;
    t.sn2 = ctx->d_acq_fg + 256 * 32;
    t.ml = ctx->ml;
    t.y_max = y_max;
    t.tol_var = tol_gp_var;
    t.acq = ctx->hp_dev;
    t.f_bar = f_bar_M ? ctx->hp_dev + mb : nullptr;
    t.var_tot = var_tot_M ? ctx->hp_dev + 2 * mb : nullptr;
    t.flag = ctx->hd_done + 7;
    t.seq = seq;
    t.cnt = ctx->d_done_cnt + 4;
#define CALL(DP) hipLaunchKernelGGL(acq_tail_small_kernel<DP>, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, ctx->stream, t)
    VBMC_DISPATCH_DP(D, CALL);
#undef CALL
    HIP_TRY(ctx, hipGetLastError());
    const auto t0 = std::chrono::steady_clock::now();
    bool seen = false;
    for (long spin = 0;; ++spin) {
      if (*flag == seq) {
        seen = true;
        break;
      }
      if ((spin & 1023) == 1023 &&
          std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 2.0)
        break;  // (a stuck queue: the stream wait below reports what happened)
      __builtin_ia32_pause();
    }
    if (!seen) HIP_TRY(ctx, stream_wait(ctx));
    if (!seen && *flag != seq) return vbmc_fail(ctx, VBMC_E_HIP, "acq_eval: the completion word did not arrive");
    __atomic_thread_fence(__ATOMIC_ACQUIRE);  // the results were written before the word: read them after it
    ctx->pack_in_flight = false;  // (everything queued before the last kernel has run)
    memcpy(acq_M, ctx->h_pinned, sizeof(double) * m);
    if (f_bar_M) memcpy(f_bar_M, ctx->h_pinned + mb, sizeof(double) * m);
    if (var_tot_M) memcpy(var_tot_M, ctx->h_pinned + 2 * mb, sizeof(double) * m);
    return VBMC_OK;
  }
  for (int64_t o = 0; o < M; o += mb) {
    const int64_t m = (M - o) < mb ? (M - o) : mb;
    HIP_TRY(ctx, hipMemcpyAsync(d_xs, xs_MxD + o * D, sizeof(double) * m * D, hipMemcpyHostToDevice,
                                ctx->stream));
    if (kind == VBMC_ACQ_NOISY)
      HIP_TRY(ctx, hipMemcpyAsync(d_sn2, sn2_M + o, sizeof(double) * m, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = launch_acq_closed(ctx, p, m, d_xs, d_sn2, kind, y_max, tol_gp_var, d_dens, d_acq))) return rc;
    if ((rc = fetch_vectors(ctx, 3, res_src, res_dst, (size_t)m, (size_t)mb, (size_t)o))) return rc;
  }
  return VBMC_OK;
}

// a13: c[i][j] = |a_i - b_j|^2 the way AbstractAcqFcn._sq_dist computes it
// (acquisition_functions/abstract_acq_fcn.py:195-222); argmin_n (nullable) = np.argmin(c, axis=1)
// (the nearest-neighbour lookup of _estimate_observation_noise, :244-252).
extern "C" int vbmc_sq_dist(vbmc_ctx* ctx, int64_t n, int64_t m, int D, const double* a_nxD,
                            const double* b_mxD, double* c_nxm, int64_t* argmin_n) {
  if (!ctx || n < 0 || m < 0 || D < 1) return VBMC_E_ARG;
  if (n > 0 && m > 0 && (!a_nxD || !b_mxD)) return VBMC_E_ARG;
  NEED_DEVICE(ctx);
  if (D > 32) return vbmc_fail(ctx, VBMC_E_UNSUP, "sq_dist: D=%d > 32 not supported", D);
  if (m > (int64_t)1 << 24) return vbmc_fail(ctx, VBMC_E_UNSUP, "sq_dist: more than 2^24 columns");
  if (argmin_n && m == 0 && n > 0)
    return vbmc_fail(ctx, VBMC_E_ARG, "sq_dist: argmin of an empty row");
  if (n == 0 || m == 0) return VBMC_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // mu = m/(n+m) mean(b) + n/(n+m) mean(a)   (:212-215)
  std::vector<double> ma(D, 0.0), mbv(D, 0.0), cen(D);
  for (int64_t i = 0; i < n; ++i)
    for (int d = 0; d < D; ++d) ma[d] += a_nxD[i * D + d];
  for (int64_t j = 0; j < m; ++j)
    for (int d = 0; d < D; ++d) mbv[d] += b_mxD[j * D + d];
  const double tot = (double)(n + m);
  for (int d = 0; d < D; ++d) cen[d] = ((double)m / tot) * (mbv[d] / m) + ((double)n / tot) * (ma[d] / n);
  const int ntiles = (int)((m + 63) / 64);
  // rows per pass: keep the n x m block under ~256 MiB
  int64_t nb = c_nxm ? ((int64_t)1 << 25) / (m > 0 ? m : 1) : ((int64_t)1 << 20);
  nb = nb < 64 ? 64 : nb;
  nb = nb > n ? n : nb;
  Scratch sc;
  const auto p_cen = sc.add((size_t)D), p_a = sc.add((size_t)nb * D), p_b = sc.add((size_t)m * D);
  const auto p_c = sc.add(c_nxm ? (size_t)nb * m : 0);
  const auto p_p = sc.add(argmin_n ? 2 * (size_t)ntiles * nb : 0);  // tile minima / indices
  const auto p_am = sc.add<int64_t>(argmin_n ? (size_t)nb : 0);
  int rc = reserve(ctx, sc);
  if (rc) return rc;
  double *d_cen = sc.ptr(p_cen), *d_a = sc.ptr(p_a), *d_b = sc.ptr(p_b), *d_p = sc.ptr(p_p);
  double* d_c = c_nxm ? sc.ptr(p_c) : nullptr;
  int64_t* d_am = argmin_n ? sc.ptr(p_am) : nullptr;
  HIP_TRY(ctx, hipMemcpyAsync(d_cen, cen.data(), sizeof(double) * D, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_b, b_mxD, sizeof(double) * m * D, hipMemcpyHostToDevice, ctx->stream));
  for (int64_t o = 0; o < n; o += nb) {
    const int64_t cnt = (n - o) < nb ? (n - o) : nb;
    HIP_TRY(ctx, hipMemcpyAsync(d_a, a_nxD + o * D, sizeof(double) * cnt * D, hipMemcpyHostToDevice, ctx->stream));
    rc = launch_sq_dist(ctx, d_a, cnt, d_b, (int)m, D, d_cen, d_c, d_p, d_am);
    if (rc) return rc;
    if (c_nxm)
      HIP_TRY(ctx, hipMemcpyAsync(c_nxm + o * m, d_c, sizeof(double) * cnt * m, hipMemcpyDeviceToHost, ctx->stream));
    if (argmin_n)
      HIP_TRY(ctx, hipMemcpyAsync(argmin_n + o, d_am, sizeof(int64_t) * cnt, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, stream_wait(ctx));
  }
  return VBMC_OK;
}
