// The kernels of optimize_vp's last stage (api_elcbo_full.hip): the per-component expected log joint I_sk kept on the
// device, and the re-weighting of a recorded I_sk / J_sjk over a set of alive components.
//
// vbmc/variational_optimization.py evaluates the full ELCBO once per pruning trial (:322-378) on the posterior with one
// component removed.  The removal leaves mu, sigma, lambd of the others unchanged, so the trial's
//   G_s    = sum_a w'_a I[s, alive[a]]
//   varG_s = sum_a w'_a^2 max(tiny, J[s, aa]) + 2 sum_{a<b} w'_a w'_b J[s, alive[a], alive[b]],  clamped at tiny
// (:1578-1586) are sums over the arrays of the first evaluation, read at their original stride K0 through the alive
// list, and the statistics over the GP samples (:1588-1596) follow from them.  The arithmetic restates the host loop of
// vbmc_gp_log_joint (api_gp.hip:246-288): upper triangle j <= k, tiny = np.spacing(1), both clamps; what differs is the
// order of the additions (a wave reduction), bounded in profiles/optimize_vp.md.
#include <cmath>

#include "common.h"
#include "fastmath.h"

namespace {

constexpr double kTiny = 2.220446049250313e-16;  // np.spacing(1)
constexpr int kMaxK = 128;

// I[s][k] = r[0] + m0 - nu / 2 (api_gp.hip glj_finalize): one thread per (s, k)
__global__ __launch_bounds__(256) void elcbo_isk_kernel(const double* __restrict__ res, const double* __restrict__ mix, MixLayout ml,
                                                        const double* __restrict__ hyp, int P, int mean_kind, int S,
                                                        double* __restrict__ I) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int D = ml.D, K = ml.K;
  if (i >= S * K) return;
  const int s = i / K, k = i - s * K;
  const double* h = hyp + (size_t)s * P;
  const double m0 = mean_kind == VBMC_MEAN_ZERO ? 0.0 : h[D + 2];
  double I_k = res[(size_t)i * (1 + 2 * D)] + m0;
  if (mean_kind == VBMC_MEAN_NEGQUAD) {
    const double sg = mix[ml.o_sig + k];
    double nu = 0.0;
    for (int d = 0; d < D; ++d) {
      const double xm = h[D + 3 + d], iom2 = exp(-2.0 * h[2 * D + 3 + d]);
      const double m = mix[ml.o_mu + k * D + d], lam = mix[ml.o_lam + d];
      nu += iom2 * (m * m + sg * sg * lam * lam - 2.0 * m * xm + xm * xm);
    }
    I_k += -0.5 * nu;
  }
  I[i] = I_k;
}

// One workgroup per GP sample s: part[s] = G_s, part[S + s] = varG_s.  Wave v takes the rows a = v, v + 4, ... of the
// alive upper triangle, its lanes the columns b >= a; every lane reaches the reductions (full waves).
__global__ __launch_bounds__(256) void elcbo_reweight_kernel(int K0, int Ka, const double* __restrict__ I, const double* __restrict__ J,
                                                             const double* __restrict__ w, const int* __restrict__ alive,
                                                             double* __restrict__ part) {
  __shared__ double s_w[kMaxK];
  __shared__ int s_al[kMaxK];
  __shared__ double s_red[2][4];
  const int s = blockIdx.x, S = gridDim.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < Ka) {
    s_w[tid] = w[tid];
    s_al[tid] = alive[tid];
  }
  __syncthreads();
  double g = 0.0, v = 0.0;
  if (tid < Ka) g = s_w[tid] * I[(size_t)s * K0 + s_al[tid]];
  if (J) {
    const double* Js = J + (size_t)s * K0 * K0;
    for (int a = wave; a < Ka; a += 4) {
      const double wa = s_w[a];
      const double* row = Js + (size_t)s_al[a] * K0;
      for (int b = a + lane; b < Ka; b += 64) {
        const double Jv = row[s_al[b]];
        if (b == a)
          v += wa * wa * (Jv > kTiny ? Jv : kTiny);
        else
          v += 2.0 * wa * s_w[b] * Jv;
      }
    }
  }
  g = fm::wave_sum_dpp(g);
  v = fm::wave_sum_dpp(v);
  if (lane == 0) {
    s_red[0][wave] = g;
    s_red[1][wave] = v;
  }
  __syncthreads();
  if (tid == 0) {
    const double G = (s_red[0][0] + s_red[0][1]) + (s_red[0][2] + s_red[0][3]);
    double vG = (s_red[1][0] + s_red[1][1]) + (s_red[1][2] + s_red[1][3]);
    if (vG < kTiny) vG = kTiny;
    part[s] = G;
    part[S + s] = J ? vG : 0.0;
  }
}

// The step over s (api_gp.hip:269-288, avg_flag on): out = G, varG, var_ss.  One wave.
__global__ __launch_bounds__(64) void elcbo_over_s_kernel(int S, int has_var, const double* __restrict__ part, double* __restrict__ out) {
  const int lane = threadIdx.x;
  double g = 0.0, v = 0.0;
  for (int s = lane; s < S; s += 64) {
    g += part[s];
    v += part[S + s];
  }
  const double Gsum = fm::wave_sum_dpp(g), vsum = fm::wave_sum_dpp(v);
  if (S == 1) {
    if (lane == 0) {
      out[0] = part[0];
      out[1] = has_var ? part[1] : 0.0;
      out[2] = 0.0;
    }
    return;
  }
  const double Gbar = Gsum / S, vmean = vsum / S;
  double dg = 0.0, dv = 0.0;
  for (int s = lane; s < S; s += 64) {
    dg += (part[s] - Gbar) * (part[s] - Gbar);
    dv += (part[S + s] - vmean) * (part[S + s] - vmean);
  }
  const double vss = fm::wave_sum_dpp(dg) / (S - 1);
  const double vstd = sqrt(fm::wave_sum_dpp(dv) / (S - 1));
  if (lane == 0) {
    out[0] = Gbar;
    out[1] = has_var ? vsum / S + vss : 0.0;
    out[2] = has_var ? vss + vstd : 0.0;
  }
}

}  // namespace

int launch_elcbo_isk(vbmc_ctx* ctx, const double* d_res, double* d_I) {
  const GpState& g = ctx->gp;
  const int n = g.S * ctx->K;
  hipLaunchKernelGGL(elcbo_isk_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, d_res, (const double*)ctx->d_mix, ctx->ml,
                     (const double*)g.d_hyp, g.P, g.mean_kind, g.S, d_I);
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

int launch_elcbo_reweight(vbmc_ctx* ctx, int S, int K0, int Ka, const double* d_I, const double* d_J, const double* d_w,
                          const int* d_alive, double* d_part, double* d_out) {
  if (S < 1 || Ka < 1 || Ka > K0 || K0 > kMaxK)
    return vbmc_fail(ctx, VBMC_E_UNSUP, "elcbo re-weighting: S=%d, K0=%d, K_alive=%d beyond 1 <= K_alive <= K0 <= %d", S, K0, Ka, kMaxK);
  hipLaunchKernelGGL(elcbo_reweight_kernel, dim3(S), dim3(256), 0, ctx->stream, K0, Ka, d_I, d_J, d_w, d_alive, d_part);
  hipLaunchKernelGGL(elcbo_over_s_kernel, dim3(1), dim3(64), 0, ctx->stream, S, d_J ? 1 : 0, (const double*)d_part, d_out);
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}
