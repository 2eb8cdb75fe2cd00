// The GP log marginal likelihood and its gradient for a batch of hyper-parameter candidates, from the factor state
// gp_post.hip leaves in ctx->gp (U, Ui = U^-1 with its zero-padded copy, alpha, r; C = sl A, U^T U = A):
//   lml      = -1/2 r.alpha - sum_i log U_ii - N/2 log(2 pi sl)
//   dlml/dth = -1/2 tr(W dC/dth),  W = A^-1 / sl - alpha alpha^T,  A^-1 = Ui Ui^T   (covariance and noise parameters)
//   dlml/dth = alpha . dm/dth                                                         (mean parameters)
// A^-1 is never stored: lml_grad_tile_kernel forms one 64 x 64 tile of it on the FP64 matrix cores (mfma_tile.h) and
// contracts it in its epilogue with dC/dth, re-formed from the scaled coordinates as gp_cov_kernel forms K (direct
// differences).  The candidate is the last grid dimension of every launch; no atomics, every sum in a fixed order, so a
// candidate's results do not depend on what else is in the batch.
#include <cmath>

#include "common.h"
#include "mfma_tile.h"

namespace {

using mfma_tile::Acc;
using mfma_tile::KDP;
using mfma_tile::Lanes;
using mfma_tile::TS;

constexpr int PB = TS;   // block side
constexpr int KC = 32;   // contraction indices staged per round ([row][k] panels of row stride KDP)
constexpr int DMX = 32;  // largest D

// 256 values (one per thread) summed in a fixed order: wave sums by DPP, then the four waves' in LDS (sW: 4 doubles)
__device__ __forceinline__ double block_sum(double v, double* sW, int tid) {
  v = fm::wave_sum_dpp(v);
  __syncthreads();  // (sW may still be read from the sum before)
  if ((tid & 63) == 0) sW[tid >> 6] = v;
  __syncthreads();
  return (sW[0] + sW[1]) + (sW[2] + sW[3]);
}

// sums[s] = (sum_i log U_ii, r.alpha): one workgroup per candidate
__global__ __launch_bounds__(256) void lml_value_kernel(const double* __restrict__ L, int N, const double* __restrict__ r,
                                                        const double* __restrict__ alpha, double* __restrict__ sums) {
  const int s = blockIdx.x, tid = threadIdx.x;
  __shared__ double sW[4];
  const double* U = L + (size_t)s * N * N;
  double lg = 0.0, ra = 0.0;
  for (int i = tid; i < N; i += 256) {
    lg += log(U[(size_t)i * N + i]);
    ra = fma(r[(size_t)s * N + i], alpha[(size_t)s * N + i], ra);
  }
  lg = block_sum(lg, sW, tid);
  ra = block_sum(ra, sW, tid);
  if (tid == 0) {
    sums[2 * s] = lg;
    sums[2 * s + 1] = ra;
  }
}

// Tile pair t = (a <= b) of candidate s: part[s][t][0 .. D - 1] = sum_ij w_ij t_d^2, [D] = sum_ij w_ij,
// [D + 1] = sum_i (Ainv_ii / sl - alpha_i^2) (diagonal tiles, else 0), with w_ij = (Ainv_ij / sl - alpha_i alpha_j) K_ij
// over the tile's rows i and columns j below N.  Ainv_ij = sum_k Ui_ik Ui_jk over k >= 64 b: Ui is zero below its
// diagonal.  LinvP is the zero-padded copy (leading dimension ld = 64 nb), so no load is guarded.
__global__ __launch_bounds__(256) void lml_grad_tile_kernel(const double* __restrict__ LinvP, int ld,
                                                            const double* __restrict__ XT, const double* __restrict__ alpha,
                                                            const double* __restrict__ hyp_all, int P, int N, int D,
                                                            const double* __restrict__ sl, int nb, double* __restrict__ part) {
  const int s = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
  int a = 0, rem = t;  // t counts the pairs row by row: (0, 0) .. (0, nb - 1), (1, 1) ..
  while (rem >= nb - a) {
    rem -= nb - a;
    ++a;
  }
  const int b = a + rem;
  // product: two [64][KDP] panels; epilogue: the scaled coordinates of the rows and of the columns, [DMX][64] each
  __shared__ double sm[2 * PB * KDP];
  __shared__ double sAl[2][PB];
  __shared__ double sRed[4][DMX + 2];
  static_assert(2 * PB * KDP >= 2 * DMX * PB, "the coordinate panels reuse the product's staging");
  double* sA = sm;
  double* sB = sm + PB * KDP;
  const double* Ra = LinvP + ((size_t)s * ld + (size_t)a * PB) * ld;
  const double* Rb = LinvP + ((size_t)s * ld + (size_t)b * PB) * ld;
  const Lanes ln = mfma_tile::lanes(tid);
  Acc acc;
  mfma_tile::zero(acc);
  for (int k0 = b * PB; k0 < ld; k0 += KC) {
    for (int idx = tid; idx < PB * KC; idx += 256) {
      const int row = idx >> 5, kk = idx & 31;
      sA[row * KDP + kk] = Ra[(size_t)row * ld + k0 + kk];
      sB[row * KDP + kk] = Rb[(size_t)row * ld + k0 + kk];
    }
    __syncthreads();
#pragma unroll
    for (int kq = 0; kq < KC / 4; ++kq) mfma_tile::step_rows(acc, ln, sA, sB, KDP, kq);
    __syncthreads();
  }
  // ---- epilogue ----
  double* sa = sm;
  double* sb = sm + DMX * PB;
  const double* hyp = hyp_all + (size_t)s * P;
  const int i0 = a * PB, j0 = b * PB;
  for (int idx = tid; idx < D * PB; idx += 256) {
    const int dd = idx >> 6, c = idx & 63;
    const double ell = exp(hyp[dd]);
    const double* row = XT + (size_t)dd * N;
    sa[dd * PB + c] = i0 + c < N ? row[i0 + c] / ell : 0.0;
    sb[dd * PB + c] = j0 + c < N ? row[j0 + c] / ell : 0.0;
  }
  if (tid < 2 * PB) {
    const int c = tid & 63, g = (tid < PB ? i0 : j0) + c;
    sAl[tid >> 6][c] = g < N ? alpha[(size_t)s * N + g] : 0.0;
  }
  __syncthreads();
  const int rbase = ln.wm * 32 + ln.lk, cbase = ln.wc * 32 + ln.li;  // row = rbase + 16 mt + 4 r, col = cbase + 16 ct
  // pass 1: squared distances in the walk's order (mt, r, ct), then w
  double w[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) w[e] = 0.0;
  for (int dd = 0; dd < D; ++dd) {
    const double c0 = sb[dd * PB + cbase], c1 = sb[dd * PB + cbase + 16];
#pragma unroll
    for (int mr = 0; mr < 8; ++mr) {
      const double ra = sa[dd * PB + rbase + 16 * (mr >> 2) + 4 * (mr & 3)];
      const double t0 = ra - c0, t1 = ra - c1;
      w[2 * mr] += t0 * t0;
      w[2 * mr + 1] += t1 * t1;
    }
  }
  const double sf2 = exp(2.0 * hyp[D]), sls = sl[s];
  double sw = 0.0, tr = 0.0;
  int e = 0;
  mfma_tile::walk(
      acc, ln,
      [&](int row, int col, double v) {
        const double ai = sAl[0][row], aj = sAl[1][col];
        const double q = v / sls - ai * aj;
        const bool in = i0 + row < N && j0 + col < N;
        const double we = in ? q * (sf2 * exp(-0.5 * w[e])) : 0.0;
        if (a == b && row == col && in) tr += q;
        w[e] = we;
        sw += we;
        ++e;
      },
      [](int) {});
  // pass 2: per dimension, sum_e w_e t_d^2
  const int lane = tid & 63, wave = tid >> 6;
  for (int dd = 0; dd < D; ++dd) {
    const double c0 = sb[dd * PB + cbase], c1 = sb[dd * PB + cbase + 16];
    double v = 0.0;
#pragma unroll
    for (int mr = 0; mr < 8; ++mr) {
      const double ra = sa[dd * PB + rbase + 16 * (mr >> 2) + 4 * (mr & 3)];
      const double t0 = ra - c0, t1 = ra - c1;
      v = fma(w[2 * mr], t0 * t0, v);
      v = fma(w[2 * mr + 1], t1 * t1, v);
    }
    v = fm::wave_sum_dpp(v);
    if (lane == 0) sRed[wave][dd] = v;
  }
  sw = fm::wave_sum_dpp(sw);
  tr = fm::wave_sum_dpp(tr);
  if (lane == 0) {
    sRed[wave][D] = sw;
    sRed[wave][D + 1] = tr;
  }
  __syncthreads();
  if (tid < D + 2)
    part[((size_t)s * gridDim.x + t) * (D + 2) + tid] = (sRed[0][tid] + sRed[1][tid]) + (sRed[2][tid] + sRed[3][tid]);
}

// mg[s][m] = alpha_s . dm/dtheta_m for the mean's parameters (constant: m0; negative quadratic: m0, xm_d, log omega_d).
// One workgroup per candidate; wave q takes the parameters q, q + 4, ..., its lanes stride over the points.
__global__ __launch_bounds__(256) void lml_mean_grad_kernel(const double* __restrict__ XT, const double* __restrict__ alpha,
                                                            const double* __restrict__ hyp_all, int P, int N, int D,
                                                            int mean_n, double* __restrict__ mg) {
  const int s = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double* hm = hyp_all + (size_t)s * P + D + 2;
  const double* al = alpha + (size_t)s * N;
  for (int m = wave; m < mean_n; m += 4) {  // (wave-uniform)
    double v = 0.0;
    if (m == 0) {
      for (int n = lane; n < N; n += 64) v += al[n];
    } else {
      const int d = (m - 1) % D;
      const bool shift = m <= D;  // xm_d, else log omega_d
      const double xm = hm[1 + d], om = exp(hm[1 + D + d]);
      const double* x = XT + (size_t)d * N;
      for (int n = lane; n < N; n += 64) {
        const double u = x[n] - xm;
        v = fma(al[n], shift ? u / (om * om) : (u / om) * (u / om), v);
      }
    }
    v = fm::wave_sum_dpp(v);
    if (lane == 0) mg[(size_t)s * mean_n + m] = v;
  }
}

// One thread per (candidate, output): output 0 is the value, output 1 + p the derivative with respect to parameter p.
// Tile partials are added in tile order, off-diagonal pairs twice.
__global__ __launch_bounds__(256) void lml_finish_kernel(int S, int N, int D, int P, int nb, int n_out,
                                                         const double* __restrict__ sums, const double* __restrict__ sl,
                                                         const double* __restrict__ dsn2, const double* __restrict__ part,
                                                         const double* __restrict__ mg, double* __restrict__ lml,
                                                         double* __restrict__ dlml) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= S * n_out) return;
  const int s = idx / n_out, o = idx % n_out;
  if (o == 0) {
    lml[s] = -0.5 * sums[2 * s + 1] - sums[2 * s] - 0.5 * N * log(2.0 * M_PI * sl[s]);
    return;
  }
  const int p = o - 1;
  double g;
  if (p < D + 2) {
    const int npairs = nb * (nb + 1) / 2;
    const double* ps = part + (size_t)s * npairs * (D + 2) + p;
    double acc = 0.0;
    int t = 0;
    for (int a = 0; a < nb; ++a)
      for (int b = a; b < nb; ++b, ++t) acc += (a == b ? 1.0 : 2.0) * ps[(size_t)t * (D + 2)];
    g = p < D ? -0.5 * acc : p == D ? -acc : -0.5 * dsn2[s] * acc;
  } else {
    g = mg[(size_t)s * (P - D - 2) + (p - D - 2)];
  }
  dlml[(size_t)s * P + p] = g;
}

}  // namespace

int launch_gp_lml(vbmc_ctx* ctx, int want_grad, const double* d_dsn2, double* d_sums, double* d_part, double* d_mg,
                  double* d_lml, double* d_dlml) {
  const GpState& g = ctx->gp;
  const int N = g.N, D = g.D, S = g.S, P = g.P, nb = (N + PB - 1) / PB, mean_n = P - D - 2;
  hipLaunchKernelGGL(lml_value_kernel, dim3(S), dim3(256), 0, ctx->stream, (const double*)g.d_L, N, (const double*)g.d_r,
                     (const double*)g.d_alpha, d_sums);
  if (want_grad) {
    hipLaunchKernelGGL(lml_grad_tile_kernel, dim3(nb * (nb + 1) / 2, S), dim3(256), 0, ctx->stream,
                       (const double*)g.d_LinvP, predict_ld(N), (const double*)g.d_XT, (const double*)g.d_alpha,
                       (const double*)g.d_hyp, P, N, D, (const double*)g.d_sl, nb, d_part);
    if (mean_n > 0)
      hipLaunchKernelGGL(lml_mean_grad_kernel, dim3(S), dim3(256), 0, ctx->stream, (const double*)g.d_XT,
                         (const double*)g.d_alpha, (const double*)g.d_hyp, P, N, D, mean_n, d_mg);
  }
  const int n_out = want_grad ? 1 + P : 1;
  hipLaunchKernelGGL(lml_finish_kernel, dim3((S * n_out + 255) / 256), dim3(256), 0, ctx->stream, S, N, D, P, nb, n_out,
                     (const double*)d_sums, (const double*)g.d_sl, d_dsn2, (const double*)d_part, (const double*)d_mg, d_lml,
                     d_dlml);
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}
