// The GP posterior on the device (gpyreg's posterior, SURVEY Appendix A "Posterior"; gp.py GP._posterior on the host):
//   A_s = K_s(X, X) / sl_s + diag(sn2_s / sn2_div_s),   U_s^T U_s = A_s,   alpha_s = U_s^-1 (U_s^-T r_s) / sl_s,
// for every hyper-parameter sample s (a grid dimension of every launch), in FP64 and with a fixed summation order: no
// atomics, so a call is bit-reproducible.
//
// Blocked upper Cholesky in place, 64 x 64 blocks on the block grid of gp.hip's trinv_*_kernel (N padded with the
// identity, never read out of bounds).  Block step j, four launches:
//   chol_diag_kernel   factors the diagonal block in registers / LDS (one wave per sample);
//   chol_dinv_kernel   inverts the factor: Dinv_j, the block launch_trinv's first stage would otherwise compute -- kept
//                      for it;
//   chol_panel_kernel  U_j,rest = Dinv_j^T A_j,rest                              (FP64 matrix cores, mfma_tile.h)
//   chol_trail_kernel  A_ab -= U_ja^T U_jb for the blocks j < a <= b              (the same tile product)
// L^-1 then comes from launch_trinv (stage 2 only) and alpha from two triangular matrix-vector kernels over L^-1.
//
// One appended point x (noise variance sn2 >= sn2_div, so sl stays): k = K(X, x) / sl, l = U^-T k,
//   d = sqrt(sf^2 / sl + sn2 / sn2_div - l.l),
//   U' = [[U, l], [0, d]],   U'^-1 = [[U^-1, -U^-1 l / d], [0, 1 / d]],
// written with the new row stride N + 1 into the buffers of the state under construction (never in place).
#include <cmath>

#include "common.h"
#include "gp_dev.h"
#include "mfma_tile.h"

namespace {

using mfma_tile::Acc;
using mfma_tile::Lanes;
using mfma_tile::LDA;
using mfma_tile::LDB;
using mfma_tile::TKD;
using mfma_tile::TS;

constexpr int PB = TS;   // block side (= TRB of gp.hip)
constexpr int DC = 32;   // dimensions of the scaled coordinates staged at a time

// m_s(x) for the three mean kinds; hm = the mean's hyper-parameters (variational_optimization.py:1383-1392 layout)
__device__ inline double post_mean_at(const double* hm, int D, int mean_kind, const double* x) {
  if (mean_kind == VBMC_MEAN_ZERO) return 0.0;
  if (mean_kind == VBMC_MEAN_CONST) return hm[0];
  double q = 0.0;
  for (int d = 0; d < D; ++d) {
    const double t = (x[d] - hm[1 + d]) / exp(hm[1 + D + d]);
    q += t * t;
  }
  return hm[0] - 0.5 * q;
}

// Upper triangle (diagonal included) of A_s, zeros below it, and the residual r_s = y - m_s(X).  A workgroup owns one
// 64 x 64 block; the squared distance is the sum of squared DIFFERENCES of the scaled coordinates (oracle/gp_ref.se_ard),
// never the |a|^2 + |b|^2 - 2ab expansion, which cancels at the diagonal.
__global__ __launch_bounds__(256) void gp_cov_kernel(const double* __restrict__ XT, const double* __restrict__ X,
                                                     const double* __restrict__ y, const double* __restrict__ hyp_all,
                                                     int P, int N, int D, int mean_kind,
                                                     const double* __restrict__ sn2, const double* __restrict__ sl,
                                                     double* __restrict__ L, double* __restrict__ r) {
  const int s = blockIdx.z, bi = blockIdx.y, bj = blockIdx.x, tid = threadIdx.x;
  const double* hyp = hyp_all + (size_t)s * P;
  double* A = L + (size_t)s * N * N;
  const int i0 = bi * PB, j0 = bj * PB;
  const int tc = tid & 63, tr = tid >> 6;  // this thread: column tc, rows tr + 4 rr
  if (bj < bi) {
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) {
      const int row = i0 + tr + 4 * rr, col = j0 + tc;
      if (row < N && col < N) A[(size_t)row * N + col] = 0.0;
    }
    return;
  }
  __shared__ double sa[DC][PB], sb[DC][PB];
  double d2[16];
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) d2[rr] = 0.0;
  for (int d0 = 0; d0 < D; d0 += DC) {
    const int dn = min(DC, D - d0);
    for (int idx = tid; idx < dn * PB; idx += 256) {
      const int dd = idx >> 6, t = idx & 63;
      const double ell = exp(hyp[d0 + dd]);
      const double* row = XT + (size_t)(d0 + dd) * N;
      sa[dd][t] = i0 + t < N ? row[i0 + t] / ell : 0.0;
      sb[dd][t] = j0 + t < N ? row[j0 + t] / ell : 0.0;
    }
    __syncthreads();
    for (int dd = 0; dd < dn; ++dd) {
      const double b = sb[dd][tc];
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) {
        const double t = sa[dd][tr + 4 * rr] - b;
        d2[rr] += t * t;
      }
    }
    __syncthreads();
  }
  const double sf2 = exp(2.0 * hyp[D]), sls = sl[s];
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) {
    const int row = i0 + tr + 4 * rr, col = j0 + tc;
    if (row < N && col < N) {
      double v = 0.0;
      if (col >= row) {
        v = sf2 * exp(-0.5 * d2[rr]) / sls;
        if (col == row) v += sn2[(size_t)s * N + row] / sls;  // (sn2_mult = 1: sl = sn2_div)
      }
      A[(size_t)row * N + col] = v;
    }
  }
  if (bi == bj && tid < PB && i0 + tid < N) {
    const int i = i0 + tid;
    r[(size_t)s * N + i] = y[i] - post_mean_at(hyp + D + 2, D, mean_kind, X + (size_t)i * D);
  }
}

// Diagonal block j of sample s: U^T U = A in place (right-looking; thread c holds column c in registers, the row of a
// step is exchanged through LDS).  A pivot that is not a positive finite number sets flag[s]; the step goes on with 1
// in its place (the host discards the results).
__global__ __launch_bounds__(64) void chol_diag_kernel(double* __restrict__ L, int N, int j, int* __restrict__ flag) {
  const int s = blockIdx.x, c = threadIdx.x;
  __shared__ double sRow[PB];
  double* A = L + (size_t)s * N * N;
  const int r0 = j * PB, gc = r0 + c, gcc = min(gc, N - 1);
  double col[PB];
#pragma unroll
  for (int r = 0; r < PB; ++r) col[r] = A[(size_t)min(r0 + r, N - 1) * N + gcc];
#pragma unroll
  for (int r = 0; r < PB; ++r) {
    const int gr = r0 + r;
    col[r] = (gr < N && gc < N) ? col[r] : (gr == gc ? 1.0 : 0.0);
  }
  bool bad = false;
#pragma unroll
  for (int k = 0; k < PB; ++k) {
    sRow[c] = col[k];
    __syncthreads();
    double p = sRow[k];
    if (!(p > 0.0 && p < INFINITY)) {
      bad = true;
      p = 1.0;
    }
    const double ukk = sqrt(p);
    const double u = (c == k) ? ukk : col[k] / ukk;
    col[k] = u;
    __syncthreads();
    sRow[c] = u;
    __syncthreads();
#pragma unroll
    for (int i = k + 1; i < PB; ++i) col[i] = fma(-sRow[i], u, col[i]);
    __syncthreads();
  }
  if (bad && c == 0) flag[s] = 1;
#pragma unroll
  for (int r = 0; r < PB; ++r) {
    const int gr = r0 + r;
    if (gr < N && gc < N) A[(size_t)gr * N + gc] = r <= c ? col[r] : 0.0;
  }
}

// Dinv_j = U_jj^-1 (tri_block_inverse of gp_dev.h, as trinv_diag_kernel) for block j alone: the block launch_trinv's
// first stage would otherwise compute.
__global__ __launch_bounds__(64) void chol_dinv_kernel(const double* __restrict__ L, int N, int j, double* __restrict__ Dinv,
                                                       int nb) {
  const int s = blockIdx.x;
  __shared__ double sUT[PB][PB];
  __shared__ double sRinv[PB];
  tri_block_inverse(L + (size_t)s * N * N, N, j * PB, threadIdx.x, sUT, sRinv, Dinv + ((size_t)s * nb + j) * PB * PB);
}

// acc = P^T Q for two blocks of 64 rows k stored [k][column] (row strides ldp, ldq; columns past pcols / qcols read as 0),
// on the workgroup tile of mfma_tile.h: 16 rows of k at a time, P transposed into the [row][k] panel.
__device__ __forceinline__ void ptq_tile(const double* __restrict__ Pm, int ldp, int pcols, const double* __restrict__ Qm,
                                         int ldq, int qcols, double* sA, double* sB, const Lanes& ln, Acc& acc, int tid) {
  mfma_tile::zero(acc);
  for (int k0 = 0; k0 < PB; k0 += TKD) {
    for (int idx = tid; idx < TKD * PB; idx += 256) {
      const int kk = idx >> 6, m = idx & 63;
      sA[m * LDA + kk] = m < pcols ? Pm[(size_t)(k0 + kk) * ldp + m] : 0.0;
      sB[kk * LDB + m] = m < qcols ? Qm[(size_t)(k0 + kk) * ldq + m] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int kq = 0; kq < TKD / 4; ++kq) mfma_tile::step_panel(acc, ln, sA, sB, kq);
    __syncthreads();
  }
}

// U_jc = Dinv_j^T A_jc for the blocks c > j of block row j (a full block row: j < nb - 1), in place.
__global__ __launch_bounds__(256) void chol_panel_kernel(double* __restrict__ L, int N, int j,
                                                         const double* __restrict__ Dinv, int nb) {
  const int s = blockIdx.y, cb = j + 1 + blockIdx.x, tid = threadIdx.x;
  __shared__ double sA[PB * LDA], sB[TKD * LDB];
  double* Q = L + (size_t)s * N * N + (size_t)j * PB * N + (size_t)cb * PB;
  const int qcols = min(PB, N - cb * PB);
  const Lanes ln = mfma_tile::lanes(tid);
  Acc acc;
  ptq_tile(Dinv + ((size_t)s * nb + j) * PB * PB, PB, PB, Q, N, qcols, sA, sB, ln, acc, tid);
  mfma_tile::walk(
      acc, ln,
      [&](int row, int col, double v) {
        if (col < qcols) Q[(size_t)row * N + col] = v;
      },
      [](int) {});
}

// A_ab -= U_ja^T U_jb for j < a <= b, on or above the diagonal only.
__global__ __launch_bounds__(256) void chol_trail_kernel(double* __restrict__ L, int N, int j) {
  const int s = blockIdx.z, a = j + 1 + blockIdx.y, b = j + 1 + blockIdx.x, tid = threadIdx.x;
  if (b < a) return;
  __shared__ double sA[PB * LDA], sB[TKD * LDB];
  double* A = L + (size_t)s * N * N;
  const double* Pm = A + (size_t)j * PB * N + (size_t)a * PB;
  const double* Qm = A + (size_t)j * PB * N + (size_t)b * PB;
  const Lanes ln = mfma_tile::lanes(tid);
  Acc acc;
  ptq_tile(Pm, N, min(PB, N - a * PB), Qm, N, min(PB, N - b * PB), sA, sB, ln, acc, tid);
  mfma_tile::walk(
      acc, ln,
      [&](int row, int col, double v) {
        const int gr = a * PB + row, gc = b * PB + col;
        if (gr < N && gc < N && gc >= gr) A[(size_t)gr * N + gc] -= v;
      },
      [](int) {});
}

// out_s = Ui_s^T v_s (Ui upper triangular, row stride N): a workgroup owns 64 outputs; its four thread groups take the
// rows k = q, q + 4, ... below the block's end and meet in LDS in a fixed order.
__global__ __launch_bounds__(256) void trmv_t_kernel(const double* __restrict__ Ui, int N, const double* __restrict__ v,
                                                     double* __restrict__ out) {
  const int s = blockIdx.y, tid = threadIdx.x, c = tid & 63, q = tid >> 6;
  const int i = blockIdx.x * PB + c, kmax = min(N, (int)(blockIdx.x + 1) * PB);
  __shared__ double sP[4][PB];
  const double* B = Ui + (size_t)s * N * N;
  const double* vs = v + (size_t)s * N;
  double acc = 0.0;
  if (i < N)
    for (int k = q; k < kmax; k += 4) acc = fma(B[(size_t)k * N + i], vs[k], acc);
  sP[q][c] = acc;
  __syncthreads();
  if (q == 0 && i < N) out[(size_t)s * N + i] = (sP[0][c] + sP[1][c]) + (sP[2][c] + sP[3][c]);
}

// out_s = (Ui_s v_s) / div_s: a workgroup owns 64 rows, a wave 16 of them one after the other; the lanes stride over the
// columns from the block's first and are summed by a fixed butterfly.
__global__ __launch_bounds__(256) void trmv_kernel(const double* __restrict__ Ui, int N, const double* __restrict__ v,
                                                   const double* __restrict__ div, double* __restrict__ out) {
  const int s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double* B = Ui + (size_t)s * N * N;
  const double* vs = v + (size_t)s * N;
  const int k0 = blockIdx.x * PB;
  for (int rr = 0; rr < 16; ++rr) {
    const int i = k0 + wave * 16 + rr;  // (wave-uniform)
    if (i >= N) break;
    double acc = 0.0;
    for (int k = k0 + lane; k < N; k += 64) acc = fma(B[(size_t)i * N + k], vs[k], acc);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) out[(size_t)s * N + i] = acc / div[s];
  }
}

// append: k_s = K_s(X, x) / sl_s and the new residual y - m_s(x)
__global__ __launch_bounds__(256) void gp_append_k_kernel(const double* __restrict__ XT, int N, int D, const double* __restrict__ x,
                                                          double y_new, const double* __restrict__ hyp_all, int P, int mean_kind,
                                                          const double* __restrict__ sl, double* __restrict__ kvec,
                                                          double* __restrict__ rnew) {
  const int s = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  const double* hyp = hyp_all + (size_t)s * P;
  if (blockIdx.x == 0 && threadIdx.x == 0) rnew[s] = y_new - post_mean_at(hyp + D + 2, D, mean_kind, x);
  if (i >= N) return;
  double d2 = 0.0;
  for (int d = 0; d < D; ++d) {
    const double ell = exp(hyp[d]);
    const double t = XT[(size_t)d * N + i] / ell - x[d] / ell;
    d2 += t * t;
  }
  kvec[(size_t)s * N + i] = exp(2.0 * hyp[D]) * exp(-0.5 * d2) / sl[s];
}

// append: d_s = sqrt(sf^2 / sl + sn2 / sn2_div - l.l); dd = [d | -d | 1 / d] (S each).  d^2 not positive and finite sets flag[s].
// sn2_new[s * sn2_stride]: the new point's noise variance in sample s.
__global__ __launch_bounds__(256) void gp_append_d_kernel(const double* __restrict__ lvec, int N, int D,
                                                          const double* __restrict__ hyp_all, int P, const double* __restrict__ sl,
                                                          const double* __restrict__ sn2_new, size_t sn2_stride, int S,
                                                          double* __restrict__ dd, int* __restrict__ flag) {
  const int s = blockIdx.x, tid = threadIdx.x;
  __shared__ double sP[256];
  double acc = 0.0;
  for (int i = tid; i < N; i += 256) {
    const double l = lvec[(size_t)s * N + i];
    acc = fma(l, l, acc);
  }
  sP[tid] = acc;
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if (tid < h) sP[tid] += sP[tid + h];
    __syncthreads();
  }
  if (tid == 0) {
    const double* hyp = hyp_all + (size_t)s * P;
    const double a = exp(2.0 * hyp[D]) * exp(-0.0) / sl[s] + sn2_new[(size_t)s * sn2_stride] / sl[s];  // the diagonal entry gp_cov_kernel forms
    const double d2 = a - sP[0];
    double d = 1.0;
    if (d2 > 0.0 && d2 < INFINITY)
      d = sqrt(d2);
    else
      flag[s] = 1;
    dd[s] = d;
    dd[S + s] = -d;
    dd[2 * S + s] = 1.0 / d;
  }
}

// append: M' (N + 1 square) = [[M, colv], [0, corner]] from M (N square), with the new row stride
__global__ __launch_bounds__(256) void gp_restride_kernel(const double* __restrict__ M, int N, const double* __restrict__ colv,
                                                          const double* __restrict__ corner, double* __restrict__ M1) {
  const int s = blockIdx.z, r = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x, N1 = N + 1;
  if (c >= N1) return;
  double v;
  if (r < N)
    v = c < N ? M[((size_t)s * N + r) * N + c] : colv[(size_t)s * N + r];
  else
    v = c < N ? 0.0 : corner[s];
  M1[((size_t)s * N1 + r) * N1 + c] = v;
}

// append: v' (S x (N + 1)) = [v, tail]
__global__ __launch_bounds__(256) void gp_extend_kernel(const double* __restrict__ v, int N, const double* __restrict__ tail,
                                                        double* __restrict__ v1) {
  const int s = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i > N) return;
  v1[(size_t)s * (N + 1) + i] = i < N ? v[(size_t)s * N + i] : tail[s];
}

}  // namespace

// alpha = U^-1 (U^-T r) / sl from ctx->gp's L^-1; t: S N doubles of workspace
static int launch_alpha(vbmc_ctx* ctx, double* t) {
  GpState& g = ctx->gp;
  const int nb = (g.N + PB - 1) / PB;
  hipLaunchKernelGGL(trmv_t_kernel, dim3(nb, g.S), dim3(256), 0, ctx->stream, (const double*)g.d_Linv, g.N,
                     (const double*)g.d_r, t);
  hipLaunchKernelGGL(trmv_kernel, dim3(nb, g.S), dim3(256), 0, ctx->stream, (const double*)g.d_Linv, g.N, (const double*)t,
                     (const double*)g.d_sl, g.d_alpha);
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

int launch_gp_post_build(vbmc_ctx* ctx, double* d_Dinv, int* d_flag) {
  GpState& g = ctx->gp;
  const int N = g.N, S = g.S, nb = (N + PB - 1) / PB;
  hipLaunchKernelGGL(gp_cov_kernel, dim3(nb, nb, S), dim3(256), 0, ctx->stream, (const double*)g.d_XT, (const double*)g.d_X,
                     (const double*)g.d_y, (const double*)g.d_hyp, g.P, N, g.D, g.mean_kind, (const double*)g.d_sn2,
                     (const double*)g.d_sl, g.d_L, g.d_r);
  int rc = timing_begin(ctx, T_GP_POST);
  if (rc) return rc;
  for (int j = 0; j < nb; ++j) {
    hipLaunchKernelGGL(chol_diag_kernel, dim3(S), dim3(64), 0, ctx->stream, g.d_L, N, j, d_flag);
    hipLaunchKernelGGL(chol_dinv_kernel, dim3(S), dim3(64), 0, ctx->stream, (const double*)g.d_L, N, j, d_Dinv, nb);
    if (j + 1 < nb) {
      const int rest = nb - 1 - j;
      hipLaunchKernelGGL(chol_panel_kernel, dim3(rest, S), dim3(256), 0, ctx->stream, g.d_L, N, j, (const double*)d_Dinv, nb);
      hipLaunchKernelGGL(chol_trail_kernel, dim3(rest, rest, S), dim3(256), 0, ctx->stream, g.d_L, N, j);
    }
  }
  if ((rc = timing_end(ctx, T_GP_POST))) return rc;
  HIP_TRY(ctx, hipGetLastError());
  rc = launch_trinv(ctx, d_Dinv);
  if (rc) return rc;
  return launch_alpha(ctx, d_Dinv);  // (the inverted blocks are not read after launch_trinv: S N <= S nb 64^2)
}

GpAppendWs gp_post_append_ws(int S, int N) {
  GpAppendWs w;
  const size_t sn = (size_t)S * N;
  w.flag = gp_post_flags(w.sc, S);
  w.kvec = w.sc.add(sn);
  w.lvec = w.sc.add(sn);
  w.uvec = w.sc.add(sn);
  w.dd = w.sc.add(3 * (size_t)S);
  w.rnew = w.sc.add((size_t)S);
  w.tvec = w.sc.add((size_t)S * (N + 1));
  return w;
}

int launch_gp_post_append(vbmc_ctx* ctx, const GpState& o, double y_new, const double* d_sn2_new, size_t sn2_stride,
                          const GpAppendWs& ws) {
  GpState& g = ctx->gp;
  const int N = o.N, S = o.S, N1 = N + 1, nb = (N + PB - 1) / PB;
  const Scratch& sc = ws.sc;
  double *kvec = sc.ptr(ws.kvec), *lvec = sc.ptr(ws.lvec), *uvec = sc.ptr(ws.uvec), *dd = sc.ptr(ws.dd), *rnew = sc.ptr(ws.rnew);
  double* tvec = sc.ptr(ws.tvec);
  int* d_flag = sc.ptr(ws.flag);
  const double* x = g.d_X + (size_t)N * g.D;
  hipLaunchKernelGGL(gp_append_k_kernel, dim3((N + 255) / 256, S), dim3(256), 0, ctx->stream, (const double*)o.d_XT, N, o.D, x,
                     y_new, (const double*)o.d_hyp, o.P, o.mean_kind, (const double*)o.d_sl, kvec, rnew);
  hipLaunchKernelGGL(trmv_t_kernel, dim3(nb, S), dim3(256), 0, ctx->stream, (const double*)o.d_Linv, N, (const double*)kvec, lvec);
  hipLaunchKernelGGL(gp_append_d_kernel, dim3(S), dim3(256), 0, ctx->stream, (const double*)lvec, N, o.D, (const double*)o.d_hyp,
                     o.P, (const double*)o.d_sl, d_sn2_new, sn2_stride, S, dd, d_flag);
  hipLaunchKernelGGL(trmv_kernel, dim3(nb, S), dim3(256), 0, ctx->stream, (const double*)o.d_Linv, N, (const double*)lvec,
                     (const double*)(dd + S), uvec);
  const dim3 rg((N1 + 255) / 256, N1, S);
  hipLaunchKernelGGL(gp_restride_kernel, rg, dim3(256), 0, ctx->stream, (const double*)o.d_L, N, (const double*)lvec,
                     (const double*)dd, g.d_L);
  hipLaunchKernelGGL(gp_restride_kernel, rg, dim3(256), 0, ctx->stream, (const double*)o.d_Linv, N, (const double*)uvec,
                     (const double*)(dd + 2 * S), g.d_Linv);
  hipLaunchKernelGGL(gp_extend_kernel, dim3((N1 + 255) / 256, S), dim3(256), 0, ctx->stream, (const double*)o.d_r, N,
                     (const double*)rnew, g.d_r);
  HIP_TRY(ctx, hipGetLastError());
  int rc = launch_pad_linv(ctx);
  if (rc) return rc;
  return launch_alpha(ctx, tvec);
}
