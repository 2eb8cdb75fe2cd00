// Step 2 of active_importance_sampling (vbmc/active_importance_sampling.py:195-262) as ONE launch: the S slice-sampling
// chains of the IMIQR / VIQR importance state, one workgroup per GP hyper-parameter sample.
//
// The sampler is Neal's (2003) coordinate-wise slice sampler with stepping out and shrinkage, as tests/slice_host.py
// states it (the reference's own sampler class, gpyreg's, is not part of the reference tree: this is not its stream).
// Chain s runs burn_in + n thin sweeps over d = 0 .. D-1; a coordinate update draws the level ly = f(x) + log u, places
// an interval of width widths_d around x_d, steps it out (at most 32 evaluations a side) while f at its end is above ly,
// then shrinks it (at most 64 proposals) until a proposal lies above ly.  Draw i of chain s is the 53-bit uniform of
// Philox block (i_lo, i_hi, s, 6) (stream 6 of sample.hip's list); the level takes the (0, 1] form.
//
// The target is the acquisition's is_log_full over gp.predict(add_noise=True) of the one-sample GP:
//   f(x) = [ln_y_fmu ? f_mu : 0] + u f_s + log1p(-exp(-2 u f_s)),   f_s = sqrt(f_s2 + sn2 sn2_mult),
//   k_n = k(x, X_n) (se_ard_direct), f_mu = m(x) + k.alpha, f_s2 = max(0, sf^2 - |L^-T (sW o k)|^2) or max(0, sf^2 + k'Lk)
// (predict_point_moments of gp_dev.h finishes both), one evaluation at a time: every thread takes part in it.
//   1. k (times sW for a Cholesky sample) goes to LDS, the partial sums of k.alpha to one slot per wave;
//   2. the product with L^-1 (upper triangular, row-major: column c = sum over rows n <= c) or L: thread = (column,
//      row stripe); a wave's 64 lanes read 64 consecutive doubles of a row, the stripes split the rows of a column
//      when the workgroup has more threads than the matrix has columns;
//   3. the stripes of a column are added in stripe order, squared (or multiplied by k) and summed: wave sums by DPP,
//      one slot per wave;
//   4. thread 0 adds the slots in wave order and finishes f.  No atomics: a chain is bit-reproducible.
//
// Control.  Thread 0 alone holds the chain's state machine; between two evaluations it consumes the value, makes every
// draw and decision, and leaves either the next point in LDS or the word "done".  The ONLY data-dependent branch the
// other threads take is on that one LDS word, read after a barrier, so all waves are in the same branch at every
// __syncthreads(); the loop that carries it is also bounded by the chain's largest possible number of evaluations.
#include <cmath>

#include "common.h"
#include "fastmath.h"
#include "gp_dev.h"
#include "mixture_dev.h"

namespace {

constexpr int MC_OUT_CAP = 32, MC_SHRINK_CAP = 64;  // evaluations per side while stepping out / proposals while shrinking
constexpr int MC_DMAX = 32;
constexpr uint32_t MC_STREAM = 6;

struct McmcArgs {
  PredView v;  // (xs is set by the kernel: the point under evaluation, in LDS)
  const double *X, *alpha, *sW, *Linv, *L;
  int N, ln_y_fmu;
  double u_q;
  const double *x0, *widths, *lb, *ub;  // x0 [S][D]
  int n, thin, burn_in;
  uint64_t seed;
  long long max_evals;                  // loop bound: 1 + sweeps D (2 MC_OUT_CAP + MC_SHRINK_CAP)
  double *Xout, *logp, *fmu, *fs2;      // [S][n][D], [S][n], [n][S], [n][S]
  long long* stats;                     // [S][4]: evaluations, draws, step-out caps, shrink caps
  int* invalid;                         // [S]
};

// states of thread 0's machine: what the evaluation just done was for / what comes next
enum { ST_INIT, ST_BEGIN, ST_TRY_L, ST_RES_L, ST_TRY_R, ST_RES_R, ST_PROPOSE, ST_RES_S, ST_NEXT };

struct ChainState {  // (lives in LDS: no initialisers; thread 0 calls reset())
  int st, d, j, kept;
  long long t, evals, caps_out, caps_shrink;
  uint64_t draws;
  double fx, cfmu, cfs2;             // f, f_mu and the noise-free f_s2 at the current x
  double ly, Lo, Hi;                 // the level and the interval
  double xd, xprop, wd, lbd, ubd;    // coordinate d: its value, the proposal, width and bounds
  double val, vfmu, vfs2;            // the evaluation just done
  double noise;                      // sn2 sn2_mult of this GP sample
  __device__ void reset() {
    st = ST_INIT; d = j = kept = 0;
    t = evals = caps_out = caps_shrink = 0;
    draws = 0;
    fx = cfmu = cfs2 = ly = Lo = Hi = xd = xprop = wd = lbd = ubd = val = vfmu = vfs2 = noise = 0.0;
  }
};

// what thread 0's machine reads and writes besides the chain state: the workgroup's LDS arrays
struct ChainLds {
  double *x, *xp;              // the current point; the point under evaluation (x with one coordinate replaced)
  const double *w, *lb, *ub;
  int smp, S, D;
  long long sweeps;
};

__device__ __forceinline__ double chain_draw(const McmcArgs& a, ChainState& cs, int smp, bool pos) {
  const Philox4 r = philox_block(cs.draws++, (uint32_t)smp, MC_STREAM, a.seed);
  return pos ? philox_u53_pos(r.x[0], r.x[1]) : philox_u53(r.x[0], r.x[1]);
}

// Thread 0, between two evaluations: consumes cs.val, draws and decides until the next point stands in k.xp (returns
// true) or the chain has ended (false).  Every path through the loop below reaches one of the two: a coordinate update
// evaluates at its first shrink proposal at the latest, and the sweeps are counted.
__device__ __forceinline__ bool chain_advance(const McmcArgs& a, ChainState& cs, const ChainLds& k, bool first) {
  // consume the value of the evaluation just done (none before the first), then run until the next point is set
  bool go = true, decided = first;  // (first: the point is x0 itself)
  while (!decided) {
    switch (cs.st) {
      case ST_INIT:  // f(x0)
        ++cs.evals;
        if (!(fabs(cs.val) < INFINITY)) {
          a.invalid[k.smp] = 1;
          go = false;
          decided = true;
          break;
        }
        cs.fx = cs.val; cs.cfmu = cs.vfmu; cs.cfs2 = cs.vfs2;
        cs.st = ST_BEGIN;  // (n, thin >= 1: there is a sweep)
        break;
      case ST_BEGIN: {  // coordinate cs.d of sweep cs.t: level and interval
        cs.xd = k.x[cs.d]; cs.wd = k.w[cs.d]; cs.lbd = k.lb[cs.d]; cs.ubd = k.ub[cs.d];
        cs.ly = cs.fx + log(chain_draw(a, cs, k.smp, true));
        cs.Lo = cs.xd - cs.wd * chain_draw(a, cs, k.smp, false);
        cs.Hi = cs.Lo + cs.wd;
        cs.Lo = fmax(cs.Lo, cs.lbd);
        cs.Hi = fmin(cs.Hi, cs.ubd);
        cs.j = 0;
        cs.st = ST_TRY_L;
        break;
      }
      case ST_TRY_L:
        if (cs.Lo <= cs.lbd) { cs.j = 0; cs.st = ST_TRY_R; break; }
        if (cs.j == MC_OUT_CAP) { ++cs.caps_out; cs.j = 0; cs.st = ST_TRY_R; break; }
        k.xp[cs.d] = cs.Lo;
        cs.st = ST_RES_L;
        decided = true;
        break;
      case ST_RES_L:
        ++cs.evals;
        if (cs.val <= cs.ly) { cs.j = 0; cs.st = ST_TRY_R; }
        else { cs.Lo = fmax(cs.Lo - cs.wd, cs.lbd); ++cs.j; cs.st = ST_TRY_L; }
        break;
      case ST_TRY_R:
        if (cs.Hi >= cs.ubd) { cs.j = 0; cs.st = ST_PROPOSE; break; }
        if (cs.j == MC_OUT_CAP) { ++cs.caps_out; cs.j = 0; cs.st = ST_PROPOSE; break; }
        k.xp[cs.d] = cs.Hi;
        cs.st = ST_RES_R;
        decided = true;
        break;
      case ST_RES_R:
        ++cs.evals;
        if (cs.val <= cs.ly) { cs.j = 0; cs.st = ST_PROPOSE; }
        else { cs.Hi = fmin(cs.Hi + cs.wd, cs.ubd); ++cs.j; cs.st = ST_TRY_R; }
        break;
      case ST_PROPOSE:
        if (cs.j == MC_SHRINK_CAP) { ++cs.caps_shrink; cs.st = ST_NEXT; break; }  // x_d stays
        cs.xprop = cs.Lo + chain_draw(a, cs, k.smp, false) * (cs.Hi - cs.Lo);
        k.xp[cs.d] = cs.xprop;
        cs.st = ST_RES_S;
        decided = true;
        break;
      case ST_RES_S:
        ++cs.evals;
        if (cs.val > cs.ly) {
          k.x[cs.d] = cs.xprop;
          cs.fx = cs.val; cs.cfmu = cs.vfmu; cs.cfs2 = cs.vfs2;
          cs.st = ST_NEXT;
        } else {
          if (cs.xprop < cs.xd) cs.Lo = cs.xprop; else cs.Hi = cs.xprop;
          ++cs.j;
          cs.st = ST_PROPOSE;
        }
        break;
      default:  // ST_NEXT: the next coordinate; after the last one of a sweep, keep the sample
        k.xp[cs.d] = k.x[cs.d];
        cs.st = ST_BEGIN;
        if (++cs.d == k.D) {
          cs.d = 0;
          if (cs.t >= a.burn_in && (cs.t - a.burn_in + 1) % a.thin == 0 && cs.kept < a.n) {
            double* xo = a.Xout + ((size_t)k.smp * a.n + cs.kept) * k.D;
            for (int q = 0; q < k.D; ++q) xo[q] = k.x[q];
            a.logp[(size_t)k.smp * a.n + cs.kept] = cs.fx;
            a.fmu[(size_t)cs.kept * k.S + k.smp] = cs.cfmu;
            a.fs2[(size_t)cs.kept * k.S + k.smp] = cs.cfs2;
            ++cs.kept;
          }
          if (++cs.t == k.sweeps) { go = false; decided = true; }
        }
        break;
    }
  }
  return go;
}

template <int NT>
__global__ __launch_bounds__(NT) void is_mcmc_kernel(McmcArgs a) {
  extern __shared__ __attribute__((aligned(16))) double dyn[];
  constexpr int NW = NT / 64;
  __shared__ double s_x[MC_DMAX], s_xp[MC_DMAX], s_w[MC_DMAX], s_lb[MC_DMAX], s_ub[MC_DMAX], s_iell[MC_DMAX];
  __shared__ double s_wf[NW], s_ws[NW];
  __shared__ int s_go;
  __shared__ ChainState s_chain;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int smp = blockIdx.x, S = gridDim.x;
  const int N = a.N, D = a.v.D;
  double* kk = dyn;         // [N]  k (non-Cholesky) or sW o k
  double* part = dyn + N;   // [R][N] stripe sums of the matrix-vector product
  const double* hyp = a.v.hyp_all + (size_t)smp * a.v.P;
  const bool chol = a.v.smeta[3 * smp] != 0.0;
  const double* B = (chol ? a.Linv : a.L) + (size_t)smp * N * N;
  const double* alpha = a.alpha + (size_t)smp * N;
  const double* sW = a.sW + (size_t)smp * N;
  const double lsf2 = 2.0 * hyp[D];
  // thread = (column col, row stripe): CP columns at a time, R stripes
  const int CP = min((N + 63) / 64 * 64, NT), R = NT / CP;
  const int col = tid % CP, stripe = tid / CP;  // (stripe >= R: no matrix work; CP is a multiple of 64: uniform per wave)
  if (tid < D) {
    s_w[tid] = a.widths[tid];
    s_lb[tid] = a.lb[tid];
    s_ub[tid] = a.ub[tid];
    s_iell[tid] = exp(-hyp[tid]);
    const double x = fmax(fmin(a.x0[(size_t)smp * D + tid], a.ub[tid]), a.lb[tid]);
    s_x[tid] = x;
    s_xp[tid] = x;
  }
  PredView view = a.v;
  view.xs = s_xp;
  view.add_noise = 0;

  // ---- thread 0's chain state (in LDS: it is touched between evaluations only, and registers are what bounds the
  // workgroup size)
  ChainState& cs = s_chain;
  if (tid == 0) {
    cs.reset();
    cs.noise = predict_noise_add(a.v, smp);
  }
  const long long sweeps = (long long)a.burn_in + (long long)a.n * a.thin;
  const ChainLds lds = {s_x, s_xp, s_w, s_lb, s_ub, smp, S, D, sweeps};

  for (long long it = 0; it <= a.max_evals; ++it) {
    if (tid == 0) s_go = chain_advance(a, cs, lds, it == 0) ? 1 : 0;
    __syncthreads();  // the point s_xp and the word s_go
    if (s_go == 0) break;

    // ---- 1. k at the point, and the partial sums of k . alpha
    double pf = 0.0;
#pragma unroll 1
    for (int n = tid; n < N; n += NT) {
      const double k = se_ard_direct(s_xp, a.X + (size_t)n * D, D, [&](int q) { return s_iell[q]; }, lsf2);
      kk[n] = chol ? k * sW[n] : k;
      pf = fma(k, alpha[n], pf);
    }
    pf = fm::wave_sum_dpp(pf);
    if (lane == 0) s_wf[wave] = pf;
    __syncthreads();
    // ---- 2. stripe sums of column c of the product: rows n <= c of L^-1, every row of L
    if (stripe < R) {
      for (int c = col; c < N; c += CP) {
        const int nend = chol ? c + 1 : N;
        // eight rows in flight per step (fixed order: stripe rows n, n + R, ..., n + 7 R into eight sums)
        const size_t step = (size_t)R * N;
        const double* p = B + (size_t)stripe * N + c;
        double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        int n = stripe;
#pragma unroll 1
        for (; n + 7 * R < nend; n += 8 * R, p += 8 * step) {
          double b[8];
#pragma unroll
          for (int q = 0; q < 8; ++q) b[q] = p[q * step];
#pragma unroll
          for (int q = 0; q < 8; ++q) acc[q] = fma(b[q], kk[n + q * R], acc[q]);
        }
#pragma unroll 1
        for (; n < nend; n += R, p += step) acc[0] = fma(p[0], kk[n], acc[0]);
        const double a0 = acc[0] + acc[4], a1 = acc[1] + acc[5], a2 = acc[2] + acc[6], a3 = acc[3] + acc[7];
        part[(size_t)stripe * N + c] = (a0 + a1) + (a2 + a3);
      }
    }
    __syncthreads();
    // ---- 3. |L^-T (sW o k)|^2 or k' L k
    double ps = 0.0;
    for (int c = tid; c < N; c += NT) {
      double tc = part[c];
      for (int r = 1; r < R; ++r) tc += part[(size_t)r * N + c];
      ps = chol ? fma(tc, tc, ps) : fma(kk[c], tc, ps);
    }
    ps = fm::wave_sum_dpp(ps);
    if (lane == 0) s_ws[wave] = ps;
    __syncthreads();
    // ---- 4. the value
    if (tid == 0) {
      double ssum = 0.0, fsum = 0.0;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        ssum += s_ws[w];
        fsum += s_wf[w];
      }
      double mu, s2;
      predict_point_moments(view, smp, 0, ssum, fsum, mu, s2);
      const double f_s = sqrt(s2 + cs.noise);
      const double added = a.u_q * f_s + log1p(-exp(-2.0 * a.u_q * f_s));
      cs.vfmu = mu;
      cs.vfs2 = s2;
      cs.val = a.ln_y_fmu ? mu + added : added;
    }
    // (no barrier here: thread 0 goes on alone to the decision, everyone else waits for it at the top of the loop)
  }
  if (tid == 0) {
    long long* so = a.stats + 4 * (size_t)smp;
    so[0] = cs.evals;
    so[1] = (long long)cs.draws;
    so[2] = cs.caps_out;
    so[3] = cs.caps_shrink;
  }
}

template <int NT>
int launch_nt(vbmc_ctx* ctx, int S, size_t lds, const McmcArgs& a) {
  static size_t lds_set[64] = {};
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (lds > 48 * 1024 && lds > lds_set[dev & 63]) {
    HIP_TRY(ctx, hipFuncSetAttribute((const void*)is_mcmc_kernel<NT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    lds_set[dev & 63] = lds;
  }
  hipLaunchKernelGGL(is_mcmc_kernel<NT>, dim3(S), dim3(NT), lds, ctx->stream, a);
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

}  // namespace

// dynamic LDS of one chain's workgroup: k and the stripe sums
size_t is_mcmc_lds_bytes(int N, int threads) {
  return sizeof(double) * ((size_t)N + (size_t)(N > threads ? N : threads));
}

// All S chains of the context's GP on ctx->stream.  The device pointers: x0 [S][D], widths / lb / ub [D]; outputs
// Xout [S][n][D], logp [S][n], fmu / fs2 [n][S], stats [S][4], invalid [S] (zeroed by the caller).
int launch_is_mcmc(vbmc_ctx* ctx, int ln_y_fmu, double u_q, const double* d_x0, const double* d_widths, const double* d_lb,
                   const double* d_ub, int n, int thin, int burn_in, uint64_t seed, double* d_X, double* d_logp,
                   double* d_fmu, double* d_fs2, long long* d_stats, int* d_invalid) {
  const GpState& g = ctx->gp;
  McmcArgs a;
  a.v = gp_pred_view(g, nullptr, 0);
  a.X = g.d_X; a.alpha = g.d_alpha; a.sW = g.d_sW; a.Linv = g.d_Linv; a.L = g.d_L;
  a.N = g.N; a.ln_y_fmu = ln_y_fmu; a.u_q = u_q;
  a.x0 = d_x0; a.widths = d_widths; a.lb = d_lb; a.ub = d_ub;
  a.n = n; a.thin = thin; a.burn_in = burn_in; a.seed = seed;
  a.max_evals = 1 + ((long long)burn_in + (long long)n * thin) * g.D * (2 * MC_OUT_CAP + MC_SHRINK_CAP);
  a.Xout = d_X; a.logp = d_logp; a.fmu = d_fmu; a.fs2 = d_fs2; a.stats = d_stats; a.invalid = d_invalid;
  const int nt = ctx->opt_is_mcmc_threads;
  const size_t lds = is_mcmc_lds_bytes(g.N, nt);
  if (nt == 256) return launch_nt<256>(ctx, g.S, lds, a);
  if (nt == 768) return launch_nt<768>(ctx, g.S, lds, a);
  return launch_nt<512>(ctx, g.S, lds, a);
}
