// GP hyper-parameter sampling (vbmc_gp_hyp_sample): C slice-sampling chains over f(h) = lml(h) + log p(h), in lockstep.
//
// One evaluation of lml is the launch sequence of launch_gp_post_build + launch_gp_lml, not something one workgroup does
// in LDS, so the chain cannot be one persistent kernel like acq_is_mcmc.hip's.  It is a state machine in global memory
// that one launch of gp_hyp_advance_kernel moves on by one evaluation: workgroup = chain, lane 0 consumes the value the
// round before produced (lml[c], flag[c]), makes every draw and decision until the next point is known, and the
// workgroup writes that point as the chain's candidate straight into the buffers the factorisation reads (its hyp row,
// sl, smeta, the cleared flag and its N noise variances).  The host queues advance / build / value rounds in plain
// stream order (api_gp_hyp.hip).
//
// The sampler is the one tests/slice_host.py states (Neal 2003, coordinate-wise, stepping out capped at 32 evaluations a
// side, shrinkage capped at 64 proposals, the keep rule after sweeps); draw i of chain c is the 53-bit uniform of Philox
// block (i_lo, i_hi, c, 6) (stream 6 of sample.hip's list), the level's in the (0, 1] form.  The transitions are those
// of acq_is_mcmc.hip's chain_advance.
//
// The prior: log p(h) = sum_p t_p, p ascending; t_p = 0 without a prior (sigma NaN), else with z = (h_p - mu_p) / sigma_p
//   t_p = c_p - 1/2 z^2 (df = +inf) or c_p - (df + 1) / 2 log(1 + z^2 / df);  c_p is the host's (gp_cand_host.h).
//
// A finished (or invalid) chain's workgroup still writes its last candidate, so every slot of a chunk stays a valid
// input of the factorisation; its state and outputs no longer change.  No atomics on global memory, no waiting on other
// workgroups: a chain's results depend on its own inputs alone.
#include <cmath>

#include "common.h"
#include "fastmath.h"
#include "gp_cand.h"
#include "mixture_dev.h"

namespace {

constexpr int HY_OUT_CAP = 32, HY_SHRINK_CAP = 64;
constexpr uint32_t HY_STREAM = 6;
constexpr int HY_PMAX = 128;  // >= 32 + 2 + 65 parameters

// ST_START = 0: a zeroed state is a chain that has not looked at its x0 yet
enum { ST_START = 0, ST_INIT, ST_BEGIN, ST_TRY_L, ST_RES_L, ST_TRY_R, ST_RES_R, ST_PROPOSE, ST_RES_S, ST_NEXT };

struct HypChain {
  int st, d, j, kept, done, pad;
  long long t, evals, caps_out, caps_shrink;
  uint64_t draws;
  double fx, cprior;         // f and the log prior at the current x
  double ly, Lo, Hi;         // the level and the interval
  double xd, xprop, wd, lbd, ubd;
  double val, vprior;        // the evaluation just done
  double pprior;             // log prior of the candidate under evaluation
};
static_assert(sizeof(HypChain) % sizeof(double) == 0, "HypChain is carved in doubles");

__device__ __forceinline__ double hyp_draw(const GpHypArgs& a, HypChain& cs, int c, bool pos) {
  const Philox4 r = philox_block(cs.draws++, (uint32_t)c, HY_STREAM, a.seed);
  return pos ? philox_u53_pos(r.x[0], r.x[1]) : philox_u53(r.x[0], r.x[1]);
}

__device__ __forceinline__ void hyp_finish(const GpHypArgs& a, HypChain& cs, int c) {
  long long* so = a.stats + 4 * (size_t)c;
  so[0] = cs.evals;
  so[1] = (long long)cs.draws;
  so[2] = cs.caps_out;
  so[3] = cs.caps_shrink;
  cs.done = 1;
}

// Lane 0 between two evaluations: consumes cs.val and runs until the next point stands in xp or the chain has ended.
// Every path through the loop reaches one of the two: a coordinate update evaluates at its first shrink proposal at the
// latest, and the sweeps are counted.
__device__ __forceinline__ void hyp_advance(const GpHypArgs& a, HypChain& cs, int c, double* x, double* xp) {
  const int P = a.P;
  const long long sweeps = (long long)a.burn_in + (long long)a.n * a.thin;
  bool decided = false;
  while (!decided) {
    switch (cs.st) {
      case ST_START: {  // x0 clipped into the box (a NaN stays one: that start is invalid without an evaluation)
        bool finite = true;
        for (int p = 0; p < P; ++p) {
          const double v0 = a.x0[(size_t)c * P + p];
          const double v = v0 != v0 ? v0 : fmax(fmin(v0, a.ub[p]), a.lb[p]);
          x[p] = v;
          xp[p] = v;
          finite = finite && fabs(v) < INFINITY;
        }
        if (!finite) {
          a.invalid[c] = 1;
          cs.done = 1;
        } else {
          cs.st = ST_INIT;
        }
        decided = true;
        break;
      }
      case ST_INIT:  // f(x0)
        ++cs.evals;
        if (!(fabs(cs.val) < INFINITY)) {
          a.invalid[c] = 1;
          cs.done = 1;
          decided = true;
          break;
        }
        cs.fx = cs.val; cs.cprior = cs.vprior;
        cs.st = ST_BEGIN;  // (n, thin >= 1: there is a sweep)
        break;
      case ST_BEGIN: {  // coordinate cs.d of sweep cs.t: level and interval
        cs.xd = x[cs.d]; cs.wd = a.widths[cs.d]; cs.lbd = a.lb[cs.d]; cs.ubd = a.ub[cs.d];
        cs.ly = cs.fx + log(hyp_draw(a, cs, c, true));
        cs.Lo = cs.xd - cs.wd * hyp_draw(a, cs, c, false);
        cs.Hi = cs.Lo + cs.wd;
        cs.Lo = fmax(cs.Lo, cs.lbd);
        cs.Hi = fmin(cs.Hi, cs.ubd);
        cs.j = 0;
        cs.st = ST_TRY_L;
        break;
      }
      case ST_TRY_L:
        if (cs.Lo <= cs.lbd) { cs.j = 0; cs.st = ST_TRY_R; break; }
        if (cs.j == HY_OUT_CAP) { ++cs.caps_out; cs.j = 0; cs.st = ST_TRY_R; break; }
        xp[cs.d] = cs.Lo;
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
        if (cs.j == HY_OUT_CAP) { ++cs.caps_out; cs.j = 0; cs.st = ST_PROPOSE; break; }
        xp[cs.d] = cs.Hi;
        cs.st = ST_RES_R;
        decided = true;
        break;
      case ST_RES_R:
        ++cs.evals;
        if (cs.val <= cs.ly) { cs.j = 0; cs.st = ST_PROPOSE; }
        else { cs.Hi = fmin(cs.Hi + cs.wd, cs.ubd); ++cs.j; cs.st = ST_TRY_R; }
        break;
      case ST_PROPOSE:
        if (cs.j == HY_SHRINK_CAP) { ++cs.caps_shrink; cs.st = ST_NEXT; break; }  // x_d stays
        cs.xprop = cs.Lo + hyp_draw(a, cs, c, false) * (cs.Hi - cs.Lo);
        xp[cs.d] = cs.xprop;
        cs.st = ST_RES_S;
        decided = true;
        break;
      case ST_RES_S:
        ++cs.evals;
        if (cs.val > cs.ly) {
          x[cs.d] = cs.xprop;
          cs.fx = cs.val; cs.cprior = cs.vprior;
          cs.st = ST_NEXT;
        } else {
          if (cs.xprop < cs.xd) cs.Lo = cs.xprop; else cs.Hi = cs.xprop;
          ++cs.j;
          cs.st = ST_PROPOSE;
        }
        break;
      default:  // ST_NEXT: the next coordinate; after the last one of a sweep, keep the sample
        xp[cs.d] = x[cs.d];
        cs.st = ST_BEGIN;
        if (++cs.d == P) {
          cs.d = 0;
          if (cs.t >= a.burn_in && (cs.t - a.burn_in + 1) % a.thin == 0 && cs.kept < a.n) {
            double* xo = a.hyp_out + ((size_t)c * a.n + cs.kept) * P;
            for (int q = 0; q < P; ++q) xo[q] = x[q];
            a.logpost[(size_t)c * a.n + cs.kept] = cs.fx;
            a.logprior[(size_t)c * a.n + cs.kept] = cs.cprior;
            ++cs.kept;
          }
          if (++cs.t == sweeps) {
            hyp_finish(a, cs, c);
            decided = true;
          }
        }
        break;
    }
  }
}

__global__ __launch_bounds__(256) void gp_hyp_advance_kernel(GpHypArgs a, int b0, int S, int state_elems) {
  const int tid = threadIdx.x, slot = blockIdx.x, c = b0 + slot;
  if (slot >= S || c >= a.C) return;  // (uniform per workgroup)
  const int N = a.N, D = a.D, P = a.P;
  __shared__ double s_t[HY_PMAX];
  HypChain& cs = *(HypChain*)(a.state + (size_t)c * state_elems);
  double* x = a.x + (size_t)c * P;
  double* xp = a.xp + (size_t)c * P;

  // ---- 1. lane 0: the value of the round before, then draws and decisions up to the next point
  if (tid == 0) {
    if (!cs.done) {
      if (cs.st != ST_START) {
        const double v = a.lml[c];
        const bool bad = a.flag[c] != 0 || !(fabs(v) < INFINITY);
        const double f = v + cs.pprior;
        cs.val = bad || !(fabs(f) < INFINITY) ? -INFINITY : f;
        cs.vprior = cs.pprior;
      }
      hyp_advance(a, cs, c, x, xp);
    }
    a.flag[c] = 0;
  }
  __syncthreads();  // xp (global memory, written by lane 0)

  // ---- 2. the candidate (gp_cand.h, shared with gp_opt.hip): xp with a coordinate that is not finite (an invalid start)
  // replaced by its lower bound, so the factorisation of this slot never reads one
  if (tid < P) {
    const double h = gp_cand_coord(xp, a.lb, tid, slot, P, a.g_hyp);
    s_t[tid] = gp_prior_term(a.pmu, a.psig, a.pdf, a.pconst, tid, h);  // its term of the log prior
  }
  __syncthreads();
  if (tid == 0) {
    double lp = 0.0;
    for (int p = 0; p < P; ++p) lp += s_t[p];
    if (!cs.done) cs.pprior = lp;
  }
  // ---- 3. its noise: sn2_n = exp(2 h[D + 1]) + s2_n, sl = sn2_div = min_n sn2_n (sn2_mult = 1)
  gp_cand_noise<256>(tid, slot, N, D, xp, a.lb, a.s2, a.s2_min, a.g_sn2, a.g_sl, a.g_smeta);
}

}  // namespace

size_t gp_hyp_state_elems() { return sizeof(HypChain) / sizeof(double); }
LockstepWord gp_hyp_done_word() { return {gp_hyp_state_elems(), offsetof(HypChain, done), 1}; }  // (done: 0 or 1)

int launch_gp_hyp_advance(vbmc_ctx* ctx, const GpHypArgs& a, int b0, int S) {
  if (a.P > HY_PMAX) return vbmc_fail(ctx, VBMC_E_ARG, "gp_hyp: P=%d > %d", a.P, HY_PMAX);
  hipLaunchKernelGGL(gp_hyp_advance_kernel, dim3(S), dim3(256), 0, ctx->stream, a, b0, S, (int)gp_hyp_state_elems());
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}
