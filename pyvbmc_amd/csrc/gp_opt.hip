// GP hyper-parameter optimisation (vbmc_gp_hyp_optimize): R quasi-Newton runs over phi(h) = -(lml(h) + log p(h)) inside
// the box [lb, ub], in lockstep.
//
// As with the slice chains (gp_hyp.hip), one evaluation is the launch sequence launch_gp_post_build + launch_gp_lml, so
// a run is a state machine in global memory that one launch of gp_opt_advance_kernel moves on by one evaluation:
// workgroup = run, ONE wave.  It consumes the value, gradient and factorisation flag the round before produced, adds
// the prior's value and gradient, takes every decision until the next trial point is known, and writes that point as
// the run's candidate straight into the buffers the factorisation reads (gp_cand.h, shared with gp_hyp.hip).  The host
// queues advance / build / value+gradient rounds in plain stream order (api_gp_opt.hip).
//
// The optimiser is the package's own (tests/gp_opt_host.py states it in NumPy; it is not SciPy's L-BFGS-B), g = grad phi:
//   start      x0 clipped into the box; phi0 not finite: the run is invalid.
//   bound set  B = {p : (x_p <= lb_p and g_p > 0) or (x_p >= ub_p and g_p < 0) or lb_p = ub_p}; pg = g, 0 on B.
//   iteration  stop on max |pg| <= tol_g (reason 1), then on iter = max_iter (2).  d = -H pg by the two-loop recursion
//              over the stored pairs, oldest to newest, scaled by gamma = s.y / y.y of the newest pair, 0 on B; g.d >= 0
//              or no pairs: the history is dropped and d = -pg.  First trial step 1 with pairs, min(1, 1 / sum |pg|)
//              without.
//   search     x_t = clip(x + t d); accepted when phi(x_t) is finite and phi(x_t) <= phi(x) + 1e-4 g.(x_t - x), else
//              t <- t / 2, at most 30 times (then reason 4).  A trial that does not factorise is a rejection.
//   update     s = x_t - x, y = g_t - g, stored when s.y > 1e-10 |s| |y| (over the oldest when m are held); then stop on
//              phi_old - phi_new <= tol_f max(1, |phi_new|) (reason 3).
// P reaches 99 (D = 32, negative-quadratic mean): lane l holds the entries l and l + 64 of every vector, and a dot
// product is the two products of a lane added, then fastmath.h's wave sum -- one fixed order, so a run's results depend
// on its own inputs alone.  No atomics on global memory, no waiting on other workgroups.
//
// A finished (or invalid) run's workgroup still writes its final point as its candidate, so every slot of a chunk stays
// a valid input of the factorisation; its state and outputs no longer change.
#include <cmath>

#include "common.h"
#include "fastmath.h"
#include "gp_cand.h"

namespace {

constexpr int OP_PMAX = 128;  // >= 32 + 2 + 65 parameters: two entries a lane
constexpr int OP_MMAX = 16, OP_HALVINGS = 30;
constexpr double OP_ARMIJO = 1e-4, OP_CURV = 1e-10;

// ST_START = 0: a zeroed state is a run that has not looked at its x0 yet
enum { ST_START = 0, ST_INIT, ST_SEARCH };
enum { STOP_TOL_G = 1, STOP_MAX_ITER, STOP_TOL_F, STOP_SEARCH };

// the scalars of a run; behind them x, g, d, x_t (P each), S, Y (m x P each), rho (m)
struct OptRun {
  int st, done, iter, npairs, head, halv, reason, pad;
  long long evals, resets;
  double phi, t, gamma;
};
static_assert(sizeof(OptRun) % sizeof(double) == 0, "OptRun is carved in doubles");

__device__ __forceinline__ double dot2(const double (&u)[2], const double (&v)[2]) {
  return fm::wave_sum_dpp(u[0] * v[0] + u[1] * v[1]);
}

__global__ __launch_bounds__(64) void gp_opt_advance_kernel(GpOptArgs a, int b0, int S, int state_elems) {
  const int lane = threadIdx.x, slot = blockIdx.x, r = b0 + slot;
  if (slot >= S || r >= a.R) return;  // (uniform per workgroup)
  const int N = a.N, D = a.D, P = a.P, m = a.m;
  __shared__ double s_t[OP_PMAX];
  __shared__ double s_al[OP_MMAX];
  double* base = a.state + (size_t)r * state_elems;
  OptRun* rs = (OptRun*)base;
  double* vx = base + sizeof(OptRun) / sizeof(double);
  double *vg = vx + P, *vd = vg + P, *vxt = vd + P, *vS = vxt + P;
  double *vY = vS + (size_t)m * P, *vrho = vY + (size_t)m * P;
  OptRun h = *rs;  // every lane carries the scalars; lane 0 writes them back
  const bool on[2] = {lane < P, lane + 64 < P};
  const int pp[2] = {lane, lane + 64};
  double lb[2], ub[2];
  for (int k = 0; k < 2; ++k) {
    lb[k] = on[k] ? a.lb[pp[k]] : 0.0;
    ub[k] = on[k] ? a.ub[pp[k]] : 0.0;
  }

  if (!h.done) {
    bool begin = false, stop = false;
    double x[2] = {0.0, 0.0}, g[2] = {0.0, 0.0}, d[2] = {0.0, 0.0};
    if (h.st == ST_START) {  // x0 clipped into the box (a NaN stays one: that start is invalid without an evaluation)
      double bad = 0.0;
      for (int k = 0; k < 2; ++k)
        if (on[k]) {
          const double v0 = a.x0[(size_t)r * P + pp[k]];
          const double v = v0 != v0 ? v0 : fmax(fmin(v0, ub[k]), lb[k]);
          vx[pp[k]] = v;
          vxt[pp[k]] = v;
          if (!(fabs(v) < INFINITY)) bad = 1.0;
        }
      bad = fm::wave_max_dpp(bad);
      if (bad > 0.0) {
        if (lane == 0) a.invalid[r] = 1;
        h.done = 1;
      } else {
        h.st = ST_INIT;
      }
    } else {
      // ---- the evaluation of the round before, at x_t: phi_t = -(lml + log prior), g_t = -(dlml + d log prior)
      ++h.evals;
      double xt[2] = {0.0, 0.0}, gt[2] = {0.0, 0.0};
      double bad = 0.0;
      for (int k = 0; k < 2; ++k)
        if (on[k]) {
          xt[k] = vxt[pp[k]];
          double dt;
          s_t[pp[k]] = gp_prior_term(a.pmu, a.psig, a.pdf, a.pconst, pp[k], xt[k], &dt);
          gt[k] = -(a.dlml[(size_t)r * P + pp[k]] + dt);
          if (!(fabs(gt[k]) < INFINITY)) {
            bad = 1.0;
            gt[k] = 0.0;
          }
        }
      __syncthreads();
      double lp = 0.0;
      for (int p = 0; p < P; ++p) lp += s_t[p];  // (p ascending, as the chains add it)
      const double lml = a.lml[r];
      if (a.flag[r] != 0 || !(fabs(lml) < INFINITY)) bad = 1.0;
      bad = fm::wave_max_dpp(bad);
      double phit = -(lml + lp);
      if (bad > 0.0 || !(fabs(phit) < INFINITY)) phit = INFINITY;
      double* ev = a.trace_cap > 0 && h.evals <= 1 + 31LL * a.trace_cap
                       ? a.trace_ev + ((size_t)r * (1 + 31 * (size_t)a.trace_cap) + (size_t)(h.evals - 1)) * 4
                       : nullptr;

      if (h.st == ST_INIT) {  // phi(x0)
        if (phit == INFINITY) {
          if (lane == 0) a.invalid[r] = 1;
          h.done = 1;
        } else {
          for (int k = 0; k < 2; ++k) {
            x[k] = xt[k];
            g[k] = gt[k];
            if (on[k]) vg[pp[k]] = g[k];
          }
          h.phi = phit;
          if (ev && lane == 0) { ev[0] = 0.0; ev[1] = 0.0; ev[2] = phit; ev[3] = 1.0; }
          begin = true;
        }
      } else {  // ST_SEARCH: the trial x_t = clip(x + t d)
        double sv[2];
        for (int k = 0; k < 2; ++k) {
          x[k] = on[k] ? vx[pp[k]] : 0.0;
          g[k] = on[k] ? vg[pp[k]] : 0.0;
          d[k] = on[k] ? vd[pp[k]] : 0.0;
          sv[k] = xt[k] - x[k];
        }
        const double gs = dot2(g, sv);
        const bool accept = phit < INFINITY && phit <= h.phi + OP_ARMIJO * gs;
        if (ev && lane == 0) { ev[0] = (double)h.iter; ev[1] = h.t; ev[2] = phit; ev[3] = accept ? 1.0 : 0.0; }
        if (accept) {
          double yv[2];
          for (int k = 0; k < 2; ++k) yv[k] = gt[k] - g[k];
          const double sy = dot2(sv, yv), ss = dot2(sv, sv), yy = dot2(yv, yv);
          if (sy > OP_CURV * (sqrt(ss) * sqrt(yy))) {  // the pair, over the oldest one when m are held
            int idx;
            if (h.npairs < m) {
              idx = (h.head + h.npairs) % m;
              ++h.npairs;
            } else {
              idx = h.head;
              h.head = (h.head + 1) % m;
            }
            for (int k = 0; k < 2; ++k)
              if (on[k]) {
                vS[(size_t)idx * P + pp[k]] = sv[k];
                vY[(size_t)idx * P + pp[k]] = yv[k];
              }
            vrho[idx] = 1.0 / sy;  // (every lane writes the same value and reads its own write below)
            h.gamma = sy / yy;
          }
          const double phi_old = h.phi;
          for (int k = 0; k < 2; ++k) {
            x[k] = xt[k];
            g[k] = gt[k];
            if (on[k]) {
              vx[pp[k]] = x[k];
              vg[pp[k]] = g[k];
            }
          }
          h.phi = phit;
          ++h.iter;
          if (phi_old - h.phi <= a.tol_f * fmax(1.0, fabs(h.phi))) {
            h.reason = STOP_TOL_F;
            stop = true;
            double* it = a.trace_cap > 0 && h.iter < a.trace_cap
                             ? a.trace_it + ((size_t)r * a.trace_cap + h.iter) * (3 * (size_t)P + 3)
                             : nullptr;
            if (it) {  // the row of the point the run ends at: no direction
              for (int k = 0; k < 2; ++k)
                if (on[k]) {
                  it[pp[k]] = x[k];
                  it[P + 1 + pp[k]] = g[k];
                  it[2 * P + 1 + pp[k]] = 0.0;
                }
              if (lane == 0) { it[P] = h.phi; it[3 * P + 1] = (double)h.npairs; it[3 * P + 2] = 0.0; }
            }
          } else {
            begin = true;
          }
        } else if (h.halv == OP_HALVINGS) {
          h.reason = STOP_SEARCH;
          stop = true;
        } else {
          ++h.halv;
          h.t *= 0.5;
          for (int k = 0; k < 2; ++k)
            if (on[k]) vxt[pp[k]] = fmax(fmin(x[k] + h.t * d[k], ub[k]), lb[k]);
        }
      }
    }

    if (begin) {
      // ---- an iteration begins at (x, g, phi): the stop tests, the direction, the first trial point
      bool inB[2];
      double pg[2];
      for (int k = 0; k < 2; ++k) {
        inB[k] = (x[k] <= lb[k] && g[k] > 0.0) || (x[k] >= ub[k] && g[k] < 0.0) || lb[k] == ub[k];
        pg[k] = on[k] && !inB[k] ? g[k] : 0.0;
      }
      const double gmax = fm::wave_max_dpp(fmax(fabs(pg[0]), fabs(pg[1])));
      int reset = 0;
      d[0] = d[1] = 0.0;
      if (gmax <= a.tol_g) {
        h.reason = STOP_TOL_G;
        stop = true;
      } else if (h.iter >= a.max_iter) {
        h.reason = STOP_MAX_ITER;
        stop = true;
      } else {
        bool steepest = h.npairs == 0;
        if (!steepest) {
          double q[2] = {pg[0], pg[1]};
          for (int j = h.npairs - 1; j >= 0; --j) {  // newest to oldest
            const int i = (h.head + j) % m;
            double sj[2], yj[2];
            for (int k = 0; k < 2; ++k) {
              sj[k] = on[k] ? vS[(size_t)i * P + pp[k]] : 0.0;
              yj[k] = on[k] ? vY[(size_t)i * P + pp[k]] : 0.0;
            }
            const double al = vrho[i] * dot2(sj, q);
            s_al[j] = al;
            for (int k = 0; k < 2; ++k) q[k] -= al * yj[k];
          }
          for (int k = 0; k < 2; ++k) q[k] *= h.gamma;
          for (int j = 0; j < h.npairs; ++j) {  // oldest to newest
            const int i = (h.head + j) % m;
            double sj[2], yj[2];
            for (int k = 0; k < 2; ++k) {
              sj[k] = on[k] ? vS[(size_t)i * P + pp[k]] : 0.0;
              yj[k] = on[k] ? vY[(size_t)i * P + pp[k]] : 0.0;
            }
            const double be = vrho[i] * dot2(yj, q);
            const double c = s_al[j] - be;
            for (int k = 0; k < 2; ++k) q[k] += sj[k] * c;
          }
          for (int k = 0; k < 2; ++k) d[k] = on[k] && !inB[k] ? -q[k] : 0.0;
          const double gtd = dot2(g, d);
          if (!(gtd < 0.0)) {  // not a descent direction: the history is dropped
            steepest = true;
            h.npairs = 0;
            h.head = 0;
            ++h.resets;
          }
        }
        if (steepest) {
          for (int k = 0; k < 2; ++k) d[k] = -pg[k];
          const double s1 = fm::wave_sum_dpp(fabs(pg[0]) + fabs(pg[1]));
          h.t = fmin(1.0, 1.0 / s1);
          reset = 1;
        } else {
          h.t = 1.0;
        }
        h.halv = 0;
        h.st = ST_SEARCH;
        for (int k = 0; k < 2; ++k)
          if (on[k]) {
            vd[pp[k]] = d[k];
            vxt[pp[k]] = fmax(fmin(x[k] + h.t * d[k], ub[k]), lb[k]);
          }
      }
      double* it = a.trace_cap > 0 && h.iter < a.trace_cap
                       ? a.trace_it + ((size_t)r * a.trace_cap + h.iter) * (3 * (size_t)P + 3)
                       : nullptr;
      if (it) {
        for (int k = 0; k < 2; ++k)
          if (on[k]) {
            it[pp[k]] = x[k];
            it[P + 1 + pp[k]] = g[k];
            it[2 * P + 1 + pp[k]] = d[k];
          }
        if (lane == 0) { it[P] = h.phi; it[3 * P + 1] = (double)h.npairs; it[3 * P + 2] = (double)reset; }
      }
    }

    if (stop) {  // the results; the final point is what the run submits from now on
      for (int k = 0; k < 2; ++k)
        if (on[k]) {
          a.hyp_out[(size_t)r * P + pp[k]] = x[k];
          a.grad[(size_t)r * P + pp[k]] = -g[k];
          vxt[pp[k]] = x[k];
        }
      if (lane == 0) {
        a.logpost[r] = -h.phi;
        long long* so = a.stats + 4 * (size_t)r;
        so[0] = h.iter;
        so[1] = h.evals;
        so[2] = h.resets;
        so[3] = h.reason;
      }
      h.done = 1;
    }
    if (lane == 0) *rs = h;
  }
  if (lane == 0) a.flag[r] = 0;
  __syncthreads();  // x_t (global memory, an entry written by the lane that holds it)

  // ---- the candidate (gp_cand.h), and d sn2 / d log sn = 2 exp(2 h[D + 1]) of constant additive noise for the gradient
  for (int k = 0; k < 2; ++k)
    if (on[k]) gp_cand_coord(vxt, a.lb, pp[k], slot, P, a.g_hyp);
  const double e = gp_cand_noise<64>(lane, slot, N, D, vxt, a.lb, a.s2, a.s2_min, a.g_sn2, a.g_sl, a.g_smeta);
  if (lane == 0) a.dsn2[slot] = 2.0 * e;
}

}  // namespace

size_t gp_opt_state_elems(int P, int m) { return sizeof(OptRun) / sizeof(double) + (4 + 2 * (size_t)m) * P + m; }
LockstepWord gp_opt_done_word(int P, int m) { return {gp_opt_state_elems(P, m), offsetof(OptRun, done), 1}; }  // (done: 0 or 1)

int launch_gp_opt_advance(vbmc_ctx* ctx, const GpOptArgs& a, int b0, int S) {
  if (a.P > OP_PMAX || a.m < 1 || a.m > OP_MMAX)
    return vbmc_fail(ctx, VBMC_E_ARG, "gp_opt: P=%d > %d or m=%d outside [1, %d]", a.P, OP_PMAX, a.m, OP_MMAX);
  hipLaunchKernelGGL(gp_opt_advance_kernel, dim3(S), dim3(64), 0, ctx->stream, a, b0, S,
                     (int)gp_opt_state_elems(a.P, a.m));
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}
