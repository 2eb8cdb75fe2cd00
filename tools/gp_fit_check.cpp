// Stand-alone host check of vbmc_gp_fit's argument check and stage sizes (pyvbmc_amd/csrc/gp_fit_host.h), through the
// check it shares with the lockstep entries (gp_cand_host.h).  Meant to be built with a host sanitizer and run on a CPU:
//
//     hipcc -std=c++17 -Xarch_host -fsanitize=address,undefined tools/gp_fit_check.cpp -o gp_fit_check && ./gp_fit_check
//
// The arrays have exactly the sizes the entry is promised (P, N, H x P), so a read past one is what the sanitizer
// reports.  Exit status 0 = every expectation held.
#include <cstdio>
#include <limits>
#include <vector>

#include "../pyvbmc_amd/csrc/gp_fit_host.h"

static int g_bad = 0;

static void expect(const char* what, bool ok) {
  std::printf("%s %s\n", ok ? "ok  " : "FAIL", what);
  if (!ok) ++g_bad;
}

struct Problem {
  int N = 63, D = 3, P = 6, mean = VBMC_MEAN_CONST, H = 3, init_N = 37, opts_N = 3, n_samples = 4, max_iter = 8, m = 8, thin = 2,
      burn = 3;
  double tol_g = 1e-5, tol_f = 1e-9;
  bool with_s2 = true, with_box = true, with_widths = true, with_hyp0 = true;
  std::vector<double> lb, ub, dlb, dub, mu, sg, df, s2, widths, hyp0;
  Problem()
      : lb(P, -1.0), ub(P, 1.0), dlb(P, -0.5), dub(P, 0.5), mu(P, 0.1), sg(P, 0.5), df(P, 3.0), s2(N, 0.01), widths(P, 0.6),
        hyp0((size_t)H * P, 0.0) {}
  int check(WarpArgErr& e, GpCandPlan& pl, GpFitShape* shape = nullptr) const {
    const GpFitShape sh = gp_fit_shape(H, init_N, opts_N, n_samples);
    if (shape) *shape = sh;
    auto own = [&](WarpArgErr& er) {
      return gp_fit_check_own(er, "check", P, H, with_hyp0 ? hyp0.data() : nullptr, init_N, with_box ? dlb.data() : nullptr,
                              with_box ? dub.data() : nullptr, lb.data(), ub.data(), opts_N, max_iter, m, tol_g, tol_f, n_samples,
                              with_widths ? widths.data() : nullptr, thin, burn);
    };
    return gp_cand_check(e, "check", 'B', N, D, sh.runs, P, mean, lb.data(), ub.data(), mu.data(), sg.data(), df.data(),
                         with_s2 ? s2.data() : nullptr, 0, own, pl);
  }
};

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  GpCandPlan pl;
  {
    Problem q;
    WarpArgErr e;
    GpFitShape sh;
    expect("good arguments", q.check(e, pl, &sh) == 0 && sh.B == 40 && sh.R == 3 && sh.C == 4 && sh.S == 4 && sh.runs == 40 &&
                                 pl.chunk == 40);
    q.opts_N = 100;
    q.n_samples = 0;
    q.init_N = 0;
    q.with_box = q.with_widths = false;
    WarpArgErr e2;
    expect("stages switched off", q.check(e2, pl, &sh) == 0 && sh.B == 3 && sh.R == 3 && sh.C == 0 && sh.S == 1 && sh.runs == 3);
    q.n_samples = 9;
    q.with_widths = true;
    WarpArgErr e3;
    expect("more samples than candidates", q.check(e3, pl, &sh) == 0 && sh.runs == 9 && pl.chunk == 9);
  }
#define CODE(what, want, edit)                                    \
  do {                                                            \
    Problem q;                                                    \
    WarpArgErr e;                                                 \
    edit;                                                         \
    const int got = q.check(e, pl);                               \
    expect(what, got == (want) && e.code == (want) && e.msg[0]);  \
  } while (0)
  CODE("no candidate", VBMC_E_ARG, (q.H = 0, q.init_N = 0));
  CODE("negative H", VBMC_E_ARG, q.H = -1);
  CODE("negative init_N", VBMC_E_ARG, q.init_N = -2);
  CODE("H without hyp0", VBMC_E_ARG, q.with_hyp0 = false);
  CODE("negative opts_N", VBMC_E_ARG, q.opts_N = -1);
  CODE("negative n_samples", VBMC_E_ARG, q.n_samples = -1);
  CODE("design without a box", VBMC_E_ARG, q.with_box = false);
  CODE("dlb below lb", VBMC_E_ARG, q.dlb[5] = -1.5);
  CODE("dub above ub", VBMC_E_ARG, q.dub[0] = 1.5);
  CODE("dlb > dub", VBMC_E_ARG, (q.dlb[2] = 0.3, q.dub[2] = 0.2));
  CODE("dlb NaN", VBMC_E_ARG, q.dlb[1] = nan);
  CODE("m = 0", VBMC_E_ARG, q.m = 0);
  CODE("tol_f NaN", VBMC_E_ARG, q.tol_f = nan);
  CODE("thin = 0", VBMC_E_ARG, q.thin = 0);
  CODE("burn < 0", VBMC_E_ARG, q.burn = -1);
  CODE("samples without widths", VBMC_E_ARG, q.with_widths = false);
  CODE("width 0 at the end", VBMC_E_ARG, q.widths[5] = 0.0);
  CODE("infinite upper bound", VBMC_E_ARG, q.ub[5] = inf);
  CODE("the shared check's prior", VBMC_E_ARG, q.sg[5] = 0.0);
  CODE("noise bound below 1e-6", VBMC_E_UNSUP, (q.lb[4] = -20.0, q.dlb[4] = -20.0, q.with_s2 = false));
  CODE("E_ARG wins over E_UNSUP", VBMC_E_ARG, (q.lb[4] = -20.0, q.with_s2 = false, q.dub[0] = 1.5));
#undef CODE
  {  // the optimiser's and the sampler's arguments are not looked at where their stage does not run
    Problem q;
    q.opts_N = 0;
    q.m = 0;
    q.n_samples = 0;
    q.thin = 0;
    q.with_widths = false;
    WarpArgErr e;
    expect("arguments of stages that do not run", q.check(e, pl) == 0);
  }
  std::printf(g_bad ? "%d expectation(s) failed\n" : "all expectations held\n", g_bad);
  return g_bad ? 1 : 0;
}
