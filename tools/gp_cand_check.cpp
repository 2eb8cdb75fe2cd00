// Stand-alone host check of what the GP candidate entries index by hand (pyvbmc_amd/csrc/gp_cand_host.h): the shared
// argument check, the workspace list of a chunk and the packing of the lockstep entries' `in` block.  Meant to be built
// with a host sanitizer and run on a CPU:
//
//     hipcc -std=c++17 -Xarch_host -fsanitize=address,undefined tools/gp_cand_check.cpp -o gp_cand_check && ./gp_cand_check
//
// The arrays have exactly the sizes the entries are promised (P, N, runs x P), so a read or a write past one is what
// the sanitizer reports.  Exit status 0 = every expectation held.
#include <cstdio>
#include <limits>
#include <vector>

#include "../pyvbmc_amd/csrc/gp_cand_host.h"

static int g_bad = 0;

static void expect(const char* what, bool ok) {
  std::printf("%s %s\n", ok ? "ok  " : "FAIL", what);
  if (!ok) ++g_bad;
}

struct Problem {
  int N = 65, D = 3, runs = 3, P = 6, mean = VBMC_MEAN_CONST;
  std::vector<double> lb, ub, mu, sg, df, s2;
  Problem() : lb(P, -1.0), ub(P, 1.0), mu(P, 0.1), sg(P, 0.5), df(P, 3.0), s2(N, 0.01) {
    sg[1] = std::numeric_limits<double>::quiet_NaN();  // no prior on parameter 1
    df[2] = std::numeric_limits<double>::infinity();
  }
  int check(bool with_s2, int own_code, GpCandPlan& pl, WarpArgErr& e, int forced = 0) const {
    auto own = [&](WarpArgErr& er) { return own_code ? warp_arg_fail(er, own_code, "own") : 0; };
    return gp_cand_check(e, "check", 'R', N, D, runs, P, mean, lb.data(), ub.data(), mu.data(), sg.data(), df.data(),
                         with_s2 ? s2.data() : nullptr, forced, own, pl);
  }
};

static void check_codes() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  GpCandPlan pl;
  {
    Problem q;
    WarpArgErr e;
    expect("good arguments", q.check(true, 0, pl, e) == 0 && pl.mean_n == 1 && pl.chunk == 3 && pl.s2_min == 0.01 && !e.msg[0]);
    WarpArgErr e2;
    expect("forced chunk", q.check(false, 0, pl, e2, 2) == 0 && pl.chunk == 2 && pl.s2_min == 0.0);
  }
#define CODE(what, want, edit)                                    \
  do {                                                            \
    Problem q;                                                    \
    WarpArgErr e;                                                 \
    bool with_s2 = true;                                          \
    int own_code = 0;                                             \
    edit;                                                         \
    const int got = q.check(with_s2, own_code, pl, e);            \
    expect(what, got == (want) && e.code == (want) && e.msg[0]);  \
    (void)with_s2;                                                \
  } while (0)
  CODE("N = 0", VBMC_E_ARG, q.N = 0);
  CODE("runs = 0", VBMC_E_ARG, q.runs = 0);
  CODE("P of another mean", VBMC_E_ARG, q.mean = VBMC_MEAN_ZERO);
  CODE("mean kind 3", VBMC_E_ARG, q.mean = 3);
  CODE("the entry's own check", VBMC_E_ARG, own_code = VBMC_E_ARG);
  CODE("infinite upper bound", VBMC_E_ARG, q.ub[5] = inf);
  CODE("lb > ub", VBMC_E_ARG, q.lb[0] = 2.0);
  CODE("prior sigma 0", VBMC_E_ARG, q.sg[5] = 0.0);
  CODE("prior df 0", VBMC_E_ARG, q.df[0] = 0.0);
  CODE("prior mu NaN", VBMC_E_ARG, q.mu[5] = nan);
  CODE("negative s2 at the end", VBMC_E_ARG, q.s2[64] = -1.0);
  CODE("noise bound below 1e-6", VBMC_E_UNSUP, (q.lb[4] = -20.0, with_s2 = false));
  CODE("E_ARG wins over E_UNSUP", VBMC_E_ARG, (q.lb[4] = -20.0, with_s2 = false, q.df[5] = -1.0));
  CODE("N too large for one candidate", VBMC_E_UNSUP, (q.N = 20000, q.s2.assign(20000, 0.01)));
#undef CODE
  {  // D = 33 with P to match: refused after every argument check
    Problem q;
    q.D = 33;
    q.P = 36;
    for (auto* v : {&q.lb, &q.ub, &q.mu, &q.sg, &q.df}) v->resize(36, 0.5);
    WarpArgErr e;
    expect("D = 33", q.check(true, 0, pl, e) == VBMC_E_UNSUP);
  }
  {  // vbmc_gp_lml's form: no box, no prior, no s2
    WarpArgErr e;
    auto own = [](WarpArgErr&) { return 0; };
    const int rc = gp_cand_check(e, "check", 'B', 65, 3, 5, 12, VBMC_MEAN_NEGQUAD, nullptr, nullptr, nullptr, nullptr, nullptr,
                                 nullptr, 0, own, pl);
    expect("no box", rc == 0 && pl.mean_n == 7 && pl.chunk == 5);
  }
}

static void check_listing() {
  // N = 65: two 64-blocks, three tile pairs; 5 slots, chunks of 2, D = 3, constant mean (P = 6)
  Scratch sc;
  const GpLmlWs w = gp_lml_ws(sc, 65, 3, 6, 1, 2, 5, 1);
  bool ok = w.flag.off == 0 && w.flag.count == 5 && w.sums.off == 4 && w.dsn2.off == 8 && w.lml.off == 10 && w.dlml.off == 15 &&
            w.clear_end == 45 && w.Dinv.off == 45 && w.Dinv.count == 2 * 2 * 4096 && w.part.off == w.Dinv.off + w.Dinv.count &&
            w.part.count == 2 * 3 * 5 && w.mg.off == w.part.off + 30 && w.mg.count == 2 && sc.total == w.mg.off + 2;
  expect("listing with the gradient", ok);
  Scratch s0;
  const GpLmlWs v = gp_lml_ws(s0, 65, 3, 6, 1, 2, 5, 0);
  ok = v.dlml.count == 0 && v.part.count == 0 && v.mg.count == 0 && v.clear_end == 15 && v.Dinv.off == 15 &&
       s0.total == 15 + 2 * 2 * 4096 && v.want_grad == 0 && v.P == 6;
  expect("listing without the gradient", ok);
}

static void check_packing() {
  const Problem q;
  std::vector<double> x0((size_t)q.runs * q.P), widths(q.P, 0.6);
  for (size_t i = 0; i < x0.size(); ++i) x0[i] = 0.01 * (double)i;
  for (int has_s2 = 0; has_s2 < 2; ++has_s2)
    for (int lead = 0; lead < 2; ++lead) {
      GpCandArgs a;
      a.N = q.N;
      a.P = q.P;
      std::vector<double> dev(gp_cand_in_elems(q.runs, q.P, lead, q.N, has_s2 != 0));  // stands for the device copy
      const double* s2 = has_s2 ? q.s2.data() : nullptr;
      const std::vector<double> in =
          lead ? gp_cand_pack(a, dev.data(), q.runs, x0.data(), {widths.data()}, q.lb.data(), q.ub.data(), q.mu.data(),
                              q.sg.data(), q.df.data(), s2)
               : gp_cand_pack(a, dev.data(), q.runs, x0.data(), {}, q.lb.data(), q.ub.data(), q.mu.data(), q.sg.data(),
                              q.df.data(), s2);
      bool ok = in.size() == dev.size();
      if (ok) dev = in;
      // every field points at its array's copy, and the last of them ends where the block ends
      const size_t P = q.P;
      ok = ok && a.x0 == dev.data() && a.x0[x0.size() - 1] == x0.back() && a.lb == a.x0 + x0.size() + lead * P &&
           (!lead || a.x0[x0.size() + P - 1] == 0.6) && a.lb[0] == -1.0 && a.ub[P - 1] == 1.0 && a.pmu[0] == 0.1 &&
           a.psig[0] == 0.5 && a.psig[1] != a.psig[1] && a.pdf[2] == std::numeric_limits<double>::infinity() &&
           a.pconst[1] == 0.0 && a.pconst[2] == gp_prior_const(0.5, a.pdf[2]) && a.pconst[0] == gp_prior_const(0.5, 3.0);
      ok = ok && (has_s2 ? a.s2 == a.pconst + P && a.s2 + q.N == dev.data() + dev.size() && a.s2[q.N - 1] == 0.01
                         : a.s2 == nullptr && a.pconst + P == dev.data() + dev.size());
      char what[64];
      std::snprintf(what, sizeof(what), "packing, %d leading arrays, s2 %s", lead, has_s2 ? "given" : "absent");
      expect(what, ok);
    }
}

int main() {
  check_codes();
  check_listing();
  check_packing();
  std::printf(g_bad ? "%d expectation(s) failed\n" : "all expectations held\n", g_bad);
  return g_bad ? 1 : 0;
}
