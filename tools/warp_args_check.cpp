// Stand-alone host check of the input-warping entry points' argument validation (pyvbmc_amd/csrc/warp_args.h) and of
// their scratch lists (pyvbmc_amd/csrc/scratch.h WarpWs), meant to be built with a host sanitizer and run on a CPU:
//
//     hipcc -std=c++17 -Xarch_host -fsanitize=address,undefined tools/warp_args_check.cpp -o warp_args_check && ./warp_args_check
//
// It calls every check with good and bad arguments (null arrays, D = 0 and 33, negative and oversized counts, a sigma
// row count that matches neither form, unknown source / mode codes, outputs that the source does not provide) and
// compares the codes; the pointers are never dereferenced by the checks, which is what the sanitizer watches.  Exit
// status 0 = every expectation held.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../pyvbmc_amd/csrc/scratch.h"
#include "../pyvbmc_amd/csrc/warp_args.h"

static int g_bad = 0;

static void expect(const char* what, int got, int want, const WarpArgErr& e) {
  const bool msg_ok = (want == 0) == (e.msg[0] == 0) && std::strlen(e.msg) < sizeof(e.msg);
  if (got != want || e.code != want || !msg_ok) {
    std::printf("FAIL %s: got %d (code %d, \"%s\"), want %d\n", what, got, e.code, e.msg, want);
    ++g_bad;
  } else {
    std::printf("ok   %-44s %d %s\n", what, got, e.msg);
  }
}

int main() {
  std::vector<double> buf(4 * 32, 0.0);
  const double* p = buf.data();
  double* q = buf.data();
  const double* nul = nullptr;

#define CHECK(what, want, call)  \
  do {                           \
    WarpArgErr e;                \
    expect(what, call, want, e); \
  } while (0)

  // vbmc_warp_points
  CHECK("points ok", 0, warp_check_points(e, 3, 4, VBMC_WARP_FROM_OLD, p, q, q, q));
  CHECK("points n = 0, no arrays", 0, warp_check_points(e, 3, 0, VBMC_WARP_FROM_OLD, nul, nul, nul, nul));
  CHECK("points D = 0", VBMC_E_ARG, warp_check_points(e, 0, 4, 0, p, q, nul, nul));
  CHECK("points D = -5", VBMC_E_ARG, warp_check_points(e, -5, 4, 0, p, q, nul, nul));
  CHECK("points D = 33", VBMC_E_UNSUP, warp_check_points(e, 33, 4, 0, p, q, nul, nul));
  CHECK("points D = 33 wins over null", VBMC_E_UNSUP, warp_check_points(e, 33, 4, 0, nul, nul, nul, nul));
  CHECK("points source 3", VBMC_E_ARG, warp_check_points(e, 3, 4, 3, p, q, nul, nul));
  CHECK("points source -1", VBMC_E_ARG, warp_check_points(e, 3, 4, -1, p, q, nul, nul));
  CHECK("points n < 0", VBMC_E_ARG, warp_check_points(e, 3, -1, 0, p, q, nul, nul));
  CHECK("points null x", VBMC_E_ARG, warp_check_points(e, 3, 4, 0, nul, q, nul, nul));
  CHECK("points no output", VBMC_E_ARG, warp_check_points(e, 3, 4, 0, p, nul, nul, nul));
  CHECK("points lj_old from orig", VBMC_E_ARG, warp_check_points(e, 3, 4, VBMC_WARP_FROM_ORIG, p, q, nul, q));
  CHECK("points lj_old in new", VBMC_E_ARG, warp_check_points(e, 3, 4, VBMC_WARP_IN_NEW, p, nul, q, q));
  CHECK("points lj_new only", 0, warp_check_points(e, 32, 4, VBMC_WARP_IN_NEW, p, nul, q, nul));

  // vbmc_warp_unscent
  CHECK("unscent ok, n rows", 0, warp_check_unscent(e, 3, 4, p, 4, p, q, q));
  CHECK("unscent ok, one row", 0, warp_check_unscent(e, 3, 4, p, 1, p, q, q));
  CHECK("unscent rows 2 of 4", VBMC_E_ARG, warp_check_unscent(e, 3, 4, p, 2, p, q, q));
  CHECK("unscent rows 0", VBMC_E_ARG, warp_check_unscent(e, 3, 4, p, 0, p, q, q));
  CHECK("unscent n = 0", VBMC_E_ARG, warp_check_unscent(e, 3, 0, p, 1, p, q, q));
  CHECK("unscent n = 2^31", VBMC_E_ARG, warp_check_unscent(e, 3, (int64_t)1 << 31, p, 1, p, q, q));
  CHECK("unscent D = 33", VBMC_E_UNSUP, warp_check_unscent(e, 33, 4, p, 1, p, q, q));
  CHECK("unscent null sigma", VBMC_E_ARG, warp_check_unscent(e, 3, 4, p, 1, nul, q, q));
  CHECK("unscent null mean", VBMC_E_ARG, warp_check_unscent(e, 3, 4, p, 1, p, nul, q));

  // vbmc_warp_gp
  CHECK("gp ok", 0, warp_check_gp(e, 3, 37, 2, 12, p, p, q));
  CHECK("gp P < D", VBMC_E_ARG, warp_check_gp(e, 3, 37, 2, 2, p, p, q));
  CHECK("gp N = 0", VBMC_E_ARG, warp_check_gp(e, 3, 0, 2, 12, p, p, q));
  CHECK("gp S = 0", VBMC_E_ARG, warp_check_gp(e, 3, 37, 0, 12, p, p, q));
  CHECK("gp S = 65536", VBMC_E_ARG, warp_check_gp(e, 3, 37, 65536, 12, p, p, q));
  CHECK("gp D = 33", VBMC_E_UNSUP, warp_check_gp(e, 33, 37, 2, 99, p, p, q));
  CHECK("gp null hyp", VBMC_E_ARG, warp_check_gp(e, 3, 37, 2, 12, p, nul, q));
  CHECK("gp state too large", VBMC_E_UNSUP, warp_check_gp(e, 32, 2000000, 8, 99, p, p, q));
  CHECK("gp int overflow sizes", VBMC_E_UNSUP, warp_check_gp(e, 32, 2147483647, 65535, 99, p, p, q));

  // vbmc_warp_box
  CHECK("box ok quantiles", 0, warp_check_box(e, 3, 1000, VBMC_WARP_FROM_ORIG, p, p, 0, q, q));
  CHECK("box ok min / max", 0, warp_check_box(e, 3, 1000, VBMC_WARP_FROM_OLD, p, p, 1, q, nul));
  CHECK("box n = 0", VBMC_E_ARG, warp_check_box(e, 3, 0, 1, p, p, 0, q, nul));
  CHECK("box n > 2^30", VBMC_E_UNSUP, warp_check_box(e, 3, ((int64_t)1 << 30) + 1, 1, p, p, 0, q, nul));
  CHECK("box mode 2", VBMC_E_ARG, warp_check_box(e, 3, 10, 1, p, p, 2, q, nul));
  CHECK("box source 7", VBMC_E_ARG, warp_check_box(e, 3, 10, 7, p, p, 0, q, nul));
  CHECK("box null lo", VBMC_E_ARG, warp_check_box(e, 3, 10, 1, nul, p, 0, q, nul));
  CHECK("box null out", VBMC_E_ARG, warp_check_box(e, 3, 10, 1, p, p, 0, nul, nul));
  CHECK("box sorted in min / max mode", VBMC_E_ARG, warp_check_box(e, 3, 10, 1, p, p, 1, q, q));
  CHECK("box D = 33", VBMC_E_UNSUP, warp_check_box(e, 33, 10, 1, p, p, 0, q, nul));

  // the scratch lists: pieces in order, none overlapping, absent pieces take no room
  {
    const WarpWs w = warp_points_ws(5, 3, true, false, true);
    if (w.x.off != 0 || w.y.off != 15 || w.lj_new.count != 0 || w.lj_old.off != 30 || w.sc.total != 35) {
      std::printf("FAIL points scratch\n");
      ++g_bad;
    }
    const WarpWs u = warp_unscent_ws(4, 3, 1, true);
    if (u.sigma.off != 12 || u.mean.off != 15 || u.sd.off != 27 || u.pts.off != 39 || u.sc.total != 39 + 7 * 4 * 3) {
      std::printf("FAIL unscent scratch\n");
      ++g_bad;
    }
    const WarpWs g = warp_gp_ws(37, 3, 2);
    if (g.out.off + g.out.count != g.sc.total || g.out.count != 2 * 3 + 2 || g.sd.off != g.mean.off + 2 * 37 * 3) {
      std::printf("FAIL gp scratch\n");
      ++g_bad;
    }
    const WarpWs b = warp_box_ws(1000, 3, false, true, 8192, false);
    // (D unsigned flags round up to whole doubles)
    if (b.x.count != 0 || b.box.off != 0 || b.y.off != 6 || b.keys.off != 3006 || b.nonfinite.off != 3006 + 3 * 8192 ||
        b.out.off != b.nonfinite.off + 2 || b.sc.total != b.out.off + 6) {
      std::printf("FAIL box scratch\n");
      ++g_bad;
    }
  }
  std::printf(g_bad ? "%d expectation(s) failed\n" : "all expectations held\n", g_bad);
  return g_bad ? 1 : 0;
}
