// Stand-alone host check of the raw-memory part of the native repeat lane (pyvbmc_amd/csrc/step_lane.h): the copy of
// theta into the argument block, the seed write, the call through the entry's address and the copy of the gradient
// out.  Meant to be built with a host sanitizer and run on a CPU:
//
//     c++ -std=c++17 -fsanitize=address,undefined -Iinclude tools/step_lane_check.cpp -o step_lane_check && ./step_lane_check
//
// Every buffer has exactly the size the block promises (n_theta doubles), so a read or a write past one is what the
// sanitizer reports.  The CPython glue around it (pyvbmc_amd/csrc/pyext_step.cpp) is not covered here.
// Exit status 0 = every expectation held.
#include <cstdio>
#include <vector>

#include "../pyvbmc_amd/csrc/step_lane.h"
#include "vbmc_hip.h"

static int g_bad = 0;

static void expect(const char* what, bool ok) {
  std::printf("%s %s\n", ok ? "ok  " : "FAIL", what);
  if (!ok) ++g_bad;
}

static int g_token;

// what the lane calls: reads all of theta, writes all of dF and the three scalars
static int entry(void* handle, const void* block) {
  const vbmc_elbo_call* c = static_cast<const vbmc_elbo_call*>(block);
  if (handle != &g_token) return VBMC_E_ARG;
  double sum = 0.0;
  for (int i = 0; i < c->n_theta; ++i) {
    sum += c->theta[i];
    c->dF[i] = 2.0 * c->theta[i] + static_cast<double>(c->opts->seed % 5);
  }
  *c->F = sum;
  *c->G = -sum;
  *c->H = static_cast<double>(c->opts->seed);
  return 0;
}

static void run(int n) {
  std::vector<double> th(n), dF(n), src(n), out(n);
  double F = 0, G = 0, H = 0;
  vbmc_elbo_opts opts{};
  vbmc_elbo_call block{};
  block.theta = th.data();
  block.n_theta = n;
  block.opts = &opts;
  block.F = &F;
  block.dF = dF.data();
  block.G = &G;
  block.H = &H;
  StepLane l;
  l.fn = entry;
  l.handle = &g_token;
  l.block = &block;
  l.th = th.data();
  l.dF = dF.data();
  l.F = &F;
  l.G = &G;
  l.H = &H;
  l.seed = &opts.seed;
  l.n_theta = n;
  double want = 0.0;
  for (int i = 0; i < n; ++i) want += (src[i] = 0.25 * i - 1.0);
  step_lane_pack(l, src.data());
  *l.seed = 0xFFFFFFFFFFFFFFFFull;  // the whole 64-bit field
  const int rc = step_lane_invoke(l);
  step_lane_grad(l, out.data());
  bool grads = true;
  for (int i = 0; i < n; ++i) grads = grads && out[i] == 2.0 * src[i] + static_cast<double>(0xFFFFFFFFFFFFFFFFull % 5);
  char what[64];
  std::snprintf(what, sizeof what, "n_theta = %d", n);
  expect(what, rc == 0 && *l.F == want && *l.G == -want && *l.H == static_cast<double>(0xFFFFFFFFFFFFFFFFull) && grads);
  step_lane_pack(l, l.th);  // theta that IS the block's buffer
  expect("pack from the block's own buffer", step_lane_invoke(l) == 0 && *l.F == want);
}

int main() {
  run(1);
  run(10);
  run(610);  // D = 10, K = 50
  return g_bad ? 1 : 0;
}
