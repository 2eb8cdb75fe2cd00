// The part of the native repeat lane (pyext_step.cpp) that touches raw memory: the addresses of one argument block of
// vbmc_neg_elcbo_call, the copy of theta into it, the seed write, the call and the copy of the gradient out of it.
// Host C++ only and free of Python, so a stand-alone program can drive it under a host sanitizer
// (tools/step_lane_check.cpp).
#pragma once
#include <cstdint>
#include <cstring>

struct StepLane {
  int (*fn)(void*, const void*) = nullptr;  // vbmc_neg_elcbo_call (nullptr: the lane is not bound)
  void* handle = nullptr;                   // vbmc_ctx*
  const void* block = nullptr;              // vbmc_elbo_call* whose theta / dF / F / G / H are the fields below
  double* th = nullptr;                     // n_theta
  const double* dF = nullptr;               // n_theta
  const double *F = nullptr, *G = nullptr, *H = nullptr;
  uint64_t* seed = nullptr;                 // &opts->seed
  int64_t n_theta = 0;
};

// `src` may be the block's own buffer (a caller that evaluates what it was handed back): memmove
static inline void step_lane_pack(const StepLane& l, const double* src) {
  std::memmove(l.th, src, sizeof(double) * static_cast<size_t>(l.n_theta));
}

static inline int step_lane_invoke(const StepLane& l) { return l.fn(l.handle, l.block); }

static inline void step_lane_grad(const StepLane& l, double* dst) {
  std::memcpy(dst, l.dF, sizeof(double) * static_cast<size_t>(l.n_theta));
}
