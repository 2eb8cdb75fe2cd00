// Test probes for the device primitives of fastmath.h (and mixture_dev.h's exp2_arg guard): each entry point runs ONE
// primitive per thread on caller-supplied inputs, so tests/test_fastmath_gpu.py can compare it with a high-precision
// reference directly instead of through a whole kernel.  Built into libvbmc_devprobe.so with the flags of the main
// library (-O3 -ffp-contract=off: the functions compile as they do inside the kernels); not linked into
// libvbmc_hip.so and not part of the C ABI (include/vbmc_hip.h).
//
// Every entry point takes host pointers, allocates, copies, launches once, copies back and frees on the current device,
// and returns the first HIP error as an int (0: none).
#include <hip/hip_runtime.h>

#include <cstddef>

#include "fastmath.h"
#include "mixture_dev.h"
#include "scratch.h"

namespace {

constexpr int BLOCK = 256;  // four full waves: the DPP reductions need full waves (fastmath.h)

enum { FN_EXP2 = 0, FN_LOG = 1, FN_RCP = 2, FN_RSQRT = 3, FN_EXP2_GUARDED = 4, FN_COUNT = 5 };
enum { OP_SUM = 0, OP_MAX = 1, OP_PROD = 2, OP_ROW16 = 3, OP_COUNT = 4 };

template <int FN>
__global__ __launch_bounds__(BLOCK) void unary_kernel(const double* __restrict__ x, double* __restrict__ y, size_t n) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const double v = x[i];
  double r;
  if (FN == FN_EXP2) r = fm::exp2_fast(v);
  else if (FN == FN_LOG) r = fm::log_fast(v);
  else if (FN == FN_RCP) r = fm::rcp_fast(v);
  else if (FN == FN_RSQRT) r = fm::rsqrt_fast(v);
  else r = fm::exp2_fast(exp2_arg(v));
  y[i] = r;
}

__global__ __launch_bounds__(BLOCK) void sincospi_kernel(const double* __restrict__ y, double* __restrict__ s,
                                                         double* __restrict__ c, size_t n) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  double sv, cv;
  fm::sincospi_fast(y[i], sv, cv);
  s[i] = sv;
  c[i] = cv;
}

// v, out: [gridDim.x][BLOCK]; no thread leaves early (the reductions run with all 64 lanes of every wave active) and
// every thread stores the value its own lane holds
template <int OP>
__global__ __launch_bounds__(BLOCK) void wave_kernel(const double* __restrict__ v, double* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  const double a = v[i];
  double r;
  if (OP == OP_SUM) r = fm::wave_sum_dpp(a);
  else if (OP == OP_MAX) r = fm::wave_max_dpp(a);
  else if (OP == OP_PROD) r = fm::wave_prod_dpp(a);
  else r = fm::row16_sum_dpp(a);
  out[i] = r;
}

// the device arrays of one call, freed on every return path
struct Buffers {
  double* d[3] = {nullptr, nullptr, nullptr};
  ~Buffers() {
    for (double* p : d)
      if (p) (void)hipFree(p);
  }
};

#define PROBE_TRY(call)                \
  do {                                 \
    const hipError_t e_ = (call);      \
    if (e_ != hipSuccess) return (int)e_; \
  } while (0)

}  // namespace

extern "C" {

int vbmc_probe_unary(int fn, const double* x, double* y, size_t n) {
  if (fn < 0 || fn >= FN_COUNT || (n && (!x || !y))) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  if (n > ((size_t)1 << 31)) return (int)hipErrorInvalidValue;
  Buffers b;
  const size_t bytes = n * sizeof(double);
  PROBE_TRY(hipMalloc(&b.d[0], bytes));
  PROBE_TRY(hipMalloc(&b.d[1], bytes));
  PROBE_TRY(hipMemcpy(b.d[0], x, bytes, hipMemcpyHostToDevice));
  const dim3 grid((unsigned)((n + BLOCK - 1) / BLOCK)), block(BLOCK);
  switch (fn) {
    case FN_EXP2: unary_kernel<FN_EXP2><<<grid, block>>>(b.d[0], b.d[1], n); break;
    case FN_LOG: unary_kernel<FN_LOG><<<grid, block>>>(b.d[0], b.d[1], n); break;
    case FN_RCP: unary_kernel<FN_RCP><<<grid, block>>>(b.d[0], b.d[1], n); break;
    case FN_RSQRT: unary_kernel<FN_RSQRT><<<grid, block>>>(b.d[0], b.d[1], n); break;
    default: unary_kernel<FN_EXP2_GUARDED><<<grid, block>>>(b.d[0], b.d[1], n); break;
  }
  PROBE_TRY(hipGetLastError());
  PROBE_TRY(hipDeviceSynchronize());
  PROBE_TRY(hipMemcpy(y, b.d[1], bytes, hipMemcpyDeviceToHost));
  return 0;
}

int vbmc_probe_sincospi(const double* y, double* s, double* c, size_t n) {
  if (n && (!y || !s || !c)) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  if (n > ((size_t)1 << 31)) return (int)hipErrorInvalidValue;
  Buffers b;
  const size_t bytes = n * sizeof(double);
  PROBE_TRY(hipMalloc(&b.d[0], bytes));
  PROBE_TRY(hipMalloc(&b.d[1], bytes));
  PROBE_TRY(hipMalloc(&b.d[2], bytes));
  PROBE_TRY(hipMemcpy(b.d[0], y, bytes, hipMemcpyHostToDevice));
  sincospi_kernel<<<dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK)>>>(b.d[0], b.d[1], b.d[2], n);
  PROBE_TRY(hipGetLastError());
  PROBE_TRY(hipDeviceSynchronize());
  PROBE_TRY(hipMemcpy(s, b.d[1], bytes, hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(c, b.d[2], bytes, hipMemcpyDeviceToHost));
  return 0;
}

int vbmc_probe_wave(int op, const double* v, double* out, int n_blocks) {
  if (op < 0 || op >= OP_COUNT || n_blocks < 0 || n_blocks > 65536 || (n_blocks && (!v || !out)))
    return (int)hipErrorInvalidValue;
  if (n_blocks == 0) return 0;
  Buffers b;
  const size_t bytes = (size_t)n_blocks * BLOCK * sizeof(double);
  PROBE_TRY(hipMalloc(&b.d[0], bytes));
  PROBE_TRY(hipMalloc(&b.d[1], bytes));
  PROBE_TRY(hipMemcpy(b.d[0], v, bytes, hipMemcpyHostToDevice));
  const dim3 grid((unsigned)n_blocks), block(BLOCK);
  switch (op) {
    case OP_SUM: wave_kernel<OP_SUM><<<grid, block>>>(b.d[0], b.d[1]); break;
    case OP_MAX: wave_kernel<OP_MAX><<<grid, block>>>(b.d[0], b.d[1]); break;
    case OP_PROD: wave_kernel<OP_PROD><<<grid, block>>>(b.d[0], b.d[1]); break;
    default: wave_kernel<OP_ROW16><<<grid, block>>>(b.d[0], b.d[1]); break;
  }
  PROBE_TRY(hipGetLastError());
  PROBE_TRY(hipDeviceSynchronize());
  PROBE_TRY(hipMemcpy(out, b.d[1], bytes, hipMemcpyDeviceToHost));
  return 0;
}

// host only: scratch.h's carver over n pieces (count, element bytes, alignment in doubles); offsets[i] and the total, in
// doubles (tests/test_scratch_layout.py)
void vbmc_probe_scratch_layout(int n, const size_t* count, const size_t* elem_bytes, const size_t* align, size_t* offsets,
                               size_t* total) {
  Scratch sc;
  for (int i = 0; i < n; ++i) offsets[i] = sc.add_bytes(count[i], elem_bytes[i], align[i]);
  *total = sc.total;
}

}  // extern "C"
