// What the lockstep entries share around their advance kernels (vbmc_search_cmaes, vbmc_gp_hyp_sample,
// vbmc_gp_hyp_optimize; common.h has the round driver, lockstep_rounds): the count of the runs that have not finished,
// and the fetch of a call's results in one copy.
#include <cstring>

#include "common.h"

namespace {

// *count = the runs of [0, n_runs) whose 32-bit word at `off` bytes into their state is not done_value.  One workgroup:
// the host reads the one int.
__global__ __launch_bounds__(256) void lockstep_count_kernel(const double* __restrict__ state, int n_runs, size_t state_elems,
                                                             size_t off, int done_value, int* __restrict__ count) {
  __shared__ int s_n;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  int n = 0;
  for (int r = threadIdx.x; r < n_runs; r += 256)
    n += *(const int*)((const char*)(state + (size_t)r * state_elems) + off) == done_value ? 0 : 1;
  if (n) atomicAdd(&s_n, n);  // (LDS, integers: the order does not matter)
  __syncthreads();
  if (threadIdx.x == 0) *count = s_n;
}

}  // namespace

int launch_lockstep_count(vbmc_ctx* ctx, const double* d_state, int n_runs, size_t state_elems, size_t word_offset_bytes,
                          int done_value, int* d_count) {
  hipLaunchKernelGGL(lockstep_count_kernel, dim3(1), dim3(256), 0, ctx->stream, d_state, n_runs, state_elems,
                     word_offset_bytes, done_value, d_count);
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

int fetch_tail(vbmc_ctx* ctx, const Scratch& sc, size_t from, std::initializer_list<FetchPiece> pieces) {
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_pinned, sc.base + from, sizeof(double) * (sc.total - from), hipMemcpyDeviceToHost,
                              ctx->stream));
  HIP_TRY(ctx, stream_wait(ctx));
  for (const FetchPiece& p : pieces)
    if (p.dst && p.bytes) memcpy(p.dst, ctx->h_pinned + (p.off - from), p.bytes);
  return VBMC_OK;
}
