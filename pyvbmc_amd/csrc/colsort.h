// Exact sort of the columns of a device matrix, shared by kde.hip (kde_1d, mtv) and warp.hip (the quantiles of
// warp_input's plausible box): order-preserving 64-bit keys, an LDS bitonic sort of 8192-key chunks (one workgroup per
// chunk) and the remaining bitonic stages over a whole column (one workgroup per column).  Integer compare-exchanges
// only: the sorted column is the input's values exactly, whatever the launch geometry.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

constexpr int kThreads = 512;          // column / chunk-sort workgroups (2 waves / SIMD: 256 VGPRs)
constexpr int kWaves = kThreads / 64;
constexpr int kChunk = 8192;           // keys per LDS sort chunk (64 KiB)

// the columns to sort: up to two matrices ("sides"), columns [0, ncol0) from side 0, the rest from side 1
struct KdeSrc {
  const double* x[2];
  int64_t n[2];
  int64_t rs[2];  // row stride (elements)
  int64_t cs[2];  // column stride
  int ncol0;      // columns of side 0
};

__host__ __device__ inline int64_t next_pow2(int64_t v) {
  int64_t p = 1;
  while (p < v) p <<= 1;
  return p;
}

__device__ inline uint64_t to_key(double v) {
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ inline double from_key(uint64_t k) {
  const uint64_t b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)b);
}

__device__ inline void cas_keys(uint64_t* a, uint64_t* b, bool asc) {
  const uint64_t x = *a, y = *b;
  if ((x > y) == asc) {
    *a = y;
    *b = x;
  }
}

// the index pair of compare-exchange number i at stride j
__device__ inline int64_t pair_lo(int64_t i, int64_t j) { return ((i & ~(j - 1)) << 1) | (i & (j - 1)); }

// bitonic passes j = jtop .. 1 of stage k on an LDS chunk whose first key has global index g0
__device__ void lds_bitonic(uint64_t* sk, int64_t g0, int64_t k, int jtop) {
  for (int j = jtop; j > 0; j >>= 1) {
    for (int i = threadIdx.x; i < kChunk / 2; i += kThreads) {
      const int lo = (int)pair_lo(i, j);
      cas_keys(&sk[lo], &sk[lo + j], ((g0 + lo) & k) == 0);
    }
    __syncthreads();
  }
}

// grid (pmax / kChunk, columns): the keys of a column, padded to a power of two (>= kChunk), each chunk sorted
__global__ __launch_bounds__(kThreads) void kde_sort_chunks_kernel(KdeSrc s, uint64_t* __restrict__ keys,
                                                                   int64_t pmax, unsigned* __restrict__ nonfinite) {
  __shared__ uint64_t sk[kChunk];
  const int c = blockIdx.y;
  const int side = c >= s.ncol0;
  const int col = side ? c - s.ncol0 : c;
  const int64_t n = s.n[side];
  const int64_t P = next_pow2(n > kChunk ? n : kChunk);
  const int64_t g0 = (int64_t)blockIdx.x * kChunk;
  if (g0 >= P) return;
  const double* x = s.x[side] + (int64_t)col * s.cs[side];
  const int64_t rs = s.rs[side];
  bool bad = false;
  for (int i = threadIdx.x; i < kChunk; i += kThreads) {
    const int64_t g = g0 + i;
    uint64_t key = ~0ull;  // padding sorts last
    if (g < n) {
      const double v = x[g * rs];
      bad |= !isfinite(v);
      key = to_key(v);
    }
    sk[i] = key;
  }
  if (bad) atomicOr(&nonfinite[c], 1u);
  __syncthreads();
  for (int64_t k = 2; k <= kChunk; k <<= 1) lds_bitonic(sk, g0, k, (int)(k >> 1));
  uint64_t* out = keys + (int64_t)c * pmax + g0;
  for (int i = threadIdx.x; i < kChunk; i += kThreads) out[i] = sk[i];
}

// the remaining bitonic stages of a column of P keys whose chunks are sorted (one workgroup owns the column): global
// passes for strides >= kChunk, LDS passes below.  sk: kChunk keys of LDS.
__device__ inline void column_merge(uint64_t* gk, int64_t P, uint64_t* sk) {
  const int tid = threadIdx.x;
  for (int64_t k = 2 * (int64_t)kChunk; k <= P; k <<= 1) {
    for (int64_t j = k >> 1; j >= kChunk; j >>= 1) {
      for (int64_t i = tid; i < P / 2; i += kThreads) {
        const int64_t lo = pair_lo(i, j);
        cas_keys(&gk[lo], &gk[lo + j], (lo & k) == 0);
      }
      __syncthreads();
    }
    for (int64_t g0 = 0; g0 < P; g0 += kChunk) {
      for (int i = tid; i < kChunk; i += kThreads) sk[i] = gk[g0 + i];
      __syncthreads();
      lds_bitonic(sk, g0, k, kChunk / 2);
      for (int i = tid; i < kChunk; i += kThreads) gk[g0 + i] = sk[i];
      __syncthreads();
    }
  }
}

}  // namespace
