// Where does the dispatcher put workgroup b of a grid with two resident workgroups per CU, and on which SIMD does each
// of a workgroup's four waves land?  The probe kernel has the wave-split entropy kernel's footprint at BASELINE
// config 3 (256 threads, 246 VGPRs = two waves per SIMD, 19 KB static + 36 KB dynamic LDS) and is launched on its two
// grids: span mode's one-dimensional grid (512 workgroups: blocks b and b + CUs are the front and the filler of a CU)
// and the paired chunk grid (10 x 50 workgroups, b = blockIdx.y * gridDim.x + blockIdx.x).
//   hipcc --offload-arch=gfx950 -O2 tools/probes/placement.hip -o /tmp/placement && /tmp/placement
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
#include <map>
#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1;} } while (0)
__global__ __launch_bounds__(256, 2) void K(unsigned* out, int spin_us) {
  extern __shared__ double lds[];
  __shared__ double stat[19104 / 8];
  const unsigned long long t0 = wall_clock64();
  asm volatile("v_mov_b32 v245, 0" ::: "v245");  // the register footprint: 246 VGPRs
  const int b = blockIdx.y * gridDim.x + blockIdx.x;
  if ((threadIdx.x & 63) == 0) {
    unsigned hw = __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));    // HW_ID
    unsigned xcc = __builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (3 << 11));   // XCC_ID
    out[2 * (4 * b + (threadIdx.x >> 6))] = hw;
    out[2 * (4 * b + (threadIdx.x >> 6)) + 1] = xcc;
  }
  lds[threadIdx.x] = (double)t0;
  stat[threadIdx.x] = (double)t0;
  while (wall_clock64() - t0 < (unsigned long long)spin_us * 100) __builtin_amdgcn_s_sleep(8);
}
static int probe(const char* what, dim3 grid, unsigned* d, int cus) {
  const int NB = grid.x * grid.y;
  const int dyn = 36 * 1024;
  for (int rep = 0; rep < 3; ++rep) {
    CHECK(hipMemset(d, 0xff, 32 * NB));
    hipLaunchKernelGGL(K, grid, dim3(256), dyn, 0, d, 30);
    CHECK(hipDeviceSynchronize());
    std::vector<unsigned> h(8 * NB); CHECK(hipMemcpy(h.data(), d, 32 * NB, hipMemcpyDeviceToHost));
    std::map<unsigned, std::vector<int>> by_cu;
    int in_order = 0, distinct = 0, one_cu = 0, perm_hist[256] = {};
    for (int b = 0; b < NB; ++b) {
      unsigned cuid[4], simd[4];
      for (int w = 0; w < 4; ++w) {
        const unsigned hw = h[2 * (4 * b + w)], xcc = h[2 * (4 * b + w) + 1] & 0xF;
        simd[w] = (hw >> 4) & 3;
        cuid[w] = (xcc << 12) | (((hw >> 13) & 7) << 8) | (((hw >> 12) & 1) << 4) | ((hw >> 8) & 0xF);
      }
      one_cu += cuid[0] == cuid[1] && cuid[0] == cuid[2] && cuid[0] == cuid[3];
      in_order += simd[0] == 0 && simd[1] == 1 && simd[2] == 2 && simd[3] == 3;
      distinct += ((1u << simd[0]) | (1u << simd[1]) | (1u << simd[2]) | (1u << simd[3])) == 0xF;
      perm_hist[simd[0] | (simd[1] << 2) | (simd[2] << 4) | (simd[3] << 6)]++;
      by_cu[cuid[0]].push_back(b);
      if (rep == 0 && (b < 6 || (b >= cus && b < cus + 6)))
        printf("  b=%3d xcc=%u se=%u sh=%u cu=%2u  simd of waves 0..3: %u %u %u %u  wave slots: %u %u %u %u\n", b, cuid[0] >> 12, (cuid[0] >> 8) & 7,
               (cuid[0] >> 4) & 1, cuid[0] & 0xF, simd[0], simd[1], simd[2], simd[3], h[2 * (4 * b)] & 0xF, h[2 * (4 * b + 1)] & 0xF,
               h[2 * (4 * b + 2)] & 0xF, h[2 * (4 * b + 3)] & 0xF);
    }
    int pairs = 0, pair_is_b_plus_cus = 0, more = 0;
    for (auto& kv : by_cu) {
      if (kv.second.size() == 2) { ++pairs; pair_is_b_plus_cus += kv.second[1] - kv.second[0] == cus; }
      more += kv.second.size() > 2;
    }
    printf("%s rep %d: %d workgroups on %zu CUs; all four waves on one CU: %d; on four different SIMDs: %d; wave w on SIMD w: %d; "
           "CUs with two workgroups: %d, of them (b, b + %d): %d; CUs with more: %d\n", what, rep, NB, by_cu.size(), one_cu, distinct,
           in_order, pairs, cus, pair_is_b_plus_cus, more);
    for (int p = 0; p < 256; ++p)
      if (perm_hist[p] && p != (0 | (1 << 2) | (2 << 4) | (3 << 6)))
        printf("    simd of waves 0..3 = %d %d %d %d: %d workgroups\n", p & 3, (p >> 2) & 3, (p >> 4) & 3, (p >> 6) & 3, perm_hist[p]);
  }
  return 0;
}
int main() {
  hipDeviceProp_t prop; CHECK(hipGetDeviceProperties(&prop, 0));
  const int cus = prop.multiProcessorCount;
  unsigned* d; CHECK(hipMalloc(&d, 32 * 1024));
  CHECK(hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize, 36 * 1024));
  printf("%d CUs\n", cus);
  if (probe("span grid", dim3(2 * cus), d, cus)) return 1;   // (all 2 * CUs slots: the GP row's workgroups stand in for the missing fillers)
  if (probe("chunk grid", dim3(10, 50), d, cus)) return 1;  // config 3 on equal chunks: K = 50 rows of 10 chunks
  return 0;
}
