// The 64 x 64 workgroup tile on v_mfma_f64_16x16x4_f64: the single definition of its lane map, its 2 x 2 step, the walk
// over its results and its per-row reduction.  Every dense GP kernel that puts a 64 x 64 tile on the FP64 matrix cores
// (the panel product, K*, sq_dist) calls these, so a change of the tile's layout is made once.
//
// v_mfma_f64_16x16x4_f64: lane l holds A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15] and 4 results
// C[row = (l >> 4) + 4 r][col = l & 15].  Workgroup = 256 threads = 4 waves; wave (wm, wc) owns rows 32 wm .. + 31 and
// columns 32 wc .. + 31 as 2 x 2 MFMA tiles: acc[mt][ct][r] is
//   row = 32 wm + 16 mt + lk + 4 r,   col = 32 wc + 16 ct + li.
// On gfx950 the FP64 MFMA peak equals the FP64 vector peak (78.6 TFLOP/s); what the matrix instruction buys is issue
// efficiency: 1024 FMAs per instruction and no per-FMA operand traffic.
#pragma once
#include "fastmath.h"

namespace mfma_tile {

typedef double double4_t __attribute__((ext_vector_type(4)));
typedef double4_t Acc[2][2];

constexpr int TS = 64;  // tile side
// LDS row strides (doubles).  Fragments are read as ds_read_b64 with lane = (li = lane & 15, lk = lane >> 4).
//   KDP: operands staged [row][k], k <= 32.  A 32-lane group covers li = 0..15, lk = 0..1, dword bank
//        (2 (stride li + lk)) mod 64.  An ODD stride (33, rounds 1-2) always puts some (li, lk = 1) on the bank of
//        another (li', lk = 0) -- 38 % of K*'s LDS cycles were conflict cycles (PMC, r02); stride = 2 mod 4 gives banks
//        4 li + 2 lk: 32 distinct ones.
//   LDA: a 16-deep panel [row][k], +1 pad: the 16 rows of an A fragment hit distinct banks.
//   LDB: a 16-deep panel [k][col], row stride = 32 banks mod 64: the 4 k-rows of a B fragment do not collide.
constexpr int TKD = 16, KDP = 32 + 2, LDA = TKD + 1, LDB = TS + 16;

struct Lanes {
  int wm, wc, li, lk;
};
__device__ __forceinline__ Lanes lanes(int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  return {wave >> 1, wave & 1, lane & 15, lane >> 4};
}

__device__ __forceinline__ void zero(Acc& acc) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (double4_t){0.0, 0.0, 0.0, 0.0};
}

// acc += the four 16 x 16 x 4 products of two row fragments and two column fragments
__device__ __forceinline__ void step(Acc& acc, double a0, double a1, double b0, double b1) {
  acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
  acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
  acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
  acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
}
// k-step kq (k = 4 kq .. 4 kq + 3) with both operands in LDS as [row][k], row stride ld (K*, sq_dist)
__device__ __forceinline__ void step_rows(Acc& acc, const Lanes& L, const double* sA, const double* sB, int ld, int kq) {
  const int k = kq * 4 + L.lk;
  step(acc, sA[(L.wm * 32 + L.li) * ld + k], sA[(L.wm * 32 + 16 + L.li) * ld + k], sB[(L.wc * 32 + L.li) * ld + k],
       sB[(L.wc * 32 + 16 + L.li) * ld + k]);
}
// the same with B as [k][col] (the panel products): sA [64][LDA], sB [TKD][LDB]
__device__ __forceinline__ void step_panel(Acc& acc, const Lanes& L, const double* sA, const double* sB, int kq) {
  const int k = kq * 4 + L.lk;
  step(acc, sA[(L.wm * 32 + L.li) * LDA + k], sA[(L.wm * 32 + 16 + L.li) * LDA + k], sB[k * LDB + L.wc * 32 + L.li],
       sB[k * LDB + L.wc * 32 + 16 + L.li]);
}

// The walk over this lane's results: for each of its 8 rows (mt, then r), elem(row, col, value) for its two columns
// (ct ascending), then row_end(row).  row and col are inside the tile.
template <class Elem, class RowEnd>
__device__ __forceinline__ void walk(const Acc& acc, const Lanes& L, Elem&& elem, RowEnd&& row_end) {
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = L.wm * 32 + mt * 16 + L.lk + 4 * r;
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) elem(row, L.wc * 32 + ct * 16 + L.li, acc[mt][ct][r]);
      row_end(row);
    }
}

// Per-row reduction over the tile's 64 columns: v = this lane's sum over its two columns of `row`; the 16 lanes that
// share the row are summed by DPP, and the two column waves meet in LDS (sRow: 2 TS doubles).  After a barrier,
// row_sum(sRow, row) is the row's total: column wave 0 + column wave 1.
__device__ __forceinline__ void row_sum_put(double* sRow, const Lanes& L, int row, double v) {
  v = fm::row16_sum_dpp(v);
  if (L.li == 0) sRow[row * 2 + L.wc] = v;
}
__device__ __forceinline__ double row_sum(const double* sRow, int row) { return sRow[row * 2] + sRow[row * 2 + 1]; }

}  // namespace mfma_tile
