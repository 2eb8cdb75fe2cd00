// The layout of one call's device scratch, listed once: a bump carver in units of double.  An entry point adds its
// pieces in order, reserves the buffer (common.h reserve: the context's scratch; reserve_in: another grown buffer) and
// forms every pointer from the piece it got back, so the size and the pointers cannot drift apart.
// Pure size_t arithmetic: no HIP header, usable from a host-only probe.
#pragma once
#include <cstddef>

// `count` elements of T at `off` doubles from the buffer's start
template <class T = double>
struct Piece {
  size_t off = 0, count = 0;
};

struct Scratch {
  size_t total = 0;        // doubles: the end of the last piece
  double* base = nullptr;  // set by reserve(): no piece has an address before

  // count elements of elem_bytes each at the next multiple of `align` doubles, rounded up to whole doubles; a piece of
  // count 0 takes no room (and no alignment padding).  Returns the piece's offset.
  size_t add_bytes(size_t count, size_t elem_bytes, size_t align = 1) {
    if (count == 0) return total;
    const size_t off = (total + align - 1) / align * align;
    total = off + (count * elem_bytes + 7) / 8;
    return off;
  }
  template <class T = double>
  Piece<T> add(size_t count, size_t align = 1) {
    Piece<T> p;
    p.off = add_bytes(count, sizeof(T), align);
    p.count = count;
    return p;
  }
  // (an empty piece's pointer is where it would lie: callers that hand null for an absent buffer say so themselves)
  template <class T>
  T* ptr(const Piece<T>& p) const {
    return base ? (T*)(base + p.off) : nullptr;
  }
};

// The scratch of the four input-warping entry points (api_warp.hip), one list each; a piece an entry does not use has
// count 0.
//   vbmc_warp_points   x (n x D) | y (n x D) | lj_new (n) | lj_old (n)
//   vbmc_warp_unscent  x (n x D) | sigma (rows x D) | mean, sd (n x D each) | pts (U x n x D, on request)
//   vbmc_warp_gp       x (N x D) | sigma = ell (S x D) | mean, sd = log ell_new (S x N x D each) | lj_new, lj_old (N) |
//                      out (S x D + 2)
//   vbmc_warp_box      x = the uniforms (n x D, uploaded draws only) | box (2 D) | y (n x D) | keys (D x pmax) and
//                      nonfinite flags (D) (quantile mode) | out (2 D) | sorted (D x n, on request)
struct WarpWs {
  Scratch sc;
  Piece<> x, sigma, box, y, mean, sd, pts, lj_new, lj_old, out, sorted;
  Piece<unsigned long long> keys;
  Piece<unsigned> nonfinite;
};
inline WarpWs warp_points_ws(size_t n, size_t D, bool want_y, bool want_new, bool want_old) {
  WarpWs w;
  w.x = w.sc.add(n * D);
  w.y = w.sc.add(want_y ? n * D : 0);
  w.lj_new = w.sc.add(want_new ? n : 0);
  w.lj_old = w.sc.add(want_old ? n : 0);
  return w;
}
inline WarpWs warp_unscent_ws(size_t n, size_t D, size_t sigma_rows, bool want_pts) {
  WarpWs w;
  w.x = w.sc.add(n * D);
  w.sigma = w.sc.add(sigma_rows * D);
  w.mean = w.sc.add(n * D);
  w.sd = w.sc.add(n * D);
  w.pts = w.sc.add(want_pts ? (2 * D + 1) * n * D : 0);
  return w;
}
inline WarpWs warp_gp_ws(size_t N, size_t D, size_t S) {
  WarpWs w;
  w.x = w.sc.add(N * D);
  w.sigma = w.sc.add(S * D);
  w.mean = w.sc.add(S * N * D);
  w.sd = w.sc.add(S * N * D);
  w.lj_new = w.sc.add(N);
  w.lj_old = w.sc.add(N);
  w.out = w.sc.add(S * D + 2);
  return w;
}
inline WarpWs warp_box_ws(size_t n, size_t D, bool uploaded, bool quantiles, size_t pmax, bool want_sorted) {
  WarpWs w;
  w.x = w.sc.add(uploaded ? n * D : 0);
  w.box = w.sc.add(2 * D);
  w.y = w.sc.add(n * D);
  w.keys = w.sc.add<unsigned long long>(quantiles ? D * pmax : 0);
  w.nonfinite = w.sc.add<unsigned>(quantiles ? D : 0);
  w.out = w.sc.add(2 * D);
  w.sorted = w.sc.add(want_sorted ? D * n : 0);
  return w;
}

// The state of one CMA-ES run of vbmc_search_cmaes in the search workspace (cmaes.hip), offsets in doubles: the head
// (phase, stop reason, counters: 8 doubles) | p_sigma, p_c, 1 / diag L (D each) | L (D x D) | the generation's points,
// steps y and repaired normals z' (lambda x D each) | the ring of generation-best values (hist).  The mean, sigma, C,
// the best point and value and the stats are the call's outputs and live in its result block.
struct CmaState {
  size_t head = 0, ps = 0, pc = 0, rdiag = 0, L = 0, X = 0, Y = 0, Z = 0, ring = 0, total = 0;
#if defined(__HIPCC__)
  __host__ __device__
#endif
  CmaState(int D, int lam, int hist) {
    const size_t d = (size_t)D, ld = (size_t)lam * d;
    size_t o = 8;
    ps = o; o += d;
    pc = o; o += d;
    rdiag = o; o += d;
    L = o; o += d * d;
    X = o; o += ld;
    Y = o; o += ld;
    Z = o; o += ld;
    ring = o; o += (size_t)hist;
    total = o;
  }
};

// The scratch of vbmc_marginals (api_marginals.hip) behind the kde pieces (kde.hip's plan: the keys of the D sorted
// columns first, which the call's own sort shares):
//   x (n x D samples, drawn or uploaded) | selector of the draw | par = ranges (2 D), quantile levels (nq), mass
//   levels (nl), uploaded | colinfo (D x 4: lo, hi, hi - lo, step) | idx (D x ns bytes, ns = n rounded up to 256: the bin
//   of every sample per dimension) | the result block, downloaded in one copy: edges (D x (bins + 1)) | quantiles
//   (nq x D) | kde_x, kde_density (D x mesh each) | colp (the kde's per-column results) | counts1 (D x bins uint64) |
//   counts2 (P x bins x bins uint64) | inside2 (P uint64) | level_counts (P x nl int64) | level_mass (P x nl) |
//   nonfinite (D unsigned)
struct MargWs {
  Piece<> x, sel, par, colinfo, edges, quant, kde_x, kde_dens, colp, level_mass;
  Piece<unsigned char> idx;
  Piece<unsigned long long> counts1, counts2, inside2;
  Piece<long long> level_counts;
  Piece<unsigned> nonfinite;
  size_t res_begin = 0, res_end = 0;  // the result block, in doubles
};
inline MargWs marginals_ws(Scratch& sc, size_t n, size_t ns, size_t D, size_t bins, size_t P, size_t nq, size_t nl,
                           size_t sel_elems, size_t mesh, size_t colp_stride) {
  MargWs w;
  w.x = sc.add(n * D);
  w.sel = sc.add(sel_elems);
  w.par = sc.add(2 * D + nq + nl);
  w.colinfo = sc.add(4 * D);
  w.idx = sc.add<unsigned char>(D * ns);
  w.edges = sc.add(D * (bins + 1));
  w.res_begin = w.edges.off;
  w.quant = sc.add(nq * D);
  w.kde_x = sc.add(D * mesh);
  w.kde_dens = sc.add(D * mesh);
  w.colp = sc.add(mesh ? D * colp_stride : 0);
  w.counts1 = sc.add<unsigned long long>(D * bins);
  w.counts2 = sc.add<unsigned long long>(P * bins * bins);
  w.inside2 = sc.add<unsigned long long>(P);
  w.level_counts = sc.add<long long>(P * nl);
  w.level_mass = sc.add(P * nl);
  w.nonfinite = sc.add<unsigned>(D);
  w.res_end = sc.total;
  return w;
}
