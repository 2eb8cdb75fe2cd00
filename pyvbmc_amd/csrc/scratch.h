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
