// kde_1d (stats/kde_1d.py:144-257) and VariationalPosterior.mtv (variational_posterior.py:921-1030) on the device.
//
// Five kernels, each stage per column (a column = the samples of one dimension of one side):
//   kde_sort_chunks_kernel  one workgroup per 8192-key chunk: the order-preserving 64-bit keys of the column,
//                           padded to a power of two, bitonic-sorted in LDS (the first log2(8192) stages)
//   kde_column_kernel       one workgroup per column: the remaining bitonic stages (global passes for strides
//                           >= 8192, LDS passes below), then min / max, len(np.unique), the mesh, the bin counts
//                           (integer) and the DCT-II through an n/2-point complex FFT in LDS
//   kde_bandwidth_kernel    one workgroup per column: _root / brentq on _fixed_point, or Scott's rule (the
//                           quartiles and std(ddof=1) of the sorted column)
//   kde_density_kernel      one workgroup per column: the smoothing, the DCT-III -- and for mtv the trapezoid
//                           normalisation and the not-a-knot cubic spline of the density
//   mtv_integral_kernel     |s1 - s2| on the three linspace(bb[j], bb[j+1], 1e5) segments of each dimension,
//                           trapezoid-weighted per-block partial sums (the host adds them in a fixed order)
// The three per-column stages are separate launches so that each kernel's live scalars fit the SGPR file: as one
// kernel it spilled 60 SGPRs.
//
// Every reduction runs in a fixed order (no float atomics; the bin counts are integer LDS atomics), so a call
// is bit-reproducible.  The mesh and bin arithmetic is written with plain operations (the build uses
// -ffp-contract=off), so the counts are the reference's exactly.
#include <cmath>
#include <cstring>
#include <vector>

#include "colsort.h"  // kThreads, kChunk, KdeSrc, the keys, kde_sort_chunks_kernel, column_merge
#include "common.h"
#include "kde.h"
#include "transform.h"

namespace {

constexpr int kMaxMesh = 1 << 14;      // n <= 2^14: the FFT buffer is n doubles (128 KiB of LDS)
constexpr int kMtvMesh = 1 << 13;     // nkde = 2**13 (:976); the spline needs 2 n doubles of LDS
constexpr int kSegPts = 100000;        // mtv: points per linspace segment (:1024)
constexpr int kIntThreads = 256;
constexpr int kIntPerThread = 4;
constexpr int kIntBlocks = (kSegPts + kIntThreads * kIntPerThread - 1) / (kIntThreads * kIntPerThread);
constexpr int kOverlap = 32;           // spline recursion warm-up: (2 - sqrt 3)^32 < 1e-18

// per-column results of kde_column_kernel (doubles)
enum { CP_X0, CP_XL, CP_STEP, CP_DX, CP_BW, CP_T, CP_DELTA, CP_LOWER, CP_N };
// per-column flags
enum { KF_SCOTT = 1, KF_NONFINITE = 2, KF_DEGENERATE = 4, KF_ROOT_STUCK = 8 };
// bound modes
enum { BND_KDE = 0, BND_MTV = 1 };

// the constants of _fixed_point per order s = 2 .. 7 (kde_1d.py:47-73), from the host's libm
struct FpConsts {
  double two_pi2s[8];    // 2 pi^(2 s)
  double two_cst_k0[8];  // 2 ((1 + 0.5^(s + 1/2)) / 3) (1 3 .. (2s - 1)) / sqrt(2 pi)
  double expo[8];        // 2 / (3 + 2 s)
  double sqrt_pi;
};

struct KdeArgs {
  KdeSrc src;
  FpConsts fc;
  uint64_t* keys;      // ncol x pmax
  int64_t pmax;
  unsigned* nonfinite; // ncol
  int nm;              // mesh size (power of two)
  int mode;            // BND_KDE / BND_MTV
  const double* lb;    // per column, nullable (BND_KDE: derive the bound)
  const double* ub;
  double* ga;          // ncol x nm scratch
  double* dens;        // ncol x nm
  double* xmesh;       // ncol x nm, nullable
  double* msp;         // ncol x nm spline second-difference coefficients, nullable (mtv)
  double* colp;        // ncol x CP_N
  int64_t* stat;       // ncol x 2: len(np.unique), flags
};

// ---- workgroup reductions (fixed order: a wave butterfly, then the wave sums in order) ----
__device__ inline double wg_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) s += red[w];
  return s;
}

__device__ inline int64_t wg_sum_i(int64_t v, int64_t* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int64_t s = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) s += red[w];
  return s;
}

__device__ inline unsigned bitrev(unsigned v, int bits) { return bits ? (__brev(v) >> (32 - bits)) : 0u; }

// in-place radix-2 decimation-in-time FFT of h complex values in LDS, input in bit-reversed order;
// sgn = -1: forward (e^{-2 pi i}), +1: unscaled inverse.  Twiddles from sincospi (exact arguments).
__device__ void fft_lds(double2* z, int h, double sgn) {
  for (int len = 2; len <= h; len <<= 1) {
    const int half = len >> 1;
    for (int b = threadIdx.x; b < h / 2; b += kThreads) {
      const int g = b / half, p = b - g * half;
      const int i0 = g * len + p, i1 = i0 + half;
      double sn, cs;
      sincospi(sgn * (double)(2 * p) / (double)len, &sn, &cs);
      const double2 a = z[i0], v = z[i1];
      const double br = v.x * cs - v.y * sn, bi = v.x * sn + v.y * cs;
      z[i0] = make_double2(a.x + br, a.y + bi);
      z[i1] = make_double2(a.x - br, a.y - bi);
    }
    __syncthreads();
  }
}

// _fixed_point (kde_1d.py:34-76) at t: six weighted sums over k = 1 .. n-1 of the LDS coefficients a[k].  The
// per-order constants come from the host's libm (FpConsts), as the reference's come from Python's.
__device__ double fixed_point(double t, double Nu, const double* a, int n, double* red, const FpConsts* fc) {
  const double pi2 = M_PI * M_PI;
  double f = 0.0;
  double time = t;
#pragma nounroll
  for (int s = 7; s >= 2; --s) {
    if (s < 7) time = pow(fc->two_cst_k0[s] / (Nu * f), fc->expo[s]);
    double part = 0.0;
    for (int k = threadIdx.x + 1; k < n; k += kThreads) {
      const double i2 = (double)k * (double)k;
      const double a2 = a[k] * a[k] / 4.0;
      part += pow(i2, (double)s) * a2 * exp(-i2 * pi2 * time);
    }
    f = fc->two_pi2s[s] * wg_sum(part, red);
    if (s == 7 && f <= 0.0) return -1.0;
  }
  const double t_opt = pow(2.0 * Nu * fc->sqrt_pi * f, -2.0 / 5.0);
  return t - t_opt;
}

// scipy.optimize.brentq(f, xa, xb, xtol=2e-12, rtol=4 eps, maxiter=100), step for step.  Returns 0 and the
// root (conv: converged), or 1 for the ValueError cases (no sign change, a NaN function value).  One call site of
// fixed_point (f(xa), f(xb), then one value per iteration) keeps a single inlined copy of it.
__device__ int brentq_fp(double xa, double xb, double Nu, const double* a, int n, double* red, const FpConsts* fc,
                         double* root, bool* conv) {
  const double xtol = 2e-12, rtol = 4.0 * 2.220446049250313e-16;
  double xpre = xa, xcur = xb, xblk = 0.0, fpre = 0.0, fcur = 0.0, fblk = 0.0, spre = 0.0, scur = 0.0;
  *conv = true;
  for (int ev = 0; ev < 102; ++ev) {
    const double fx = fixed_point(ev == 0 ? xpre : xcur, Nu, a, n, red, fc);
    if (isnan(fx)) return 1;
    if (ev == 0) {
      fpre = fx;
      continue;
    }
    fcur = fx;
    if (ev == 1) {
      if (fpre == 0.0) { *root = xpre; return 0; }
      if (fcur == 0.0) { *root = xcur; return 0; }
      if (signbit(fpre) == signbit(fcur)) return 1;
    }
    if (ev == 101) break;  // maxiter iterations done
    // iteration ev - 1
    if (fpre != 0.0 && fcur != 0.0 && (signbit(fpre) != signbit(fcur))) {
      xblk = xpre;
      fblk = fpre;
      spre = scur = xcur - xpre;
    }
    if (fabs(fblk) < fabs(fcur)) {
      xpre = xcur; xcur = xblk; xblk = xpre;
      fpre = fcur; fcur = fblk; fblk = fpre;
    }
    const double delta = (xtol + rtol * fabs(xcur)) / 2.0;
    const double sbis = (xblk - xcur) / 2.0;
    if (fcur == 0.0 || fabs(sbis) < delta) { *root = xcur; return 0; }
    if (fabs(spre) > delta && fabs(fcur) < fabs(fpre)) {
      double stry;
      if (xpre == xblk) {
        stry = -fcur * (xcur - xpre) / (fcur - fpre);
      } else {
        const double dpre = (fpre - fcur) / (xpre - xcur);
        const double dblk = (fblk - fcur) / (xblk - xcur);
        stry = -fcur * (fblk * dblk - fpre * dpre) / (dblk * dpre * (fblk - fpre));
      }
      const double lim = fmin(fabs(spre), 3.0 * fabs(sbis) - delta);
      if (2.0 * fabs(stry) < lim) {
        spre = scur;
        scur = stry;
      } else {
        spre = sbis;
        scur = sbis;
      }
    } else {
      spre = sbis;
      scur = sbis;
    }
    xpre = xcur;
    fpre = fcur;
    if (fabs(scur) > delta) xcur += scur;
    else xcur += (sbis > 0.0 ? delta : -delta);
  }
  *conv = false;
  *root = xcur;
  return 0;
}

// the Thomas coefficients c'_j = 1 / (4 - c'_{j-1}) of the interior rows [1 4 1] (c'_0 = 1/4), j = 0 .. 48: the
// recurrence is constant to rounding from ~20 rows on, so c'_j = c'_48 beyond (the same IEEE divisions as a sweep)
constexpr int kThomasRows = 49;
struct ThomasTable {
  double c[kThomasRows];
  constexpr ThomasTable() : c() {
    c[0] = 0.25;
    for (int j = 1; j < kThomasRows; ++j) c[j] = 1.0 / (4.0 - c[j - 1]);
  }
};
__constant__ ThomasTable kThomas = ThomasTable();
__device__ inline double thomas_c(int j) { return kThomas.c[j < kThomasRows - 1 ? j : kThomasRows - 1]; }

__global__ __launch_bounds__(kThreads) void kde_column_kernel(KdeArgs A) {
  extern __shared__ __attribute__((aligned(16))) double sh[];
  __shared__ int64_t redi[kWaves];
  const int c = blockIdx.x;
  const int tid = threadIdx.x;
  const int side = c >= A.src.ncol0;
  const int64_t n = A.src.n[side];
  const int64_t P = next_pow2(n > kChunk ? n : kChunk);
  uint64_t* gk = A.keys + (int64_t)c * A.pmax;
  const int nm = A.nm, h = nm / 2;
  double* cp = A.colp + (int64_t)c * CP_N;
  double* dens = A.dens + (int64_t)c * nm;
  double* ga = A.ga + (int64_t)c * nm;
  const bool bad = A.nonfinite[c] != 0;

  // ---- 1. the remaining bitonic stages (one workgroup owns the column) ----
  if (!bad) {
    column_merge(gk, P, (uint64_t*)sh);
  }

  // ---- 2. statistics of the sorted column ----
  const double vmin = from_key(gk[0]), vmax = from_key(gk[n - 1]);
  int64_t nu = 0;
  const int64_t per = (n + kThreads - 1) / kThreads;
  const int64_t r0 = (int64_t)tid * per, r1 = r0 + per < n ? r0 + per : n;
  for (int64_t i = r0 < 1 ? 1 : r0; i < r1; ++i) nu += from_key(gk[i]) != from_key(gk[i - 1]);
  nu = wg_sum_i(nu, redi) + 1;  // len(np.unique(samples)); -0.0 == 0.0 counts once

  double lower, upper;
  const double rng = vmax - vmin;
  if (A.mode == BND_MTV) {
    // np.maximum(min - range / 10, lb_orig), np.minimum(max + range / 10, ub_orig)  (:981-986)
    const double lo = vmin - rng / 10.0, hi = vmax + rng / 10.0;
    lower = lo < A.lb[c] ? A.lb[c] : lo;
    upper = hi > A.ub[c] ? A.ub[c] : hi;
  } else {
    // min(samples) - 0.1 * delta when not given (kde_1d.py:218-225)
    lower = A.lb ? A.lb[c] : vmin - 0.1 * rng;
    upper = A.ub ? A.ub[c] : vmax + 0.1 * rng;
  }
  // np.linspace(lower, upper, n): i * step + start, the last point = stop
  const double delta = upper - lower;
  const double div = (double)(nm - 1);
  const double step = delta / div;
  const double x1 = step == 0.0 ? (1.0 / div) * delta + lower : 1.0 * step + lower;
  const double x0 = (step == 0.0 ? (0.0 / div) * delta : 0.0 * step) + lower;
  const double xl = upper;
  const double dx = x1 - x0;
  if (A.xmesh) {
    double* xm = A.xmesh + (int64_t)c * nm;
    for (int i = tid; i < nm; i += kThreads)
      xm[i] = i == nm - 1 ? xl : (step == 0.0 ? ((double)i / div) * delta : (double)i * step) + lower;
  }
  int64_t flags = bad ? KF_NONFINITE : 0;
  if (!(dx > 0.0) || !isfinite(dx) || !isfinite(x0) || !isfinite(xl)) flags |= KF_DEGENERATE;
  if (tid == 0) {
    cp[CP_X0] = x0;
    cp[CP_XL] = xl;
    cp[CP_STEP] = step;
    cp[CP_DX] = dx;
    cp[CP_DELTA] = delta;
    cp[CP_LOWER] = lower;
  }
  if (flags) {
    for (int i = tid; i < nm; i += kThreads) {
      dens[i] = NAN;
      if (A.msp) A.msp[(int64_t)c * nm + i] = NAN;
    }
    if (tid == 0) {
      cp[CP_BW] = NAN;
      cp[CP_T] = NAN;
      A.stat[2 * c] = nu;
      A.stat[2 * c + 1] = flags;
    }
    return;
  }

  // ---- 3. bin counts (_linear_binning, kde_1d.py:6-31): runs of equal bins -> one integer LDS atomic ----
  unsigned* cnt = (unsigned*)sh;
  for (int i = tid; i < nm; i += kThreads) cnt[i] = 0u;
  __syncthreads();
  {
    const double off = x0 - 0.5 * dx;
    int cur = -1;
    unsigned run = 0;
    for (int64_t i = r0; i < r1; ++i) {
      const double v = from_key(gk[i]);
      if (!(v >= x0 && v <= xl)) continue;
      double fb = floor((v - off) / dx);
      fb = fb < 0.0 ? 0.0 : (fb > (double)(nm - 1) ? (double)(nm - 1) : fb);
      const int b = (int)fb;
      if (b != cur) {
        if (run) atomicAdd(&cnt[cur], run);
        cur = b;
        run = 0;
      }
      ++run;
    }
    if (run) atomicAdd(&cnt[cur], run);
  }
  __syncthreads();
  int64_t tot = 0;
  for (int i = tid; i < nm; i += kThreads) tot += cnt[i];
  const double total = (double)wg_sum_i(tot, redi);

  // ---- 4. a = fftpack.dct(counts / sum(counts), type=2) through an h-point complex FFT (Makhoul) ----
  // v[j] = x[2j], v[n-1-j] = x[2j+1]; z[m] = v[2m] + i v[2m+1], stored bit-reversed (via ga: the LDS
  // counts and the complex buffer overlap)
  const int lg = 31 - __clz(h);
  for (int m = tid; m < h; m += kThreads) {
    const int e = 2 * m, o = 2 * m + 1;
    const int ie = e < h ? 2 * e : 2 * nm - 1 - 2 * e;
    const int io = o < h ? 2 * o : 2 * nm - 1 - 2 * o;
    const unsigned r = bitrev((unsigned)m, lg);
    ga[2 * r] = (double)cnt[ie] / total;
    ga[2 * r + 1] = (double)cnt[io] / total;
  }
  __syncthreads();
  double2* z = (double2*)sh;
  for (int m = tid; m < h; m += kThreads) z[m] = make_double2(ga[2 * m], ga[2 * m + 1]);
  __syncthreads();
  fft_lds(z, h, -1.0);
  // V[k] = E + e^{-2 pi i k/n} O, E = (Z[k] + conj Z[h-k]) / 2, O = -i (Z[k] - conj Z[h-k]) / 2, k = 0 .. h;
  // P = e^{-i pi k / 2n} V[k]: y[k] = 2 Re P, y[n-k] = -2 Im P
  for (int k = tid; k <= h; k += kThreads) {
    const double2 zk = z[k % h], zc = z[(h - k) % h];
    const double er = 0.5 * (zk.x + zc.x), ei = 0.5 * (zk.y - zc.y);
    const double dr = zk.x - zc.x, di = zk.y + zc.y;  // Z[k] - conj Z[h-k]
    const double orr = 0.5 * di, oi = -0.5 * dr;      // -i/2 (dr + i di)
    double sn, cs;
    sincospi(-2.0 * (double)k / (double)nm, &sn, &cs);
    const double vr = er + (orr * cs - oi * sn), vi = ei + (orr * sn + oi * cs);
    sincospi(-(double)k / (double)(2 * nm), &sn, &cs);
    const double pr = vr * cs - vi * sn, pi = vr * sn + vi * cs;
    ga[k] = 2.0 * pr;
    if (k > 0 && k < h) ga[nm - k] = -2.0 * pi;
  }
  __syncthreads();
  if (tid == 0) {
    A.stat[2 * c] = nu;
    A.stat[2 * c + 1] = 0;
  }
}

// t* and the bandwidth from the DCT coefficients kde_column_kernel left in ga.  The sort / DCT, the bandwidth search
// and the density are three launches so that each kernel's live scalars fit the SGPR file (one kernel spilled)
__global__ __launch_bounds__(kThreads) void kde_bandwidth_kernel(KdeArgs A) {
  extern __shared__ __attribute__((aligned(16))) double sh[];
  __shared__ double red[kWaves];
  const int c = blockIdx.x;
  const int tid = threadIdx.x;
  if (A.stat[2 * c + 1] != 0) return;  // non-finite or degenerate: kde_column_kernel wrote the NaN outputs
  const int side = c >= A.src.ncol0;
  const int64_t n = A.src.n[side];
  const uint64_t* gk = A.keys + (int64_t)c * A.pmax;
  const int nm = A.nm;
  double* cp = A.colp + (int64_t)c * CP_N;
  const double* ga = A.ga + (int64_t)c * nm;
  const int64_t nu = A.stat[2 * c];
  const double delta = cp[CP_DELTA];
  const int64_t per = (n + kThreads - 1) / kThreads;
  const int64_t r0 = (int64_t)tid * per, r1 = r0 + per < n ? r0 + per : n;
  int64_t flags = 0;
  double* a = sh;
  for (int k = tid; k < nm; k += kThreads) a[k] = ga[k];
  // the constants through LDS: read inside the search loop, not held in scalar registers across it
  __shared__ FpConsts fcs;
  if (tid == 0) fcs = A.fc;
  __syncthreads();

  // ---- 5. t_star: _root (kde_1d.py:79-108) on _fixed_point; Scott's rule when it fails ----
  const double Nu = (double)nu;
  double Ncl = Nu < 1050.0 ? Nu : 1050.0;
  Ncl = Ncl > 50.0 ? Ncl : 50.0;
  double tol = 1e-12 + 0.01 * (Ncl - 50.0) / 1000.0;
  double tstar = 0.0;
  bool found = false;
  for (;;) {
    double x = 0.0;
    bool conv = false;
    const int err = brentq_fp(0.0, tol, Nu, a, nm, red, &fcs, &x, &conv);
    bool converged;
    if (err) {
      x = 0.0;
      tol *= 2.0;
      converged = false;
    } else {
      converged = conv;
    }
    if (x <= 0.0) converged = false;
    if (tol >= 1.0) break;
    if (converged) {
      tstar = x;
      found = true;
      break;
    }
    if (!err) {
      // the reference repeats the same brentq call forever here (no sign failure, not converged)
      flags |= KF_ROOT_STUCK;
      break;
    }
  }
  double bw;
  if (found) {
    bw = sqrt(tstar) * delta;
  } else {
    // _scott_rule_1d (kde_1d.py:111-130): min(std(ddof=1), IQR / 1.349) * len^-1/5 over all samples
    flags |= KF_SCOTT;
    double s = 0.0;
    for (int64_t i = r0; i < r1; ++i) s += from_key(gk[i]);
    const double mean = wg_sum(s, red) / (double)n;
    double q = 0.0;
    for (int64_t i = r0; i < r1; ++i) {
      const double d = from_key(gk[i]) - mean;
      q += d * d;
    }
    const double sd = sqrt(wg_sum(q, red) / (double)(n - 1));
    double qv[2];
    for (int w = 0; w < 2; ++w) {
      // np.quantile(method="linear"): virtual index n q + (1 - q) - 1, _lerp of its neighbours
      const double qq = w ? 0.75 : 0.25;
      const double vi = (double)n * qq + (1.0 + qq * -1.0) - 1.0;
      const double pf = floor(vi);
      const double g = vi - pf;
      int64_t ip = (int64_t)pf, inx = ip + 1;
      if (ip < 0) ip = 0;
      if (ip > n - 1) ip = n - 1;
      if (inx > n - 1) inx = n - 1;
      const double va = from_key(gk[ip]), vb = from_key(gk[inx]);
      const double d = vb - va;
      qv[w] = g >= 0.5 ? vb - d * (1.0 - g) : va + d * g;
    }
    const double siqr = (qv[1] - qv[0]) / 1.3489795003921634;
    const double sg = sd < siqr ? sd : siqr;  // min(sigma, sigma_iqr)
    bw = sg * pow((double)n, -1.0 / 5.0);
    tstar = (bw / delta) * (bw / delta);
  }
  if (tid == 0) {
    cp[CP_BW] = bw;
    cp[CP_T] = tstar;
    A.stat[2 * c] = nu;
    A.stat[2 * c + 1] = flags;
  }
}

// the density from the coefficients in ga and t* in colp (a launch of its own, like kde_bandwidth_kernel)
__global__ __launch_bounds__(kThreads) void kde_density_kernel(KdeArgs A) {
  extern __shared__ __attribute__((aligned(16))) double sh[];
  __shared__ double red[kWaves];
  const int c = blockIdx.x;
  const int tid = threadIdx.x;
  if (A.stat[2 * c + 1] & (KF_NONFINITE | KF_DEGENERATE)) return;
  const int nm = A.nm, h = nm / 2;
  const int lg = 31 - __clz(h);
  const double* cp = A.colp + (int64_t)c * CP_N;
  double* dens = A.dens + (int64_t)c * nm;
  double* ga = A.ga + (int64_t)c * nm;
  const double delta = cp[CP_DELTA], dx = cp[CP_DX], tstar = cp[CP_T];
  double2* z = (double2*)sh;
  double* a = sh;
  for (int k = tid; k < nm; k += kThreads) a[k] = ga[k];
  __syncthreads();

  // ---- 6. density = fftpack.idct(a * exp(-k^2 pi^2 t / 2)) / (2 delta), negatives -> 0 ----
  // W[k] = e^{i pi k / 2n} (at[k] - i at[n-k]) / 2 (at[n] = 0); Z[k] = (W[k] + W[k+h]) + i (W[k] - W[k+h])
  // e^{2 pi i k / n}, z = unscaled inverse FFT; idct[2m] = 2 Re(z[m/2]) / Im, idct[2m+1] from v'[n-1-m]
  const double pi2 = M_PI * M_PI;
  for (int k = tid; k < h; k += kThreads) {
    double wr[2], wi[2];
    for (int s2 = 0; s2 < 2; ++s2) {
      const int kk = k + s2 * h;
      const int kr = nm - kk;
      const double dk = (double)kk, dr = (double)kr;
      const double ak = a[kk] * exp(-(dk * dk) * pi2 * tstar / 2.0);
      const double ar = kr < nm ? a[kr] * exp(-(dr * dr) * pi2 * tstar / 2.0) : 0.0;
      double sn, cs;
      sincospi(dk / (double)(2 * nm), &sn, &cs);
      // (cs + i sn)(ak - i ar) / 2
      wr[s2] = 0.5 * (cs * ak + sn * ar);
      wi[s2] = 0.5 * (sn * ak - cs * ar);
    }
    const double er = wr[0] + wr[1], ei = wi[0] + wi[1];
    const double dr0 = wr[0] - wr[1], di0 = wi[0] - wi[1];
    double sn, cs;
    sincospi(2.0 * (double)k / (double)nm, &sn, &cs);
    const double orr = dr0 * cs - di0 * sn, oi = dr0 * sn + di0 * cs;
    const unsigned r = bitrev((unsigned)k, lg);
    ga[2 * r] = er - oi;      // E + i O
    ga[2 * r + 1] = ei + orr;
  }
  __syncthreads();
  for (int m = tid; m < h; m += kThreads) z[m] = make_double2(ga[2 * m], ga[2 * m + 1]);
  __syncthreads();
  fft_lds(z, h, 1.0);
  const double twod = 2.0 * delta;
  const bool spline = A.msp != nullptr;
  double* y = sh + nm;  // spline: the density in LDS after the FFT buffer (nm <= 2^13)
  double trap = 0.0;
  for (int j = tid; j < nm; j += kThreads) {
    const int mm = (j & 1) ? nm - 1 - (j >> 1) : (j >> 1);  // index into v'
    const double2 zz = z[mm >> 1];
    const double vp = (mm & 1) ? zz.y : zz.x;
    double d = 2.0 * vp / twod;
    if (d < 0.0) d = 0.0;
    if (spline) y[j] = d;
    else dens[j] = d;
  }
  if (!spline) return;
  __syncthreads();

  // ---- 7. mtv: yy / (trapezoid(yy) dx), then the not-a-knot cubic spline (interp1d kind="cubic") ----
  for (int j = tid; j < nm - 1; j += kThreads) trap += (y[j + 1] + y[j]) / 2.0;
  const double norm = wg_sum(trap, red) * dx;
  for (int j = tid; j < nm; j += kThreads) {
    const double v = y[j] / norm;
    y[j] = v;
    dens[j] = v;
  }
  __syncthreads();
  // with m_i = h^2 M_i / 6: m_{i-1} + 4 m_i + m_{i+1} = y_{i-1} - 2 y_i + y_{i+1} (i = 1 .. n-2), and
  // not-a-knot m_0 = 2 m_1 - m_2, m_{n-1} = 2 m_{n-2} - m_{n-3}, which make rows 1 and n-2 read 6 m = r.
  // The rows 2 .. n-3 (unknowns j = i - 2, mu = n - 4 of them) are a Dirichlet [1 4 1] system: Thomas,
  // each thread's chunk started kOverlap rows early from zero (the error decays by c' ~ 0.268 a row).
  double* msp = A.msp + (int64_t)c * nm;
  double* dp = sh;  // d'_j (the FFT buffer is free again)
  const int mu = nm - 4;
  const double m1 = (y[0] - 2.0 * y[1] + y[2]) / 6.0;
  const double mn2 = (y[nm - 3] - 2.0 * y[nm - 2] + y[nm - 1]) / 6.0;
  const int L = (mu + kThreads - 1) / kThreads;
  const int j0 = tid * L, j1 = j0 + L < mu ? j0 + L : mu;
  if (j0 < j1) {
    const int s0 = j0 - kOverlap > 0 ? j0 - kOverlap : 0;
    double dprev = 0.0;
    for (int j = s0; j < j1; ++j) {
      const int i = j + 2;
      double b = y[i - 1] - 2.0 * y[i] + y[i + 1];
      if (j == 0) b -= m1;
      if (j == mu - 1) b -= mn2;
      const double cj = thomas_c(j);
      const double dj = (b - dprev) * cj;
      if (j >= j0) dp[j] = dj;
      dprev = dj;
    }
  }
  __syncthreads();
  if (j0 < j1) {
    const int e0 = j1 - 1 + kOverlap < mu - 1 ? j1 - 1 + kOverlap : mu - 1;
    double mnext = 0.0;
    for (int j = e0; j >= j0; --j) {
      const double mj = j == mu - 1 ? dp[j] : dp[j] - thomas_c(j) * mnext;
      if (j < j1) msp[j + 2] = mj;
      mnext = mj;
    }
  }
  __syncthreads();
  if (tid == 0) {
    msp[1] = m1;
    msp[nm - 2] = mn2;
    msp[0] = 2.0 * m1 - msp[2];
    msp[nm - 1] = 2.0 * mn2 - msp[nm - 3];
  }
}

// the spline of column c at x; 0 outside [x0, xl] (interp1d fill_value=0, bounds_error=False)
__device__ inline double spline_at(const double* cp, const double* y, const double* m, int nm, double x) {
  const double x0 = cp[CP_X0], xl = cp[CP_XL], step = cp[CP_STEP], lower = cp[CP_LOWER];
  if (!(x >= x0 && x <= xl)) return 0.0;
  double fi = floor((x - x0) / step);
  fi = fi >= 0.0 ? (fi > (double)(nm - 2) ? (double)(nm - 2) : fi) : 0.0;
  const int i = (int)fi;
  const double xi = (double)i * step + lower;
  const double xi1 = i + 1 == nm - 1 ? xl : (double)(i + 1) * step + lower;
  const double t = (x - xi) / (xi1 - xi), u = 1.0 - t;
  return u * y[i] + t * y[i + 1] + (u * u * u - u) * m[i] + (t * t * t - t) * m[i + 1];
}

__device__ inline void sort4(double* b) {
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 3 - i; ++j)
      if (b[j + 1] < b[j]) {
        const double t = b[j];
        b[j] = b[j + 1];
        b[j + 1] = t;
      }
}

// grid (kIntBlocks, 3, D): segment j of dimension d; columns d and D + d
__global__ __launch_bounds__(kIntThreads) void mtv_integral_kernel(const double* __restrict__ colp,
                                                                   const double* __restrict__ dens,
                                                                   const double* __restrict__ msp, int nm, int D,
                                                                   double* __restrict__ part) {
  __shared__ double red[kIntThreads / 64];
  const int d = blockIdx.z, seg = blockIdx.y;
  const double* c1 = colp + (int64_t)d * CP_N;
  const double* c2 = colp + (int64_t)(D + d) * CP_N;
  const double* y1 = dens + (int64_t)d * nm;
  const double* y2 = dens + (int64_t)(D + d) * nm;
  const double* m1 = msp + (int64_t)d * nm;
  const double* m2 = msp + (int64_t)(D + d) * nm;
  double bb[4] = {c1[CP_X0], c1[CP_XL], c2[CP_X0], c2[CP_XL]};
  sort4(bb);
  const double start = bb[seg], stop = bb[seg + 1];
  const double div = (double)(kSegPts - 1);
  const double delta = stop - start;
  const double step = delta / div;
  double s = 0.0;
  for (int q = 0; q < kIntPerThread; ++q) {
    const int i = (blockIdx.x * kIntPerThread + q) * kIntThreads + threadIdx.x;
    if (i >= kSegPts) break;
    const double x = i == kSegPts - 1 ? stop : (step == 0.0 ? ((double)i / div) * delta : (double)i * step) + start;
    const double f = fabs(spline_at(c1, y1, m1, nm, x) - spline_at(c2, y2, m2, nm, x));
    s += (i == 0 || i == kSegPts - 1) ? 0.5 * f : f;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < kIntThreads / 64; ++w) t += red[w];
    part[((int64_t)d * 3 + seg) * kIntBlocks + blockIdx.x] = t;
  }
}

size_t lds_bytes(int nm, bool spline) {
  size_t b = (size_t)kChunk * sizeof(uint64_t);
  const size_t f = (size_t)nm * sizeof(double) * (spline ? 2 : 1);
  return f > b ? f : b;
}

// device layout of one kde / mtv call: the first pieces of the call's scratch list (offsets in doubles)
struct KdePlan {
  int ncol = 0, nm = 0;
  int64_t pmax = 0;
  size_t o_keys = 0, o_ga = 0, o_dens = 0, o_xm = 0, o_msp = 0, o_colp = 0, o_stat = 0, o_nf = 0, o_bnd = 0,
         o_part = 0;
  void plan(Scratch& sc, int ncol_, int nm_, int64_t nmax, bool want_xmesh, bool want_spline, int D) {
    ncol = ncol_;
    nm = nm_;
    pmax = next_pow2(nmax > kChunk ? nmax : kChunk);
    o_keys = sc.add((size_t)ncol * pmax).off;
    o_ga = sc.add((size_t)ncol * nm).off;
    o_dens = sc.add((size_t)ncol * nm).off;
    o_xm = sc.add(want_xmesh ? (size_t)ncol * nm : 0).off;
    o_msp = sc.add(want_spline ? (size_t)ncol * nm : 0).off;
    o_colp = sc.add((size_t)ncol * CP_N).off;
    o_stat = sc.add<int64_t>((size_t)ncol * 2).off;
    o_nf = sc.add<unsigned>((size_t)ncol).off;
    o_bnd = sc.add(2 * (size_t)ncol).off;
    o_part = sc.add(want_spline ? (size_t)D * 3 * kIntBlocks : 0).off;
  }
};

FpConsts fixed_point_consts() {
  FpConsts f = {};
  for (int s = 2; s <= 7; ++s) {
    double odd = 1.0;
    for (int q = 1; q <= 2 * s - 1; q += 2) odd *= (double)q;
    const double K0 = odd / std::sqrt(2.0 * M_PI);
    const double cst = (1.0 + std::pow(0.5, (double)s + 0.5)) / 3.0;
    f.two_pi2s[s] = 2.0 * std::pow(M_PI, 2.0 * (double)s);
    f.two_cst_k0[s] = 2.0 * cst * K0;
    f.expo[s] = 2.0 / (3.0 + 2.0 * (double)s);
  }
  f.sqrt_pi = std::sqrt(M_PI);
  return f;
}

int launch_kde(vbmc_ctx* ctx, const KdePlan& pl, const KdeSrc& src, double* base, int mode, bool has_lb, bool has_ub,
               bool want_xmesh, bool want_spline) {
  static const FpConsts fc = fixed_point_consts();
  KdeArgs A;
  A.src = src;
  A.fc = fc;
  A.keys = (uint64_t*)(base + pl.o_keys);
  A.pmax = pl.pmax;
  A.nonfinite = (unsigned*)(base + pl.o_nf);
  A.nm = pl.nm;
  A.mode = mode;
  A.lb = has_lb ? base + pl.o_bnd : nullptr;
  A.ub = has_ub ? base + pl.o_bnd + pl.ncol : nullptr;
  A.ga = base + pl.o_ga;
  A.dens = base + pl.o_dens;
  A.xmesh = want_xmesh ? base + pl.o_xm : nullptr;
  A.msp = want_spline ? base + pl.o_msp : nullptr;
  A.colp = base + pl.o_colp;
  A.stat = (int64_t*)(base + pl.o_stat);
  HIP_TRY(ctx, hipMemsetAsync(A.nonfinite, 0, sizeof(unsigned) * pl.ncol, ctx->stream));
  hipLaunchKernelGGL(kde_sort_chunks_kernel, dim3((unsigned)(pl.pmax / kChunk), (unsigned)pl.ncol), dim3(kThreads), 0,
                     ctx->stream, src, A.keys, pl.pmax, A.nonfinite);
  HIP_TRY(ctx, hipGetLastError());
  const size_t lds = lds_bytes(pl.nm, want_spline);
  HIP_TRY(ctx, hipFuncSetAttribute((const void*)kde_column_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kde_column_kernel, dim3((unsigned)pl.ncol), dim3(kThreads), lds, ctx->stream, A);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipFuncSetAttribute((const void*)kde_bandwidth_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kde_bandwidth_kernel, dim3((unsigned)pl.ncol), dim3(kThreads), lds, ctx->stream, A);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipFuncSetAttribute((const void*)kde_density_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kde_density_kernel, dim3((unsigned)pl.ncol), dim3(kThreads), lds, ctx->stream, A);
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

int check_flags(vbmc_ctx* ctx, const char* who, const int64_t* stat, int ncol) {
  for (int c = 0; c < ncol; ++c) {
    if (stat[2 * c + 1] & KF_NONFINITE)
      return vbmc_fail(ctx, VBMC_E_NONFINITE, "%s: column %d holds a non-finite sample", who, c);
  }
  return 0;
}

}  // namespace

extern "C" int vbmc_kde_1d(vbmc_ctx* ctx, int ncol, int64_t n, const double* x_colxn, int n_mesh,
                           const double* lb_col, const double* ub_col, double* density_colxm, double* xmesh_colxm,
                           double* bandwidth_col, int64_t* info_colx2) {
  if (!ctx || ncol < 1 || n < 1 || !x_colxn || !density_colxm || !bandwidth_col || !info_colx2) return VBMC_E_ARG;
  if (n_mesh < 2 || (n_mesh & (n_mesh - 1)))
    return vbmc_fail(ctx, VBMC_E_ARG, "kde_1d: n_mesh=%d must be a power of two >= 2", n_mesh);
  if (n_mesh > kMaxMesh) return vbmc_fail(ctx, VBMC_E_UNSUP, "kde_1d: n_mesh=%d > 2^14", n_mesh);
  if (n > ((int64_t)1 << 30)) return vbmc_fail(ctx, VBMC_E_UNSUP, "kde_1d: %lld samples > 2^30", (long long)n);
  NEED_DEVICE(ctx);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  Scratch sc;
  KdePlan pl;
  pl.plan(sc, ncol, n_mesh, n, true, false, 0);
  const size_t nx = (size_t)ncol * n;
  const auto p_x = sc.add(nx);
  int rc = reserve(ctx, sc);
  if (rc) return rc;
  double *base = sc.base, *d_x = sc.ptr(p_x);
  HIP_TRY(ctx, hipMemcpyAsync(d_x, x_colxn, sizeof(double) * nx, hipMemcpyHostToDevice, ctx->stream));
  if (lb_col) HIP_TRY(ctx, hipMemcpyAsync(base + pl.o_bnd, lb_col, sizeof(double) * ncol, hipMemcpyHostToDevice, ctx->stream));
  if (ub_col)
    HIP_TRY(ctx, hipMemcpyAsync(base + pl.o_bnd + ncol, ub_col, sizeof(double) * ncol, hipMemcpyHostToDevice, ctx->stream));
  KdeSrc src = {};
  src.x[0] = src.x[1] = d_x;
  src.n[0] = src.n[1] = n;
  src.rs[0] = src.rs[1] = 1;
  src.cs[0] = src.cs[1] = n;
  src.ncol0 = ncol;
  rc = launch_kde(ctx, pl, src, base, BND_KDE, lb_col != nullptr, ub_col != nullptr, true, false);
  if (rc) return rc;
  std::vector<double> colp((size_t)ncol * CP_N);
  HIP_TRY(ctx, hipMemcpyAsync(density_colxm, base + pl.o_dens, sizeof(double) * ncol * n_mesh, hipMemcpyDeviceToHost,
                              ctx->stream));
  if (xmesh_colxm)
    HIP_TRY(ctx, hipMemcpyAsync(xmesh_colxm, base + pl.o_xm, sizeof(double) * ncol * n_mesh, hipMemcpyDeviceToHost,
                                ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(colp.data(), base + pl.o_colp, sizeof(double) * colp.size(), hipMemcpyDeviceToHost,
                              ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(info_colx2, base + pl.o_stat, sizeof(int64_t) * 2 * ncol, hipMemcpyDeviceToHost,
                              ctx->stream));
  HIP_TRY(ctx, stream_wait(ctx));
  for (int c = 0; c < ncol; ++c) bandwidth_col[c] = colp[(size_t)c * CP_N + CP_BW];
  return check_flags(ctx, "kde_1d", info_colx2, ncol);
}

extern "C" int vbmc_mtv(vbmc_ctx* ctx, int D, const vbmc_mtv_side* s1, const vbmc_mtv_side* s2, int K2,
                        const double* mu2_KxD, const double* sigma2_K, const double* lambd2_D, const double* w2_K,
                        double* mtv_D, int64_t* info_2Dx2) {
  if (!ctx || D < 1 || !s1 || !s2 || !mtv_D) return VBMC_E_ARG;
  const vbmc_mtv_side* sd[2] = {s1, s2};
  bool need_mix2 = false;
  for (int s = 0; s < 2; ++s) {
    const vbmc_mtv_side& q = *sd[s];
    if (q.n < 1 || !q.lb_D || !q.ub_D) return vbmc_fail(ctx, VBMC_E_ARG, "mtv: side %d: n=%lld, bounds required", s + 1, (long long)q.n);
    if (q.n > ((int64_t)1 << 30)) return vbmc_fail(ctx, VBMC_E_UNSUP, "mtv: %lld samples > 2^30", (long long)q.n);
    if (q.source == VBMC_MTV_HOST && !q.x_NxD) return vbmc_fail(ctx, VBMC_E_ARG, "mtv: side %d: no samples", s + 1);
    if (q.source < VBMC_MTV_HOST || q.source > VBMC_MTV_MIX2) return vbmc_fail(ctx, VBMC_E_ARG, "mtv: bad source");
    if (q.source != VBMC_MTV_HOST && (!ctx->mix_set || ctx->D != D))
      return vbmc_fail(ctx, VBMC_E_ARG, "mtv: mixture not set or D differs");
    need_mix2 |= q.source == VBMC_MTV_MIX2;
  }
  XfView t1 = {}, t2 = {};
  for (int s = 0; s < 2; ++s) {
    if (sd[s]->source == VBMC_MTV_MIX1 && !xf_view_slot(ctx, 0, D, t1)) return vbmc_fail(ctx, VBMC_E_ARG, "mtv: transformer slot 0 not set for D=%d", D);
    if (sd[s]->source == VBMC_MTV_MIX2 && !xf_view_slot(ctx, 1, D, t2)) return vbmc_fail(ctx, VBMC_E_ARG, "mtv: transformer slot 1 not set for D=%d", D);
  }
  MixLayout ml2;
  std::vector<double> pack2;
  if (need_mix2) {
    if (K2 < 1 || !mu2_KxD || !sigma2_K || !lambd2_D || !w2_K) return vbmc_fail(ctx, VBMC_E_ARG, "mtv: second mixture missing");
    const int rc2 = make_mixture2(ctx, "mtv", VBMC_E_ARG, D, K2, mu2_KxD, sigma2_K, lambd2_D, w2_K, ml2, pack2);
    if (rc2) return rc2;
  }
  NEED_DEVICE(ctx);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int ncol = 2 * D, nm = kMtvMesh;
  Scratch sc;
  KdePlan pl;
  pl.plan(sc, ncol, nm, s1->n > s2->n ? s1->n : s2->n, false, true, D);
  const int Kmax = ctx->K > K2 ? ctx->K : K2;
  const Piece<> p_x[2] = {sc.add((size_t)s1->n * D), sc.add((size_t)s2->n * D)};
  const auto p_pack = sc.add(pack2.size()), p_sel = sc.add(selector_elems(Kmax > 0 ? Kmax : 1));
  int rc = reserve(ctx, sc);
  if (rc) return rc;
  double* base = sc.base;
  if (need_mix2)
    HIP_TRY(ctx, hipMemcpyAsync(sc.ptr(p_pack), pack2.data(), sizeof(double) * pack2.size(), hipMemcpyHostToDevice, ctx->stream));
  std::vector<double> bnd(2 * (size_t)ncol);
  for (int s = 0; s < 2; ++s)
    for (int d = 0; d < D; ++d) {
      bnd[(size_t)s * D + d] = sd[s]->lb_D[d];
      bnd[(size_t)ncol + s * D + d] = sd[s]->ub_D[d];
    }
  HIP_TRY(ctx, hipMemcpyAsync(base + pl.o_bnd, bnd.data(), sizeof(double) * bnd.size(), hipMemcpyHostToDevice, ctx->stream));
  KdeSrc src = {};
  for (int s = 0; s < 2; ++s) {
    const vbmc_mtv_side& q = *sd[s];
    double* d_x = sc.ptr(p_x[s]);
    if (q.source == VBMC_MTV_HOST) {
      HIP_TRY(ctx, hipMemcpyAsync(d_x, q.x_NxD, sizeof(double) * q.n * D, hipMemcpyHostToDevice, ctx->stream));
    } else {
      // sample(N, True, True, rng="philox", seed): balanced draws of the mixture, then its transformer's inverse
      const bool m2 = q.source == VBMC_MTV_MIX2;
      rc = launch_sample(ctx, m2 ? sc.ptr(p_pack) : ctx->d_mix, m2 ? ml2 : ctx->ml, m2 ? w2_K : ctx->w.data(), q.n,
                         q.seed, 1, sc.ptr(p_sel), d_x, nullptr, INFINITY);
      if (rc) return rc;
      rc = launch_xf_apply(ctx, m2 ? t2 : t1, q.n, 1, d_x, d_x);
      if (rc) return rc;
    }
    src.x[s] = d_x;
    src.n[s] = q.n;
    src.rs[s] = D;
    src.cs[s] = 1;
  }
  src.ncol0 = D;
  rc = launch_kde(ctx, pl, src, base, BND_MTV, true, true, false, true);
  if (rc) return rc;
  double* d_part = base + pl.o_part;
  hipLaunchKernelGGL(mtv_integral_kernel, dim3(kIntBlocks, 3, D), dim3(kIntThreads), 0, ctx->stream,
                     base + pl.o_colp, base + pl.o_dens, base + pl.o_msp, nm, D, d_part);
  HIP_TRY(ctx, hipGetLastError());
  std::vector<double> part((size_t)D * 3 * kIntBlocks), colp((size_t)ncol * CP_N);
  std::vector<int64_t> stat((size_t)ncol * 2);
  HIP_TRY(ctx, hipMemcpyAsync(part.data(), d_part, sizeof(double) * part.size(), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(colp.data(), base + pl.o_colp, sizeof(double) * colp.size(), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(stat.data(), base + pl.o_stat, sizeof(int64_t) * stat.size(), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, stream_wait(ctx));
  if (info_2Dx2) std::memcpy(info_2Dx2, stat.data(), sizeof(int64_t) * stat.size());
  rc = check_flags(ctx, "mtv", stat.data(), ncol);
  if (rc) return rc;
  for (int d = 0; d < D; ++d) {
    // bb = sort(x1mesh[0], x1mesh[-1], x2mesh[0], x2mesh[-1]); mtv += 0.5 trapezoid(f(xx)) (xx[1] - xx[0]) (:1019-1029)
    double bb[4] = {colp[(size_t)d * CP_N + CP_X0], colp[(size_t)d * CP_N + CP_XL], colp[(size_t)(D + d) * CP_N + CP_X0],
                    colp[(size_t)(D + d) * CP_N + CP_XL]};
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 3 - i; ++j)
        if (bb[j + 1] < bb[j]) std::swap(bb[j], bb[j + 1]);
    double acc = 0.0;
    for (int j = 0; j < 3; ++j) {
      double tr = 0.0;
      for (int b = 0; b < kIntBlocks; ++b) tr += part[((size_t)d * 3 + j) * kIntBlocks + b];
      const double delta = bb[j + 1] - bb[j], div = (double)(kSegPts - 1);
      const double step = delta / div;
      const double dxj = step == 0.0 ? ((1.0 / div) * delta + bb[j]) - bb[j] : (1.0 * step + bb[j]) - bb[j];
      acc = acc + 0.5 * tr * dxj;
    }
    mtv_D[d] = acc;
  }
  return VBMC_OK;
}

// kde.h: the plan and the stages above for a caller outside this file (vbmc_marginals)
KdeCols kde_cols_plan(Scratch& sc, int ncol, int nm, int64_t n) {
  KdePlan pl;
  pl.plan(sc, ncol, nm, n, true, false, 0);
  KdeCols kc;
  kc.ncol = ncol;
  kc.nm = nm;
  kc.pmax = pl.pmax;
  kc.o_keys = pl.o_keys;
  kc.o_nf = pl.o_nf;
  kc.o_bnd = pl.o_bnd;
  kc.o_dens = pl.o_dens;
  kc.o_xm = pl.o_xm;
  kc.o_colp = pl.o_colp;
  kc.o_ga = pl.o_ga;
  kc.o_stat = pl.o_stat;
  kc.colp_stride = CP_N;
  kc.colp_bw = CP_BW;
  return kc;
}

int kde_cols_launch(vbmc_ctx* ctx, const KdeCols& kc, const double* d_x, int64_t n, int64_t rs, int64_t cs, double* base) {
  KdePlan pl;
  pl.ncol = kc.ncol;
  pl.nm = kc.nm;
  pl.pmax = kc.pmax;
  pl.o_keys = kc.o_keys;
  pl.o_ga = kc.o_ga;
  pl.o_dens = kc.o_dens;
  pl.o_xm = kc.o_xm;
  pl.o_colp = kc.o_colp;
  pl.o_stat = kc.o_stat;
  pl.o_nf = kc.o_nf;
  pl.o_bnd = kc.o_bnd;
  KdeSrc src = {};
  src.x[0] = src.x[1] = d_x;
  src.n[0] = src.n[1] = n;
  src.rs[0] = src.rs[1] = rs;
  src.cs[0] = src.cs[1] = cs;
  src.ncol0 = kc.ncol;
  return launch_kde(ctx, pl, src, base, BND_KDE, true, true, true, false);
}
