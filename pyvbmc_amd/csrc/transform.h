// The reference's ParameterTransformer on the device (parameter_transformer/parameter_transformer.py):
// original space x <-> transformed space u, and log |det J| of u -> x.
//
//   forward  x -> u : per dimension  unbounded (x - mu) / delta,  bounded center(g(to_unit(x)));
//                     then u @ R_mat, then / scale                                    (:135-181)
//   inverse  u -> x : * scale, then @ R_mat^T (the transpose, as the reference: R is not assumed
//                     orthogonal), then per dimension  delta x + mu  or  from_unit(g^-1(uncenter(x)))  (:183-227)
//   log|J|   (u)    : undo scale and rotation, per-dimension terms (+ log scale_d), summed      (:229-269)
//
// with g = logit (type 3), probit (12: -sqrt(2) erfcinv(2 z)), student4 (13), and the boundary handling of
// the reference's helpers (:476-545): the nextafter nudges of _to_unit_interval / _from_unit_interval,
// _logit's +-inf at z = 0 / 1, _inverse_logit's overflow mask, _student4's aa == 0 case.  Every
// expression keeps NumPy's order of operations; NaN propagates where NumPy's does (np.maximum /
// np.minimum, np.sign).  The per-dimension sum of log|J| is NumPy's pairwise sum of a row (D < 8:
// left to right; D >= 8: eight running sums), so only the rotation's dot products (BLAS there) and
// the libm functions differ from the reference, by rounding.
//
// One thread = one point: the D coordinates live in a register array of the padded width DP.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

enum { XF_UNBOUNDED = 0, XF_LOGIT = 3, XF_PROBIT = 12, XF_STUDENT4 = 13 };

// Device descriptor: one allocation of doubles, D each of the per-dimension rows below, then R (D x D,
// row-major) when present.  Host-side values that the reference recomputes on every call (log(ub - lb),
// log(delta), log(scale), the nudged bounds) are computed once by the host's libm at upload.
struct XfLayout {
  enum { TYPE, LB, UB, MU, DELTA, LB_UP, UB_DN, LOG_SPAN, LOG_DELTA, SCALE, LOG_SCALE, NROWS };
  static __host__ __device__ inline int row(int r, int D) { return r * D; }
  static __host__ __device__ inline int o_R(int D) { return NROWS * D; }
  static __host__ __device__ inline int total(int D, bool has_R) { return NROWS * D + (has_R ? D * D : 0); }
};

struct XfView {
  const double* p = nullptr;
  int D = 0;
  int has_R = 0, has_scale = 0;
};

namespace xf {

constexpr double kLogDblMax = 0x1.62e42fefa39efp+9;       // np.log(np.finfo(np.float64).max)
constexpr double kHalfLog2Pi = -0x1.d67f1c864beb4p-1;     // -0.5 * np.log(2 * np.pi)
constexpr double kLog3_8 = -0x1.f62f40794a7b8p-1;         // np.log(3 / 8)
constexpr double kOneDown = 0x1.fffffffffffffp-1;         // np.nextafter(1, -np.inf)
constexpr double kZeroUp = 4.9406564584124654e-324;       // np.nextafter(0, np.inf)
constexpr double kSqrt2 = 1.4142135623730951;             // np.sqrt(2)

__device__ __forceinline__ double sign(double v) {  // np.sign
  return v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : (v == 0.0 ? 0.0 : v));
}

// bounded dimension, x -> g(z)
__device__ __forceinline__ double bounded_g(int type, double x, double lb, double ub) {
  double z = (x - lb) / (ub - lb);
  if (z == 0.0 && x != lb) z = kZeroUp;
  if (z == 1.0 && x != ub) z = kOneDown;
  if (type == XF_LOGIT) {
    if (z == 0.0) return -INFINITY;
    if (z == 1.0) return INFINITY;
    return log(z / (1.0 - z));
  }
  if (type == XF_PROBIT) return -kSqrt2 * erfcinv(2.0 * z);
  const double aa = sqrt(4.0 * z * (1.0 - z));
  const double q = aa == 0.0 ? INFINITY : cos(acos(aa) / 3.0) / aa;
  return sign(z - 0.5) * (2.0 * sqrt(q - 1.0));
}

// bounded dimension, y (uncentred) -> z in the unit interval
__device__ __forceinline__ double bounded_ginv(int type, double u) {
  if (type == XF_LOGIT) return (-u > kLogDblMax) ? 0.0 : 1.0 / (1.0 + exp(-u));
  if (type == XF_PROBIT) {
    // SciPy's erfc (Cephes) returns 0 / 2 once a^2 > log(DBL_MAX) instead of a subnormal value / 2 - tiny:
    // the same here, so that the nudge of _from_unit_interval sees the reference's z
    const double a = -u / kSqrt2;
    if (a * a > kLogDblMax) return a < 0.0 ? 1.0 : 0.0;
    return 0.5 * erfc(a);
  }
  const double t2 = u * u;
  return 0.5 + (3.0 / 8.0) * (u / sqrt(1.0 + t2 / 4.0)) * (1.0 - t2 / (1.0 + t2 / 4.0) / 12.0);
}

// bounded dimension, per-dimension log|J| term of the uncentred y
__device__ __forceinline__ double bounded_lj(int type, double y) {
  if (type == XF_LOGIT) {
    const double z = -log1p(exp(-y));
    return -y + 2.0 * z;
  }
  if (type == XF_PROBIT) return kHalfLog2Pi - 0.5 * (y * y);
  return kLog3_8 - (5.0 / 2.0) * log1p(y * y / 4.0);
}

// d bounded_lj / dy and d^2 bounded_lj / dy^2 (the mode search's gradient and Hessian, mode.hip):
//   logit     lj = -y - 2 log1p(e^-y)              lj' = -tanh(y / 2)                 lj'' = -1 / (2 cosh^2(y / 2))
//   probit    lj = c - y^2 / 2                     lj' = -y                           lj'' = -1
//   student4  lj = c - 5/2 log1p(y^2 / 4)          lj' = -5/4 y / (1 + y^2 / 4)       lj'' = -5/4 (1 - y^2/4) / (1 + y^2/4)^2
__device__ __forceinline__ double bounded_lj_d1(int type, double y) {
  if (type == XF_LOGIT) return -tanh(0.5 * y);
  if (type == XF_PROBIT) return -y;
  return -1.25 * y / (1.0 + y * y / 4.0);
}

__device__ __forceinline__ double bounded_lj_d2(int type, double y) {
  if (type == XF_LOGIT) {
    const double t = tanh(0.5 * y);
    return -0.5 * (1.0 - t * t);
  }
  if (type == XF_PROBIT) return -1.0;
  const double q = 1.0 + y * y / 4.0;
  return -1.25 * (1.0 - y * y / 4.0) / (q * q);
}

// NumPy's pairwise sum of a short contiguous row (numpy/_core/src/umath/loops_utils.h.src, n <= 128)
template <int DP>
__device__ __forceinline__ double row_sum(const double (&v)[DP], int n) {
  if (n < 8) {
    double s = 0.0;
#pragma unroll
    for (int d = 0; d < DP; ++d)
      if (d < n) s += v[d];
    return s;
  }
  double r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = (j < DP) ? v[j] : 0.0;
  const int n8 = n - (n % 8);
#pragma unroll
  for (int i = 8; i < DP; i += 8)
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (i < n8 && i + j < DP) r[j] += v[i + j];
  double s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
#pragma unroll
  for (int d = 8; d < DP; ++d)
    if (d >= n8 && d < n) s += v[d];
  return s;
}

// v <- v @ M (TRANS = false) or v @ M^T (TRANS = true), M D x D row-major
template <int DP, bool TRANS>
__device__ __forceinline__ void rotate(const double* __restrict__ M, int D, double (&v)[DP]) {
  double w[DP];
#pragma unroll
  for (int j = 0; j < DP; ++j) {
    double s = 0.0;
    if (j < D)
#pragma unroll
      for (int i = 0; i < DP; ++i)
        if (i < D) s = fma(v[i], TRANS ? M[j * D + i] : M[i * D + j], s);
    w[j] = s;
  }
#pragma unroll
  for (int j = 0; j < DP; ++j) v[j] = w[j];
}

}  // namespace xf

// x -> u in place (ParameterTransformer.__call__)
template <int DP>
__device__ inline void xf_forward(const XfView& t, double (&v)[DP]) {
  const int D = t.D;
  const double* P = t.p;
#pragma unroll
  for (int d = 0; d < DP; ++d)
    if (d < D) {
      const int type = (int)P[XfLayout::row(XfLayout::TYPE, D) + d];
      const double mu = P[XfLayout::row(XfLayout::MU, D) + d], dl = P[XfLayout::row(XfLayout::DELTA, D) + d];
      if (type == XF_UNBOUNDED) {
        v[d] = (v[d] - mu) / dl;
      } else {
        const double g = xf::bounded_g(type, v[d], P[XfLayout::row(XfLayout::LB, D) + d],
                                       P[XfLayout::row(XfLayout::UB, D) + d]);
        v[d] = (g - mu) / dl;
      }
    }
  if (t.has_R) xf::rotate<DP, false>(P + XfLayout::o_R(D), D, v);
  if (t.has_scale)
#pragma unroll
    for (int d = 0; d < DP; ++d)
      if (d < D) v[d] = v[d] / P[XfLayout::row(XfLayout::SCALE, D) + d];
}

// scale and rotation undone (the first two steps of inverse and log|J|)
template <int DP>
__device__ __forceinline__ void xf_unrotate(const XfView& t, double (&v)[DP]) {
  const int D = t.D;
  if (t.has_scale)
#pragma unroll
    for (int d = 0; d < DP; ++d)
      if (d < D) v[d] = v[d] * t.p[XfLayout::row(XfLayout::SCALE, D) + d];
  if (t.has_R) xf::rotate<DP, true>(t.p + XfLayout::o_R(D), D, v);
}

// u -> x in place (ParameterTransformer.inverse)
template <int DP>
__device__ inline void xf_inverse(const XfView& t, double (&v)[DP]) {
  const int D = t.D;
  const double* P = t.p;
  xf_unrotate<DP>(t, v);
#pragma unroll
  for (int d = 0; d < DP; ++d)
    if (d < D) {
      const int type = (int)P[XfLayout::row(XfLayout::TYPE, D) + d];
      const double y = v[d] * P[XfLayout::row(XfLayout::DELTA, D) + d] + P[XfLayout::row(XfLayout::MU, D) + d];
      if (type == XF_UNBOUNDED) {
        v[d] = y;
      } else {
        const double lb = P[XfLayout::row(XfLayout::LB, D) + d], ub = P[XfLayout::row(XfLayout::UB, D) + d];
        double r = xf::bounded_ginv(type, y) * (ub - lb) + lb;
        const double lo = P[XfLayout::row(XfLayout::LB_UP, D) + d], hi = P[XfLayout::row(XfLayout::UB_DN, D) + d];
        r = (r < lo) ? lo : r;  // np.maximum / np.minimum: NaN stays NaN
        r = (r > hi) ? hi : r;
        v[d] = r;
      }
    }
}

// log |det J| at u (ParameterTransformer.log_abs_det_jacobian); v is overwritten
template <int DP>
__device__ inline double xf_log_abs_det(const XfView& t, double (&v)[DP]) {
  const int D = t.D;
  const double* P = t.p;
  xf_unrotate<DP>(t, v);
#pragma unroll
  for (int d = 0; d < DP; ++d)
    if (d < D) {
      const int type = (int)P[XfLayout::row(XfLayout::TYPE, D) + d];
      const double ld = P[XfLayout::row(XfLayout::LOG_DELTA, D) + d];
      double p;
      if (type == XF_UNBOUNDED) {
        p = ld;
      } else {
        const double y = v[d] * P[XfLayout::row(XfLayout::DELTA, D) + d] + P[XfLayout::row(XfLayout::MU, D) + d];
        p = (P[XfLayout::row(XfLayout::LOG_SPAN, D) + d] + xf::bounded_lj(type, y)) + ld;
      }
      if (t.has_scale) p = p + P[XfLayout::row(XfLayout::LOG_SCALE, D) + d];
      v[d] = p;
    }
  return xf::row_sum<DP>(v, D);
}

// x strictly inside the original bounds in every dimension (VariationalPosterior.pdf's mask; NaN is outside)
template <int DP>
__device__ __forceinline__ bool xf_inside(const XfView& t, const double (&v)[DP]) {
  bool in = true;
#pragma unroll
  for (int d = 0; d < DP; ++d)
    if (d < t.D) in = in && (v[d] > t.p[XfLayout::row(XfLayout::LB, t.D) + d]) && (v[d] < t.p[XfLayout::row(XfLayout::UB, t.D) + d]);
  return in;
}

// host side (transform.hip): a slot's descriptor when it is set for D (xf_need: or the failure, prefixed `who`), and
// the launchers of its kernels on n device points.  apply: dir 0 x -> u, 1 u -> x, 2 log|J|(u).  prep / finish: the
// front and back of pdf(orig_flag=True) around the density of u.
struct vbmc_ctx;
bool xf_view_slot(vbmc_ctx* ctx, int slot, int D, XfView& v);
int xf_need(vbmc_ctx* ctx, int slot, int D, const char* who, XfView& v);
int launch_xf_apply(vbmc_ctx* ctx, const XfView& t, int64_t n, int dir, const double* d_in, double* d_out);
int launch_xf_prep(vbmc_ctx* ctx, const XfView& t, int64_t n, const double* d_x, double* d_u, double* d_lj, double* d_in);
int launch_xf_finish(vbmc_ctx* ctx, int64_t n, int log_flag, const double* d_lj, const double* d_in, double* d_y);
