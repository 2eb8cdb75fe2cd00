"""A reference-shaped parameter transformer for the tests: the fields of the reference's
``ParameterTransformer`` (type, lb_orig, ub_orig, mu, delta, R_mat, scale) taken from
tests/golden/transform.npz or transform_wide.npz, and its three maps evaluated dimension by dimension from a table of
per-type formulas -- the host side that ``VBMC_HIP_TRANSFORM=0`` runs.

Per bounded dimension (z in the unit interval, y the uncentred transformed value):

    type  y = g(z)                              z = g^-1(y)                            log|dz/dy|
     3    log(z / (1 - z)),  -inf / +inf at 0/1  0 where -y > log(DBL_MAX), else 1/(1+e^-y)   -y - 2 log1p(e^-y)
    12    -sqrt(2) erfcinv(2 z)                  erfc(-y / sqrt(2)) / 2                  -log(2 pi)/2 - y^2/2
    13    sign(z - 1/2) 2 sqrt(q - 1),           1/2 + 3/8 y / sqrt(1 + y^2/4)           log(3/8) - 5/2 log1p(y^2/4)
          q = cos(acos(a)/3) / a, a = sqrt(4z(1-z)) (q = inf at a = 0)   * (1 - y^2/(1 + y^2/4)/12)

with z nudged one step inside (0, 1) when x is not on the bound itself, and x clipped one ulp inside
(lb, ub) on the way back; then centring (mu, delta), rotation R and scale.  The order of every
floating-point operation is the reference's; tests/test_transform_host.py pins this module against
the reference's stored outputs."""
import numpy as np
from scipy.special import erfc, erfcinv

CASES = ("logit", "probit", "student4", "mixed", "roto")
# transform_wide.npz: one case per padded width of the device kernels, D = the number in the name
WIDE_CASES = ("w1", "w2", "w6", "w7", "w8", "w9", "w12", "w16", "w17", "w24", "w25", "w32")

_TINY = np.nextafter(0.0, 1.0)
_BELOW_ONE = np.nextafter(1.0, 0.0)
_LOG_MAX = np.log(np.finfo(np.float64).max)
_SQRT2 = np.sqrt(2.0)


def _student4_fwd(z):
    a = np.sqrt(4 * z * (1 - z))
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(a == 0.0, np.inf, np.cos(np.arccos(a) / 3) / a)
    return np.sign(z - 0.5) * (2 * np.sqrt(q - 1))


def _student4_inv(y):
    s = y**2
    c = 1 + s / 4
    return 0.5 + (3 / 8) * (y / np.sqrt(c)) * (1 - s / c / 12)


def _logit_fwd(z):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(z == 0, -np.inf, np.where(z == 1, np.inf, np.log(z / (1 - z))))


def _logit_inv(y):
    with np.errstate(over="ignore"):
        return np.where(-y > _LOG_MAX, 0.0, 1 / (1 + np.exp(-y)))


# type code -> (g, g^-1, log|dz/dy| of y)
_TABLE = {
    3: (_logit_fwd, _logit_inv, lambda y: -y + 2 * (-np.log1p(np.exp(-y)))),
    12: (lambda z: -_SQRT2 * erfcinv(2 * z), lambda y: 0.5 * erfc(-y / _SQRT2),
         lambda y: -0.5 * np.log(2 * np.pi) - 0.5 * y**2),
    13: (_student4_fwd, _student4_inv, lambda y: np.log(3 / 8) - (5 / 2) * np.log1p(y**2 / 4)),
}


class RefShapedTransformer:
    """Duck type with the reference transformer's fields and calls."""

    def __init__(self, type, lb_orig, ub_orig, mu, delta, R_mat=None, scale=None):
        self.type = np.asarray(type, dtype=np.float64)
        self.lb_orig = np.asarray(lb_orig, dtype=np.float64).reshape(1, -1)
        self.ub_orig = np.asarray(ub_orig, dtype=np.float64).reshape(1, -1)
        self.mu = np.asarray(mu, dtype=np.float64).copy()
        self.delta = np.asarray(delta, dtype=np.float64).copy()
        self.R_mat = None if R_mat is None else np.asarray(R_mat, dtype=np.float64).copy()
        self.scale = None if scale is None else np.asarray(scale, dtype=np.float64).copy()

    @classmethod
    def from_golden(cls, g, name):
        R, s = g[f"{name}_R"], g[f"{name}_scale"]
        return cls(g[f"{name}_type"], g[f"{name}_lb"], g[f"{name}_ub"], g[f"{name}_mu"], g[f"{name}_delta"],
                   R if R.size else None, s if s.size else None)

    def _dims(self):
        """(column, type code, lb, ub, mu, delta) of every dimension."""
        return [(d, int(self.type[d]), self.lb_orig[0, d], self.ub_orig[0, d], self.mu[d], self.delta[d])
                for d in range(self.type.size)]

    def _whitened_to_centred(self, u):
        """Scale, then the transpose of R applied: the first steps of inverse and log|J|."""
        v = np.array(np.atleast_2d(u), dtype=np.float64)
        if self.scale is not None:
            v = v * self.scale
        if self.R_mat is not None:
            v = np.dot(v, self.R_mat.T)
        return v

    def __call__(self, x):
        dims = np.ndim(x)
        x = np.array(np.atleast_2d(x), dtype=np.float64)
        out = np.empty_like(x)
        for d, t, lb, ub, mu, dl in self._dims():
            col = x[:, d]
            if t == 0:
                out[:, d] = (col - mu) / dl
                continue
            z = (col - lb) / (ub - lb)
            z = np.where((z == 0) & (col != lb), _TINY, z)
            z = np.where((z == 1) & (col != ub), _BELOW_ONE, z)
            out[:, d] = (_TABLE[t][0](z) - mu) / dl
        if self.R_mat is not None:
            out = np.dot(out, self.R_mat)
        if self.scale is not None:
            out = out / self.scale
        return out.ravel() if dims == 1 else out

    def inverse(self, u):
        dims = np.ndim(u)
        v = self._whitened_to_centred(u)
        out = np.empty_like(v)
        for d, t, lb, ub, mu, dl in self._dims():
            y = v[:, d] * dl + mu
            if t == 0:
                out[:, d] = y
            else:
                out[:, d] = np.clip(_TABLE[t][1](y) * (ub - lb) + lb, np.nextafter(lb, np.inf), np.nextafter(ub, -np.inf))
        return out.ravel() if dims == 1 else out

    def log_abs_det_jacobian(self, u):
        dims = np.ndim(u)
        v = self._whitened_to_centred(u)
        terms = np.empty_like(v)
        for d, t, lb, ub, mu, dl in self._dims():
            if t == 0:
                terms[:, d] = np.log(dl)
            else:
                terms[:, d] = np.log(ub - lb) + _TABLE[t][2](v[:, d] * dl + mu) + np.log(dl)
        if self.scale is not None:
            terms = terms + np.log(self.scale)
        total = terms.sum(axis=1)
        return total.ravel()[0] if dims == 1 else total


def golden_vp(VariationalPosterior, g, name, pt, ctx=None):
    """The fixture's small mixture (the one the reference's pdf values were taken with) around ``pt``."""
    mu = g[f"{name}_vp_mu"]
    D, K = mu.shape
    vp = VariationalPosterior(D, K, parameter_transformer=pt)
    if ctx is not None:
        vp.ctx = ctx
    vp.mu = mu.copy()
    vp.sigma = g[f"{name}_vp_sigma"].reshape(1, -1).copy()
    vp.lambd = g[f"{name}_vp_lambd"].reshape(-1, 1).copy()
    vp.w = g[f"{name}_vp_w"].reshape(1, -1).copy()
    vp.eta = np.log(vp.w)
    return vp
