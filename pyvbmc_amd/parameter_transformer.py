"""``ParameterTransformer``: the host class behind the device transformer (pyvbmc_amd/transformer.py wraps one; this
module builds one).  Mirror of the reference's ``parameter_transformer/parameter_transformer.py`` (:10-133 the
constructor, :134-269 the three maps); line numbers below cite that file.

Per dimension the map is ``x -> z -> y -> (y - mu) / delta``, then rotation ``R_mat`` and ``scale`` over all dimensions:

    type 0   unbounded                 y = x
    type 3   logit      z = (x - lb) / (ub - lb)   y = log(z / (1 - z))
    type 12  probit                                y = -sqrt(2) erfcinv(2 z)
    type 13  student4                              y = sign(z - 1/2) 2 sqrt(cos(acos(a) / 3) / a - 1),  a = sqrt(4 z (1 - z))

``mu`` and ``delta`` centre the plausible box on (-1/2, 1/2) in the transformed space (:120-132).  The fields the device
route reads (``transformer.transformer_fields``) are the reference's: ``type``, ``lb_orig``, ``ub_orig``, ``mu``,
``delta``, ``R_mat``, ``scale``; ``transformer.candidate`` accepts an instance, so every device route runs with it.
"""
import numpy as np
from scipy.special import erfc, erfcinv

TRANSFORM_TYPES = {"logit": 3, "norminv": 12, "probit": 12, "student4": 13}
_LOG_MAX = np.log(np.finfo(np.float64).max)
_SQRT2 = np.sqrt(2)


def _logit(z):
    u = np.zeros_like(z)
    u[z == 0] = -np.inf
    u[z == 1] = np.inf
    m = u == 0
    u[m] = np.log(z[m] / (1 - z[m]))
    return u


def _logit_inv(y):
    z = np.zeros_like(y)
    m = ~(-y > _LOG_MAX)  # (beyond it exp overflows: z = 0)
    z[m] = 1 / (1 + np.exp(-y[m]))
    return z


def _student4(z):
    a = np.sqrt(4 * z * (1 - z))
    q = np.full_like(z, np.inf)
    m = a != 0.0
    q[m] = np.cos(np.arccos(a[m]) / 3) / a[m]
    return np.sign(z - 0.5) * (2 * np.sqrt(q - 1))


def _student4_inv(y):
    t2 = y**2
    return 0.5 + (3 / 8) * (y / np.sqrt(1 + t2 / 4)) * (1 - t2 / (1 + t2 / 4) / 12)


# type code -> (z -> y, y -> z, y -> log |dz / dy|)
_MAPS = {
    3: (_logit, _logit_inv, lambda y: -y + 2 * (-np.log1p(np.exp(-y)))),
    12: (lambda z: -_SQRT2 * erfcinv(2 * z), lambda y: 0.5 * erfc(-y / _SQRT2),
         lambda y: -0.5 * np.log(2 * np.pi) - 0.5 * y**2),
    13: (_student4, _student4_inv, lambda y: np.log(3 / 8) - (5 / 2) * np.log1p(y**2 / 4)),
}


def _rows(x):
    """handle_0D_1D_input: ``(ndim, x as float rows)``."""
    return np.ndim(x), np.array(np.atleast_2d(x), dtype=np.float64)


class ParameterTransformer:
    """``ParameterTransformer(D, lb_orig, ub_orig, plb_orig, pub_orig, scale, rotation_matrix, transform_type)``: the
    reference's arguments, defaults, fields and ``ValueError``s."""

    def __init__(self, D, lb_orig=None, ub_orig=None, plb_orig=None, pub_orig=None, scale=None, rotation_matrix=None,
                 transform_type="logit"):
        self.scale = scale
        self.R_mat = rotation_matrix
        if lb_orig is None:
            lb_orig = np.full((1, D), -np.inf)
        if ub_orig is None:
            ub_orig = np.full((1, D), np.inf)
        if plb_orig is None:
            plb_orig = np.copy(lb_orig)
        if pub_orig is None:
            pub_orig = np.copy(ub_orig)
        if not (np.all(lb_orig <= plb_orig) and np.all(plb_orig < pub_orig) and np.all(pub_orig <= ub_orig)):
            raise ValueError("Variable bounds should be LB <= PLB < PUB <= UB for all variables.")
        self.lb_orig = lb_orig
        self.ub_orig = ub_orig

        if isinstance(transform_type, str):
            if transform_type not in TRANSFORM_TYPES:
                raise ValueError(f"Unrecognized bounded transform {transform_type}.")
            bounded_type = TRANSFORM_TYPES[transform_type]
        else:
            if transform_type not in TRANSFORM_TYPES.values():
                raise ValueError(f"Unrecognized bounded transform {transform_type}.")
            bounded_type = transform_type
        self.bounded_types = [bounded_type]

        lb, ub = np.reshape(lb_orig, (1, -1)), np.reshape(ub_orig, (1, -1))
        self.type = np.zeros(D)
        self.type[(np.isfinite(lb) & np.isfinite(ub) & (lb < ub))[0]] = bounded_type
        self.mu = np.zeros(D)
        self.delta = np.ones(D)
        if not (np.all(plb_orig == self.lb_orig) and np.all(pub_orig == self.ub_orig)):  # :121-132
            plb_tran = self(np.atleast_2d(plb_orig))
            pub_tran = self(np.atleast_2d(pub_orig))
            ok = np.isfinite(plb_tran[0]) & np.isfinite(pub_tran[0])
            self.mu[ok] = (0.5 * (plb_tran[0] + pub_tran[0]))[ok]
            self.delta[ok] = (pub_tran[0] - plb_tran[0])[ok]

    # ---- the three maps
    def _bounded(self):
        """(type code, column mask, lb, ub) of every bounded type present."""
        for t in self.bounded_types:
            m = self.type == t
            if np.any(m):
                yield t, m, self.lb_orig[:, m], self.ub_orig[:, m]

    def _unwhiten(self, u):
        if self.scale is not None:
            u = u * self.scale
        if self.R_mat is not None:
            u = u @ np.transpose(self.R_mat)
        return u

    def __call__(self, x):
        dims, x = _rows(x)
        u = np.copy(x)
        m = self.type == 0
        if np.any(m):
            u[:, m] = (x[:, m] - self.mu[m]) / self.delta[m]
        for t, m, lb, ub in self._bounded():
            xm = x[:, m]
            z = (xm - lb) / (ub - lb)
            # a point that is not on the bound itself stays one step inside the unit interval (:476-485)
            z[(z == 0) & (xm != lb)] = np.nextafter(0, np.inf)
            z[(z == 1) & (xm != ub)] = np.nextafter(1, -np.inf)
            u[:, m] = (_MAPS[t][0](z) - self.mu[m]) / self.delta[m]
        if self.R_mat is not None:
            u = u @ self.R_mat
        if self.scale is not None:
            u = u / self.scale
        return u.ravel() if dims <= 1 else u

    def inverse(self, u):
        dims, u = _rows(u)
        v = self._unwhiten(np.copy(u))
        x = np.copy(v)
        m = self.type == 0
        if np.any(m):
            x[:, m] = v[:, m] * self.delta[m] + self.mu[m]
        for t, m, lb, ub in self._bounded():
            y = _MAPS[t][1](v[:, m] * self.delta[m] + self.mu[m]) * (ub - lb) + lb
            x[:, m] = np.minimum(np.maximum(y, np.nextafter(lb, np.inf)), np.nextafter(ub, -np.inf))  # :488-493
        return x.ravel() if dims <= 1 else x

    def log_abs_det_jacobian(self, u):
        dims, u = _rows(u)
        v = self._unwhiten(np.copy(u))
        p = np.zeros(v.shape)
        m = self.type == 0
        if np.any(m):
            p[:, m] = np.log(self.delta[m])[np.newaxis]
        for t, m, lb, ub in self._bounded():
            p[:, m] = np.log(ub - lb) + _MAPS[t][2](v[:, m] * self.delta[m] + self.mu[m]) + np.log(self.delta[m])
        if self.scale is not None:
            p = p + np.log(self.scale)
        p = np.sum(p, axis=1)
        return p[0] if dims <= 1 else p

    def __eq__(self, other):
        """By value (:405-419), over the fields the device reads and the bounded type."""
        if not isinstance(other, ParameterTransformer):
            return NotImplemented

        def same(a, b):
            if a is None or b is None:
                return a is None and b is None
            return np.shape(a) == np.shape(b) and bool(np.all(np.asarray(a) == np.asarray(b)))

        return self.bounded_types == other.bounded_types and all(
            same(getattr(self, f), getattr(other, f)) for f in ("scale", "R_mat", "lb_orig", "ub_orig", "type", "mu", "delta"))


__all__ = ["ParameterTransformer", "TRANSFORM_TYPES"]
