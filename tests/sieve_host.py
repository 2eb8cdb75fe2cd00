"""The sieve's candidate generation, stated in NumPy.  TEST INFRASTRUCTURE: the yardstick of tests/test_sieve_host.py
(bit-equal to the reference's recorded arrays, tests/golden/sieve.npz) and of tests/test_sieve_gpu.py (the device's
thetas).

One candidate at a time, one statement per statement of the reference's ``_vb_init``
(pyvbmc/vbmc/variational_optimization.py:813-988), then ``get_parameters`` (variational_posterior.py:642-676),
``set_parameters`` (:702-759) and the eta assignment of ``_neg_elcbo`` (variational_optimization.py:1080-1085) as
``_sieve`` applies them to every candidate (:775-787).  The same NumPy calls on the same operands: nothing is vectorised
over candidates, because that would change summation orders.

Where the draws come from is the ``source``:

``NumpySource``   every draw is the reference's call on NumPy's global stream, in the reference's order.
``PhiloxSource``  every draw is a slot of the candidate's Philox row, as csrc/sieve.hip defines it: normal slot j is
                  element j % 2 of the pair at counter (candidate, j // 2, 10); spawned component j's parent is
                  floor(u K) with u at counter (candidate, 2 j, 11), its xi the uniform at (candidate, 2 j + 1, 11);
                  type 3 takes the min(K_new, N_star) training points of smallest key (counter (candidate, n, 12)),
                  ties by index, in that order.  Type 2's single sigma0 draw is
                  ``np.random.default_rng(seed).standard_normal((1, K_new))``.
"""
import math
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from oracle import philox_ref  # noqa: E402

GOLDEN = Path(__file__).resolve().parent / "golden" / "sieve.npz"
FLAG_SETS = {"all": (1, 1, 1, 1), "now": (1, 1, 1, 0), "nolam": (1, 1, 0, 1), "nomu": (0, 1, 1, 1)}  # mu, sigma, lambd, w
OPTION_KEYS = ("hpd_frac", "tol_length", "tol_weight", "tol_con_loss", "weight_penalty", "ns_ent", "ns_ent_fast", "ns_elbo")


def get_hpd(X, y, hpd_frac=0.8):
    """stats/get_hpd.py:30-45."""
    N, D = X.shape
    order = np.argsort(y, axis=None)[::-1]
    hpd_N = round(hpd_frac * N)
    indices = order[0:hpd_N]
    hpd_X, hpd_y = X[indices], y[indices]
    hpd_range = np.max(hpd_X, axis=0) - np.min(hpd_X, axis=0) if hpd_N > 0 else np.full((D), np.nan)
    return hpd_X, hpd_y, hpd_range, indices


class NumpySource:
    def at(self, b):
        pass

    def sigma2(self, Kn):
        return np.random.randn(1, Kn)

    def parent(self, j, K):
        return np.random.randint(0, K)

    def spawn_mu(self, j, D):
        return np.random.randn(D, 1)

    def spawn_sigma(self, j, D):
        return np.random.randn()

    def spawn_xi(self, j):
        return np.random.rand()

    def selection(self, N_star, m):
        return np.random.permutation(N_star)

    def sigma3(self, Kn):
        return np.random.randn(1, Kn)

    def jitter_mu(self, D, Kn):
        return np.random.randn(D, Kn)

    def jitter_sigma(self, Kn):
        return np.random.randn(1, Kn)

    def jitter_lambd(self, D):
        return np.random.randn(D, 1)

    def jitter_w(self, Kn):
        return np.random.randn(1, Kn)


class PhiloxSource:
    def __init__(self, seed, D, K, Kn):
        self.seed, self.D, self.K, self.Kn = int(seed), D, K, Kn
        self.s_s3 = (Kn - K) * (D + 1)
        self.s_mu = self.s_s3 + Kn
        self.s_sg = self.s_mu + D * Kn
        self.s_lm = self.s_sg + Kn
        self.s_w = self.s_lm + D
        self.s_u = self.s_w + Kn

    def at(self, b):
        self.b = b
        self.z = philox_ref.normals([b], self.s_u, self.seed, 10)[0]

    def _words(self, c2, c3):
        b = np.uint64(self.b)
        lo = np.full(np.shape(c2), b & philox_ref.MASK, dtype=np.uint64).astype(np.uint32)
        hi = np.full(np.shape(c2), b >> np.uint64(32), dtype=np.uint64).astype(np.uint32)
        x0, x1, _, _ = philox_ref.philox4x32_10(lo, hi, np.asarray(c2, dtype=np.uint32), np.full(np.shape(c2), c3, dtype=np.uint32),
                                                self.seed & 0xFFFFFFFF, (self.seed >> 32) & 0xFFFFFFFF)
        return ((x0.astype(np.uint64) << np.uint64(32)) | x1.astype(np.uint64)) >> np.uint64(11)

    def _uniform(self, c2):
        return float(self._words(np.array([c2]), 11)[0]) * 2.0**-53

    def sigma2(self, Kn):
        return np.random.default_rng(self.seed).standard_normal((1, Kn))

    def parent(self, j, K):
        return int(math.floor(self._uniform(2 * j) * K))

    def spawn_mu(self, j, D):
        return self.z[j * (D + 1) : j * (D + 1) + D].reshape(D, 1)

    def spawn_sigma(self, j, D):
        return self.z[j * (D + 1) + D]

    def spawn_xi(self, j):
        return self._uniform(2 * j + 1)

    def selection(self, N_star, m):
        return np.argsort(self._words(np.arange(N_star), 12), kind="stable")

    def sigma3(self, Kn):
        return self.z[self.s_s3 : self.s_mu].reshape(1, Kn)

    def jitter_mu(self, D, Kn):
        return self.z[self.s_mu : self.s_sg].reshape(D, Kn)

    def jitter_sigma(self, Kn):
        return self.z[self.s_sg : self.s_lm].reshape(1, Kn)

    def jitter_lambd(self, D):
        return self.z[self.s_lm : self.s_w].reshape(D, 1)

    def jitter_w(self, Kn):
        return self.z[self.s_w : self.s_u].reshape(1, Kn)


def vb_init_host(base, flags, vb_type, opts_N, K_new, X_star, y_star, source, b0=0):
    """The ``opts_N`` candidates of one ``_vb_init`` call as dicts of ``mu`` (D, K_new), ``sigma`` (1, K_new), ``lambd``
    (D, 1), ``w`` (1, K_new), ``eta`` (1, K_new) -- what the reference's new posteriors hold on return.  ``base``: the same
    five of the starting posterior; ``flags``: optimize_(mu, sigma, lambd, weights); ``b0``: the first candidate's index
    in the whole set (the Philox counter)."""
    o_mu, o_sg, o_lm, o_w = (bool(f) for f in flags)
    D, K = base["mu"].shape
    N_star = X_star.shape[0]
    lambd0, mu0, w0 = base["lambd"].copy(), base["mu"].copy(), base["w"].copy()
    if vb_type == 1:
        sigma0 = base["sigma"].copy()
    elif vb_type == 2:
        if o_mu:
            order = np.argsort(y_star, axis=None)[::-1]
            idx_order = np.tile(range(0, min(K_new, N_star)), (math.ceil(K_new / N_star),))
            mu0 = X_star[order[idx_order[0:K_new]], :].T
        V = np.var(mu0, axis=1, ddof=1) if K > 1 else np.var(X_star, axis=0, ddof=1)
        sigma0 = np.sqrt(np.mean(V / lambd0**2) / K_new) * np.exp(0.2 * source.sigma2(K_new))
    else:
        if o_mu:
            mu0 = np.zeros((D, K))
        sigma0 = np.zeros((1, K))
    out = []
    for i in range(opts_N):
        source.at(b0 + i)
        add_jitter = True
        mu, sigma, lambd = mu0.copy(), sigma0.copy(), lambd0.copy()
        if o_w:
            w = w0.copy()
        if vb_type == 1:
            if i == 0:
                add_jitter = False
            for i_new in range(K, K_new):
                j = i_new - K
                idx = source.parent(j, K)
                mu = np.hstack((mu, mu[:, idx : idx + 1]))
                sigma = np.hstack((sigma, sigma[0:1, idx : idx + 1]))
                mu[:, i_new : i_new + 1] += 0.5 * sigma[0, i_new] * lambd * source.spawn_mu(j, D)
                if o_sg:
                    sigma[0, i_new] *= np.exp(0.2 * source.spawn_sigma(j, D))
                if o_w:
                    xi = 0.25 + 0.25 * source.spawn_xi(j)
                    w = np.hstack((w, xi * w[0:1, idx : idx + 1]))
                    w[0, idx] *= 1 - xi
        elif vb_type == 2:
            if i == 0:
                add_jitter = False
            if o_lm:
                lambd = np.reshape(np.std(X_star, axis=0, ddof=1), (-1, 1))
                lambd *= np.sqrt(D / np.sum(lambd**2))
            if o_w:
                w = np.ones((1, K_new)) / K_new
        else:
            if o_mu:
                order = source.selection(N_star, min(K_new, N_star))
                idx_order = np.tile(range(0, min(K_new, N_star)), (math.ceil(K_new / N_star),))
                mu = X_star[order[idx_order[0:K_new]], :].T
            else:
                mu = mu0.copy()
            if o_sg:
                V = np.var(mu, axis=1, ddof=1) if K > 1 else np.var(X_star, axis=0, ddof=1)
                sigma = np.sqrt(np.mean(V) / K_new) * np.exp(0.2 * source.sigma3(K_new))
            if o_lm:
                lambd = np.reshape(np.std(X_star, axis=0, ddof=1), (-1, 1))
                lambd *= np.sqrt(D / np.sum(lambd**2))
            if o_w:
                w = np.ones((1, K_new)) / K_new
        if add_jitter:
            if o_mu:
                mu += sigma * lambd * source.jitter_mu(mu.shape[0], mu.shape[1])
            if o_sg:
                sigma *= np.exp(0.2 * source.jitter_sigma(K_new))
            if o_lm:
                lambd *= np.exp(0.2 * source.jitter_lambd(D))
            if o_w:
                w *= np.exp(0.2 * source.jitter_w(K_new))
                w /= np.sum(w)
        out.append({"mu": mu if o_mu else mu0.copy(), "sigma": sigma, "lambd": lambd,
                    "w": w if o_w else np.ones((1, K_new)) / K_new, "eta": np.ones((1, K_new)) / K_new})
    return out


def finish(c, flags):
    """``theta = get_parameters()``, ``set_parameters(theta)`` and the eta assignment, as ``_sieve``'s loop applies them
    to a candidate: returns ``theta`` (the eta tail max-shifted) and the candidate's five arrays afterwards."""
    o_mu, o_sg, o_lm, o_w = (bool(f) for f in flags)
    D, K = c["mu"].shape
    mu, sigma, lambd, w = c["mu"], c["sigma"], c["lambd"], c["w"]
    nl = np.sqrt(np.sum(lambd**2) / D)
    lambd = lambd.reshape(-1, 1) / nl
    sigma = sigma.reshape(1, -1) * nl
    if o_w:
        w = w.reshape(1, -1) / np.sum(w)
    theta = mu.ravel(order="F") if o_mu else np.array([])
    cp = np.array([])
    if o_sg:
        cp = np.concatenate((cp, sigma.ravel()))
    if o_lm:
        cp = np.concatenate((cp, lambd.ravel()))
    if o_w:
        cp = np.concatenate((cp, w.ravel()))
    theta = np.concatenate((theta, np.log(cp)))
    t = theta.copy()
    start = 0
    if o_mu:
        mu = np.reshape(t[: D * K], (D, K), order="F")
        start = D * K
    if o_sg:
        sigma = np.exp(t[start : start + K])
        start += K
    if o_lm:
        lambd = np.exp(t[start : start + D]).T
    if o_w:
        eta = t[-K:]
        eta = eta - np.amax(eta)
        w = np.exp(eta.T)[:, np.newaxis]
    nl = np.sqrt(np.sum(lambd**2) / D)
    lambd = lambd.reshape(-1, 1) / nl
    sigma = sigma.reshape(1, -1) * nl
    if o_w:
        w = w.reshape(1, -1) / np.sum(w)
    eta_out = c["eta"]
    if o_w:
        theta[-K:] -= np.amax(theta[-K:])
        eta_out = np.reshape(theta[-K:], (1, -1))
    return theta, {"mu": mu, "sigma": sigma, "lambd": lambd, "w": w, "eta": eta_out}


def split(init_N, best_N):
    """How ``_sieve`` splits ``init_N`` over the three types (:756-768)."""
    if best_N == 1:
        return (init_N, 0, 0)
    n = math.ceil(init_N / 3)
    return (n, n, max(0, init_N - 2 * n))


def candidates_host(base, flags, counts, K_new, X_star, y_star, source):
    """All candidates of a sieve in set order: ``(raw dicts, thetas (B, n_theta), finished dicts, types)``."""
    raw, types, b0 = [], [], 0
    for t, n in zip((1, 2, 3), counts):
        if n > 0:
            raw += vb_init_host(base, flags, t, n, K_new, X_star, y_star, source, b0)
            types += [float(t)] * n
            b0 += n
    fin = [finish(c, flags) for c in raw]
    return raw, np.stack([f[0] for f in fin]), [f[1] for f in fin], np.array(types)


# ---- the fixture ---------------------------------------------------------------------------------------------------------

def case_names(z):
    return [str(n) for n in z["cases"]]


def load_case(z, name):
    """A case of tests/golden/sieve.npz as a dict (keys without the ``name_`` prefix)."""
    p = name + "_"
    return {k[len(p):]: z[k] for k in z.files if k.startswith(p)}


def base_of(c):
    return {k: np.array(c["base_" + k]) for k in ("mu", "sigma", "lambd", "w", "eta")}


def options_of(c):
    o = {k: float(v) for k, v in zip(OPTION_KEYS, c["options"])}
    return o
