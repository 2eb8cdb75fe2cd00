"""The one-launch families of the active-sampling side at every padded width of ``VBMC_DISPATCH_DP`` (csrc/common.h):
the search points, rounding, mask and values (csrc/search.hip, csrc/api_search.hip), the importance state
(csrc/acq_is_prep.hip, csrc/api_acq_is.hip), input warping (csrc/warp.hip) and the mode search (csrc/mode.hip) at the
dimensions of tests/width_cases.py -- the benchmark's D = 10 and 20 among them -- where their own test files stop at
D = 2, 3, 4 and one D = 32 case.

Nothing is restated here: every comparison is the assertion function of the family's own test file, at its tolerance, on
a case built at the swept D.  The lines starting ``WIDTH |`` are the largest error of a quantity as a fraction of its
bound; profiles/width_sweep.md holds those of one run.

What the swept dimensions reach that the families' own cases do not: the Philox pair loops whose second element lands on
index D at an odd D (``search_fill_kernel``, the ``gen == 2`` branch of ``warp_points_kernel``, ``is_box_sample_kernel``);
``warp_unscent_kernel``'s LDS block of (2 DP + 1) DP doubles with U = 2 D + 1 active threads and its two descriptors
staged into arrays sized by DP; the integer mask's bit D - 1 next to a padded lane.
"""

import numpy as np
import pytest

import ais_host
import ais_mcmc_cases
import mode_host as mh
import search_host as sh
import whitening_host as wh
from width_cases import MODE_D, SWEEP_D

import test_ais_gpu as t_ais
import test_mode_gpu as t_mode
import test_search_gpu as t_search
import test_whitening_gpu as t_warp

pytestmark = pytest.mark.gpu

# the Philox key of the search points per D: the first of 1, 2, ... under which no element of the restatement's points is a
# sum that cancels by more than a factor 100 (test_search_gpu.POINT_SEEDS' condition, asserted by check_philox_points)
SEARCH_SEEDS = {D: 1 for D in SWEEP_D}
SEARCH_ACQS = ("AcqFcnLog", "AcqFcnNoisy", "AcqFcnVIQR")


@pytest.fixture(scope="module")
def ctx():
    from pyvbmc_amd import _lib

    c = _lib.Context(0)
    _lib.set_default_context(c)
    yield c
    _lib.set_default_context(None)
    c.close()


def row(family, D, what, err, bound):
    print(f"WIDTH | {family} | {D} | {what} | {err:.2e} | {bound:.1e} | {err / bound:.3f} |")


# ---------------------------------------------------------------------------------------------- search
def int_dims(D):
    return (0, D // 2, D - 1)  # the mask's first bit, one in the middle, and the last: the bit next to the padded lanes


def cutting_bounds(c, X):
    """Hard bounds in the original space that cut part of the points X (transformed space) off: an upper bound in
    dimensions 0 and D - 1 and a lower one in dimension D // 2, each halfway between two neighbouring coordinates of the
    set (so that no point sits on a bound), the other dimensions open."""
    Xo = c.pt.inverse(X)
    D = Xo.shape[1]
    lo, hi = Xo.min(0) - 1.0, Xo.max(0) + 1.0

    def between(d, q):  # halfway between the two distinct coordinates around the q-quantile (clamped points share theirs)
        u = np.unique(Xo[:, d])
        i = min(max(int(np.searchsorted(u, np.quantile(Xo[:, d], q))) - 1, 0), u.size - 2)
        return 0.5 * (u[i] + u[i + 1])

    for d in {0, D - 1}:
        hi[d] = between(d, 0.9)
    lo[D // 2] = between(D // 2, 0.1)
    width = hi - lo
    assert np.min(np.abs(Xo - lo) / width) > 1e-9 and np.min(np.abs(Xo - hi) / width) > 1e-9
    return lo, hi


@pytest.mark.parametrize("D", SWEEP_D)
def test_search_points_and_rounding(ctx, D):
    """The Philox points at D (N = 40, 300 points, every source on), then integer dimensions 0, D // 2 and D - 1."""
    c = sh.wide_case(D=D)
    assert c.number_of_points == 300 and c.flog.X.shape == (40, D)
    e_cache, e_other = t_search.check_philox_points(ctx, c, SEARCH_SEEDS[D], f"wide D={D}")
    row("search points", D, "cache rows (transformer)", e_cache, 1e-12)
    row("search points", D, "drawn rows", e_other, 1e-13)
    t_search.check_integer_rounding(ctx, c, int_dims(D), SEARCH_SEEDS[D])


def values_at(ctx, c, D, acq_name, seed, what, points_conditioned=True, length_mult=1.0):
    """One search with hard bounds that cut part of the set off: the mask and the values."""
    s = t_search.search_setup(c, ctx, S=2, acq_name=acq_name, length_mult=length_mult)
    Xh, _, _ = sh.points_philox(c.number_of_points, c.optim_state, c.flog, c.mix, c.options, seed)
    s.state["lb_eps_orig"], s.state["ub_eps_orig"] = cutting_bounds(c, Xh)
    mask = sh.hard_bound_mask(Xh, c.pt, s.state)
    assert 0 < mask.sum() < mask.size  # the bounds cut off part of the set
    res, X, (e_own, e_host) = t_search.check_values(ctx, c, s, acq_name, seed, what, points_conditioned=points_conditioned)
    np.testing.assert_array_equal(np.isposinf(res.acq_fast), sh.hard_bound_mask(X, c.pt, s.state))
    np.testing.assert_array_equal(np.isposinf(res.acq_fast), mask)
    assert np.all(res.acq_fast[res.order[-int(mask.sum()):]] == np.inf)
    row("search values", D, what + " vs own call", e_own, 1e-9)
    row("search values", D, what + " vs restatement", e_host, 1e-9)
    return res


def grown(D):
    """Length scales that grow with sqrt(D): two of the case's points (spread 1.2 per dimension) then stay a few length
    scales apart at every D, and the GP's cross-covariances are part of what the values compare."""
    return max(1.0, float(np.sqrt(D / 4.0)))


@pytest.mark.parametrize("lengths", ["fixture", "grown"])
@pytest.mark.parametrize("acq_name", SEARCH_ACQS)
@pytest.mark.parametrize("D", SWEEP_D)
def test_search_values(ctx, D, acq_name, lengths):
    """The fixture's GP as it is, and with its length scales grown with sqrt(D): at the fixture's own, the median
    covariance of a search point and a training point is 9e-6 sf^2 at D = 10, 3e-12 at D = 20 and 4e-17 at D = 32, so
    that at most points the values test the mean function and the mixture only."""
    values_at(ctx, sh.wide_case(D=D), D, acq_name, SEARCH_SEEDS[D], f"{acq_name} ({lengths} lengths) D={D}",
              length_mult=grown(D) if lengths == "grown" else 1.0)


@pytest.mark.parametrize("D", SWEEP_D)
def test_search_values_noisy_where_it_is_not_flat(ctx, D):
    """AcqFcnNoisy is a product with exp(f_bar - y_max) p(x): on the wide case around 25 it underflows to -0 at most points
    from D = 10 and at all of them from D = 13, where the comparison above holds trivially.  The same case around 0 with
    half the mixture widths has values of order 1e-3 and more at dozens of points.  (Around 0 a coordinate is a sum that
    cancels: the points' relative precondition does not hold, and they are compared relative to the largest coordinate.)"""
    c = sh.wide_case(D=D, centre=0.0, sigma_scale=0.5)
    res = values_at(ctx, c, D, "AcqFcnNoisy", 1, f"AcqFcnNoisy (centre 0) D={D}", points_conditioned=False, length_mult=grown(D))
    assert int((np.abs(res.acq_fast[np.isfinite(res.acq_fast)]) > 1e-3).sum()) >= 30


# ---------------------------------------------------------------------------------------------- importance state
def ais_case(D):
    """GP and mixture as tests/ais_mcmc_cases.py builds them at (D, N = 70, S = 2), with evaluation points and a
    per-point noise table like ``ais_host.larger_case``'s."""
    ogp, mix = ais_mcmc_cases.gp_at(D, 70, 2)
    rng = np.random.default_rng(1000 + D)
    return ogp, mix, 1.3 * rng.standard_normal((100, D)), 0.01 + rng.random(70)


@pytest.mark.parametrize("D", SWEEP_D)
def test_importance_state(ctx, D):
    """vbmc_is_proposal, vbmc_acq_is_build and vbmc_acq_is_eval at D: 40 + 30 points of NumPy's stream against
    ``ais_host.from_points`` (test_tile_edges_vs_host's comparison), then the Philox route at 30 + 18."""
    from pyvbmc_amd.active_importance_sampling import active_importance_sampling

    ogp, mix, Xs, sn2_new = ais_case(D)
    gp, length = t_ais.plain_gp(ogp, sn2_new)
    vp, acq = t_ais.PlainVP(mix), t_ais.mirror_acq(ais_host.IMIQR)
    n_vp, n_box = 40, 30
    opts = ais_host.Opts(active_importance_sampling_vp_samples=n_vp, active_importance_sampling_box_samples=n_box,
                         active_importance_sampling_mcmc_samples=0, active_importance_sampling_mcmc_thin=1)
    np.random.seed(7)
    out = active_importance_sampling(vp, gp, acq, opts, sampler=ais_host.StandInSampler)
    assert out["X"].shape == (n_vp + n_box, D)
    with np.errstate(all="ignore"):
        host = ais_host.from_points(ogp, mix, out["X"], ais_host.IMIQR, n_vp, n_box)
    e_c = t_ais.check_state(out, host, ogp, f"D={D} {n_vp}+{n_box}")
    row("importance state", D, "C_tmp", e_c, 10 * t_ais.CTMP_REL_MEASURED)
    row("importance state", D, "acquisition", t_ais.check_quantile_acq(acq, gp, vp, ogp, length, sn2_new, Xs, out, host), 1e-9)
    e_c = t_ais.check_philox_imiqr(ogp, mix, sn2_new, 30, 18, what=f"D={D} philox")
    row("importance state", D, "C_tmp (philox)", e_c, 10 * t_ais.CTMP_REL_MEASURED)


# ---------------------------------------------------------------------------------------------- warp
@pytest.fixture(scope="module")
def wide_golden(golden):
    return golden("transform_wide")


@pytest.mark.parametrize("D", SWEEP_D)
def test_warp_points_and_unscent(ctx, wide_golden, D):
    c = wh.wide_case(D, wide_golden=wide_golden)
    assert sorted(set(c.old.type.astype(int))) == [0, 3, 12, 13] and c.old.R is not None and c.old.scale is not None
    assert c.K == 3 and c.new.R.shape == (D, D) and np.all(c.new.mu == 0) and np.all(c.new.delta == 1)
    t_warp.check_points(ctx, c, c.name)
    t_warp.check_unscent(ctx, c, c.name)


@pytest.mark.parametrize("D", SWEEP_D)
def test_warp_gp_and_box(ctx, wide_golden, D):
    c = wh.wide_case(D, wide_golden=wide_golden)
    assert c.gp_X.shape == (37, D) and c.hyp.shape[0] == c.S == 2
    t_warp.check_gp(ctx, c, c.name)
    t_warp.check_box(ctx, c, c.name)
    t_warp.check_box_philox(t_warp.route(ctx, c), D, np.ravel(c.plb_orig), np.ravel(c.pub_orig), t_warp.N_BOX, two_sample=False)


# ---------------------------------------------------------------------------------------------- mode
def mode_vp(ctx, D):
    """A five-component posterior behind a rotated and scaled transformer with logit dimensions (test_mode_gpu._roto_vp)."""
    vp, pt = t_mode._roto_vp(D, 5, D)
    vp.ctx = ctx
    return vp, pt


@pytest.mark.parametrize("orig", [False, True])
@pytest.mark.parametrize("D", MODE_D)
def test_mode_philox(ctx, D, orig, monkeypatch):
    vp, pt = mode_vp(ctx, D)
    obj = mh.Objective(vp.mu, vp.sigma, vp.lambd, vp.w, pt, orig)
    x, f = t_mode.check_philox_mode(vp, pt, obj, orig, monkeypatch)
    assert x.shape == (D,) and np.isfinite(f) and vp.mode_info["device"]


@pytest.mark.parametrize("orig", [False, True])
@pytest.mark.parametrize("D", MODE_D)
def test_mode_start_selection(ctx, D, orig):
    vp, _ = mode_vp(ctx, D)
    t_mode.check_start_selection(ctx, vp, orig, 65)
