"""Stand-ins and cases of the ``train_gp`` mirror's tests (pyvbmc_amd/gaussian_process_train.py).  TEST INFRASTRUCTURE shared by
tests/test_train_gp_host.py, tests/test_gp_fit_gpu.py's end-to-end test and tools/train_gp_golden.py, which records
tests/golden/train_gp.npz by giving THE SAME plain dicts to the reference's functions.

Everything is a plain dict or a small namespace: the functions under test read ``options[...]``, ``optim_state[...]``,
``iteration_history[...]`` and a function logger's ``X``, ``y``, ``S``, ``X_flag``, ``noise_flag``, ``fun_eval_time``."""
from types import SimpleNamespace

import numpy as np

SAMPLERS = ("slicesample", "npv", "mala", "slicelite", "splitsample", "covsample", "laplace")
MEANS = ("zero", "const", "negquad")
D, N = 2, 63
P_OF = {"zero": D + 2, "const": D + 3, "negquad": D + 3 + 2 * D}


def options(**kw):
    o = dict(hpd_frac=0.8, tol_gp_noise=np.sqrt(1e-5), noise_size=[], upper_gp_length_factor=0.5, gp_quadratic_mean_bound=True,
             tol_sd=0.1, gp_length_prior_mean=np.sqrt(D / 6), gp_length_prior_std=0.5 * np.log(1e3), ns_gp_max=80,
             ns_gp_max_warmup=8, ns_gp_max_main=np.inf, stable_gp_sampling=200 + 10 * D, stable_gp_vp_k=np.inf,
             stable_gp_samples=0, gp_sample_thin=5, gp_train_init_method="rand", gp_tol_opt=1e-5, gp_tol_opt_mcmc=1e-2,
             gp_hyp_sampler="slicesample", gp_sample_widths=5, cov_sample_thresh=10, gp_train_n_init=1024,
             gp_train_n_init_final=64, fun_eval_start=10, max_fun_evals=50 * (2 + D), gp_retrain_threshold=1,
             weighted_hyp_cov=True, hyp_run_weight=0.9, fun_evals_per_iter=5, tol_skl=0.01 * np.sqrt(D), tol_cov_weight=0)
    o.update(kw)
    return o


def optim_state(**kw):
    s = dict(iter=0, N=N, n_eff=N, warmup=True, vp_K=2, stop_sampling=0, recompute_var_post=True, uncertainty_handling_level=0,
             gp_mean_fun="negquad", gp_cov_fun=1, gp_noise_fun=[1, 0, 0])
    s.update(kw)
    return s


def data(noisy=False, seed=11):
    """(X, y, S): N points around a bump in D = 2; S (noise standard deviations) where ``noisy``."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (N, D))
    y = (-0.5 * np.sum((X / np.array([0.7, 1.3])) ** 2, axis=1) + 0.05 * rng.standard_normal(N)).reshape(-1, 1)
    S = 0.1 + 0.05 * rng.random((N, 1)) if noisy else None
    return X, y, S


def logger(noisy=False, spare=5):
    """A function-logger stand-in holding ``data`` in its first rows and ``spare`` unused ones."""
    X, y, S = data(noisy)
    pad = lambda a: np.vstack([a, np.full((spare, a.shape[1]), np.nan)])
    flag = np.concatenate([np.ones(N, dtype=bool), np.zeros(spare, dtype=bool)])
    return SimpleNamespace(X=pad(X), y=pad(y), S=None if S is None else pad(S), X_flag=flag, noise_flag=noisy,
                           fun_eval_time=pad(np.full((N, 1), 1e-5)), n_evals=pad(np.ones((N, 1))))


PLB, PUB = np.full((1, D), -1.5), np.full((1, D), 1.5)


def history(n_iter, n_samples=4, P=P_OF["negquad"], seed=3):
    """An iteration history of ``n_iter`` past iterations: ``r_index``, ``sKL``, ``gp_hyp_full`` (samples, P) -- no ``gp``."""
    rng = np.random.default_rng(seed)
    return dict(r_index=np.array([np.inf, 3.0, 0.5, 1.7, 0.2, 0.9][:n_iter] + [0.8] * max(n_iter - 6, 0)),
                sKL=np.array([np.inf] + [0.5 / (i + 1) for i in range(max(n_iter - 1, 0))] + [0.01]),
                gp_hyp_full=[0.3 * rng.standard_normal((n_samples, P)) - 1.0 for _ in range(n_iter)])


def training_option_cases():
    """name -> (optim_state, iteration_history, options, hyp_dict, gp_s_N) for ``_get_gp_training_options`` /
    ``_get_hyp_cov``: every sampler name; the ``opts_N`` / ``init_N`` / ``burn`` branches by ``recompute_var_post``, the
    reliability index and ``gp_s_N = 0``; the weighted covariance with and without its early break, and the running one."""
    P = P_OF["negquad"]
    run_cov = np.diag(np.linspace(0.01, 0.4, P))
    out = {}
    for s in SAMPLERS:
        out[f"first_{s}"] = (optim_state(), history(0), options(gp_hyp_sampler=s), dict(run_cov=None), 8)
        out[f"later_{s}"] = (optim_state(iter=3, recompute_var_post=False, n_eff=40), history(3),
                             options(gp_hyp_sampler=s, gp_retrain_threshold=2.0), dict(run_cov=run_cov), 6)
    out["laplace_small"] = (optim_state(iter=2, n_eff=20), history(2), options(gp_hyp_sampler="laplace"), dict(run_cov=run_cov), 5)
    out["cov_over_thresh"] = (optim_state(iter=2, n_eff=40), history(2), options(gp_hyp_sampler="covsample", cov_sample_thresh=1.0),
                              dict(run_cov=run_cov), 5)
    out["mala_step"] = (optim_state(iter=2, gp_mala_step_size=0.3), history(2), options(gp_hyp_sampler="mala"),
                        dict(run_cov=run_cov), 5)
    out["recompute_no_samples"] = (optim_state(iter=3), history(3), options(), dict(run_cov=run_cov), 0)
    out["retrain_samples"] = (optim_state(iter=3, recompute_var_post=False), history(3), options(), dict(run_cov=run_cov), 4)
    out["retrain_no_samples"] = (optim_state(iter=3, recompute_var_post=False), history(3), options(), dict(run_cov=run_cov), 0)
    out["no_retrain_unreliable"] = (optim_state(iter=4, recompute_var_post=False), history(4), options(), dict(run_cov=run_cov), 4)
    out["no_retrain_unreliable_no_samples"] = (optim_state(iter=4, recompute_var_post=False), history(4), options(),
                                               dict(run_cov=run_cov), 0)
    out["running_cov"] = (optim_state(iter=5), history(5), options(weighted_hyp_cov=False), dict(run_cov=run_cov), 4)
    out["weighted_break"] = (optim_state(iter=6), history(6), options(tol_cov_weight=0.3), dict(run_cov=run_cov), 4)
    out["no_widths"] = (optim_state(iter=3), history(3), options(gp_sample_widths=0), dict(run_cov=run_cov), 4)
    out["late_n_eff"] = (optim_state(iter=3, n_eff=150), history(3), options(), dict(run_cov=run_cov), 4)
    return out


def gp_hyp_cases():
    """name -> (optim_state, options, noisy) for ``_gp_hyp``: the three means, ``uncertainty_handling_level`` 0 (with and
    without ``noise_size``) and 2, and the ``stop_sampling`` rules."""
    out = {}
    for m in MEANS:
        out[f"mean_{m}"] = (optim_state(gp_mean_fun=m), options(), False)
    out["noise_size"] = (optim_state(), options(noise_size=0.02), False)
    out["noise_size_small"] = (optim_state(), options(noise_size=1e-6), False)
    out["level2"] = (optim_state(uncertainty_handling_level=2, gp_noise_fun=[1, 1, 0]), options(noise_size=0.02), True)
    out["no_quadratic_bound"] = (optim_state(), options(gp_quadratic_mean_bound=False), False)
    out["no_length_factor"] = (optim_state(), options(upper_gp_length_factor=0), False)
    out["main_phase"] = (optim_state(warmup=False), options(), False)
    out["stable_by_N"] = (optim_state(), options(stable_gp_sampling=N, stable_gp_samples=3), False)
    out["stable_by_K"] = (optim_state(vp_K=7), options(stable_gp_vp_k=5, stable_gp_samples=2), False)
    out["stopped"] = (optim_state(stop_sampling=40), options(stable_gp_samples=1), False)
    return out
