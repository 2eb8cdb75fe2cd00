"""``FunctionLogger``: evaluates the target, keeps every evaluation in original and transformed space, and is what
``active_sample``, ``train_gp``, ``whitening`` and ``gp.training_data`` read.  Mirror of the reference's
``function_logger/function_logger.py`` (:36-421; line numbers below cite that file): attributes, growth of the arrays,
repeated points, the log-Jacobian term and the errors are the reference's.

Arrays (``cache_size`` rows at first, grown by half when full): ``X_orig``, ``y_orig``, ``X``, ``y``, ``n_evals``,
``fun_eval_time``, ``S`` under noise; ``X_flag`` marks the rows in the training set, ``Xn`` the last filled row.  A point
evaluated again updates its row: the running mean of ``y_orig``, or under noise the precision-weighted mean with the
combined ``S``.
"""
import time

import numpy as np

_ROW_FILL = (("X_orig", np.nan), ("y_orig", np.nan), ("X", np.nan), ("y", np.nan), ("S", np.nan),
             ("fun_eval_time", np.nan), ("n_evals", 0))


class FunctionLogger:
    def __init__(self, fun, D, noise_flag, uncertainty_handling_level, cache_size=500, parameter_transformer=None):
        self.fun = fun
        self.D = D
        self.noise_flag = noise_flag
        self.uncertainty_handling_level = uncertainty_handling_level
        self.transform_parameters = parameter_transformer is not None
        self.parameter_transformer = parameter_transformer
        self.func_count = 0
        self.cache_count = 0
        self.X_orig = np.full([cache_size, D], np.nan)
        self.y_orig = np.full([cache_size, 1], np.nan)
        self.X = np.full([cache_size, D], np.nan)
        self.y = np.full([cache_size, 1], np.nan)
        self.n_evals = np.full([cache_size, 1], 0)
        if noise_flag:
            self.S = np.full([cache_size, 1], np.nan)
        self.Xn = -1
        self.X_flag = np.full((cache_size,), False, dtype=bool)
        self.y_max = float("-Inf")
        self.fun_eval_time = np.full([cache_size, 1], np.nan)
        self.total_fun_eval_time = 0

    # ---- the two entry points
    def _point(self, x):
        """``(x as a 1-D row, the same point in original space)`` (:102-117)."""
        x = np.asarray(x)
        shape = x.shape
        if x.ndim > 1:
            x = x.squeeze()
        if x.ndim == 0:
            x = np.atleast_1d(x)
        if x.size != x.shape[0]:
            raise ValueError(f"Input should be one-dimensional but has shape {shape}.")
        if self.transform_parameters:
            return x, self.parameter_transformer.inverse(np.reshape(x, (1, x.shape[0])))[0]
        return x, x

    def _check(self, f_val_orig, f_sd):
        if not np.isscalar(f_val_orig) or not np.isfinite(f_val_orig) or not np.isreal(f_val_orig):
            raise ValueError("FunctionLogger:InvalidFuncValue: The returned function value must be a finite real-valued "
                             f"scalar (returned value {f_val_orig})")
        if self.noise_flag and (not np.isscalar(f_sd) or not np.isfinite(f_sd) or not np.isreal(f_sd) or f_sd <= 0.0):
            raise ValueError("FunctionLogger:InvalidNoiseValue The returned estimated SD (second function output) must be "
                             f"a finite, positive real-valued scalar (returned SD: {f_sd})")

    def __call__(self, x):
        """Evaluate the target at ``x`` (transformed space, (1, D) or (D,)) and record it: ``(f_val, f_sd, idx)``."""
        x, x_orig = self._point(x)
        t0 = time.perf_counter()
        try:
            if self.noise_flag and self.uncertainty_handling_level == 2:
                f_val_orig, f_sd = self.fun(x_orig)
            else:
                f_val_orig = self.fun(x_orig)
                f_sd = 1 if self.noise_flag else None
            if isinstance(f_val_orig, np.ndarray):
                f_val_orig = f_val_orig.item()  # (only an array of size 1 has one)
        except Exception as err:
            err.args += ("FunctionLogger:FuncError Error in executing the logged function with input: " + str(x_orig),)
            raise
        funtime = time.perf_counter() - t0
        if not np.isscalar(f_val_orig) and np.size(f_val_orig) == 1:
            f_val_orig = np.array(f_val_orig).flat[0]
        self._check(f_val_orig, f_sd)
        self.func_count += 1
        f_val, idx = self._record(x_orig, x, f_val_orig, f_sd, funtime)
        return f_val, f_sd, idx

    def add(self, x, f_val_orig, f_sd=None, fun_eval_time=np.nan):
        """Record a value evaluated elsewhere (the starting cache): ``(f_val, f_sd, idx)``."""
        x, x_orig = self._point(x)
        f_sd = (1 if f_sd is None else f_sd) if self.noise_flag else None
        self._check(f_val_orig, f_sd)
        self.cache_count += 1
        f_val, idx = self._record(x_orig, x, f_val_orig, f_sd, fun_eval_time)
        return f_val, f_sd, idx

    def finalize(self):
        """Drop the unused rows (:276-290)."""
        n = self.Xn + 1
        for name in ("X_orig", "y_orig", "X", "y", "X_flag", "fun_eval_time") + (("S",) if self.noise_flag else ()):
            setattr(self, name, getattr(self, name)[:n])

    # ---- storage
    def _expand_arrays(self, resize_amount=None):
        if resize_amount is None:
            resize_amount = int(np.max((np.ceil(self.Xn / 2), 1)))
        for name, fill in _ROW_FILL:
            a = getattr(self, name, None)
            if a is not None:
                setattr(self, name, np.append(a, np.full([resize_amount, a.shape[1]], fill), axis=0))
        self.X_flag = np.append(self.X_flag, np.full((resize_amount,), False, dtype=bool))

    def _record(self, x_orig, x, f_val_orig, f_sd, fun_eval_time):
        """:331-421."""
        duplicate_flag = (self.X == x).all(axis=1)
        if np.any(duplicate_flag):
            if np.sum(duplicate_flag) > 1:
                raise ValueError("More than one match for duplicate entry.")
            idx = np.argwhere(duplicate_flag)[0, 0]
            N = self.n_evals[idx]
            if f_sd is not None:
                tau_n = 1 / self.S[idx] ** 2
                tau_1 = 1 / f_sd**2
                self.y_orig[idx] = (tau_n * self.y_orig[idx] + tau_1 * f_val_orig) / (tau_n + tau_1)
                self.S[idx] = 1 / np.sqrt(tau_n + tau_1)
            else:
                self.y_orig[idx] = (N * self.y_orig[idx] + f_val_orig) / (N + 1)
            # (a view of the row, as in the reference: the Jacobian term added below lands in y_orig as well, :388-391)
            f_val = self.y_orig[idx]
            if self.transform_parameters:
                f_val += self.parameter_transformer.log_abs_det_jacobian(x)
            self.y[idx] = f_val
            self.fun_eval_time[idx] = (N * self.fun_eval_time[idx] + fun_eval_time) / (N + 1)
            self.n_evals[idx] += 1
            return f_val, idx
        self.Xn += 1
        if self.Xn > self.X_orig.shape[0] - 1:
            self._expand_arrays()
        if not np.isnan(fun_eval_time):
            self.fun_eval_time[self.Xn] = fun_eval_time
            self.total_fun_eval_time += fun_eval_time
        self.X_orig[self.Xn] = x_orig
        self.X[self.Xn] = x
        self.y_orig[self.Xn] = f_val_orig
        f_val = f_val_orig
        if self.transform_parameters:
            f_val += self.parameter_transformer.log_abs_det_jacobian(np.reshape(x, (1, x.shape[0])))[0]
        self.y[self.Xn] = f_val
        if f_sd is not None:
            self.S[self.Xn] = f_sd
        self.X_flag[self.Xn] = True
        self.n_evals[self.Xn] += 1
        self.y_max = np.nanmax(self.y[self.X_flag])
        return f_val, self.Xn


__all__ = ["FunctionLogger"]
