"""`GaussianProcessRegressor` with the estimator seam the reference calls, computed on MI355X.

Drop-in for the object the reference stores under `'gp_model'` (`src/px4/simple_gp.py:170-177`,
`src/px4/train_gp_offline.py:188-194`): same constructor arguments, `fit(X, y)`,
`predict(X, return_std=False)`, `log_marginal_likelihood(theta, eval_gradient)`, attributes
`kernel_`, `X_train_`, `y_train_`, `alpha_`, `L_`, `n_features_in_`,
`log_marginal_likelihood_value_`, and it pickles.  The arithmetic follows scikit-learn 1.7.2's
`GaussianProcessRegressor` (Rasmussen & Williams Alg. 2.1; `sklearn/gaussian_process/_gpr.py`)
but every O(N^2)/O(N^3) step runs in the HIP kernels behind libgpk:

    K1 gram -> K2 potrf -> K3 potrs -> K6 lml / gradient      (fit, per optimiser evaluation)
    K4 fused mean, K5 variance (trsm + column norms)           (predict)

There is no CPU fallback: without the GPU library `fit`/`predict` raise.
"""
from __future__ import annotations

import copy
import warnings

import numpy as np
import scipy.optimize

from .device import DeviceGP, check_queries, get_backend
from .kernels import RBF, ConstantKernel, Kernel, KernelComponents, WhiteKernel  # noqa: F401
from ._lib import NotPositiveDefinite

LOG_2PI = float(np.log(2.0 * np.pi))


def _rng_from(random_state):
    """`sklearn.utils.check_random_state` semantics (`sklearn/gaussian_process/_gpr.py:249`):
    None -> numpy's global RandomState (so `np.random.seed(0)` pins the restarts, as in the
    reference's trainer), int -> fresh RandomState, RandomState -> itself."""
    if random_state is None or random_state is np.random:
        return np.random.mtrand._rand
    if isinstance(random_state, (int, np.integer)):
        return np.random.RandomState(int(random_state))
    return random_state


def cholesky_draws(mean, cov, n_samples=1, random_state=0, active=None):
    """Draws from B independent Gaussians over the same M rows: mean (M, B), cov (M, M, B) -> (M, B, n_samples).  Pure NumPy.

    ONE z = standard_normal((B, M, n_samples)) from `_rng_from(random_state)`, then samples[:, b, :] = mean[:, b, None] +
    cholesky(cov[..., b]) @ z[b]: a stable function of the covariance, unlike `multivariate_normal`'s SVD draw (repeated
    singular values let a 1e-12 perturbation of the covariance rotate it).  A covariance that does not factorise gets
    1e-10 * max(diag) added to its diagonal once; a second failure raises `np.linalg.LinAlgError`.  active: boolean (B,) -
    models marked False are skipped and return zeros (z is drawn for all B either way, so a model's draw does not depend on
    which others are present)."""
    mean = np.asarray(mean, dtype=np.float64)
    cov = np.asarray(cov, dtype=np.float64)
    M, B = mean.shape
    z = _rng_from(random_state).standard_normal((B, M, n_samples))
    out = np.zeros((M, B, n_samples))
    for b in range(B):
        if active is not None and not active[b]:
            continue
        c = cov[..., b]
        try:
            L = np.linalg.cholesky(c)
        except np.linalg.LinAlgError:
            L = np.linalg.cholesky(c + 1e-10 * np.max(np.diag(c)) * np.eye(M))
        out[:, b, :] = mean[:, b, None] + L @ z[b]
    return out


def constrained_optimization(optimizer, obj, theta0, bounds):
    """`sklearn/gaussian_process/_gpr.py:654-670`: one run of the optimiser on obj(theta) -> (value, gradient), both to be
    minimised, from theta0 within bounds; returns (theta, value).  Shared with `SparseGP.train`."""
    if optimizer == "fmin_l_bfgs_b":
        res = scipy.optimize.minimize(obj, theta0, method="L-BFGS-B", jac=True, bounds=bounds)
        if res.status != 0 and "CONVERGENCE" not in str(res.message):
            warnings.warn(f"lbfgs failed to converge (status={res.status}): {res.message}")
        return res.x, res.fun
    if callable(optimizer):
        return optimizer(obj, theta0, bounds=bounds)
    raise ValueError(f"Unknown optimizer {optimizer}.")


class GaussianProcessRegressor:
    def __init__(self, kernel=None, *, alpha=1e-10, optimizer="fmin_l_bfgs_b", n_restarts_optimizer=0,
                 normalize_y=False, copy_X_train=True, n_targets=None, random_state=None, device=None,
                 predict_dtype="float64", var_method="auto"):
        self.kernel = kernel
        self.alpha = alpha
        self.optimizer = optimizer
        self.n_restarts_optimizer = n_restarts_optimizer
        self.normalize_y = normalize_y
        self.copy_X_train = copy_X_train
        self.n_targets = n_targets
        self.random_state = random_state
        self.device = device
        self.predict_dtype = predict_dtype
        self.var_method = var_method      # 'auto' | 'inverse' | 'solve' | 'inverse_split' | 'inverse_split2' (fp32 only): DeviceGP.predict_var_dev
        self.fp32_gate = True             # predict_dtype="float32": route ill-conditioned models / tiny variances to fp64
        self._dev = None

    # ------------------------------------------------------------------ fit
    def fit(self, X, y):
        """`sklearn/gaussian_process/_gpr.py:225-365`."""
        if self.kernel is None:  # sklearn default: C(1.0, fixed) * RBF(1.0, fixed)
            self.kernel_ = ConstantKernel(1.0, constant_value_bounds="fixed") * RBF(1.0, length_scale_bounds="fixed")
        else:
            self.kernel_ = copy.deepcopy(self.kernel)
        self._rng = _rng_from(self.random_state)
        X = np.array(X, dtype=np.float64, ndmin=2)
        y = np.asarray(y, dtype=np.float64)
        if X.shape[0] != y.shape[0]:
            raise ValueError("X and y have inconsistent numbers of samples")
        if not (np.isfinite(X).all() and np.isfinite(y).all()):
            raise ValueError("Input contains NaN or infinity")
        if np.iterable(self.alpha):
            raise ValueError("per-sample alpha is not supported by the MI355X path")
        self._y_1d = y.ndim == 1
        y2 = y.reshape(X.shape[0], -1)
        if self.n_targets is not None and y2.shape[1] != self.n_targets:
            raise ValueError("The number of targets seen in `y` is different from the parameter `n_targets`.")
        # normalise targets: population std, zero std -> 1   (_gpr.py:271-282)
        if self.normalize_y:
            self._y_train_mean = np.mean(y2, axis=0)
            std = np.std(y2, axis=0)
            self._y_train_std = np.where(std < 10 * np.finfo(np.float64).eps, 1.0, std)
            yn = (y2 - self._y_train_mean) / self._y_train_std
        else:
            self._y_train_mean = np.zeros(y2.shape[1])
            self._y_train_std = np.ones(y2.shape[1])
            yn = y2.copy()
        self.X_train_ = X.copy() if self.copy_X_train else X
        self._yn = yn
        self.y_train_ = yn[:, 0].copy() if self._y_1d else yn
        self.n_features_in_ = X.shape[1]
        self._comp_check()
        self._dev = DeviceGP(self.X_train_, yn, get_backend(self.device))

        if self.optimizer is not None and self.kernel_.n_dims > 0:
            def obj(theta):
                lml, grad = self._lml_on_device(theta, eval_gradient=True)
                return -lml, -grad

            bounds = self.kernel_.bounds
            starts = [self.kernel_.theta]
            if self.n_restarts_optimizer > 0:
                if not np.isfinite(bounds).all():
                    raise ValueError("Multiple optimizer restarts (n_restarts_optimizer>0) requires that all "
                                     "bounds are finite.")
                # (scikit-learn draws a restart's start after the previous run, _gpr.py:316-327 - from a generator the runs do
                # not touch: drawing them up front gives the same starts)
                starts += [self._rng.uniform(bounds[:, 0], bounds[:, 1]) for _ in range(self.n_restarts_optimizer)]
            optima = self._optimise_from(starts, bounds, obj, yn)
            vals = [o[1] for o in optima]
            self.kernel_.theta = optima[int(np.argmin(vals))][0]
            self.log_marginal_likelihood_value_ = -float(np.min(vals))
            self._dev.release_grad_buffers()
            lml_from_final_factor = False
        else:
            # fixed theta: the reference evaluates the LML (one Cholesky) and then factorises again for
            # prediction (_gpr.py:339-349); here the one factorisation below serves both
            lml_from_final_factor = True

        # final factorisation at the selected theta (_gpr.py:343-364); not-PD raises here
        dev = self._dev
        try:
            logdet_half, quad = self._refactor()
        except NotPositiveDefinite as exc:
            exc.args = (f"The kernel, {self.kernel_}, is not returning a positive definite matrix. Try gradually "
                        "increasing the 'alpha' parameter of your GaussianProcessRegressor estimator.",) + exc.args
            raise
        if lml_from_final_factor:
            self.log_marginal_likelihood_value_ = float(
                np.sum(-0.5 * quad - logdet_half - 0.5 * dev.N * LOG_2PI))
        self._alpha_host = None
        self._L_host = None
        return self

    # the restarts run side by side while all their device models together stay below this many bytes ...
    CONCURRENT_RESTART_BYTES = 48e9
    # ... and while one evaluation leaves most of the chip idle: from ~8000 rows on it fills it and two chains side by side only
    # take each other's matrix pipe (fit with one restart, side by side / one after the other: N = 6000 244 / 255 ms,
    # 8000 562 / 555, 10 000 1091 / 1058: profiles/r05_train_restarts_ab.log)
    CONCURRENT_RESTART_MAX_NP = 7168

    def _optimise_from(self, starts, bounds, obj, yn):
        """One optimiser run per start, results in the order of `starts`.  The runs are independent (same data, their own
        start): with more than one they run side by side, each on its own libgpk handle, stream and scratch model from its own
        host thread - at the reference's sizes an evaluation is a chain of latency-bound launches that leaves most of the
        chip idle, and two chains interleave.  Same results as one after the other (every run is deterministic)."""
        n = len(starts)
        per_run = 3.3 * self._dev.Np * self._dev.Np * 8.0
        if (n == 1 or not getattr(self, "concurrent_restarts", True) or n * per_run > self.CONCURRENT_RESTART_BYTES
                or self._dev.Np > self.CONCURRENT_RESTART_MAX_NP):
            return [self._constrained_optimization(obj, t0, bounds) for t0 in starts]
        import torch
        from concurrent.futures import ThreadPoolExecutor
        from .device import worker_backends
        workers = worker_backends(self._dev.be.device_index, n)
        torch.cuda.current_stream(self._dev.be.device).synchronize()

        def run(i):
            be, stream = workers[i]
            with torch.cuda.stream(stream):
                dev = DeviceGP(self.X_train_, yn, be)

                def obj_i(theta):
                    lml, grad = self._lml_on_device(theta, True, dev)
                    return -lml, -grad

                out = self._constrained_optimization(obj_i, starts[i], bounds)
                stream.synchronize()
            return out

        with ThreadPoolExecutor(max_workers=n) as ex:
            return list(ex.map(run, range(n)))

    def _comp_check(self):
        comp = self.kernel_.components()
        comp.ls_vector(self.n_features_in_)
        return comp

    def _constrained_optimization(self, obj, theta0, bounds):
        return constrained_optimization(self.optimizer, obj, theta0, bounds)

    # ------------------------------------------------------------------ LML
    def _lml_on_device(self, theta, eval_gradient, dev=None):
        """One evaluation of `_gpr.py:537-652` on the GPU: K1, K2, K3, K6a (+ K^-1 and K6b).  Works on `dev`
        (default: the estimator's own device model, whose factor it overwrites - what `fit` wants)."""
        dev = dev if dev is not None else self._dev
        kern = self.kernel_.clone_with_theta(theta)
        comp = kern.components()
        D = self.n_features_in_
        N = dev.N
        if dev.Np <= dev.INVERSE_EAGER_NP and D <= 16:
            # the whole evaluation as one chain of launches with one synchronisation (gpk_lml_eval)
            try:
                logdet_half, quad, g = dev.lml_eval(comp.ls_vector(D), comp.sf2, (comp.noise or 0.0) + float(self.alpha),
                                                    comp.noise or 0.0, eval_gradient)
            except NotPositiveDefinite:
                return (-np.inf, np.zeros_like(theta)) if eval_gradient else -np.inf
            lml = float(np.sum(-0.5 * quad - logdet_half - 0.5 * N * LOG_2PI))
            return (lml, comp.map_gradient(g, D)) if eval_gradient else lml
        try:
            dev.factorize(comp.ls_vector(D), comp.sf2, (comp.noise or 0.0) + float(self.alpha))
        except NotPositiveDefinite:
            return (-np.inf, np.zeros_like(theta)) if eval_gradient else -np.inf
        dev.solve_alpha()
        logdet_half, quad = dev.lml_terms()
        lml = float(np.sum(-0.5 * quad - logdet_half - 0.5 * N * LOG_2PI))
        if not eval_gradient:
            return lml
        g = dev.lml_grad(comp.noise or 0.0)
        return lml, comp.map_gradient(g, D)

    def log_marginal_likelihood(self, theta=None, eval_gradient=False, clone_kernel=True):
        if theta is None:
            if eval_gradient:
                raise ValueError("Gradient can only be evaluated for theta!=None")
            return self.log_marginal_likelihood_value_
        if not hasattr(self, "X_train_"):
            raise RuntimeError("This GaussianProcessRegressor instance is not fitted yet.")
        theta = np.asarray(theta, dtype=np.float64)
        # Non-mutating, as in scikit-learn (_gpr.py:537-652 works on fresh arrays): the trial theta is factorised
        # in a scratch device model, so the fitted factor in HBM - which a predict() on another thread may be
        # reading - is never touched.  The scratch (a second N x N matrix) is kept for the next evaluation;
        # `release_lml_scratch()` frees it.
        scratch = getattr(self, "_lml_dev", None)
        if scratch is None or scratch.N != self.X_train_.shape[0]:
            scratch = self._lml_dev = DeviceGP(self.X_train_, self._yn, get_backend(self.device))
        out = self._lml_on_device(theta, eval_gradient, scratch)
        if not clone_kernel:
            self.kernel_.theta = theta
        return out

    def release_lml_scratch(self):
        self._lml_dev = None

    # ------------------------------------------------------------------ predict
    def predict(self, X, return_std=False, return_cov=False):
        """`sklearn/gaussian_process/_gpr.py:367-496`.

        return_cov=True returns (y_mean, y_cov), y_cov of shape (M, M) - (M, M, P) for 2-D targets with P > 1 - scaled by
        the target std squared as scikit-learn does.  The covariance is always computed by the fp64 kernels (there is no
        fp32 covariance): a model with predict_dtype="float32" serves it, and the mean that goes with it, in fp64.  One call
        takes at most VAR_PANEL_MAX queries and a V = L^-1 K*^T that fits VAR_PANEL_BYTES (ValueError otherwise)."""
        if return_std and return_cov:
            raise RuntimeError("At most one of return_std or return_cov can be requested.")
        X = check_queries(X)               # scikit-learn's input validation (_gpr.py:404-412 -> check_array)
        if not hasattr(self, "X_train_"):  # prior (unfitted) prediction, _gpr.py:416-440
            n_t = self.n_targets if self.n_targets is not None else 1
            kern = self.kernel if self.kernel is not None else (
                ConstantKernel(1.0, constant_value_bounds="fixed") * RBF(1.0, length_scale_bounds="fixed"))
            comp = kern.components()
            mean = np.zeros((X.shape[0], n_t)).squeeze()
            if return_cov:                 # kernel(X), _gpr.py:425-431: built on the device by the Gram kernel
                from .device import prior_cov
                cov = prior_cov(X, comp.ls_vector(X.shape[1]), comp.sf2, comp.noise or 0.0, self.device)
                if n_t > 1:
                    cov = np.repeat(np.expand_dims(cov, -1), repeats=n_t, axis=-1)
                return mean, cov
            if return_std:
                var = np.full((X.shape[0], n_t), comp.sf2 + (comp.noise or 0.0)).squeeze()
                return mean, np.sqrt(var)
            return mean
        self._ensure_device()
        dev = self._dev
        if return_cov:
            return self._predict_cov(X)
        if (self.predict_dtype != "float32" and self.var_method in ("auto", "inverse")
                and dev.host_path_ok(X.shape[0], return_std)):
            # small batches (the control loop's 1..25 rows): one C call, one synchronisation
            kss = None
            if return_std:
                comp = self.kernel_.components()
                kss = comp.sf2 + (comp.noise or 0.0)
            mean, var = dev.predict_host(X, self._y_train_mean, self._y_train_std, kss, 0.0)
            if not return_std:
                return mean[:, 0] if mean.shape[1] == 1 else mean
            var = np.outer(var, self._y_train_std ** 2)
            if mean.shape[1] == 1:
                mean, var = mean[:, 0], var[:, 0]
            return mean, np.sqrt(var)
        import torch
        # fp32 serving is gated (DeviceGP.predict_gated_dev): a model whose mean would leave the stated 1e-4 goes through
        # the fp64 kernels, and so do single queries whose fp32 variance is too small a fraction of the prior's to carry a
        # 1e-3-accurate standard deviation
        gated = getattr(self, "fp32_gate", True)
        kss = None
        if return_std:
            comp = self.kernel_.components()
            kss = comp.sf2 + (comp.noise or 0.0)        # kernel_.diag(X): RBF diag + WhiteKernel level
        mean_d, var_d = dev.predict_gated_dev(X, self._y_train_mean, self._y_train_std, kss, 0.0, self.predict_dtype,
                                              self.var_method, gated)   # variance clipped at 0 (_gpr.py:479-485)
        if not return_std:
            mean = mean_d.double().cpu().numpy()       # float64 whatever dtype served it, as scikit-learn returns
            return mean[:, 0] if mean.shape[1] == 1 else mean
        both = torch.cat([mean_d.double(), var_d[:, None]], dim=1).cpu().numpy()     # one device->host copy
        mean, var = both[:, :-1], both[:, -1]
        var = np.outer(var, self._y_train_std ** 2)
        if mean.shape[1] == 1:
            mean, var = mean[:, 0], var[:, 0]
        return mean, np.sqrt(var)

    def _predict_cov(self, X):
        """Fitted model, return_cov=True: `_gpr.py:441-469` - the mean and Sigma = kernel_(X) - V^T V, un-normalised."""
        dev = self._dev
        comp = self.kernel_.components()
        noise = comp.noise or 0.0
        M = X.shape[0]
        dev.cov_panel_check(M)
        method = {"inverse": "inverse", "solve": "solve"}.get(self.var_method, "auto")
        if method != "solve" and dev.host_path_ok(M, True):
            # small batches (the MPC horizon): one C call, one synchronisation; up to 32 rows two launches
            mean, cov = dev.predict_cov_host(X, self._y_train_mean, self._y_train_std, noise)
        else:
            q = dev._as_queries(X, __import__("torch").float64)
            mean = dev.predict_mean_dev(q, self._y_train_mean, self._y_train_std, "float64").cpu().numpy()
            cov = dev.predict_cov_dev(q, noise, method).contiguous().cpu().numpy()
        if mean.shape[1] == 1:
            mean = mean[:, 0]
        # undo normalisation (_gpr.py:462-467): y_cov[i, j, p] = Sigma[i, j] y_std[p]^2, squeezed for one output
        std2 = self._y_train_std ** 2
        if std2.shape[0] == 1:
            return mean, cov * std2[0]
        return mean, cov[:, :, None] * std2[None, None, :]

    def predict_jacobian(self, X, return_var=False):
        """Posterior mean and its Jacobian with respect to the inputs - the first-order terms a model-predictive controller
        linearises with - and, with return_var=True, the posterior variance and its input gradient.  scikit-learn has no such
        call; both gradients are the closed forms of the RBF kernel, evaluated on the GPU (K8):

            dmean[m, p, d] = y_std[p] sum_j k(x_m, x_j) (x_jd - x_md) / ls_d^2 alpha_jp
            dvar[m, p, d]  = -2 y_std[p]^2 sum_j k(x_m, x_j) (x_jd - x_md) / ls_d^2 (K^-1 k_m)_j

        Returns (y_mean, dmean) or (y_mean, dmean, y_var, dvar).  Shapes follow `predict`'s squeezing: y_mean (M, P) / (M,),
        dmean (M, P, D) / (M, D) for one target; y_var = predict(X, return_std=True)[1] ** 2 (clipped at 0 like it), shaped
        as y_mean; dvar shaped as dmean - the gradient of the unclipped variance.  The gradient of the standard deviation is
        dvar / (2 std) (not returned: it is singular where std = 0).  Always computed by the fp64 kernels: a model with
        predict_dtype="float32" serves them, and the mean and variance that go with them, in fp64.  Same input validation as
        `predict`; an unfitted model returns the prior mean / variance and zero gradients."""
        X = check_queries(X)
        M, D = X.shape
        if not hasattr(self, "X_train_"):  # prior: constant mean and variance, zero gradients
            n_t = self.n_targets if self.n_targets is not None else 1
            kern = self.kernel if self.kernel is not None else (
                ConstantKernel(1.0, constant_value_bounds="fixed") * RBF(1.0, length_scale_bounds="fixed"))
            comp = kern.components()
            mean = np.zeros((M, n_t))
            dmean = np.zeros((M, n_t, D))
            if n_t == 1:
                mean, dmean = mean[:, 0], dmean[:, 0]
            if not return_var:
                return mean, dmean
            return mean, dmean, np.full(mean.shape, comp.sf2 + (comp.noise or 0.0)), np.zeros(dmean.shape)
        self._ensure_device()
        dev = self._dev
        kss = None
        if return_var:
            comp = self.kernel_.components()
            kss = comp.sf2 + (comp.noise or 0.0)
        if dev.host_path_ok(M, return_var):
            # small batches (the MPC horizon): one C call, one synchronisation; up to 32 rows one launch (three with the variance)
            mean, var, dmean, dvar = dev.predict_grad_host(X, self._y_train_mean, self._y_train_std, kss, 0.0)
        else:
            import torch
            q = dev._as_queries(X, torch.float64)
            mean = dev.predict_mean_dev(q, self._y_train_mean, self._y_train_std, "float64").cpu().numpy()
            dmean_d, var_d, dvar_d = dev.predict_grad_dev(q, self._y_train_std, kss, 0.0)
            dmean = dmean_d.cpu().numpy()
            var = var_d.cpu().numpy() if return_var else None
            dvar = dvar_d.cpu().numpy() if return_var else None
        one = mean.shape[1] == 1
        if one:
            mean, dmean = mean[:, 0], dmean[:, 0]
        if not return_var:
            return mean, dmean
        std2 = self._y_train_std ** 2       # undo normalisation (_gpr.py:487-489)
        y_var = np.outer(var, std2)
        dvar = dvar[:, None, :] * std2[None, :, None]
        if one:
            y_var, dvar = y_var[:, 0], dvar[:, 0]
        return mean, dmean, y_var, dvar

    def predict_hessian(self, X):
        """Posterior mean with its first and second input derivatives - what an exact-Hessian SQP step, the second-order mean
        correction tr(H Sigma) / 2 and the state sensitivity of a linearisation need.  scikit-learn has no such call; the
        Hessian is the closed form of the RBF kernel, evaluated on the GPU (K8), with delta_j = (x_m - x_j) / ls:

            hess[m, p, d, e] = y_std[p] / (ls_d ls_e) sum_j k(x_m, x_j) alpha_jp (delta_jd delta_je - [d = e])

        Returns (y_mean, dmean, hess): y_mean and dmean exactly as `predict_jacobian(X)` returns them (the same launches, the
        same bits), hess (M, P, D, D), or (M, D, D) for one target, every D x D block symmetric bit for bit.  Always the fp64
        kernels.  Same input validation as `predict`; an unfitted model returns the prior mean and zero derivatives."""
        X = check_queries(X)
        M, D = X.shape
        if not hasattr(self, "X_train_"):
            mean, dmean = self.predict_jacobian(X)
            return mean, dmean, np.zeros(dmean.shape + (D,))
        self._ensure_device()
        dev = self._dev
        if dev.host_path_ok(M, False):
            mean, dmean, hess = dev.predict_hess_host(X, self._y_train_mean, self._y_train_std)
        else:
            import torch
            q = dev._as_queries(X, torch.float64)
            mean = dev.predict_mean_dev(q, self._y_train_mean, self._y_train_std, "float64").cpu().numpy()
            dmean = dev.predict_mean_grad_dev(q, self._y_train_std).cpu().numpy()
            hess = dev.predict_mean_hess_dev(q, self._y_train_std).cpu().numpy()
        if mean.shape[1] == 1:
            mean, dmean, hess = mean[:, 0], dmean[:, 0], hess[:, 0]
        return mean, dmean, hess

    def predict_moments(self, X, Sigma, var_includes_noise=False):
        """The posterior at GAUSSIAN queries q ~ N(X[m], Sigma[m]) in closed form (exact moment matching; [C.]RBF[+White] kernels):
        X (M, D), M <= 32; Sigma (M, nx, nx) or (nx, nx), symmetric, the covariance of the LEADING nx <= D coordinates of the
        query (the rest are certain), or None (zero).  Returns (mean (M, P) = E[y], cov (M, P, P) = Cov[y] - the variance of the
        mean under the query plus the expected posterior variance on the diagonal, with the WhiteKernel level when
        var_includes_noise - and xcov (M, P, D) = Cov[q_d, y_p], zero beyond nx).  One C call (`gpk_moments_host`: five launches,
        one synchronisation) over K^-1, which the device model forms once per fit.  Up to 16 384 training rows (ValueError
        beyond, or with the backend option small_path=0); a fitted model only (RuntimeError)."""
        from . import propagate as _pg
        if not hasattr(self, "X_train_"):
            raise RuntimeError("This GaussianProcessRegressor instance is not fitted yet.")
        X, S, M, nx = _pg.check_gaussian_queries(X, Sigma, self.n_features_in_)
        self._ensure_device()
        dev = self._dev
        if not dev.moments_ok():
            raise ValueError("predict_moments needs the small-batch path: at most 16384 training rows, D <= 16, small_path != 0")
        comp = self.kernel_.components()
        kss = comp.sf2 + ((comp.noise or 0.0) if var_includes_noise else 0.0)
        return dev.moments_host(self._y_train_mean, self._y_train_std, kss, 0.0, X, S)

    def predict_moments_vjp(self, X, Sigma, grad_mean=None, grad_cov=None, grad_xcov=None, var_includes_noise=False):
        """`predict_moments` with the vector-Jacobian product of its results: for l = <grad_mean, mean> + <grad_cov, cov> +
        <grad_xcov, xcov> returns (mean, cov, xcov, dX (M, D) = dl/dX, dSigma (M, nx, nx) = dl/dSigma) - the controls' columns of
        dX included, dSigma symmetric bit for bit.  grad_mean (M, P), grad_cov (M, P, P), grad_xcov (M, P, D), None: zero; the
        entries are taken as independent: (g + g^T) / 2 is used for grad_cov, as for `propagate_gradient`'s grad_Sigma, and the
        columns >= nx of grad_xcov (where xcov is zero) are ignored.  The expected variance enters through the derivative of what
        is computed: nothing where its clip at zero is active.  mean, cov and xcov have the bits of `predict_moments`.  One C call
        (`gpk_moments_vjp_host`: ten launches, one synchronisation); limits and errors as `predict_moments`."""
        from . import propagate as _pg
        if not hasattr(self, "X_train_"):
            raise RuntimeError("This GaussianProcessRegressor instance is not fitted yet.")
        X, S, M, nx = _pg.check_gaussian_queries(X, Sigma, self.n_features_in_)
        gm, gc, gxc = _pg.check_moment_seeds(grad_mean, grad_cov, grad_xcov, M, self._yn.shape[1], self.n_features_in_)
        self._ensure_device()
        dev = self._dev
        if not dev.moments_ok():
            raise ValueError("predict_moments_vjp needs the small-batch path: at most 16384 training rows, D <= 16, small_path != 0")
        comp = self.kernel_.components()
        kss = comp.sf2 + ((comp.noise or 0.0) if var_includes_noise else 0.0)
        return dev.moments_vjp_host(self._y_train_mean, self._y_train_std, kss, 0.0, X, S, gm, gc, gxc)

    def propagate_moments_gradient(self, x0, U, lin, grad_traj, grad_Sigma=None, Sigma0=None, process_noise=None,
                                   var_includes_noise=False, route="auto"):
        """`propagate(method="moment")` with the gradient of a differentiable horizon cost l(traj, Sigma) with respect to the
        controls, the start state and the start covariance, through the exact moments of every stage (`propagate`'s module
        docstring has the sweep).  Arguments and results as `propagate_gradient`: (traj, Sigma, dU (R, H, nu), dx0 (R, P),
        dSigma0 (R, P, P)), traj and Sigma with the bits of `propagate(method="moment")`.  One C call per horizon
        (`gpk_propagate_mm_grad_host`: six launches per stage forward, seven backward, one synchronisation); route="host": the
        same sweep on the host over `predict_moments` and `predict_moments_vjp`.  ValueError where `propagate(method="moment")`
        raises one, and for seeds of a wrong shape or with NaN or infinity."""
        from . import propagate as _pg
        if not hasattr(self, "X_train_"):
            raise RuntimeError("This GaussianProcessRegressor instance is not fitted yet.")
        P, D = self._yn.shape[1], self.n_features_in_
        x0, U, lin, S0, Q, R, H = _pg.check_horizon(x0, U, lin, P, D, Sigma0, process_noise)
        gx, gS = _pg.check_seeds(grad_traj, grad_Sigma, R, H, P)
        _pg.check_method("moment", 1, "propagate_moments_gradient", Sigma0=S0, process_noise=Q)
        _pg.check_route(route)
        self._ensure_device()
        dev = self._dev
        if not dev.moments_ok():
            raise ValueError("propagate_moments_gradient needs the small-batch path: at most 16384 training rows, small_path != 0")
        if route == "host":
            return _pg.host_adjoint_moments(
                lambda q, S: self.predict_moments(q, S, var_includes_noise=var_includes_noise),
                lambda q, S, gm, gc, gxc: self.predict_moments_vjp(q, S, gm, gc, gxc, var_includes_noise=var_includes_noise),
                list(range(P)), x0, U, lin, S0, Q, R, H, gx, gS)
        comp = self.kernel_.components()
        kss = comp.sf2 + ((comp.noise or 0.0) if var_includes_noise else 0.0)
        return dev.propagate_mm_grad_host(self._y_train_mean, self._y_train_std, kss, 0.0, x0, U, lin, S0, Q, R, H, gx, gS)

    def propagate(self, x0, U, lin, Sigma0=None, process_noise=None, var_includes_noise=False, return_stages=False,
                  route="auto", order=1, method="linear"):
        """The posterior's own closed-loop horizon: the mean trajectory under the learned dynamics and the state covariance that
        the model's uncertainty induces along it, to first order (`propagate`'s module docstring has the recursion).  The state
        is the model's P outputs; a query is q = [x, u] (D = P + nu).  x0 (P,) or (R, P), U (H, nu) or (R, H, nu), lin (P, D) the
        nominal increment; Sigma0 (P, P) or (R, P, P), symmetric (default zero); process_noise (P, P), symmetric, added at
        every stage.  var_includes_noise: the stage variances include the WhiteKernel level, as `predict(return_std=True)`'s
        do (default: the latent function's variance).  Returns (traj (H + 1, R, P), Sigma (H + 1, R, P, P)) - R = 1 keeps its
        axis - and with return_stages=True also {"mean" (H, R, P), "var" (H, R, P), "jac" (H, R, P, D)}, the stage quantities as
        used: with var_includes_noise=True they have the bits of `predict_jacobian(q, return_var=True)` at the returned rows.
        One C call per horizon (three launches per stage, one synchronisation) up to 16 384 training rows; beyond that, or with
        the backend option small_path=0, or with route="host", the same recursion as a host loop over `predict_jacobian`.
        order=2: the mean takes the second-order term of E[mu(x)] for x ~ N(x_h, Sigma_h), c = tr(H Sigma_h) / 2 over the state
        block of the mean's Hessian, added last to each stage's mean; A_h and Sigma are formed as at first order.  Still one C
        call (`gpk_propagate2_host`: four launches per stage, no Hessian is formed); the host loop contracts `predict_hessian`.
        The stages gain "corr" (H, R, P).  Any other order: ValueError.
        method="moment": every stage's mean, covariance and input-output covariance are the EXACT moments of the posterior at
        the Gaussian query N([x_h, u_h], Sigma_h) (`predict_moments`; the module docstring has the recursion) instead of their
        linearisation: one C call (`gpk_propagate_mm_host`, five launches per stage), route="host" the same recursion as a host
        loop over `predict_moments`; the stages are {"mean" (H, R, P), "cov" (H, R, P, P), "xcov" (H, R, P, D)}.  order=2 with
        it is a ValueError.  The default method="linear" is the first-order chain above, untouched.
        A fitted model only (RuntimeError); ValueError for a wrong shape, R > 32, H outside 1 .. 256, non-finite input."""
        from . import propagate as _pg
        order = _pg.check_order(order)
        _pg.check_method(method, order)
        if not hasattr(self, "X_train_"):
            raise RuntimeError("This GaussianProcessRegressor instance is not fitted yet.")
        P, D = self._yn.shape[1], self.n_features_in_
        x0, U, lin, S0, Q, R, H = _pg.check_horizon(x0, U, lin, P, D, Sigma0, process_noise)
        self._ensure_device()
        dev = self._dev
        comp = self.kernel_.components()
        noise = comp.noise or 0.0
        if route not in ("auto", "host"):
            raise ValueError("route must be 'auto' or 'host'")
        if method == "moment":
            _pg.check_method(method, order, Sigma0=S0, process_noise=Q)
            if not dev.moments_ok():
                raise ValueError("method='moment' needs the small-batch path: at most 16384 training rows, small_path != 0")
            if route == "auto":
                traj, Sigma, mean, cov, xcov = dev.propagate_mm_host(self._y_train_mean, self._y_train_std,
                                                                     comp.sf2 + (noise if var_includes_noise else 0.0), 0.0, x0, U,
                                                                     lin, S0, Q, R, H, return_stages)
                stages = {"mean": mean, "cov": cov, "xcov": xcov}
            else:
                traj, Sigma, stages = _pg.host_loop_moments(
                    lambda q, S: self.predict_moments(q, S, var_includes_noise=var_includes_noise), list(range(P)), x0, U, lin,
                    S0, Q, R, H)
            return (traj, Sigma, stages) if return_stages else (traj, Sigma)
        if route == "auto" and dev.propagate_ok():
            # (the noise enters through the prior variance the clip starts from, as in predict_jacobian: the same bits)
            traj, Sigma, mean, var, jac, *corr = dev.propagate_host(self._y_train_mean, self._y_train_std,
                                                                    comp.sf2 + (noise if var_includes_noise else 0.0), 0.0, False,
                                                                    0.0, x0, U, lin, S0, Q, R, H, return_stages, order)
            stages = {"mean": mean, "var": var, "jac": jac}
            if order == 2:
                stages["corr"] = corr[0]
            return (traj, Sigma, stages) if return_stages else (traj, Sigma)
        std2 = self._y_train_std ** 2

        def stage(q):
            mean, dmean, var, _ = self.predict_jacobian(q, return_var=True)
            var = var.reshape(R, P)
            if not var_includes_noise:      # predict's variance carries the noise level: the latent variance, clipped again
                var = np.maximum(var - noise * std2[None, :], 0.0)
            return mean.reshape(R, P), dmean.reshape(R, P, D), var

        hess_stage = (lambda q: self.predict_hessian(q)[2]) if order == 2 else None
        traj, Sigma, stages = _pg.host_loop(stage, list(range(P)), x0, U, lin, S0, Q, R, H, hess_stage)
        return (traj, Sigma, stages) if return_stages else (traj, Sigma)

    def propagate_gradient(self, x0, U, lin, grad_traj, grad_Sigma=None, Sigma0=None, process_noise=None,
                           var_includes_noise=False, route="auto", order=1, method="linear"):
        """`propagate` with the gradient of a differentiable horizon cost l(traj, Sigma) with respect to the controls, the start
        state and the start covariance (`propagate`'s module docstring has the backward sweep).  grad_traj (H + 1, R, P) =
        dl/dx_h and grad_Sigma (H + 1, R, P, P) = dl/dSigma_h (default zero; entries taken as independent, (g + g^T) / 2 is
        used); with R = 1 the rollout axis may be left out.  Returns (traj, Sigma, dU (R, H, nu), dx0 (R, P), dSigma0 (R, P, P)):
        traj and Sigma with the bits of `propagate` on the same arguments, one gradient row per rollout (rollouts that share
        x0, U or Sigma0: add their rows).  The variance enters through the gradient of the unclipped variance, as
        `predict_jacobian(return_var=True)` returns it.  One C call per horizon (`gpk_propagate_grad_host`: six launches per
        stage, one synchronisation, no Hessian formed) where `propagate` makes one; otherwise, or with route="host", the same
        sweep on the host over `predict_jacobian` and `predict_hessian`.  order: 1 only - the derivative of the second-order
        mean term needs third derivatives of the mean (ValueError)."""
        from . import propagate as _pg
        _pg.check_grad_order(order)
        _pg.refuse_moment(method, "propagate_gradient")
        if not hasattr(self, "X_train_"):
            raise RuntimeError("This GaussianProcessRegressor instance is not fitted yet.")
        P, D = self._yn.shape[1], self.n_features_in_
        x0, U, lin, S0, Q, R, H = _pg.check_horizon(x0, U, lin, P, D, Sigma0, process_noise)
        gx, gS = _pg.check_seeds(grad_traj, grad_Sigma, R, H, P)
        if route not in ("auto", "host"):
            raise ValueError("route must be 'auto' or 'host'")
        self._ensure_device()
        dev = self._dev
        comp = self.kernel_.components()
        noise = comp.noise or 0.0
        if route == "auto" and dev.propagate_ok():
            return dev.propagate_grad_host(self._y_train_mean, self._y_train_std, comp.sf2 + (noise if var_includes_noise else 0.0),
                                           x0, U, lin, S0, Q, R, H, gx, gS)
        std2 = self._y_train_std ** 2

        def stage(q):
            mean, dmean, var, dvar = self.predict_jacobian(q, return_var=True)
            var = var.reshape(R, P)
            if not var_includes_noise:
                var = np.maximum(var - noise * std2[None, :], 0.0)
            return mean.reshape(R, P), dmean.reshape(R, P, D), var, dvar.reshape(R, P, D)

        return _pg.host_adjoint(stage, lambda q: self.predict_hessian(q)[2], list(range(P)), x0, U, lin, S0, Q, R, H, gx, gS)

    def sample_y(self, X, n_samples=1, random_state=0):
        """`sklearn/gaussian_process/_gpr.py:498-535`: draws from the joint posterior (or the prior, unfitted) at X - the
        mean and covariance from `predict(X, return_cov=True)` (GPU), the draw by NumPy's `multivariate_normal` (an SVD of
        the M x M covariance on the host), one target at a time.  Shape (M, n_samples), or (M, P, n_samples)."""
        rng = _rng_from(random_state)
        y_mean, y_cov = self.predict(X, return_cov=True)
        if y_mean.ndim == 1:
            return rng.multivariate_normal(y_mean, y_cov, n_samples).T
        y_samples = [rng.multivariate_normal(y_mean[:, t], y_cov[..., t], n_samples).T[:, np.newaxis]
                     for t in range(y_mean.shape[1])]
        return np.hstack(y_samples)

    def sample_paths(self, n_paths, n_features=1024, random_state=0):
        """`n_paths` posterior function draws as explicit functions (pathwise conditioning, `paths.PosteriorPaths`): unlike
        `sample_y`, whose draws live on one fixed batch, a path can be evaluated anywhere, call after call, and stays the same
        function - what a sampled closed-loop rollout needs.  n_features: random Fourier features of the prior term (the only
        approximation).  random_state as in `sample_y`; the draw order is `paths.draw_path_randomness`'s.  A fitted model
        only (RuntimeError otherwise); scikit-learn has no such call."""
        from .paths import PosteriorPaths, check_path_shape, draw_path_randomness
        self._ensure_device()
        dev = self._dev
        check_path_shape(dev.D, dev.P, int(n_paths), int(n_features))
        comp = self.kernel_.components()
        r = draw_path_randomness(_rng_from(random_state), dev.N, dev.D, int(n_features), int(n_paths), dev.P,
                                 comp.ls_vector(dev.D), (comp.noise or 0.0) + float(self.alpha))
        return PosteriorPaths.from_randomness(self, **r)

    # ------------------------------------------------------------------ host views / persistence
    @property
    def alpha_(self):
        self._ensure_device()
        if getattr(self, "_alpha_host", None) is None:
            a = self._dev.alpha_host()
            self._alpha_host = a[:, 0] if self._y_1d else a
        return self._alpha_host

    @property
    def L_(self):
        self._ensure_device()
        if getattr(self, "_L_host", None) is None:
            self._L_host = self._dev.L_host()
        return self._L_host

    def _refactor(self):
        """The model's factorisation at `kernel_` (final step of fit, and again after unpickling: same route, same bits):
        Gram, factor, inverse factor, alpha and the LML terms as ONE launch chain with one synchronisation (gpk_lml_eval, value
        only; up to 4608 rows factor and inverse factor are one launch) - or, beyond 32 768 rows and 16 features, call by call.
        Returns (log-det / 2, [y_p . alpha_p]).  Raises NotPositiveDefinite."""
        comp = self.kernel_.components()
        dev, D = self._dev, self.n_features_in_
        diag = (comp.noise or 0.0) + float(self.alpha)
        if dev.Np <= dev.INVERSE_EAGER_NP and D <= 16:
            logdet_half, quad, _ = dev.lml_eval(comp.ls_vector(D), comp.sf2, diag, comp.noise or 0.0, False)
            dev.release_grad_buffers()
            return logdet_half, quad
        dev.factorize(comp.ls_vector(D), comp.sf2, diag)
        dev.solve_alpha()
        return dev.lml_terms()

    def _ensure_device(self):
        """Re-create the HBM state after unpickling (deterministic refactorisation)."""
        if self._dev is None:
            if not hasattr(self, "X_train_"):
                raise RuntimeError("This GaussianProcessRegressor instance is not fitted yet.")
            self._dev = DeviceGP(self.X_train_, self._yn, get_backend(self.device))
            imported = getattr(self, "_imported_factor", None)
            comp = self.kernel_.components()
            if imported is not None:
                self._dev.load_factor(imported["L"], comp.ls_vector(self.n_features_in_), comp.sf2)
                self._dev.set_alpha(imported["alpha"])
            else:
                self._refactor()

    def __getstate__(self):
        st = self.__dict__.copy()
        st["_dev"] = None
        st.pop("_lml_dev", None)
        if not isinstance(st.get("device"), (int, type(None))):     # a private Backend (handle + stream): keep its index
            st["device"] = getattr(st["device"], "device_index", None)
        st.pop("_rng", None)
        st["_alpha_host"] = None
        st["_L_host"] = None
        return st

    def __setstate__(self, st):
        self.__dict__.update(st)
        self._dev = None

    @classmethod
    def from_sklearn(cls, skl, device=None, predict_dtype="float64"):
        """Ingest a fitted scikit-learn GaussianProcessRegressor (e.g. unpickled from the
        reference's `gp_models/*.pkl`, `src/px4/simple_gp.py:50-73`): X_train_, alpha_, L_,
        kernel_ parameters and the target normalisation are taken as they are."""
        kern = _convert_sklearn_kernel(skl.kernel_)
        self = cls(kernel=kern, alpha=float(np.ravel(skl.alpha)[0]) if np.ndim(skl.alpha) else float(skl.alpha),
                   optimizer=None, normalize_y=bool(skl.normalize_y), device=device, predict_dtype=predict_dtype)
        self.kernel_ = copy.deepcopy(kern)
        self.X_train_ = np.array(skl.X_train_, dtype=np.float64)
        yn = np.asarray(skl.y_train_, dtype=np.float64)
        self._y_1d = yn.ndim == 1
        self._yn = yn.reshape(self.X_train_.shape[0], -1)
        self.y_train_ = yn
        self._y_train_mean = np.asarray(skl._y_train_mean, dtype=np.float64).reshape(-1)
        self._y_train_std = np.asarray(skl._y_train_std, dtype=np.float64).reshape(-1)
        self.n_features_in_ = self.X_train_.shape[1]
        self.log_marginal_likelihood_value_ = float(getattr(skl, "log_marginal_likelihood_value_", np.nan))
        self._imported_factor = {"L": np.array(skl.L_, dtype=np.float64),
                                 "alpha": np.asarray(skl.alpha_, dtype=np.float64).reshape(self._yn.shape)}
        self._alpha_host = None
        self._L_host = None
        return self


def _convert_sklearn_kernel(k):
    """Map a scikit-learn kernel object (duck-typed by class name) to this package's spec."""
    name = type(k).__name__
    if name == "RBF":
        return RBF(np.array(k.length_scale, dtype=np.float64) if np.iterable(k.length_scale)
                   else float(k.length_scale), k.length_scale_bounds)
    if name == "WhiteKernel":
        return WhiteKernel(float(k.noise_level), k.noise_level_bounds)
    if name == "ConstantKernel":
        return ConstantKernel(float(k.constant_value), k.constant_value_bounds)
    if name == "Sum":
        return _convert_sklearn_kernel(k.k1) + _convert_sklearn_kernel(k.k2)
    if name == "Product":
        return _convert_sklearn_kernel(k.k1) * _convert_sklearn_kernel(k.k2)
    raise ValueError(f"unsupported scikit-learn kernel {name}")
