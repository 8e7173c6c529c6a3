"""Sparse inducing-point GP: fit on every row of a flight log, serve through m inducing inputs.

The Titsias / DTC predictor of GPflow's SGPR on this package's kernel `[C *] RBF [+ WhiteKernel]`, shared by all outputs.
The training rows enter through additive fp64 statistics of size m x m (`gpk_sparse_update`: N m^2 flops on the fp64
matrix cores), so `partial_fit` appends rows at any time; the model is assembled from them lazily at the next `predict`
(`gpk_sparse_finalize`: an m x m factorisation) and served at the cost of an exact model of m rows
(`gpk_sparse_predict`: two launches for up to 32 rows; `predict_jacobian`, `predict(return_cov=True)` and `sample_y`
serve the controller's linearisation and joint draws the same way).  `fit` / `partial_fit` do not optimise: the hyper-parameters are the
kernel's, e.g. those of an exact fit on a subset (`SparseGP.from_exact`).  `train` does: it keeps the rows on the device
(`hold`, `gpk_sparse_hold`) and maximises the collapsed bound over the kernel's free parameters with L-BFGS-B, as GPflow's
SGPR does; every evaluation (`log_bound`, `gpk_sparse_eval`) is the statistics pass, the m x m assembly and, for the
gradient, one more pass over the rows.  `train(train_inducing=True)` optimises the inducing inputs together with the kernel,
as SGPR does: `gpk_sparse_eval_z` moves Z and adds the bound's gradient with respect to it (a second pass over the rows and
an m x m kernel); by default the inducing inputs stay where they are.  Where they start is the caller's array, a seeded
random subset of the rows, or the rows picked by greedy conditional variance (`select_inducing`, `gpk_sparse_select`:
`from_exact(selection="greedy")`, `train(select_inducing="greedy")`).

`approximation="fitc"` selects the FITC posterior (Snelson & Ghahramani 2006; GPflow's GPRFITC) instead of the default DTC one:
every row gets the part of its prior variance that the inducing inputs cannot explain, sf2 - |Wuu k_u(x_i)|^2, as noise of its
own, through weighted statistics (`gpk_sparse_set_approximation`; DESIGN.md, K9, "FITC").  Fitting, serving, pickling and
`log_bound(theta)` work unchanged and `bound()` is the FITC log-marginal likelihood; its gradient is not built, so `train` and
the gradient flags raise a ValueError that names the recipe: train as DTC, then build the FITC model from that kernel and Z.

The class keeps one libgpk handle of its own: the sparse model is the object behind that handle (include/gpk.h), the
arrays that cross the boundary are host NumPy arrays.
"""
from __future__ import annotations

import ctypes as C
import copy

import numpy as np

from . import _lib
from .device import Backend, check_queries, get_backend

_ptr = _lib.host_ptr


def hyper_from_theta(kernel, theta):
    """theta (the kernel's layout: log-parameters, fixed ones excluded) -> (the kernel at theta, its components, the
    length-scales as `gpk_sparse_eval` takes them: one value for an isotropic kernel, D for ARD)."""
    kern = kernel.clone_with_theta(np.asarray(theta, dtype=np.float64))
    comp = kern.components()
    return kern, comp, np.ascontiguousarray(comp.ls, dtype=np.float64)


def gradient_to_theta(comp, g):
    """`gpk_sparse_eval`'s gradient [ls .. (n_ls values; isotropic: already summed over the features), noise, sf2] -> the
    gradient in theta's layout (fixed parameters dropped)."""
    return comp.map_gradient(np.asarray(g, dtype=np.float64), len(g) - 2)


def pack_inducing(theta, Z):
    """The optimisation vector of `train(train_inducing=True)`: [theta, Z.ravel()] (Z row-major, raw coordinates)."""
    return np.concatenate([np.asarray(theta, dtype=np.float64).ravel(), np.asarray(Z, dtype=np.float64).ravel()])


def unpack_inducing(v, n_theta, shape):
    """[theta, Z.ravel()] -> (theta, Z of `shape`), copies."""
    v = np.asarray(v, dtype=np.float64)
    if v.shape != (n_theta + shape[0] * shape[1],):
        raise ValueError(f"expected {n_theta} + {shape[0]} x {shape[1]} values, got {v.shape}")
    return v[:n_theta].copy(), v[n_theta:].reshape(shape).copy()


APPROXIMATIONS = ("dtc", "fitc")       # the C side's kinds, GPK_SPARSE_DTC = 0 and GPK_SPARSE_FITC = 1, by index

_FITC_NO_GRADIENT = ("the gradient of the FITC likelihood is not available (approximation='fitc'): lambda depends on the "
                     "hyper-parameters and on the inducing inputs, and that gradient is not built.  Supported recipe: train as DTC "
                     "(approximation='dtc') or as an exact model, then build the FITC model from that kernel and those inducing "
                     "inputs (SparseGP(kernel_, inducing_, approximation='fitc'), SparseGP.from_exact(..., approximation='fitc'))")


def check_approximation(approximation):
    """'dtc' or 'fitc' (ValueError otherwise)."""
    if approximation not in APPROXIMATIONS:
        raise ValueError(f"approximation must be 'dtc' or 'fitc', got {approximation!r}")
    return approximation


class SparseGP:
    def __init__(self, kernel, inducing, *, alpha=1e-10, jitter_uu=None, y_mean=None, y_std=None, device=None,
                 approximation="dtc"):
        self.approximation_ = check_approximation(approximation)
        self.kernel = kernel
        self.kernel_ = copy.deepcopy(kernel)
        comp = self.kernel_.components()          # rejects anything but [C *] RBF [+ WhiteKernel], as gpr.py does
        Z = np.array(inducing, dtype=np.float64, ndmin=2)
        if Z.ndim != 2 or Z.shape[0] < 1 or Z.shape[1] < 1:
            raise ValueError("inducing inputs must be (m, D)")
        if not np.isfinite(Z).all():
            raise ValueError("Input contains NaN or infinity")
        if np.iterable(alpha):
            raise ValueError("per-sample alpha is not supported by the MI355X path")
        self.inducing_ = np.ascontiguousarray(Z)
        self._inducing0 = self.inducing_.copy()       # where train(train_inducing=True) starts Z from, every time
        self.n_features_in_ = Z.shape[1]
        comp.ls_vector(self.n_features_in_)       # anisotropic kernels must match the inputs
        self.alpha = float(alpha)
        self.jitter_uu = 1e-8 * comp.sf2 if jitter_uu is None else float(jitter_uu)
        self.y_mean = None if y_mean is None else np.atleast_1d(np.asarray(y_mean, dtype=np.float64)).copy()
        self.y_std = None if y_std is None else np.atleast_1d(np.asarray(y_std, dtype=np.float64)).copy()
        self.device = device
        self._be = None
        self._live = False          # the object behind the handle exists
        self._final = False         # ... and is assembled from the current statistics
        self._P = None
        self._y_1d = True
        self._state = None          # statistics waiting to be imported (after unpickling)
        self._held = False          # the rows behind the statistics are on the device (hold)

    # ------------------------------------------------------------------ construction from an exact model
    @classmethod
    def from_exact(cls, gpr, inducing=None, random_state=0, jitter_uu=None, selection="random", approximation="dtc"):
        """Kernel, `alpha` and target normalisation of a fitted `GaussianProcessRegressor`; inducing inputs: an array, an
        integer (that many of its training rows, picked by a seeded permutation) or None (all of them).  The sparse model
        starts with no rows: `partial_fit` the flight log (the exact model's own rows included, if they are to count).
        `selection="greedy"` picks the integer's rows by greedy conditional variance under the regressor's kernel instead
        (`select_inducing`); ValueError if fewer than that many rows are usable (duplicates, say).  `approximation`: "dtc" or
        "fitc", as the constructor takes it (the selection does not depend on it)."""
        check_approximation(approximation)
        if selection not in ("random", "greedy"):
            raise ValueError(f"selection must be 'random' or 'greedy', got {selection!r}")
        if not hasattr(gpr, "X_train_"):
            raise RuntimeError("This GaussianProcessRegressor instance is not fitted yet.")
        X = gpr.X_train_
        if inducing is None:
            Z = X
        elif isinstance(inducing, (int, np.integer)):
            if not 1 <= int(inducing) <= len(X):
                raise ValueError(f"inducing must be in [1, {len(X)}]")
            if selection == "greedy":
                probe = cls(gpr.kernel_, X[:1], alpha=gpr.alpha, jitter_uu=jitter_uu, device=gpr.device)
                Z = X[probe._select_exactly(X, int(inducing))]
                return cls._like(gpr, Z, jitter_uu, approximation)
            Z = X[np.sort(np.random.default_rng(random_state).permutation(len(X))[:int(inducing)])]
        else:
            Z = inducing
        return cls._like(gpr, Z, jitter_uu, approximation)

    @classmethod
    def _like(cls, gpr, Z, jitter_uu, approximation="dtc"):
        out = cls(gpr.kernel_, Z, alpha=gpr.alpha, jitter_uu=jitter_uu, y_mean=gpr._y_train_mean, y_std=gpr._y_train_std, device=gpr.device,
                  approximation=approximation)
        out._y_1d = bool(getattr(gpr, "_y_1d", True))
        return out

    # ------------------------------------------------------------------ the object behind the handle
    def _backend(self):
        if self._be is None:
            main = get_backend(self.device)
            self._be = main if isinstance(self.device, Backend) else Backend(main.device_index)
        return self._be

    def _hyper(self):
        comp = self.kernel_.components()
        ls = np.ascontiguousarray(comp.ls, dtype=np.float64)
        return comp, ls

    def _begin(self, P):
        if not 1 <= P <= _lib.GPK_MAX_P:
            raise ValueError(f"P must be in [1, {_lib.GPK_MAX_P}]")
        ym = np.zeros(P) if self.y_mean is None else self.y_mean
        ys = np.ones(P) if self.y_std is None else self.y_std
        if ym.shape != (P,) or ys.shape != (P,):
            raise ValueError(f"y_mean / y_std must have {P} entries")
        self._ym, self._ys = np.ascontiguousarray(ym), np.ascontiguousarray(ys)
        comp, ls = self._hyper()
        be = self._backend()
        Z = self.inducing_
        with be.lock:            # (the call and the state it consumes: one step)
            st = self._state
            if st is None:
                be.call("gpk_sparse_begin", _ptr(Z), Z.shape[0], Z.shape[1], P, _ptr(ls), ls.size, comp.sf2, comp.noise or 0.0,
                        self.alpha, self.jitter_uu, _ptr(self._ym), _ptr(self._ys))
            else:
                be.call("gpk_sparse_import", _ptr(Z), Z.shape[0], Z.shape[1], P, _ptr(ls), ls.size, comp.sf2, comp.noise or 0.0,
                        self.alpha, self.jitter_uu, _ptr(self._ym), _ptr(self._ys), _ptr(st["G"]), _ptr(st["g"]),
                        _ptr(st["yy"]), int(st["n_rows"]))
                self._state = None
            if self._fitc:       # (GPK_NOT_PD - Kuu + jitter_uu I, factored at once - raises LinAlgError as the finalisation does)
                info = C.c_int(0)
                if st is None:
                    be.call("gpk_sparse_set_approximation", 1, C.byref(info))
                else:
                    be.call("gpk_sparse_restore_approximation", 1, float(st.get("log_lambda_sum", 0.0)), C.byref(info))
        self._P, self._live, self._final, self._held = P, True, False, False

    @property
    def _fitc(self):
        """(objects unpickled from before the attribute existed are DTC)"""
        return self.__dict__.get("approximation_", "dtc") == "fitc"

    def _ensure(self):
        """The assembled model: created (the prior, if no row was ever given) and finalised."""
        if not self._live:
            P = self._P if self._P is not None else (1 if self.y_mean is None else self.y_mean.size)
            self._begin(P)
        if not self._final:
            info = C.c_int(0)
            self._backend().call("gpk_sparse_finalize", C.byref(info))      # GPK_NOT_PD raises LinAlgError
            self._final = True

    # ------------------------------------------------------------------ rows
    def _check_rows(self, X, y):
        X = np.array(X, dtype=np.float64, ndmin=2)
        y = np.asarray(y, dtype=np.float64)
        if X.shape[0] != y.shape[0]:
            raise ValueError("X and y have inconsistent numbers of samples")
        if X.shape[1] != self.n_features_in_:
            raise ValueError(f"X must be (N, {self.n_features_in_})")
        if not (np.isfinite(X).all() and np.isfinite(y).all()):
            raise ValueError("Input contains NaN or infinity")
        return np.ascontiguousarray(X), np.ascontiguousarray(y.reshape(X.shape[0], -1)), y.ndim == 1

    def partial_fit(self, X, y):
        """Appends the rows X (n, D), y (n,) or (n, P) to the statistics; the model is reassembled at the next predict."""
        X, y2, y_1d = self._check_rows(X, y)
        if self._P is None and self._state is None:
            self._y_1d = y_1d
        if not self._live:
            self._begin(y2.shape[1] if self._P is None else self._P)
        if y2.shape[1] != self._P:
            raise ValueError(f"y must have {self._P} columns")
        if X.shape[0] == 0:
            return self
        self._backend().call("gpk_sparse_update", _ptr(X), _ptr(y2), X.shape[0])
        self._final, self._held = False, False
        self._touch()
        return self

    def fit(self, X, y):
        """Forgets the rows seen so far, then `partial_fit(X, y)`."""
        self._live, self._final, self._P, self._state = False, False, None, None
        self._touch()
        return self.partial_fit(X, y)

    # ------------------------------------------------------------------ training
    def hold(self, X, y):
        """Forgets the rows seen so far and keeps X (n, D), y (n,) or (n, P) on the device: the statistics are theirs, and
        `log_bound` can evaluate the bound of exactly these rows at any hyper-parameters.  A later `partial_fit` releases
        them."""
        X, y2, y_1d = self._check_rows(X, y)
        if X.shape[0] == 0:
            raise ValueError("hold needs at least one row")
        self._live, self._final, self._P, self._state = False, False, None, None
        self._touch()
        self._y_1d = y_1d
        self._begin(y2.shape[1])
        self._backend().call("gpk_sparse_hold", _ptr(X), _ptr(y2), X.shape[0])
        self._held = True
        return self

    def log_bound(self, theta=None, eval_gradient=False, inducing=None, eval_inducing_gradient=False):
        """The collapsed bound of the held rows at theta (the kernel's own layout: log-parameters, fixed ones excluded), and
        its gradient: the semantics of `GaussianProcessRegressor.log_marginal_likelihood`.  theta=None: the bound of the
        current model.  `inducing` (m, D) moves the inducing inputs there first (`inducing_` follows);
        `eval_inducing_gradient` returns (value, grad_theta, grad_Z), grad_Z (m, D) in raw coordinates.  A matrix that is not
        positive definite gives -inf and zero gradients.  After the call the object is the model at theta (`kernel_` follows)
        and at these inducing inputs.  Without the two inducing arguments the call is `gpk_sparse_eval`, launch for launch."""
        if self._fitc and (eval_gradient or eval_inducing_gradient):
            raise ValueError("log_bound: " + _FITC_NO_GRADIENT)
        if theta is None:
            if eval_gradient or eval_inducing_gradient or inducing is not None:
                raise ValueError("Gradient can only be evaluated for theta!=None")
            return self.bound()
        if not (self._live and getattr(self, "_held", False)):
            raise RuntimeError("log_bound(theta) needs held rows: call hold(X, y) first")
        theta = np.asarray(theta, dtype=np.float64)
        kern, comp, ls = hyper_from_theta(self.kernel_, theta)
        Z = None
        if inducing is not None:
            Z = np.ascontiguousarray(np.array(inducing, dtype=np.float64, ndmin=2))
            if Z.shape != self.inducing_.shape:
                raise ValueError(f"inducing inputs must be {self.inducing_.shape}")
            if not np.isfinite(Z).all():
                raise ValueError("Input contains NaN or infinity")
        b, info = C.c_double(0.0), C.c_int(0)
        g = np.zeros(ls.size + 2)
        gZ = np.zeros(self.inducing_.shape) if eval_inducing_gradient else None
        be = self._backend()
        with be.lock:            # (the evaluation and the Python state that follows it: one step)
            if Z is None and gZ is None:
                rc = be.status("gpk_sparse_eval", _ptr(ls), ls.size, comp.sf2, comp.noise or 0.0, C.byref(b),
                               _ptr(g) if eval_gradient else None, C.byref(info))
            else:
                rc = be.status("gpk_sparse_eval_z", _ptr(Z), _ptr(ls), ls.size, comp.sf2, comp.noise or 0.0, C.byref(b),
                               _ptr(g) if eval_gradient or gZ is not None else None, _ptr(gZ), C.byref(info))
            self.kernel_ = kern
            if Z is not None:
                self.inducing_ = Z
            self._touch()
            if rc == _lib.GPK_NOT_PD:
                self._final = False
                if gZ is not None:
                    return -np.inf, np.zeros_like(theta), np.zeros_like(gZ)
                return (-np.inf, np.zeros_like(theta)) if eval_gradient else -np.inf
            be.check(rc)
        self._final = True
        value = float(b.value)
        if gZ is not None:
            return value, gradient_to_theta(comp, g), gZ
        return (value, gradient_to_theta(comp, g)) if eval_gradient else value

    # ------------------------------------------------------------------ choosing the inducing inputs
    def select_inducing(self, X=None, m=None, tol=0.0, min_var=1e-10):
        """Greedy conditional-variance selection (`gpk_sparse_select`; Burt, Rasmussen, van der Wilk 2020) among the rows X
        (n, D) - None: the held rows - under the current kernel: each step takes the row whose prior variance, conditioned
        on the rows taken so far, is largest (the lowest index among equals).  At most m rows (None: as many as the object
        has inducing inputs); stops early once the largest conditional variance is at most min_var sf2, or the trace
        tr(Kff - Qff) at most tol n sf2.  Returns (indices, trace): trace[t] = tr(Kff - Qff) with Z = X[indices[:t + 1]].
        The model, its statistics and `inducing_` stay as they are."""
        if X is None:
            if not (self._live and getattr(self, "_held", False)):
                raise RuntimeError("select_inducing() needs held rows: call hold(X, y) first, or pass X")
            n = self.n_rows_
        else:
            X = np.array(X, dtype=np.float64, ndmin=2)
            if X.ndim != 2 or X.shape[1] != self.n_features_in_:
                raise ValueError(f"X must be (n, {self.n_features_in_})")
            if not np.isfinite(X).all():
                raise ValueError("Input contains NaN or infinity")
            X = np.ascontiguousarray(X)
            n = X.shape[0]
            if not self._live:
                self._begin(self.n_outputs_)
        m = self.inducing_.shape[0] if m is None else int(m)
        if not 1 <= m <= n:
            raise ValueError(f"m must be in [1, {n}]")
        if not (tol >= 0.0 and min_var >= 0.0):
            raise ValueError("tol and min_var must be non-negative")
        idx = np.full(m, -1, dtype=np.int64)
        trace, dmax = np.full(m, np.nan), np.full(m, np.nan)
        sel = C.c_int64(0)
        self._backend().call("gpk_sparse_select", _ptr(X), n, m, float(min_var), float(tol),
                             idx.ctypes.data_as(C.POINTER(C.c_int64)), _ptr(trace), _ptr(dmax), C.byref(sel))
        return idx[:sel.value].copy(), trace[:sel.value].copy()

    def _select_exactly(self, X, m, min_var=1e-10):
        idx, _ = self.select_inducing(X, m, min_var=min_var)
        if len(idx) < m:
            raise ValueError(f"greedy selection found {len(idx)} usable rows, fewer than the {m} asked for "
                             "(duplicate rows, or a kernel under which fewer rows explain all the variance)")
        return idx

    def train(self, X, y, n_restarts_optimizer=0, optimizer="fmin_l_bfgs_b", random_state=None, train_inducing=False,
              select_inducing=None, selection_rounds=1):
        """Holds the rows and maximises the bound over the kernel's free parameters within its bounds (L-BFGS-B, as
        `GaussianProcessRegressor.fit`; restarts start from draws within finite bounds and run one after the other).  Sets
        `kernel_` and `bound_value_` and leaves the finalised model at the optimum.  `train_inducing=True`: the optimisation
        vector is [theta, Z.ravel()] with Z unbounded, as GPflow's SGPR trains its inducing variable; every start begins
        at the constructor's inducing inputs (restarts redraw theta only), and `inducing_` is the trained Z afterwards.
        `select_inducing="greedy"`: each of the `selection_rounds` rounds first re-selects the inducing inputs among the held
        rows under the current kernel (`select_inducing`), then trains the kernel with them fixed - the reselect-then-train
        alternation of the literature; with `train_inducing=True` the last round trains Z as well, from the greedy Z.  The
        object keeps its number of inducing inputs: a round takes rows below the variance floor too, and raises ValueError
        only if fewer than that many rows have any conditional variance left (exact duplicates)."""
        from .gpr import _rng_from
        if self._fitc:
            raise ValueError("train: " + _FITC_NO_GRADIENT)
        if select_inducing not in (None, "greedy"):
            raise ValueError(f"select_inducing must be None or 'greedy', got {select_inducing!r}")
        if select_inducing is not None and int(selection_rounds) < 1:
            raise ValueError("selection_rounds must be at least 1")
        if self.kernel_.n_dims == 0:
            raise ValueError("train: the kernel has no free parameter")
        Z0 = self.__dict__.get("_inducing0", self.inducing_).copy() if train_inducing else self.inducing_
        self.hold(X, y)
        rng = [None]

        def draw():      # one generator for all rounds, made at the first restart as before
            if rng[0] is None:
                rng[0] = _rng_from(random_state)
            return rng[0]

        if select_inducing is None:
            return self._maximise(optimizer, n_restarts_optimizer, draw, train_inducing, Z0)
        rows = np.array(X, dtype=np.float64, ndmin=2)
        m, rounds = self.inducing_.shape[0], int(selection_rounds)
        for r in range(rounds):
            # (min_var = 0: the object keeps its m inducing inputs, so rows under the variance floor are taken too, largest
            # remainder first - a trained kernel with long length-scales leaves fewer than m above it; jitter_uu carries them)
            Z = np.ascontiguousarray(rows[self._select_exactly(None, m, min_var=0.0)])
            if not np.isfinite(self.log_bound(self.kernel_.theta, inducing=Z)):
                raise np.linalg.LinAlgError("train: the model at the selected inducing inputs is not positive definite")
            self._maximise(optimizer, n_restarts_optimizer, draw, train_inducing and r == rounds - 1, Z)
        return self

    def _maximise(self, optimizer, n_restarts_optimizer, draw, train_inducing, Z0):
        """L-BFGS-B on the bound of the held rows from the current kernel (and Z0, with train_inducing); leaves the model at
        the optimum."""
        from .gpr import constrained_optimization
        nt = self.kernel_.n_dims

        if train_inducing:
            def obj(v):
                theta, Z = unpack_inducing(v, nt, Z0.shape)
                value, grad, gZ = self.log_bound(theta, eval_gradient=True, inducing=Z, eval_inducing_gradient=True)
                return -value, -pack_inducing(grad, gZ)
        else:
            def obj(theta):
                value, grad = self.log_bound(theta, eval_gradient=True)
                return -value, -grad

        bounds = self.kernel_.bounds
        starts = [self.kernel_.theta]
        if n_restarts_optimizer > 0:
            if not np.isfinite(bounds).all():
                raise ValueError("Multiple optimizer restarts (n_restarts_optimizer>0) requires that all bounds are finite.")
            rng = draw()
            starts += [rng.uniform(bounds[:, 0], bounds[:, 1]) for _ in range(n_restarts_optimizer)]
        if train_inducing:
            starts = [pack_inducing(t0, Z0) for t0 in starts]
            bounds = np.vstack([bounds, np.tile([-np.inf, np.inf], (Z0.size, 1))])
        optima = [constrained_optimization(optimizer, obj, t0, bounds) for t0 in starts]
        vals = [o[1] for o in optima]
        best = optima[int(np.argmin(vals))][0]
        # the model at the optimum (the last evaluation need not be the best one)
        if train_inducing:
            theta, Z = unpack_inducing(best, nt, Z0.shape)
            value = self.log_bound(theta, inducing=Z)
        else:
            value = self.log_bound(best)
        if not np.isfinite(value):
            raise np.linalg.LinAlgError("train: the model at the optimum is not positive definite")
        self.bound_value_ = value
        return self

    # ------------------------------------------------------------------ predict
    def _queries(self, X):
        return check_queries(X, self.n_features_in_)

    @property
    def n_outputs_(self):
        """Output columns of the model (1 until rows or a target normalisation say otherwise)."""
        if self._P is not None:
            return self._P
        return 1 if self.y_mean is None else self.y_mean.size

    @property
    def _y_train_std(self):
        """The target scale per output, under the exact model's name (what `SimpleQuadrotorGP` reads the output count from)."""
        return np.ones(self.n_outputs_) if self.y_std is None else self.y_std

    def predict(self, X, return_std=False, return_cov=False):
        """Posterior mean (and standard deviation, with the WhiteKernel level as scikit-learn's `predict` has it) at the rows
        X.  Up to 32 rows: one call, two launches, one synchronisation, whatever the number of outputs.

        return_cov=True returns (y_mean, y_cov) as `GaussianProcessRegressor.predict` does: y_cov of shape (M, M) - (M, M, P)
        for 2-D targets - scaled by the target std squared, the WhiteKernel level on its diagonal
        (`gpk_sparse_predict_cov`; at most 16 384 rows)."""
        if return_std and return_cov:
            raise RuntimeError("At most one of return_std or return_cov can be requested.")
        X = self._queries(X)
        self._ensure()
        M, P = X.shape[0], self._P
        squeeze = P == 1 and self._y_1d
        mean = np.empty((M, P))
        if return_cov:
            cov = np.empty((P, M, M))
            if M > 0:
                self._backend().call("gpk_sparse_predict_cov", _ptr(X), M, _ptr(mean), _ptr(cov))
            return (mean[:, 0], cov[0]) if squeeze else (mean, np.ascontiguousarray(np.moveaxis(cov, 0, -1)))
        var = np.empty((M, P)) if return_std else None
        if M > 0:
            self._backend().call("gpk_sparse_predict", _ptr(X), M, _ptr(mean), _ptr(var), 1)
        if not return_std:
            return mean[:, 0] if squeeze else mean
        std = np.sqrt(var)
        return (mean[:, 0], std[:, 0]) if squeeze else (mean, std)

    def predict_jacobian(self, X, return_var=False):
        """Posterior mean and its Jacobian with respect to the inputs and, with return_var=True, the posterior variance and
        its input gradient: the call of `GaussianProcessRegressor.predict_jacobian` on the sparse posterior
        (`gpk_sparse_predict_grad`), with k = k_u(x), u_jd = (z_jd - x_d) / ls_d^2:

            dmean[m, p, d] = y_std[p] sum_j k_mj u_jd alpha_u[j, p]
            dvar[m, p, d]  = -2 y_std[p]^2 sum_j k_mj u_jd (Kuu^-1 k_m - Sigma~ k_m)_j

        Returns (y_mean, dmean) or (y_mean, dmean, y_var, dvar).  Shapes follow `predict`'s squeezing: y_mean (M, P) / (M,),
        dmean (M, P, D) / (M, D) for one target; y_var = predict(X, return_std=True)[1] ** 2 (clipped at 0 like it), shaped
        as y_mean; dvar shaped as dmean - the gradient of the unclipped variance.  Same input validation as `predict`; a model
        without rows returns the prior mean / variance and zero gradients through the same call.  Up to 32 rows: one launch,
        three with the variance, one synchronisation, whatever the number of outputs."""
        X = self._queries(X)
        self._ensure()
        M, D, P = X.shape[0], X.shape[1], self._P
        mean, dmean = np.empty((M, P)), np.empty((M, P, D))
        var = np.empty((M, P)) if return_var else None
        dvar = np.empty((M, P, D)) if return_var else None
        if M > 0:
            self._backend().call("gpk_sparse_predict_grad", _ptr(X), M, _ptr(mean), _ptr(var), _ptr(dmean), _ptr(dvar), 1)
        if P == 1 and self._y_1d:
            mean, dmean = mean[:, 0], dmean[:, 0]
            if return_var:
                var, dvar = var[:, 0], dvar[:, 0]
        return (mean, dmean, var, dvar) if return_var else (mean, dmean)

    def predict_hessian(self, X):
        """Posterior mean with its first and second input derivatives: the call of
        `GaussianProcessRegressor.predict_hessian` on the sparse posterior (`gpk_sparse_predict_hess`).  The sparse mean is
        that of an exact model over (Z, alpha_u) and its Hessian involves no inverse factor, with delta_j = (x_m - z_j) / ls:

            hess[m, p, d, e] = y_std[p] / (ls_d ls_e) sum_j k_mj alpha_u[j, p] (delta_jd delta_je - [d = e])

        Returns (y_mean, dmean, hess): y_mean and dmean as `predict_jacobian(X)` returns them, bit for bit; hess (M, P, D, D),
        or (M, D, D) for one target, every D x D block symmetric bit for bit.  A model without rows returns the prior mean and
        zero derivatives through the same call."""
        X = self._queries(X)
        self._ensure()
        M, D, P = X.shape[0], X.shape[1], self._P
        mean, dmean, hess = np.empty((M, P)), np.empty((M, P, D)), np.empty((M, P, D, D))
        if M > 0:
            self._backend().call("gpk_sparse_predict_hess", _ptr(X), M, _ptr(mean), _ptr(dmean), _ptr(hess))
        if P == 1 and self._y_1d:
            mean, dmean, hess = mean[:, 0], dmean[:, 0], hess[:, 0]
        return mean, dmean, hess

    def sample_y(self, X, n_samples=1, random_state=0):
        """Draws from the joint posterior (the prior, without rows) at X, as `GaussianProcessRegressor.sample_y`: the mean and
        covariance from `predict(X, return_cov=True)` (GPU), the draw by NumPy's `multivariate_normal`, one target at a time.
        Shape (M, n_samples), or (M, P, n_samples)."""
        from .gpr import _rng_from
        rng = _rng_from(random_state)
        y_mean, y_cov = self.predict(X, return_cov=True)
        if y_mean.ndim == 1:
            return rng.multivariate_normal(y_mean, y_cov, n_samples).T
        y_samples = [rng.multivariate_normal(y_mean[:, t], y_cov[..., t], n_samples).T[:, np.newaxis]
                     for t in range(y_mean.shape[1])]
        return np.hstack(y_samples)

    def propagate(self, x0, U, lin, Sigma0=None, process_noise=None, var_includes_noise=False, return_stages=False,
                  route="auto", order=1, method="linear"):
        """`GaussianProcessRegressor.propagate` on the sparse posterior: the mean rollout with the linearised state covariance,
        same arguments and results.  route="auto" and "host": the recursion as a host loop over
        `predict_jacobian(..., return_var=True)`, one call and one synchronisation per stage.  route="chain": ONE C call per
        horizon (`gpk_sparse_propagate`: three launches per stage, one synchronisation; with var_includes_noise=True the stage
        quantities have the bits of `predict_jacobian(q, return_var=True)` at the returned rows; with False the latent
        variance is kss = sf2 clipped at 1e-10 y_std^2 where the loop forms max(noisy - level, 0) - a difference in rounding
        while neither clip is active).  ValueError where `propagate_ok()` does not hold, with the reason, or where the entry
        refuses its arguments, with the library's message.  order=2: the second-order mean, on every route (chain:
        `gpk_sparse_propagate2`, four launches per stage, the mean's model (Z, alpha_u) as in `predict_hessian`; the host loop
        contracts `predict_hessian`); the stages gain "corr" (H, R, P).  method: "linear" only - exact moment matching
        is `propagate_moments` on this class; method="moment" here: ValueError."""
        from . import propagate as _pg
        order = _pg.check_order(order)
        _pg.refuse_moment(method, "SparseGP")
        _pg.check_route(route, ("auto", "host", "chain"))
        P, D = self.n_outputs_, self.n_features_in_
        x0, U, lin, S0, Q, R, H = _pg.check_horizon(x0, U, lin, P, D, Sigma0, process_noise)
        if route == "chain":
            why = self._propagate_refusal()
            if why:
                raise ValueError(f"route='chain' is not available: {why}")
            self._ensure()
            traj, Sigma, more = _pg.horizon_call(
                lambda *t: self._backend().call("gpk_sparse_propagate" if order == 1 else "gpk_sparse_propagate2",
                                                int(bool(var_includes_noise)), *t),
                x0, U, lin, S0, Q, R, H, ((P,), (P,), (P, D)) if return_stages else None, None if order == 1 else order)
            return (traj, Sigma, dict(zip(("mean", "var", "jac", "corr"), more))) if return_stages else (traj, Sigma)
        noise = self.kernel_.components().noise or 0.0
        std2 = np.broadcast_to(np.asarray(self._y_train_std, dtype=np.float64).reshape(-1), (P,)) ** 2

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
        """`GaussianProcessRegressor.propagate_gradient` on the sparse posterior: `propagate` with the gradient of a horizon cost
        with respect to the controls, the start state and the start covariance; same arguments and results.  route="auto" and
        "host": the sweep on the host over `predict_jacobian(..., return_var=True)` and `predict_hessian`.  route="chain": ONE C
        call per horizon (`gpk_sparse_propagate_grad`: six launches per stage, one synchronisation; traj and Sigma with the
        bits of `propagate(route="chain")`); ValueError where `propagate_ok()` does not hold.  order: 1 only (ValueError)."""
        from . import propagate as _pg
        _pg.check_grad_order(order)
        _pg.refuse_moment(method, "SparseGP.propagate_gradient")
        _pg.check_route(route, ("auto", "host", "chain"))
        P, D = self.n_outputs_, self.n_features_in_
        x0, U, lin, S0, Q, R, H = _pg.check_horizon(x0, U, lin, P, D, Sigma0, process_noise)
        gx, gS = _pg.check_seeds(grad_traj, grad_Sigma, R, H, P)
        if route == "chain":
            why = self._propagate_refusal()
            if why:
                raise ValueError(f"route='chain' is not available: {why}")
            self._ensure()
            traj, Sigma, more = _pg.horizon_call(
                lambda *t: self._backend().call("gpk_sparse_propagate_grad", int(bool(var_includes_noise)), *t),
                x0, U, lin, S0, Q, R, H, seeds=(gx, gS))
            return (traj, Sigma, *more)
        noise = self.kernel_.components().noise or 0.0
        std2 = np.broadcast_to(np.asarray(self._y_train_std, dtype=np.float64).reshape(-1), (P,)) ** 2

        def stage(q):
            mean, dmean, var, dvar = self.predict_jacobian(q, return_var=True)
            var = var.reshape(R, P)
            if not var_includes_noise:
                var = np.maximum(var - noise * std2[None, :], 0.0)
            return mean.reshape(R, P), dmean.reshape(R, P, D), var, dvar.reshape(R, P, D)

        return _pg.host_adjoint(stage, lambda q: self.predict_hessian(q)[2], list(range(P)), x0, U, lin, S0, Q, R, H, gx, gS)

    # ------------------------------------------------------------------ exact moment matching (K11, the sparse posterior)
    def _moments_ready(self, what):
        """ValueError where `propagate_ok()` does not hold (the limits of the moment entries are the chain's)."""
        why = self._propagate_refusal()
        if why:
            raise ValueError(f"{what} is not available: {why}")

    def _moments_entry(self, entry, *args):
        try:
            self._backend().call(entry, *args)
        except _lib.GPKError as e:      # a limit of the entry: the caller's arguments, with the library's message
            if e.code == _lib.GPK_BAD_ARG:
                raise ValueError(str(e)) from None
            raise

    def predict_moments(self, X, Sigma, var_includes_noise=False):
        """`GaussianProcessRegressor.predict_moments` on the sparse posterior: its exact moments at GAUSSIAN queries q ~ N(X[m],
        Sigma[m]).  The sparse posterior is the exact model's form over the inducing inputs - weights alpha_u, and Q = Kuu^-1 -
        Sigma~ where K^-1 stands - so the closed forms carry over.  X (M, D), M <= 32; Sigma (M, nx, nx) or (nx,
        nx), symmetric positive semi-definite, over the LEADING nx <= D coordinates, or None.  Returns (mean (M, P), cov (M, P, P),
        xcov (M, P, D)); var_includes_noise adds the WhiteKernel level to cov's diagonal.  One C call (`gpk_sparse_moments`: five
        launches, one synchronisation; Q is formed on the device on the first call after the model was assembled, and again
        after it has taken rows).  RuntimeError without inducing inputs; ValueError where `propagate_ok()` does not hold."""
        from . import propagate as _pg
        if getattr(self, "inducing_", None) is None:
            raise RuntimeError("predict_moments: this SparseGP has no inducing inputs")
        X, S, M, nx = _pg.check_gaussian_queries(X, Sigma, self.n_features_in_)
        self._moments_ready("predict_moments")
        self._ensure()
        P, D = self._P, self.n_features_in_
        mean, cov, xcov = np.empty((M, P)), np.empty((M, P, P)), np.empty((M, P, D))
        self._moments_entry("gpk_sparse_moments", int(bool(var_includes_noise)), nx, _ptr(X), _ptr(S), M, _ptr(mean), _ptr(cov),
                            _ptr(xcov))
        return mean, cov, xcov

    def propagate_moments(self, x0, U, lin, Sigma0=None, process_noise=None, var_includes_noise=False, return_stages=False,
                          route="chain"):
        """`GaussianProcessRegressor.propagate(method="moment")` on the sparse posterior: the horizon with every stage's EXACT
        moments at the Gaussian query N([x_h, u_h], Sigma_h) (`predict_moments`), same arguments and results.  route="chain":
        ONE C call per horizon (`gpk_sparse_propagate_mm`: five launches per stage, one synchronisation); route="host": the same
        recursion as a host loop over `predict_moments` (`propagate.host_loop_moments`).  With return_stages the stages {"mean"
        (H, R, P), "cov" (H, R, P, P), "xcov" (H, R, P, D)}, on the chain with the bits of `predict_moments` at the returned
        rows.  RuntimeError without inducing inputs; ValueError where `propagate_ok()` does not hold or an argument is refused."""
        from . import propagate as _pg
        if getattr(self, "inducing_", None) is None:
            raise RuntimeError("propagate_moments: this SparseGP has no inducing inputs")
        _pg.check_route(route, ("chain", "host"))
        P, D = self.n_outputs_, self.n_features_in_
        x0, U, lin, S0, Q, R, H = _pg.check_horizon(x0, U, lin, P, D, Sigma0, process_noise)
        _pg.check_method("moment", 1, "propagate_moments", Sigma0=S0, process_noise=Q)
        self._moments_ready("propagate_moments")
        if route == "host":
            traj, Sigma, stages = _pg.host_loop_moments(
                lambda q, S: self.predict_moments(q, S, var_includes_noise=var_includes_noise), list(range(P)), x0, U, lin, S0, Q, R,
                H)
            return (traj, Sigma, stages) if return_stages else (traj, Sigma)
        self._ensure()
        traj, Sigma, more = _pg.horizon_call(
            lambda *t: self._backend().call("gpk_sparse_propagate_mm", int(bool(var_includes_noise)), *t),
            x0, U, lin, S0, Q, R, H, ((P,), (P, P), (P, D)) if return_stages else None)
        return (traj, Sigma, dict(zip(("mean", "cov", "xcov"), more))) if return_stages else (traj, Sigma)

    def predict_moments_vjp(self, X, Sigma, grad_mean=None, grad_cov=None, grad_xcov=None, var_includes_noise=False):
        """`GaussianProcessRegressor.predict_moments_vjp` on the sparse posterior: `predict_moments` and, for l = <grad_mean, mean>
        + <grad_cov, cov> + <grad_xcov, xcov>, dX (M, D) = dl/dX and dSigma (M, nx, nx) = dl/dSigma (symmetric bit for bit).  Seeds
        grad_mean (M, P), grad_cov (M, P, P; (g + g^T) / 2 is used), grad_xcov (M, P, D), None: zero.  Returns (mean, cov, xcov,
        dX, dSigma), the first three with the bits of `predict_moments`.  One C call (`gpk_sparse_moments_vjp`: ten launches,
        one synchronisation; Q is a constant of the adjoint).  Limits and errors as `predict_moments`."""
        from . import propagate as _pg
        if getattr(self, "inducing_", None) is None:
            raise RuntimeError("predict_moments_vjp: this SparseGP has no inducing inputs")
        P, D = self.n_outputs_, self.n_features_in_
        X, S, M, nx = _pg.check_gaussian_queries(X, Sigma, D)
        gm, gc, gxc = _pg.check_moment_seeds(grad_mean, grad_cov, grad_xcov, M, P, D)
        self._moments_ready("predict_moments_vjp")
        self._ensure()
        mean, cov, xcov = np.empty((M, P)), np.empty((M, P, P)), np.empty((M, P, D))
        dX, dS = np.empty((M, D)), np.empty((M, nx, nx))
        self._moments_entry("gpk_sparse_moments_vjp", int(bool(var_includes_noise)), nx, _ptr(X), _ptr(S), M, _ptr(mean), _ptr(cov),
                            _ptr(xcov), _ptr(gm), _ptr(gc), _ptr(gxc), _ptr(dX), _ptr(dS))
        return mean, cov, xcov, dX, dS

    def propagate_moments_gradient(self, x0, U, lin, grad_traj, grad_Sigma=None, Sigma0=None, process_noise=None,
                                   var_includes_noise=False, route="chain"):
        """`propagate_moments` with the gradient of a horizon cost l(traj, Sigma) with respect to the controls, the start state
        and the start covariance, through the exact moments of every stage
        (`GaussianProcessRegressor.propagate_moments_gradient` on the sparse posterior).  grad_traj (H + 1, R, P), grad_Sigma
        (H + 1, R, P, P) or None.  Returns (traj, Sigma, dU (R, H, nu), dx0 (R, P), dSigma0 (R, P, P)), traj and Sigma with the
        bits of `propagate_moments`.  route="chain": ONE C call per horizon (`gpk_sparse_propagate_mm_grad`: every stage's work
        block kept on the device while the horizon's fit the backend option moments_tape_mb - five launches per stage forward,
        four backward; beyond it six and seven; the same bits; one synchronisation).  route="host": the sweep on the host over
        `predict_moments` and `predict_moments_vjp` (`propagate.host_adjoint_moments`).  RuntimeError without inducing inputs;
        ValueError where `propagate_ok()` does not hold or an argument is refused."""
        from . import propagate as _pg
        if getattr(self, "inducing_", None) is None:
            raise RuntimeError("propagate_moments_gradient: this SparseGP has no inducing inputs")
        _pg.check_route(route, ("chain", "host"))
        P, D = self.n_outputs_, self.n_features_in_
        x0, U, lin, S0, Q, R, H = _pg.check_horizon(x0, U, lin, P, D, Sigma0, process_noise)
        gx, gS = _pg.check_seeds(grad_traj, grad_Sigma, R, H, P)
        _pg.check_method("moment", 1, "propagate_moments_gradient", Sigma0=S0, process_noise=Q)
        self._moments_ready("propagate_moments_gradient")
        if route == "host":
            return _pg.host_adjoint_moments(
                lambda q, S: self.predict_moments(q, S, var_includes_noise=var_includes_noise),
                lambda q, S, gm, gc, gxc: self.predict_moments_vjp(q, S, gm, gc, gxc, var_includes_noise=var_includes_noise),
                list(range(P)), x0, U, lin, S0, Q, R, H, gx, gS)
        self._ensure()
        traj, Sigma, more = _pg.horizon_call(
            lambda *t: self._backend().call("gpk_sparse_propagate_mm_grad", int(bool(var_includes_noise)), *t),
            x0, U, lin, S0, Q, R, H, seeds=(gx, gS))
        return (traj, Sigma, *more)

    def _propagate_refusal(self):
        """Why the one-call chain does not apply (a string), or None where it does."""
        from . import propagate as _pg
        if int(self._backend().options.get("small_path", 1)) == 0:
            return "the backend option small_path is 0"
        return _pg.chain_sizes_ok(self.inducing_.shape[0], self.n_features_in_, self.n_outputs_)

    def propagate_ok(self):
        """The one-call horizon propagation (`gpk_sparse_propagate`, route="chain") applies: the small-batch path is on and
        the sizes are within its limits (at most 16 384 padded inducing points, P <= D <= 16)."""
        return self._propagate_refusal() is None

    def sample_paths(self, n_paths, n_features=1024, random_state=0):
        """`n_paths` posterior function draws as explicit functions, conditioned on the inducing variables
        (`paths.SparsePosteriorPaths`; `GaussianProcessRegressor.sample_paths` for the sparse model): evaluated anywhere, call
        after call, each the same function - `step` two launches over m + n_features basis rows however many rows were fitted, a
        closed-loop `rollout` one call per horizon.  Every output draws its own numbers; the draw order is
        `paths.draw_sparse_path_randomness`'s; random_state as in `sample_y`.  A model without rows yields draws of the prior
        conditioned on nothing, as `predict` yields the prior.  The set is a snapshot of the model as it is now
        (`revision_`)."""
        from .gpr import _rng_from
        from .paths import SparsePosteriorPaths, check_path_shape, draw_sparse_path_randomness
        m, D = self.inducing_.shape
        P = self.n_outputs_
        check_path_shape(D, P, int(n_paths), int(n_features))
        ls = self.kernel_.components().ls_vector(D)
        r = draw_sparse_path_randomness(_rng_from(random_state), m, D, int(n_features), int(n_paths), P, ls)
        return SparsePosteriorPaths.from_randomness(self, **r)

    @property
    def revision_(self):
        """A counter that moves whenever the served model may have changed (rows taken, refitted, trained, hyper-parameters or
        inducing inputs moved): what a cached path set of this model is keyed by."""
        return self.__dict__.get("_rev", 0)

    def _touch(self):
        self._rev = self.__dict__.get("_rev", 0) + 1

    def bound(self):
        """The collapsed lower bound on the log-marginal likelihood of the rows seen so far, in normalised-target units (the
        exact log-marginal likelihood when the inducing inputs are the training inputs).  approximation="fitc": the FITC
        log-marginal likelihood log N(y | 0, Qff + diag(lambda)) - not a bound on the exact one; equal to it when Z = X."""
        self._ensure()
        b, n = C.c_double(0.0), C.c_int64(0)
        self._backend().call("gpk_sparse_bound", C.byref(b), C.byref(n))
        return float(b.value)

    @property
    def n_rows_(self):
        if self._state is not None:
            return int(self._state["n_rows"])
        if not self._live:
            return 0
        n = C.c_int64(0)
        self._backend().call("gpk_sparse_export", None, None, None, None, None, None, None, None, C.byref(n), None, None, None,
                             None)
        return int(n.value)

    def statistics(self):
        """The additive statistics as host arrays: {"G" (m, m), "g" (m, P), "yy" (P,), "n_rows"}; approximation="fitc": the
        weighted ones, and "log_lambda_sum" (the sum of log lambda_i over the rows, the likelihood's extra scalar)."""
        if self._state is not None:
            return dict(self._state)
        if not self._live:
            return None
        extra = {}
        if self._fitc:
            kind, lam = C.c_int(0), C.c_double(0.0)
            self._backend().call("gpk_sparse_get_approximation", C.byref(kind), C.byref(lam))
            extra["log_lambda_sum"] = float(lam.value)
        m, P = self.inducing_.shape[0], self._P
        G, g, yy = np.empty((m, m)), np.empty((m, P)), np.empty(P)
        n = C.c_int64(0)
        self._backend().call("gpk_sparse_export", None, None, None, None, None, _ptr(G), _ptr(g), _ptr(yy), C.byref(n), None, None,
                             None, None)
        return {"G": G, "g": g, "yy": yy, "n_rows": int(n.value), **extra}

    # ------------------------------------------------------------------ pickling: Z, the statistics, the hyper-parameters
    def __getstate__(self):
        st = self.__dict__.copy()
        st["_state"] = self.statistics()
        st["_be"], st["_live"], st["_final"], st["_held"] = None, False, False, False
        if isinstance(st["device"], Backend):
            st["device"] = st["device"].device_index
        return st

    def __setstate__(self, st):
        self.__dict__.update(st)
        self.__dict__.setdefault("approximation_", "dtc")      # (pickles written before the attribute existed)

    def __del__(self):
        be = self.__dict__.get("_be")
        if be is not None and not isinstance(self.__dict__.get("device"), Backend):
            try:
                be.close()
            except Exception:
                pass
