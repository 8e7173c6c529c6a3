"""The per-axis batch of sparse GPs (DESIGN.md, K9 "the per-axis batch"): up to eight single-output `SparseGP` models of equal
m and D - each with its own kernel, noise, target normalisation and inducing inputs - served for one query batch in ONE C call
(`gpk_sparse_predict_multi[_grad|_cov]`: up to 32 rows one to three launches and one synchronisation for all models).

The class adds nothing to how one model is fitted or trained: every `SparseGP` keeps its own handle, statistics, pickling,
`train` and `select_inducing`.  The serving calls return what `BatchedARDGP` returns for exact models - means (M, B),
Jacobians (M, B, D), covariances (M, M, B) - so that `PreTrainedGP` uses either.
"""
from __future__ import annotations

import contextlib
import ctypes as C

import numpy as np

from . import _lib
from .device import check_queries
from .gpr import cholesky_draws
from .sparse import SparseGP, _ptr

MAX_MODELS = 8


class BatchedSparseGP:
    def __init__(self, models):
        models = list(models)
        if not 1 <= len(models) <= MAX_MODELS:
            raise ValueError(f"a batch holds 1 to {MAX_MODELS} models, got {len(models)}")
        for m in models:
            if not isinstance(m, SparseGP):
                raise ValueError(f"every model must be a SparseGP, got {type(m).__name__}")
            if m.n_outputs_ != 1:
                raise ValueError("every model of a batch must have one output")
        shape = models[0].inducing_.shape
        for m in models[1:]:
            if m.inducing_.shape != shape:
                raise ValueError(f"the models must agree in m and D: {m.inducing_.shape} against {shape}")
        if len({id(m) for m in models}) != len(models):
            raise ValueError("a model may appear once in a batch")
        self.models = models

    @classmethod
    def from_exact(cls, gprs, inducing=None, selection="random", random_state=0, approximation="dtc"):
        """`SparseGP.from_exact` per model: gprs is a list of fitted single-output `GaussianProcessRegressor`s or a fitted
        `BatchedARDGP`; `inducing` as there (an integer: that many of each model's own training rows); `approximation`: "dtc"
        or "fitc" for all of them.  (A batch built from models may mix the two: serving does not depend on the kind.)"""
        gprs = getattr(gprs, "models", gprs)
        return cls([SparseGP.from_exact(g, inducing, random_state=random_state, selection=selection, approximation=approximation)
                    for g in gprs])

    @property
    def approximations_(self):
        """The models' kinds, "dtc" or "fitc" each."""
        return [m.approximation_ for m in self.models]

    @property
    def n_features_in_(self):
        return self.models[0].n_features_in_

    # ------------------------------------------------------------------ rows: column b of Y goes to model b
    def _columns(self, Y):
        Y = np.asarray(Y, dtype=np.float64)
        if Y.ndim == 1 and len(self.models) == 1:
            Y = Y.reshape(-1, 1)
        if Y.ndim != 2 or Y.shape[1] != len(self.models):
            raise ValueError(f"Y must be (n, {len(self.models)})")
        return Y

    def partial_fit(self, X, Y):
        Y = self._columns(Y)
        for b, m in enumerate(self.models):
            m.partial_fit(X, np.ascontiguousarray(Y[:, b]))
        return self

    def fit(self, X, Y):
        Y = self._columns(Y)
        for b, m in enumerate(self.models):
            m.fit(X, np.ascontiguousarray(Y[:, b]))
        return self

    def train(self, X, Y, **kw):
        """`SparseGP.train(X, Y[:, b], **kw)` for each model in turn: sequential - nothing of the six trainings is fused."""
        Y = self._columns(Y)
        for b, m in enumerate(self.models):
            m.train(X, np.ascontiguousarray(Y[:, b]), **kw)
        return self

    # ------------------------------------------------------------------ serving
    def _queries(self, X):
        return check_queries(X, self.n_features_in_)

    def _ensure(self):
        """Every model assembled (lazily, as `SparseGP.predict` does); returns the serving backend - the first model's - and
        the array of handles."""
        for m in self.models:
            m._ensure()
            if m._P != 1:
                raise ValueError("every model of a batch must have one output")
        bes = [m._backend() for m in self.models]
        if len({id(be) for be in bes}) != len(bes):
            raise ValueError("the models of a batch need a handle each (do not share a Backend between them)")
        handles = (C.c_void_p * len(bes))(*[be.h.value for be in bes])
        return bes, handles

    @contextlib.contextmanager
    def _serving(self):
        bes, handles = self._ensure()
        with contextlib.ExitStack() as stack:
            for be in bes:      # list order: two batches over the same models take the locks in the same order
                stack.enter_context(be.lock)
            yield bes[0], handles

    def predict(self, Xq, return_std=False, return_cov=False):
        """Means (M, B); with return_std the standard deviations (M, B), each model's WhiteKernel level included as
        `SparseGP.predict` has it; with return_cov every model's joint covariance over the rows, (mean (M, B),
        cov (M, M, B)) in target units (at most 16 384 rows).  Up to 32 rows: one C call, one launch for the means, two with
        either second result, one synchronisation - for all models; column b has the bits of `models[b].predict`."""
        if return_std and return_cov:
            raise RuntimeError("At most one of return_std or return_cov can be requested.")
        X = self._queries(Xq)
        M, B = X.shape[0], len(self.models)
        mean = np.full((M, B), np.nan)
        if return_cov:
            cov = np.full((B, M, M), np.nan)
            if M > 0:
                with self._serving() as (be, handles):
                    be.call("gpk_sparse_predict_multi_cov", B, handles, _ptr(X), M, _ptr(mean), _ptr(cov))
            return mean, np.ascontiguousarray(np.moveaxis(cov, 0, -1))
        var = np.full((M, B), np.nan) if return_std else None
        if M > 0:
            with self._serving() as (be, handles):
                be.call("gpk_sparse_predict_multi", B, handles, _ptr(X), M, _ptr(mean), _ptr(var), 1)
        return (mean, np.sqrt(var)) if return_std else mean

    def predict_jacobian(self, Xq, return_var=False):
        """(mean (M, B), dmean (M, B, D)) and, with return_var, (var (M, B), dvar (M, B, D)): `SparseGP.predict_jacobian` of
        every model in one call (`gpk_sparse_predict_multi_grad`; up to 32 rows one launch, three with the variances, one
        synchronisation).  The shapes of `BatchedARDGP.predict_jacobian`."""
        X = self._queries(Xq)
        M, D, B = X.shape[0], X.shape[1], len(self.models)
        mean, dmean = np.full((M, B), np.nan), np.full((M, B, D), np.nan)
        var = np.full((M, B), np.nan) if return_var else None
        dvar = np.full((M, B, D), np.nan) if return_var else None
        if M > 0:
            with self._serving() as (be, handles):
                be.call("gpk_sparse_predict_multi_grad", B, handles, _ptr(X), M, _ptr(mean), _ptr(var), _ptr(dmean),
                        _ptr(dvar), 1)
        return (mean, dmean, var, dvar) if return_var else (mean, dmean)

    def predict_hessian(self, Xq):
        """(mean (M, B), dmean (M, B, D), hess (M, B, D, D)): `SparseGP.predict_hessian` of every model in one call
        (`gpk_sparse_predict_multi_hess`, one synchronisation up to 32 rows); mean and dmean are those of `predict_jacobian`
        bit for bit, column b has the bits of `models[b].predict_hessian`.  The shapes of `BatchedARDGP.predict_hessian`."""
        X = self._queries(Xq)
        M, D, B = X.shape[0], X.shape[1], len(self.models)
        mean, dmean, hess = np.full((M, B), np.nan), np.full((M, B, D), np.nan), np.full((M, B, D, D), np.nan)
        if M > 0:
            with self._serving() as (be, handles):
                be.call("gpk_sparse_predict_multi_hess", B, handles, _ptr(X), M, _ptr(mean), _ptr(dmean), _ptr(hess))
        return mean, dmean, hess

    def propagate(self, x0, U, lin, coord=None, in_scaler=None, Sigma0=None, process_noise=None, var_includes_noise=False,
                  return_stages=False, out_scaler=None, route="auto", order=1, method="linear"):
        """`BatchedARDGP.propagate` on the sparse posteriors: the batch's mean rollout with the linearised state covariance in
        raw units, same arguments and results.  route="auto" and "host": the recursion as a host loop over
        `predict_jacobian(..., return_var=True)` - one C call for all models and one synchronisation per stage.
        route="chain": ONE C call per horizon for all models (`gpk_sparse_propagate_multi`: three launches per stage, one
        synchronisation; the scalers go into the call; the latent variance as `SparseGP.propagate` describes it).  ValueError
        where `propagate_ok()` does not hold, with the reason, or where the entry refuses its arguments.  order=2: the
        second-order mean on every route (chain: `gpk_sparse_propagate2_multi`, four launches per stage; the host loop contracts
        `predict_hessian`); the stages gain "corr" (H, R, B).  method: "linear" only - exact moment matching
        is `propagate_moments` on this class; method="moment" here: ValueError."""
        from . import propagate as _pg
        order = _pg.check_order(order)
        _pg.refuse_moment(method, "BatchedSparseGP")
        B, D = len(self.models), self.n_features_in_
        x0, U, lin, S0, Q, R, H, coord, in_shift, in_scale, o_mean, o_scale = _pg.check_batch(
            B, D, x0, U, lin, coord, in_scaler, out_scaler, Sigma0, process_noise, route, routes=("auto", "host", "chain"))
        if route == "chain":
            nx = lin.shape[0]
            why = self._propagate_refusal(nx)
            if why:
                raise ValueError(f"route='chain' is not available: {why}")
            traj, Sigma, more = _pg.horizon_call(
                self._chain_call("gpk_sparse_propagate_multi" if order == 1 else "gpk_sparse_propagate2_multi", var_includes_noise, nx,
                                 coord, in_shift, in_scale, out_scaler, o_mean, o_scale),
                x0, U, lin, S0, Q, R, H, ((B,), (B,), (B, D)) if return_stages else None, None if order == 1 else order)
            return (traj, Sigma, dict(zip(("mean", "var", "jac", "corr"), more))) if return_stages else (traj, Sigma)
        stage = _pg.batch_stage(self.predict_jacobian, _pg.noise_levels(self.models), in_shift, in_scale, o_mean, o_scale,
                                var_includes_noise)
        hess_stage = _pg.batch_hess_stage(self.predict_hessian, in_shift, in_scale, o_scale) if order == 2 else None
        traj, Sigma, stages = _pg.host_loop(stage, coord, x0, U, lin, S0, Q, R, H, hess_stage)
        return (traj, Sigma, stages) if return_stages else (traj, Sigma)

    def propagate_gradient(self, x0, U, lin, grad_traj, grad_Sigma=None, coord=None, in_scaler=None, Sigma0=None,
                           process_noise=None, var_includes_noise=False, out_scaler=None, route="auto", order=1, method="linear"):
        """`BatchedARDGP.propagate_gradient` on the sparse posteriors: `propagate` with the gradient of a horizon cost, raw
        units, same arguments and results.  route="auto" and "host": the sweep on the host over `predict_jacobian` and
        `predict_hessian` (one C call each for all models per stage).  route="chain": ONE C call per horizon for all models
        (`gpk_sparse_propagate_grad_multi`: six launches per stage, one synchronisation; traj and Sigma with the bits of
        `propagate(route="chain")`); ValueError where `propagate_ok()` does not hold.  order: 1 only (ValueError)."""
        from . import propagate as _pg
        _pg.check_grad_order(order)
        _pg.refuse_moment(method, "BatchedSparseGP.propagate_gradient")
        B, D = len(self.models), self.n_features_in_
        x0, U, lin, S0, Q, R, H, coord, in_shift, in_scale, o_mean, o_scale = _pg.check_batch(
            B, D, x0, U, lin, coord, in_scaler, out_scaler, Sigma0, process_noise, route, routes=("auto", "host", "chain"))
        nx = lin.shape[0]
        gx, gS = _pg.check_seeds(grad_traj, grad_Sigma, R, H, nx)
        if route == "chain":
            why = self._propagate_refusal(nx)
            if why:
                raise ValueError(f"route='chain' is not available: {why}")
            traj, Sigma, more = _pg.horizon_call(
                self._chain_call("gpk_sparse_propagate_grad_multi", var_includes_noise, nx, coord, in_shift, in_scale, out_scaler,
                                 o_mean, o_scale),
                x0, U, lin, S0, Q, R, H, seeds=(gx, gS))
            return (traj, Sigma, *more)
        stage = _pg.batch_stage(self.predict_jacobian, _pg.noise_levels(self.models), in_shift, in_scale, o_mean, o_scale,
                                var_includes_noise, with_dvar=True)
        hess_stage = _pg.batch_hess_stage(self.predict_hessian, in_shift, in_scale, o_scale)
        return _pg.host_adjoint(stage, hess_stage, coord, x0, U, lin, S0, Q, R, H, gx, gS)

    # ------------------------------------------------------------------ exact moment matching (K11, the sparse posteriors)
    def _moments_ready(self, what, nx=None):
        """ValueError where `propagate_ok()` does not hold (the limits of the moment entries are the chain's)."""
        why = self._propagate_refusal(nx)
        if why:
            raise ValueError(f"{what} is not available: {why}")

    def predict_moments(self, X, Sigma, in_scaler=None, out_scaler=None, var_includes_noise=False):
        """`BatchedARDGP.predict_moments` on the sparse posteriors, in raw units: the joint posterior of the B models at GAUSSIAN
        queries q ~ N(X[m], Sigma[m]), all B (B + 1) / 2 pairs of models included, each model on its own inducing inputs with Q =
        Kuu^-1 - Sigma~ where K^-1 stands (`SparseGP.predict_moments`).  X (M, D) raw, M <= 32; Sigma (M, nx, nx) or (nx, nx) or
        None; in_scaler / out_scaler as `propagate`.  Returns (mean (M, B), cov (M, B, B), xcov (M, B, D)).  One C call
        (`gpk_sparse_moments_multi`, five launches for all models and pairs, one synchronisation).  RuntimeError without models;
        ValueError where `propagate_ok()` does not hold."""
        from . import propagate as _pg
        if not getattr(self, "models", None):
            raise RuntimeError("predict_moments: this BatchedSparseGP has no models (no inducing inputs)")
        B, D = len(self.models), self.n_features_in_
        X, S, M, nx = _pg.check_gaussian_queries(X, Sigma, D)
        in_shift, in_scale, o_mean, o_scale = _pg.check_scalers(B, D, in_scaler, out_scaler)
        self._moments_ready("predict_moments", nx)
        scaled = out_scaler is not None
        om = np.ascontiguousarray(o_mean, dtype=np.float64) if scaled else None
        osc = np.ascontiguousarray(o_scale, dtype=np.float64) if scaled else None
        mean, cov, xcov = np.full((M, B), np.nan), np.full((M, B, B), np.nan), np.full((M, B, D), np.nan)
        try:
            with self._serving() as (be, handles):
                be.call("gpk_sparse_moments_multi", B, handles, int(bool(var_includes_noise)), nx, _ptr(in_shift), _ptr(in_scale),
                        _ptr(om), _ptr(osc), _ptr(X), _ptr(S), M, _ptr(mean), _ptr(cov), _ptr(xcov))
        except _lib.GPKError as e:      # a limit of the entry: the caller's arguments, with the library's message
            if e.code == _lib.GPK_BAD_ARG:
                raise ValueError(str(e)) from None
            raise
        return mean, cov, xcov

    def propagate_moments(self, x0, U, lin, coord=None, in_scaler=None, Sigma0=None, process_noise=None, var_includes_noise=False,
                          return_stages=False, out_scaler=None, route="chain"):
        """`BatchedARDGP.propagate(method="moment")` on the sparse posteriors: the batch's horizon with every stage's EXACT
        moments (`predict_moments`), raw units, same arguments and results.  route="chain": ONE C call per horizon for all models
        (`gpk_sparse_propagate_mm_multi`: five launches per stage, one synchronisation; the scalers go into the call);
        route="host": the same recursion as a host loop over `predict_moments`.  The stages are {"mean" (H, R, B), "cov" (H, R,
        B, B), "xcov" (H, R, B, D)}.  RuntimeError without models; ValueError where `propagate_ok()` does not hold or an argument
        is refused."""
        from . import propagate as _pg
        if not getattr(self, "models", None):
            raise RuntimeError("propagate_moments: this BatchedSparseGP has no models (no inducing inputs)")
        B, D = len(self.models), self.n_features_in_
        x0, U, lin, S0, Q, R, H, coord, in_shift, in_scale, o_mean, o_scale = _pg.check_batch(
            B, D, x0, U, lin, coord, in_scaler, out_scaler, Sigma0, process_noise, route, routes=("chain", "host"))
        _pg.check_method("moment", 1, "propagate_moments", Sigma0=S0, process_noise=Q)
        nx = lin.shape[0]
        self._moments_ready("propagate_moments", nx)
        if route == "host":
            traj, Sigma, stages = _pg.host_loop_moments(
                lambda q, S: self.predict_moments(q, S, in_scaler=in_scaler, out_scaler=out_scaler,
                                                  var_includes_noise=var_includes_noise), coord, x0, U, lin, S0, Q, R, H)
            return (traj, Sigma, stages) if return_stages else (traj, Sigma)
        traj, Sigma, more = _pg.horizon_call(
            self._chain_call("gpk_sparse_propagate_mm_multi", var_includes_noise, nx, coord, in_shift, in_scale, out_scaler, o_mean,
                             o_scale),
            x0, U, lin, S0, Q, R, H, ((B,), (B, B), (B, D)) if return_stages else None)
        return (traj, Sigma, dict(zip(("mean", "cov", "xcov"), more))) if return_stages else (traj, Sigma)

    def predict_moments_vjp(self, X, Sigma, grad_mean=None, grad_cov=None, grad_xcov=None, in_scaler=None, out_scaler=None,
                            var_includes_noise=False):
        """`BatchedARDGP.predict_moments_vjp` on the sparse posteriors, in raw units: `predict_moments` and, for the seeds
        grad_mean (M, B), grad_cov (M, B, B; (g + g^T) / 2 is used), grad_xcov (M, B, D) (None: zero), dX (M, D) and dSigma (M, nx,
        nx; symmetric bit for bit) per unit of the raw query and its raw covariance.  Returns (mean, cov, xcov, dX, dSigma), the
        first three with the bits of `predict_moments`.  One C call (`gpk_sparse_moments_vjp_multi`: ten launches for all models
        and pairs, one synchronisation).  Limits and errors as `predict_moments`."""
        from . import propagate as _pg
        if not getattr(self, "models", None):
            raise RuntimeError("predict_moments_vjp: this BatchedSparseGP has no models (no inducing inputs)")
        B, D = len(self.models), self.n_features_in_
        X, S, M, nx = _pg.check_gaussian_queries(X, Sigma, D)
        gm, gc, gxc = _pg.check_moment_seeds(grad_mean, grad_cov, grad_xcov, M, B, D)
        in_shift, in_scale, o_mean, o_scale = _pg.check_scalers(B, D, in_scaler, out_scaler)
        self._moments_ready("predict_moments_vjp", nx)
        scaled = out_scaler is not None
        om = np.ascontiguousarray(o_mean, dtype=np.float64) if scaled else None
        osc = np.ascontiguousarray(o_scale, dtype=np.float64) if scaled else None
        mean, cov, xcov = np.full((M, B), np.nan), np.full((M, B, B), np.nan), np.full((M, B, D), np.nan)
        dX, dS = np.full((M, D), np.nan), np.full((M, nx, nx), np.nan)
        try:
            with self._serving() as (be, handles):
                be.call("gpk_sparse_moments_vjp_multi", B, handles, int(bool(var_includes_noise)), nx, _ptr(in_shift), _ptr(in_scale),
                        _ptr(om), _ptr(osc), _ptr(X), _ptr(S), M, _ptr(mean), _ptr(cov), _ptr(xcov), _ptr(gm), _ptr(gc), _ptr(gxc),
                        _ptr(dX), _ptr(dS))
        except _lib.GPKError as e:      # a limit of the entry: the caller's arguments, with the library's message
            if e.code == _lib.GPK_BAD_ARG:
                raise ValueError(str(e)) from None
            raise
        return mean, cov, xcov, dX, dS

    def propagate_moments_gradient(self, x0, U, lin, grad_traj, grad_Sigma=None, coord=None, in_scaler=None, Sigma0=None,
                                   process_noise=None, var_includes_noise=False, out_scaler=None, route="chain"):
        """`propagate_moments` with the gradient of a horizon cost, in raw units: `BatchedARDGP.propagate_moments_gradient` on the
        sparse posteriors (coord, in_scaler, out_scaler as `propagate`).  Returns (traj, Sigma, dU (R, H, nu), dx0 (R, nx),
        dSigma0 (R, nx, nx)), traj and Sigma with the bits of `propagate_moments`.  route="chain": ONE C call per horizon for all
        models and pairs (`gpk_sparse_propagate_mm_grad_multi`; the launches as `SparseGP.propagate_moments_gradient` describes
        them); route="host": the sweep on the host over `predict_moments` and `predict_moments_vjp`.  RuntimeError without
        models; ValueError where `propagate_ok()` does not hold or an argument is refused."""
        from . import propagate as _pg
        if not getattr(self, "models", None):
            raise RuntimeError("propagate_moments_gradient: this BatchedSparseGP has no models (no inducing inputs)")
        B, D = len(self.models), self.n_features_in_
        x0, U, lin, S0, Q, R, H, coord, in_shift, in_scale, o_mean, o_scale = _pg.check_batch(
            B, D, x0, U, lin, coord, in_scaler, out_scaler, Sigma0, process_noise, route, routes=("chain", "host"))
        nx = lin.shape[0]
        gx, gS = _pg.check_seeds(grad_traj, grad_Sigma, R, H, nx)
        _pg.check_method("moment", 1, "propagate_moments_gradient", Sigma0=S0, process_noise=Q)
        self._moments_ready("propagate_moments_gradient", nx)
        if route == "host":
            kw = dict(in_scaler=in_scaler, out_scaler=out_scaler, var_includes_noise=var_includes_noise)
            return _pg.host_adjoint_moments(lambda q, S: self.predict_moments(q, S, **kw),
                                            lambda q, S, gm, gc, gxc: self.predict_moments_vjp(q, S, gm, gc, gxc, **kw),
                                            coord, x0, U, lin, S0, Q, R, H, gx, gS)
        traj, Sigma, more = _pg.horizon_call(
            self._chain_call("gpk_sparse_propagate_mm_grad_multi", var_includes_noise, nx, coord, in_shift, in_scale, out_scaler,
                             o_mean, o_scale),
            x0, U, lin, S0, Q, R, H, seeds=(gx, gS))
        return (traj, Sigma, *more)

    def _chain_call(self, entry, var_includes_noise, nx, coord, in_shift, in_scale, out_scaler, o_mean, o_scale):
        """The call of a chain entry of the batch for `propagate.horizon_call`, which supplies the horizon's arguments."""
        B = len(self.models)
        scaled = out_scaler is not None
        om = np.ascontiguousarray(o_mean, dtype=np.float64) if scaled else None
        osc = np.ascontiguousarray(o_scale, dtype=np.float64) if scaled else None

        def call(*tail):
            with self._serving() as (be, handles):
                be.call(entry, B, handles, int(bool(var_includes_noise)), nx, (C.c_int * B)(*coord), _ptr(in_shift), _ptr(in_scale),
                        _ptr(om), _ptr(osc), *tail)
        return call

    def _propagate_refusal(self, nx=None):
        """Why the one-call chain does not apply (a string), or None where it does; nx: the state width (default B)."""
        from . import propagate as _pg
        if int(self.models[0]._backend().options.get("small_path", 1)) == 0:
            return "the backend option small_path is 0"
        return _pg.chain_sizes_ok(self.models[0].inducing_.shape[0], self.n_features_in_, len(self.models) if nx is None else nx)

    def propagate_ok(self):
        """The one-call horizon propagation (`gpk_sparse_propagate_multi`, route="chain") applies: the small-batch path of the
        serving backend (the first model's) is on and the sizes are within its limits (at most 16 384 padded inducing points,
        B <= nx <= D <= 16)."""
        return self._propagate_refusal() is None

    def sample_y(self, Xq, n_samples=1, random_state=0):
        """Draws from every model's joint posterior at the rows Xq: (M, B, n_samples), through the Cholesky factor of each
        covariance (`gpr.cholesky_draws`), as `BatchedARDGP.sample_y`."""
        mean, cov = self.predict(Xq, return_cov=True)
        return cholesky_draws(mean, cov, n_samples, random_state)

    def sample_paths(self, n_paths, n_features=1024, random_state=0):
        """`n_paths` posterior function draws of EVERY model as explicit functions (`paths.BatchedSparsePosteriorPaths`), each
        conditioned on its model's own inducing variables: evaluated anywhere, call after call, all models in one call - `step`
        two launches (`gpk_paths_step_multi_z`), a closed-loop `rollout` one call per horizon.  The draw order is
        `paths.draw_sparse_batch_path_randomness`'s (model by model from the one generator); random_state as in `sample_y`.
        The set is a snapshot of the models as they are now (`revision_`)."""
        from .gpr import _rng_from
        from .paths import BatchedSparsePosteriorPaths, check_batch_path_shape, draw_sparse_batch_path_randomness
        m, D = self.models[0].inducing_.shape
        check_batch_path_shape(len(self.models), D, int(n_paths), int(n_features))
        ls = np.stack([mm.kernel_.components().ls_vector(D) for mm in self.models])
        r = draw_sparse_batch_path_randomness(_rng_from(random_state), m, D, int(n_features), int(n_paths), ls)
        return BatchedSparsePosteriorPaths.from_randomness(self, **r)

    @property
    def revision_(self):
        """The models' revisions (`SparseGP.revision_`): what a cached path set of the batch is keyed by."""
        return tuple(mm.revision_ for mm in self.models)

    # ------------------------------------------------------------------ pickling: the models' own state
    def __getstate__(self):
        return {"models": self.models}

    def __setstate__(self, st):
        self.models = st["models"]
