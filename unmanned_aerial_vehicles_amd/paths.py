"""Posterior function draws of the exact GP by pathwise conditioning, on MI355X.

A posterior draw as an explicit function (Wilson et al. 2020), in normalised-target units:

    f_s(x) = phi(x)^T w_s + k(x, X) v_s,    v_s = K^-1 (y_n - Phi w_s - eps_s),    K = k(X, X) + (noise + alpha) I
    phi_f(x) = sqrt(2 sf2 / F) cos(omega_f . x + b_f),  omega_f ~ N(0, diag(1 / ls^2)),  b_f ~ U(0, 2 pi),
    w_s ~ N(0, I_F),  eps_s ~ N(0, (noise + alpha) I)

and the value served is y_mean + y_std f_s(x).  After the one-time set-up (`gpk_paths_prepare`: three tile GEMMs through the
inverse factor the serving path already holds) every path is ONE column block of a coefficient matrix over N + F basis rows, so
that S paths can each be evaluated at their own point - the state their own last draw produced - in one streaming pass
(`gpk_paths_step`), and a whole closed-loop horizon in one call (`gpk_paths_rollout`).  A path stays the same function from
call to call.  The only approximation is the finite F of the prior term.  fp64, one GPU, the exact model only; there is no CPU
fallback.

The per-axis batch (`BatchedARDGP`: B single-output models on shared inputs, each with its own kernel) has the same three
surfaces in `BatchedPosteriorPaths`: one model-major coefficient matrix, set up by one `gpk_paths_prepare` per model, `step` for all
models in two launches (`gpk_paths_step_multi`), a horizon in raw units in one call (`gpk_paths_rollout_multi`).

The sparse models (`SparseGP`, `BatchedSparseGP`) have them too, conditioned on the inducing variables: `SparsePosteriorPaths` and
`BatchedSparsePosteriorPaths` at the end of this file - the same coefficient matrix over m + F basis rows, set up by
`gpk_sparse_paths_prepare`; the batch through `gpk_paths_step_multi_z` / `gpk_paths_rollout_multi_z` (basis points per model).
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .device import DeviceGP, _hp, _p, _torch, _vec, check_queries, padded

MAX_PATHS, MAX_FEATURES, MAX_HORIZON = 4096, 16384, 256


def draw_path_randomness(rng, N, D, F, S, P, ls, noise_plus_alpha):
    """The random numbers of a path set, pure NumPy: dict(omega (F, D), phase (F,), weights (F, S, P), eps (N, S, P)).

    Draw order, from `rng` (a `numpy.random.RandomState` or `Generator`):
      1. z = rng.standard_normal((F, D));   omega = z / ls           (ls: scalar or (D,))
      2. phase = rng.uniform(0, 2 pi, F)
      3. weights = rng.standard_normal((F, S, P))
      4. eps = sqrt(noise_plus_alpha) * rng.standard_normal((N, S, P))"""
    N, D, F, S, P = (int(v) for v in (N, D, F, S, P))
    if min(N, D, F, S, P) < 1:
        raise ValueError("N, D, F, S and P must be at least 1")
    if not noise_plus_alpha >= 0.0:
        raise ValueError("noise_plus_alpha must be non-negative")
    ls = _vec(ls, D)
    omega = rng.standard_normal((F, D)) / ls
    phase = rng.uniform(0.0, 2.0 * np.pi, F)
    weights = rng.standard_normal((F, S, P))
    eps = np.sqrt(float(noise_plus_alpha)) * rng.standard_normal((N, S, P))
    return {"omega": omega, "phase": phase, "weights": weights, "eps": eps}


def check_path_shape(D, P, S, F, H=None):
    """The limits of the family (include/gpk.h, K10) as ValueErrors, before any launch."""
    if not 1 <= D <= DeviceGP.MAX_FEATURES:
        raise ValueError(f"D must be in [1, {DeviceGP.MAX_FEATURES}] (got {D})")
    if not 1 <= P <= _lib.GPK_MAX_P:
        raise ValueError(f"P must be in [1, {_lib.GPK_MAX_P}] (got {P})")
    if not 1 <= S <= MAX_PATHS:
        raise ValueError(f"the number of paths must be in [1, {MAX_PATHS}] (got {S})")
    if not 1 <= F <= MAX_FEATURES:
        raise ValueError(f"the number of features must be in [1, {MAX_FEATURES}] (got {F})")
    if H is not None and not 1 <= H <= MAX_HORIZON:
        raise ValueError(f"the horizon must be in [1, {MAX_HORIZON}] stages (got {H})")


class PosteriorPaths:
    """S posterior function draws of a fitted `GaussianProcessRegressor`, resident on its GPU.

    paths(X)                    all paths at the same M points: (M, S), or (M, P, S) for P > 1 (`sample_y`'s convention)
    paths.step(Xs)              Xs (S, D): path s at row s -> (S,) or (S, P); the hot path, two launches
    paths.rollout(x0, U, lin)   a closed-loop horizon in one call -> (H + 1, S, P)
    paths.randomness            dict(omega, phase, weights, eps) it was built from
    paths.coef                  the device coefficient matrix (N + F, S P), column s P + p"""

    def __init__(self):
        raise TypeError("use GaussianProcessRegressor.sample_paths or PosteriorPaths.from_randomness")

    @classmethod
    def from_randomness(cls, gp, omega, phase, weights, eps):
        """The path set of the fitted model `gp` from arrays of the caller's own: omega (F, D), phase (F,), weights (F, S, P)
        (or (F, S) for one output) = the w_s, eps (N, S, P) (or (N, S)) = the eps_s, already scaled by sqrt(noise + alpha)."""
        gp._ensure_device()
        dev = gp._dev
        if dev.replica:
            raise RuntimeError("a serving replica holds no fp64 inverse factor: paths are drawn on the rank that fitted the model")
        N, D, P = dev.N, dev.D, dev.P
        omega = np.ascontiguousarray(omega, dtype=np.float64)
        phase = np.ascontiguousarray(phase, dtype=np.float64)
        weights = np.ascontiguousarray(weights, dtype=np.float64)
        eps = np.ascontiguousarray(eps, dtype=np.float64)
        if omega.ndim != 2 or omega.shape[1] != D:
            raise ValueError(f"omega must be (F, {D})")
        F = omega.shape[0]
        if phase.shape != (F,):
            raise ValueError(f"phase must be ({F},)")
        if weights.ndim == 2 and P == 1:
            weights = weights[:, :, None]
        if eps.ndim == 2 and P == 1:
            eps = eps[:, :, None]
        if weights.ndim != 3 or weights.shape[0] != F or weights.shape[2] != P:
            raise ValueError(f"weights must be ({F}, S, {P})")
        S = weights.shape[1]
        if eps.shape != (N, S, P):
            raise ValueError(f"eps must be ({N}, {S}, {P})")
        check_path_shape(D, P, S, F)
        if padded(N) + padded(F) > 65535:
            raise ValueError("gpk_padded(N) + gpk_padded(F) must not exceed 65535")
        for name, a in (("omega", omega), ("phase", phase), ("weights", weights), ("eps", eps)):
            if not np.isfinite(a).all():
                raise ValueError(f"{name} contains NaN or infinity.")
        self = object.__new__(cls)
        torch = _torch()
        be = dev.be
        self.gp, self._dev, self.be = gp, dev, be
        self._X = dev.X
        self.N, self.D, self.P, self.F, self.S = N, D, P, F, S
        self.randomness = {"omega": omega, "phase": phase, "weights": weights, "eps": eps}
        self._ls = np.ascontiguousarray(dev.ls, dtype=np.float64).copy()
        self._sf2 = float(dev.sf2)
        self._y_mean = _vec(gp._y_train_mean, P)
        self._y_std = _vec(gp._y_train_std, P)
        self._omega = be.upload(omega)
        self._phase = be.upload(phase)
        C = S * P
        self.coef = be.empty((N + F, C), torch.float64)
        with be.lock:
            W = dev.inverse_factor(False)
            w_d = be.upload(weights.reshape(F, C))
            e_d = be.upload(eps.reshape(N, C))
            be.call("gpk_paths_prepare", _p(dev.X), N, D, _p(dev.Yn), P, _p(W), dev.Np, dev.Np, _p(self._omega), _p(self._phase),
                    F, self._sf2, _p(w_d), _p(e_d), S, _p(self.coef), C)
            be.sync()       # (w_d and e_d are released here: the set-up is not the hot path)
        return self

    # ---- the model's side of every call: X, N, D, ls, sf2, Omega, phase, F, Coef, ldc, S, P, y_mean, y_std
    def _model_args(self):
        return (_p(self._X), self.N, self.D, _hp(self._ls), self._sf2, _p(self._omega), _p(self._phase), self.F,
                _p(self.coef), self.S * self.P, self.S, self.P, _hp(self._y_mean), _hp(self._y_std))

    def _squeeze(self, a):
        return a[..., 0] if self.P == 1 else a

    def __call__(self, X):
        """Every path at the same M points: (M, S), or (M, P, S) for P > 1.  Built from gpk_cross_gram_t, gpk_rff_features and
        two gpk_gemm_tiles products; not a hot path."""
        torch = _torch()
        X = check_queries(X, self.D)
        M = X.shape[0]
        if M == 0:
            return np.empty((0, self.S) if self.P == 1 else (0, self.P, self.S))
        be = self.be
        N, F, D, C = self.N, self.F, self.D, self.S * self.P
        Np, Fp, Mp, Cp = padded(N), padded(F), padded(M), padded(C)
        q = be.upload(X)
        # the two row blocks of Coef in the padded shape of the tile GEMM, zeros in the padding
        cv = torch.zeros((Np, Cp), dtype=torch.float64, device=be.device)
        cw = torch.zeros((Fp, Cp), dtype=torch.float64, device=be.device)
        cv[:N, :C] = self.coef[:N]
        cw[:F, :C] = self.coef[N:]
        kt = be.empty((Np, Mp), torch.float64)
        phi = be.empty((Mp, Fp), torch.float64)
        out = be.empty((Mp, Cp), torch.float64)
        with be.lock:
            be.call("gpk_cross_gram_t", _lib.GPK_F64, _p(self._X), N, _p(q), M, D, _hp(self._ls), self._sf2, _p(kt), Mp)
            be.call("gpk_rff_features", _p(q), M, D, _p(self._omega), _p(self._phase), F, 1.0, _p(phi), Fp)
            # out = K*^T V (kt is stored training-row major: ta = 1) + Phi(Xq) W~
            be.call("gpk_gemm_tiles", _lib.GPK_F64, 1, 1, _p(kt), Mp, _p(cv), Cp, _p(out), Cp, Mp, Cp, Np, 1.0, 0.0, 0)
            be.call("gpk_gemm_tiles", _lib.GPK_F64, 0, 1, _p(phi), Fp, _p(cw), Cp, _p(out), Cp, Mp, Cp, Fp, 1.0, 1.0, 0)
        f = out[:M, :C].reshape(M, self.S, self.P).cpu().numpy()
        f = self._y_mean + self._y_std * f
        return f[:, :, 0] if self.P == 1 else np.ascontiguousarray(f.transpose(0, 2, 1))

    def step(self, Xs):
        """Path s at ITS OWN point Xs[s] (gpk_paths_step): Xs (S, D) -> (S,), or (S, P) for P > 1."""
        torch = _torch()
        Xs = check_queries(Xs, self.D)
        if Xs.shape[0] != self.S:
            raise ValueError(f"step takes one row per path: ({self.S}, {self.D})")
        be = self.be
        q = be.upload(Xs)
        out = be.empty((self.S, self.P), torch.float64)
        be.call("gpk_paths_step", *self._model_args(), _p(q), _p(out))
        return self._squeeze(out.cpu().numpy())

    def rollout(self, x0, U, lin):
        """A closed-loop horizon in one call (gpk_paths_rollout).  The state has P coordinates - the model's outputs are its
        residuals - and the query of path s at stage h is q_s = [x_s, U[h]]:

            x_s <- x_s + lin q_s + path_s(q_s)

        x0 (S, P), or (P,) as the start of every path; U (H, D - P); lin (P, D).  Returns the trajectory (H + 1, S, P), stage
        0 = x0.  The next stage's queries never leave the device: 2 H launches, one synchronisation."""
        P, D, S = self.P, self.D, self.S
        if P > D:
            raise ValueError(f"rollout needs a state of P = {P} <= D = {D} coordinates")
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        if x0.shape not in ((P,), (S, P)):
            raise ValueError(f"x0 must be ({S}, {P}) or ({P},)")
        U = np.ascontiguousarray(U, dtype=np.float64)
        if U.ndim == 1 and D - P == 1:
            U = U[:, None]
        if U.ndim != 2 or U.shape[1] != D - P:
            raise ValueError(f"U must be (H, {D - P})")
        H = U.shape[0]
        lin = np.ascontiguousarray(lin, dtype=np.float64)
        if lin.shape != (P, D):
            raise ValueError(f"lin must be ({P}, {D})")
        check_path_shape(D, P, S, self.F, H)
        if not (np.isfinite(x0).all() and np.isfinite(U).all() and np.isfinite(lin).all()):
            raise ValueError("Input X contains NaN or infinity.")
        traj = np.empty((H + 1, S, P))
        self.be.call("gpk_paths_rollout", *self._model_args(), _hp(x0), 1 if x0.ndim == 1 else S,
                     _hp(U) if D > P else None, H, _hp(lin), _hp(traj))
        return traj


# ---- the per-axis batch: B single-output models on shared inputs, each with its own kernel -------------------------------------
MAX_BATCH = 8


def draw_batch_path_randomness(rng, N, D, F, S, ls, noise_plus_alpha):
    """The random numbers of a batch path set, pure NumPy: dict(omega (B, F, D), phase (B, F), weights (B, F, S), eps (B, N, S))
    for B models with length-scales ls (B, D) and noise levels noise_plus_alpha (B,).

    Draw order, from the one `rng`: model 0, 1, ..., B - 1 in turn, each `draw_path_randomness(rng, N, D, F, S, 1, ls[b],
    noise_plus_alpha[b])` - that is, per model, standard_normal((F, D)) / ls[b], uniform(0, 2 pi, F), standard_normal((F, S, 1)),
    sqrt(noise_plus_alpha[b]) standard_normal((N, S, 1)) - so that model 0's numbers are the single-model draw's."""
    ls = np.array(ls, dtype=np.float64, ndmin=2)
    s2 = np.array(noise_plus_alpha, dtype=np.float64, ndmin=1)
    B = ls.shape[0]
    if ls.ndim != 2 or ls.shape[1] != int(D) or s2.shape != (B,):
        raise ValueError(f"ls must be (B, {int(D)}) and noise_plus_alpha (B,)")
    if not 1 <= B <= MAX_BATCH:
        raise ValueError(f"the number of models must be in [1, {MAX_BATCH}] (got {B})")
    rs = [draw_path_randomness(rng, N, D, F, S, 1, ls[b], s2[b]) for b in range(B)]
    return {"omega": np.stack([r["omega"] for r in rs]), "phase": np.stack([r["phase"] for r in rs]),
            "weights": np.stack([r["weights"][:, :, 0] for r in rs]), "eps": np.stack([r["eps"][:, :, 0] for r in rs])}


def check_batch_path_shape(B, D, S, F, H=None):
    """The limits of the batch entries (include/gpk.h, K10, the per-axis batch) as ValueErrors, before any launch."""
    if not 1 <= B <= MAX_BATCH:
        raise ValueError(f"the number of models must be in [1, {MAX_BATCH}] (got {B})")
    check_path_shape(D, 1, S, F, H)


class BatchedPosteriorPaths:
    """S posterior function draws of every model of a fitted `BatchedARDGP` (B models on shared inputs), resident on its GPU.

    paths(X)                            all paths of all models at the same M points: (M, B, S)
    paths.step(Xs)                      Xs (S, D): path s of every model at row s -> (S, B); the hot path, two launches
    paths.rollout(x0, U, lin, ...)      a closed-loop horizon in one call -> (H + 1, S, nx)
    paths.randomness                    dict(omega, phase, weights, eps) it was built from
    paths.coef                          the device coefficient matrix (N + F, B mstride), model-major: model b, path s is
                                        column b mstride + s, mstride = S rounded up to a multiple of 8 (`paths.mstride`)

    Column b of `step` and model b's column block of `coef` have the bits of `PosteriorPaths.from_randomness(models[b], ...)` on
    the same randomness.  The values are in the models' target units, y_mean_b + y_std_b f; `set_output_scaler` puts a further
    affine map per model behind them (a trainer's target scaler)."""

    _STEP, _ROLLOUT = "gpk_paths_step_multi", "gpk_paths_rollout_multi"

    def __init__(self):
        raise TypeError("use BatchedARDGP.sample_paths or BatchedPosteriorPaths.from_randomness")

    def _basis(self, b):
        """The device basis points model b's kernel rows are formed against (here: the shared training inputs)."""
        return self._X

    @classmethod
    def from_randomness(cls, bg, omega, phase, weights, eps):
        """The path set of the fitted batch `bg` from arrays of the caller's own: omega (B, F, D), phase (B, F), weights (B, F, S)
        = the w_s of every model, eps (B, N, S) = the eps_s, already scaled by sqrt(noise_b + alpha).  The set-up is one
        `gpk_paths_prepare` (P = 1) per model on that model's own handle, pointed at its column block."""
        from .device import get_backend
        import ctypes as C
        ms = list(getattr(bg, "models", ()))
        if not ms:
            raise RuntimeError("this BatchedARDGP is not fitted yet")
        B = len(ms)
        if B > MAX_BATCH:
            raise ValueError(f"a batch path set takes at most {MAX_BATCH} models (got {B})")
        for m in ms:
            m._ensure_device()
        devs = [m._dev for m in ms]
        if any(d.replica for d in devs):
            raise RuntimeError("a serving replica holds no fp64 inverse factor: paths are drawn on the rank that fitted the models")
        if not bg._alike(devs):
            raise RuntimeError("the models cannot share a launch: single-output models of one size on one device are needed")
        if not bg._shared_inputs():
            raise RuntimeError("the models were fitted on different training inputs: a batch path set reads one shared X")
        d0 = devs[0]
        N, D = d0.N, d0.D
        if D > DeviceGP.MAX_FEATURES:
            raise ValueError(f"D must be in [1, {DeviceGP.MAX_FEATURES}] (got {D})")
        omega = np.ascontiguousarray(omega, dtype=np.float64)
        phase = np.ascontiguousarray(phase, dtype=np.float64)
        weights = np.ascontiguousarray(weights, dtype=np.float64)
        eps = np.ascontiguousarray(eps, dtype=np.float64)
        if omega.ndim != 3 or omega.shape[0] != B or omega.shape[2] != D:
            raise ValueError(f"omega must be ({B}, F, {D})")
        F = omega.shape[1]
        if phase.shape != (B, F):
            raise ValueError(f"phase must be ({B}, {F})")
        if weights.ndim != 3 or weights.shape[:2] != (B, F):
            raise ValueError(f"weights must be ({B}, {F}, S)")
        S = weights.shape[2]
        if eps.shape != (B, N, S):
            raise ValueError(f"eps must be ({B}, {N}, {S})")
        check_batch_path_shape(B, D, S, F)
        if padded(N) + padded(F) > 65535:
            raise ValueError("gpk_padded(N) + gpk_padded(F) must not exceed 65535")
        for name, a in (("omega", omega), ("phase", phase), ("weights", weights), ("eps", eps)):
            if not np.isfinite(a).all():
                raise ValueError(f"{name} contains NaN or infinity.")
        self = object.__new__(cls)
        torch = _torch()
        be = get_backend(bg.device)
        self.bg, self.be, self._devs = bg, be, devs
        self.N, self.D, self.B, self.F, self.S = N, D, B, F, S
        self.mstride = (S + 7) // 8 * 8          # every model's run of columns starts 64-byte aligned
        self.ldc = B * self.mstride
        self.randomness = {"omega": omega, "phase": phase, "weights": weights, "eps": eps}
        self._ls = np.ascontiguousarray(np.stack([np.asarray(d.ls, dtype=np.float64) for d in devs]))
        self._sf2 = np.ascontiguousarray([float(d.sf2) for d in devs], dtype=np.float64)
        self._y_mean = np.ascontiguousarray([float(np.ravel(m._y_train_mean)[0]) for m in ms], dtype=np.float64)
        self._y_std = np.ascontiguousarray([float(np.ravel(m._y_train_std)[0]) for m in ms], dtype=np.float64)
        self._shift, self._scale = self._y_mean.copy(), self._y_std.copy()
        with torch.cuda.device(be.device):
            torch.cuda.synchronize()              # the models may have been fitted on their own streams
            self._X = d0.X.to(be.device)
            self._omega = be.upload(omega)
            self._phase = be.upload(phase)
            self.coef = be.empty((N + F, self.ldc), torch.float64)
            for b, dev in enumerate(devs):
                mb = dev.be
                with mb.lock:
                    W = dev.inverse_factor(False)
                    w_d = mb.upload(weights[b])
                    e_d = mb.upload(eps[b])
                    block = C.c_void_p(self.coef.data_ptr() + 8 * b * self.mstride)
                    mb.call("gpk_paths_prepare", _p(dev.X), N, D, _p(dev.Yn), 1, _p(W), dev.Np, dev.Np, _p(self._omega[b]),
                            _p(self._phase[b]), F, float(self._sf2[b]), _p(w_d), _p(e_d), S, block, self.ldc)
                    mb.sync()       # (w_d and e_d are released here: the set-up is not the hot path)
            torch.cuda.synchronize()
        return self

    def set_output_scaler(self, mean, scale):
        """Puts the affine map mean[b] + scale[b] y per model behind the values (a trainer's target scaler): folded on the host
        into the one shift / scale pair the launches apply, shift_b = mean_b + scale_b y_mean_b, scale_b <- scale_b y_std_b."""
        mean, scale = _vec(mean, self.B), _vec(scale, self.B)
        if not (np.isfinite(mean).all() and np.isfinite(scale).all()):
            raise ValueError("the output scaler contains NaN or infinity.")
        self._shift = np.ascontiguousarray(mean + scale * self._y_mean)
        self._scale = np.ascontiguousarray(scale * self._y_std)
        return self

    # ---- the models' side of both calls: X, N, D, B, ls, sf2, Omega, phase, F, Coef, ldc, mstride, S, shift, scale
    def _model_args(self):
        return (_p(self._X), self.N, self.D, self.B, _hp(self._ls), _hp(self._sf2), _p(self._omega), _p(self._phase), self.F,
                _p(self.coef), self.ldc, self.mstride, self.S, _hp(self._shift), _hp(self._scale))

    def __call__(self, X):
        """Every path of every model at the same M points: (M, B, S).  Per model gpk_cross_gram_t, gpk_rff_features and two
        gpk_gemm_tiles products; not a hot path."""
        torch = _torch()
        X = check_queries(X, self.D)
        M = X.shape[0]
        if M == 0:
            return np.empty((0, self.B, self.S))
        be = self.be
        N, F, D, S = self.N, self.F, self.D, self.S
        Np, Fp, Mp, Sp = padded(N), padded(F), padded(M), padded(S)
        q = be.upload(X)
        res = np.empty((M, self.B, S))
        for b in range(self.B):
            # the two row blocks of the model's columns in the padded shape of the tile GEMM, zeros in the padding
            cv = torch.zeros((Np, Sp), dtype=torch.float64, device=be.device)
            cw = torch.zeros((Fp, Sp), dtype=torch.float64, device=be.device)
            cols = self.coef[:, b * self.mstride:b * self.mstride + S]
            cv[:N, :S] = cols[:N]
            cw[:F, :S] = cols[N:]
            kt = be.empty((Np, Mp), torch.float64)
            phi = be.empty((Mp, Fp), torch.float64)
            out = be.empty((Mp, Sp), torch.float64)
            with be.lock:
                be.call("gpk_cross_gram_t", _lib.GPK_F64, _p(self._basis(b)), N, _p(q), M, D, _hp(self._ls[b]), float(self._sf2[b]),
                        _p(kt), Mp)
                be.call("gpk_rff_features", _p(q), M, D, _p(self._omega[b]), _p(self._phase[b]), F, 1.0, _p(phi), Fp)
                be.call("gpk_gemm_tiles", _lib.GPK_F64, 1, 1, _p(kt), Mp, _p(cv), Sp, _p(out), Sp, Mp, Sp, Np, 1.0, 0.0, 0)
                be.call("gpk_gemm_tiles", _lib.GPK_F64, 0, 1, _p(phi), Fp, _p(cw), Sp, _p(out), Sp, Mp, Sp, Fp, 1.0, 1.0, 0)
            res[:, b, :] = self._shift[b] + self._scale[b] * out[:M, :S].cpu().numpy()
        return res

    def step(self, Xs):
        """Path s of every model at ITS OWN point Xs[s] (gpk_paths_step_multi): Xs (S, D) -> (S, B)."""
        torch = _torch()
        Xs = check_queries(Xs, self.D)
        if Xs.shape[0] != self.S:
            raise ValueError(f"step takes one row per path: ({self.S}, {self.D})")
        be = self.be
        q = be.upload(Xs)
        out = be.empty((self.S, self.B), torch.float64)
        be.call(self._STEP, *self._model_args(), _p(q), _p(out))
        return out.cpu().numpy()

    def rollout(self, x0, U, lin, coord=None, in_scaler=None):
        """A closed-loop horizon in one call (gpk_paths_rollout_multi), in raw units.  The state has nx = len(lin) coordinates,
        B <= nx <= D; model b's output is added to state coordinate coord[b] (default 0 .. B - 1; distinct); a coordinate
        without a model advances by `lin` alone.  The models read the scaled query: stage h, path s,

            q_s = [x_s, U[h]];   z_s = (q_s - in_shift) / in_scale;   x_s <- x_s + lin q_s + sum_b e_coord[b] path_{b,s}(z_s)

        x0 (S, nx), or (nx,) as the start of every path; U (H, D - nx); lin (nx, D); in_scaler: None (identity), a pair
        (shift (D,), scale (D,)) or an object with `mean_` / `scale_`.  Returns the trajectory (H + 1, S, nx), stage 0 = x0.
        The next stage's queries never leave the device: 2 H launches, one synchronisation."""
        B, D, S = self.B, self.D, self.S
        lin = np.ascontiguousarray(lin, dtype=np.float64)
        if lin.ndim != 2 or lin.shape[1] != D:
            raise ValueError(f"lin must be (nx, {D})")
        nx = lin.shape[0]
        if not B <= nx <= D:
            raise ValueError(f"rollout needs a state of {B} <= nx <= {D} coordinates (got {nx})")
        coord = np.arange(B) if coord is None else np.asarray(coord)
        if coord.shape != (B,) or not np.issubdtype(coord.dtype, np.integer):
            raise ValueError(f"coord must be {B} integers")
        if coord.min() < 0 or coord.max() >= nx:
            raise ValueError(f"coord must be in [0, {nx})")
        if len(set(coord.tolist())) != B:
            raise ValueError("coord must be distinct")
        coord = np.ascontiguousarray(coord, dtype=np.intc)
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        if x0.shape not in ((nx,), (S, nx)):
            raise ValueError(f"x0 must be ({S}, {nx}) or ({nx},)")
        U = np.ascontiguousarray(U, dtype=np.float64)
        if U.ndim == 1 and D - nx == 1:
            U = U[:, None]
        if U.ndim != 2 or U.shape[1] != D - nx:
            raise ValueError(f"U must be (H, {D - nx})")
        H = U.shape[0]
        check_batch_path_shape(B, D, S, self.F, H)
        if not (np.isfinite(x0).all() and np.isfinite(U).all() and np.isfinite(lin).all()):
            raise ValueError("Input X contains NaN or infinity.")
        in_shift = in_scale = None
        if in_scaler is not None:
            pair = (in_scaler.mean_, in_scaler.scale_) if hasattr(in_scaler, "mean_") else in_scaler
            in_shift, in_scale = _vec(pair[0], D), _vec(pair[1], D)
            if not (np.isfinite(in_shift).all() and np.isfinite(in_scale).all()):
                raise ValueError("the input scaler contains NaN or infinity.")
            if not in_scale.all():
                raise ValueError("in_scale must be non-zero")
        import ctypes as C
        traj = np.empty((H + 1, S, nx))
        self.be.call(self._ROLLOUT, *self._model_args(), nx, coord.ctypes.data_as(C.POINTER(C.c_int)),
                     _hp(in_shift), _hp(in_scale), _hp(x0), 1 if x0.ndim == 1 else S, _hp(U) if D > nx else None, H, _hp(lin),
                     _hp(traj))
        return traj


# ---- the sparse models: paths conditioned on the inducing variables --------------------------------------------------------------
#     f_s(x) = phi(x)^T w_s + k_u(x)^T v_s,   v_s = alpha_u + WS^T xi_s - Wuu^T (Wuu Phi_Z w_s),   xi_s ~ N(0, I_m),  w_s ~ N(0, I_F)
# (include/gpk.h, K10 "the sparse models"): the coefficient matrix of the exact model with N := m and X := Z, so `step`, `rollout`
# and `__call__` are the exact classes'; only the set-up (`gpk_sparse_paths_prepare`) and, for the batch, the basis points per
# model (`gpk_paths_step_multi_z`, `gpk_paths_rollout_multi_z`) differ.
def draw_sparse_path_randomness(rng, m, D, F, S, P, ls):
    """The random numbers of a sparse model's path set, pure NumPy: dict(omega (F, D), phase (F,), weights (F, S, P),
    xi (m, S, P)).

    Draw order, from `rng` (a `numpy.random.RandomState` or `Generator`) - `draw_path_randomness`'s with unit noise:
      1. z = rng.standard_normal((F, D));   omega = z / ls           (ls: scalar or (D,))
      2. phase = rng.uniform(0, 2 pi, F)
      3. weights = rng.standard_normal((F, S, P))
      4. xi = rng.standard_normal((m, S, P))"""
    r = draw_path_randomness(rng, m, D, F, S, P, ls, 1.0)
    r["xi"] = r.pop("eps")
    return r


def draw_sparse_batch_path_randomness(rng, m, D, F, S, ls):
    """The random numbers of a sparse batch path set, pure NumPy: dict(omega (B, F, D), phase (B, F), weights (B, F, S),
    xi (B, m, S)) for B models with length-scales ls (B, D).

    Draw order, from the one `rng`: model 0, 1, ..., B - 1 in turn, each `draw_sparse_path_randomness(rng, m, D, F, S, 1, ls[b])`,
    so that model 0's numbers are the single-model draw's."""
    ls = np.array(ls, dtype=np.float64, ndmin=2)
    B = ls.shape[0]
    if ls.ndim != 2 or ls.shape[1] != int(D):
        raise ValueError(f"ls must be (B, {int(D)})")
    if not 1 <= B <= MAX_BATCH:
        raise ValueError(f"the number of models must be in [1, {MAX_BATCH}] (got {B})")
    rs = [draw_sparse_path_randomness(rng, m, D, F, S, 1, ls[b]) for b in range(B)]
    return {"omega": np.stack([r["omega"] for r in rs]), "phase": np.stack([r["phase"] for r in rs]),
            "weights": np.stack([r["weights"][:, :, 0] for r in rs]), "xi": np.stack([r["xi"][:, :, 0] for r in rs])}


def check_sparse_randomness(m, D, P, omega, phase, weights, xi, batch=None):
    """Shapes, limits and finiteness of a sparse path set's randomness as ValueErrors, before any launch; returns the four
    arrays as contiguous float64 and (F, S).  batch=B: the batch layout (B leading, no output axis)."""
    omega = np.ascontiguousarray(omega, dtype=np.float64)
    phase = np.ascontiguousarray(phase, dtype=np.float64)
    weights = np.ascontiguousarray(weights, dtype=np.float64)
    xi = np.ascontiguousarray(xi, dtype=np.float64)
    if batch is None:
        if omega.ndim != 2 or omega.shape[1] != D:
            raise ValueError(f"omega must be (F, {D})")
        F = omega.shape[0]
        if phase.shape != (F,):
            raise ValueError(f"phase must be ({F},)")
        if weights.ndim == 2 and P == 1:
            weights = weights[:, :, None]
        if xi.ndim == 2 and P == 1:
            xi = xi[:, :, None]
        if weights.ndim != 3 or weights.shape[0] != F or weights.shape[2] != P:
            raise ValueError(f"weights must be ({F}, S, {P})")
        S = weights.shape[1]
        if xi.shape != (m, S, P):
            raise ValueError(f"xi must be ({m}, {S}, {P})")
        check_path_shape(D, P, S, F)
    else:
        B = batch
        if omega.ndim != 3 or omega.shape[0] != B or omega.shape[2] != D:
            raise ValueError(f"omega must be ({B}, F, {D})")
        F = omega.shape[1]
        if phase.shape != (B, F):
            raise ValueError(f"phase must be ({B}, {F})")
        if weights.ndim != 3 or weights.shape[:2] != (B, F):
            raise ValueError(f"weights must be ({B}, {F}, S)")
        S = weights.shape[2]
        if xi.shape != (B, m, S):
            raise ValueError(f"xi must be ({B}, {m}, {S})")
        check_batch_path_shape(B, D, S, F)
    if padded(m) + padded(F) > 65535:
        raise ValueError("gpk_padded(m) + gpk_padded(F) must not exceed 65535")
    for name, a in (("omega", omega), ("phase", phase), ("weights", weights), ("xi", xi)):
        if not np.isfinite(a).all():
            raise ValueError(f"{name} contains NaN or infinity.")
    return omega, phase, weights, xi, F, S


class SparsePosteriorPaths(PosteriorPaths):
    """S posterior function draws of a `SparseGP`, resident on its GPU: `PosteriorPaths` over the m inducing inputs - `__call__`,
    `step`, `rollout`, `.coef` ((m + F, S P), column s P + p) as there; `.randomness` = dict(omega, phase, weights, xi).  The set
    is a snapshot: it keeps its own copy of Z and stays the same function when the model takes further rows."""

    def __init__(self):
        raise TypeError("use SparseGP.sample_paths or SparsePosteriorPaths.from_randomness")

    @classmethod
    def from_randomness(cls, sp, omega, phase, weights, xi):
        """The path set of the sparse model `sp` (assembled here if it is not; without rows: the prior) from arrays of the
        caller's own: omega (F, D), phase (F,), weights (F, S, P) (or (F, S) for one output) = the w_s, xi (m, S, P) (or (m, S))
        = the xi_s."""
        m, D = sp.inducing_.shape
        P = sp.n_outputs_
        omega, phase, weights, xi, F, S = check_sparse_randomness(m, D, P, omega, phase, weights, xi)
        sp._ensure()
        comp = sp.kernel_.components()
        self = object.__new__(cls)
        torch = _torch()
        be = sp._backend()
        self.gp, self._dev, self.be = sp, None, be
        self.N, self.D, self.P, self.F, self.S = m, D, P, F, S
        self.randomness = {"omega": omega, "phase": phase, "weights": weights, "xi": xi}
        self._ls = np.ascontiguousarray(comp.ls_vector(D), dtype=np.float64).copy()
        self._sf2 = float(comp.sf2)
        self._y_mean, self._y_std = sp._ym.copy(), sp._ys.copy()
        C = S * P
        with be.lock:
            self._omega = be.upload(omega)
            self._phase = be.upload(phase)
            self._X = be.empty((m, D), torch.float64)
            self.coef = be.empty((m + F, C), torch.float64)
            w_d = be.upload(weights.reshape(F, C))
            x_d = be.upload(xi.reshape(m, C))
            be.call("gpk_sparse_paths_prepare", _p(self._omega), _p(self._phase), F, _p(w_d), _p(x_d), S, _p(self.coef), C,
                    _p(self._X))
            be.sync()       # (w_d and x_d are released here: the set-up is not the hot path)
        return self


class BatchedSparsePosteriorPaths(BatchedPosteriorPaths):
    """S posterior function draws of every model of a `BatchedSparseGP` (B single-output sparse models of equal m and D, each
    with its own kernel and inducing inputs): `BatchedPosteriorPaths` with N := m and the basis points per model - `__call__`
    (M, B, S), `step` (S, B) in two launches (`gpk_paths_step_multi_z`), `rollout` one call per horizon
    (`gpk_paths_rollout_multi_z`), `set_output_scaler`, `.coef` model-major.  Column b of `step` has the bits of
    `SparsePosteriorPaths.from_randomness(models[b], ...)` on the same randomness."""

    _STEP, _ROLLOUT = "gpk_paths_step_multi_z", "gpk_paths_rollout_multi_z"

    def __init__(self):
        raise TypeError("use BatchedSparseGP.sample_paths or BatchedSparsePosteriorPaths.from_randomness")

    def _basis(self, b):
        return self._X[b]

    @classmethod
    def from_randomness(cls, bg, omega, phase, weights, xi):
        """The path set of the sparse batch `bg` from arrays of the caller's own: omega (B, F, D), phase (B, F), weights
        (B, F, S), xi (B, m, S).  The set-up is one `gpk_sparse_paths_prepare` per model on that model's own handle, pointed at
        its column block and its slice of the basis points."""
        import ctypes as C
        ms = list(bg.models)
        B = len(ms)
        m, D = ms[0].inducing_.shape
        omega, phase, weights, xi, F, S = check_sparse_randomness(m, D, 1, omega, phase, weights, xi, batch=B)
        bes, _ = bg._ensure()
        self = object.__new__(cls)
        torch = _torch()
        be = bes[0]
        if any(b.device_index != be.device_index for b in bes):
            raise RuntimeError("the models of a batch must be on one device")
        comps = [mm.kernel_.components() for mm in ms]
        self.bg, self.be, self._devs = bg, be, None
        self.N, self.D, self.B, self.F, self.S = m, D, B, F, S
        self.mstride = (S + 7) // 8 * 8          # every model's run of columns starts 64-byte aligned
        self.ldc = B * self.mstride
        self.randomness = {"omega": omega, "phase": phase, "weights": weights, "xi": xi}
        self._ls = np.ascontiguousarray(np.stack([np.asarray(c.ls_vector(D), dtype=np.float64) for c in comps]))
        self._sf2 = np.ascontiguousarray([float(c.sf2) for c in comps], dtype=np.float64)
        self._y_mean = np.ascontiguousarray([float(mm._ym[0]) for mm in ms], dtype=np.float64)
        self._y_std = np.ascontiguousarray([float(mm._ys[0]) for mm in ms], dtype=np.float64)
        self._shift, self._scale = self._y_mean.copy(), self._y_std.copy()
        with torch.cuda.device(be.device):
            torch.cuda.synchronize()              # the models may have been assembled on their own streams
            self._omega = be.upload(omega)
            self._phase = be.upload(phase)
            self._X = be.empty((B, m, D), torch.float64)
            self.coef = be.empty((m + F, self.ldc), torch.float64)
            for b, mb in enumerate(bes):
                with mb.lock:
                    w_d = mb.upload(weights[b])
                    x_d = mb.upload(xi[b])
                    block = C.c_void_p(self.coef.data_ptr() + 8 * b * self.mstride)
                    mb.call("gpk_sparse_paths_prepare", _p(self._omega[b]), _p(self._phase[b]), F, _p(w_d), _p(x_d), S, block,
                            self.ldc, _p(self._X[b]))
                    mb.sync()       # (w_d and x_d are released here: the set-up is not the hot path)
            torch.cuda.synchronize()
        return self
