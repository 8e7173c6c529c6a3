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

Path gradients: `step` and `rollout` of all four classes take `return_jacobian=True` and then also return the input Jacobian of
every path at the point it was evaluated at (the `*_grad` entries: closed form, the same two launches per stage; the values keep
their bits), so that a sampled rollout can be linearised with the function that produced it.

The four classes share their frame: `check_randomness`, `_init_single` / `_init_batch` (+ `_prepare_models`), `_dense_paths`
behind `__call__`, `check_rollout_args`; a class's own part is its prepare call.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .device import DeviceGP, _hp, _p, _torch, _vec, check_queries, padded

MAX_PATHS, MAX_FEATURES, MAX_HORIZON, MAX_BATCH = 4096, 16384, 256, 8


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


def _stack_model_draws(rng, n, D, F, S, ls, noise_plus_alpha=None, name="eps"):
    """The batch draw: model 0, 1, ..., B - 1 in turn from the one `rng`, each `draw_path_randomness(rng, n, D, F, S, 1, ls[b],
    noise_plus_alpha[b])` (None: unit noise), stacked with B leading and the output axis dropped; the fourth array as `name`."""
    ls = np.array(ls, dtype=np.float64, ndmin=2)
    B = ls.shape[0]
    if ls.ndim != 2 or ls.shape[1] != int(D):
        raise ValueError(f"ls must be (B, {int(D)})")
    s2 = np.ones(B) if noise_plus_alpha is None else np.array(noise_plus_alpha, dtype=np.float64, ndmin=1)
    if s2.shape != (B,):
        raise ValueError("noise_plus_alpha must be (B,)")
    if not 1 <= B <= MAX_BATCH:
        raise ValueError(f"the number of models must be in [1, {MAX_BATCH}] (got {B})")
    rs = [draw_path_randomness(rng, n, D, F, S, 1, ls[b], s2[b]) for b in range(B)]
    r = {k: np.stack([d[k][:, :, 0] if d[k].ndim == 3 else d[k] for d in rs]) for k in ("omega", "phase", "weights", "eps")}
    r[name] = r.pop("eps")
    return r


def draw_batch_path_randomness(rng, N, D, F, S, ls, noise_plus_alpha):
    """The random numbers of a batch path set, pure NumPy: dict(omega (B, F, D), phase (B, F), weights (B, F, S), eps (B, N, S))
    for B models with length-scales ls (B, D) and noise levels noise_plus_alpha (B,).

    Draw order, from the one `rng`: model 0, 1, ..., B - 1 in turn, each `draw_path_randomness(rng, N, D, F, S, 1, ls[b],
    noise_plus_alpha[b])` - that is, per model, standard_normal((F, D)) / ls[b], uniform(0, 2 pi, F), standard_normal((F, S, 1)),
    sqrt(noise_plus_alpha[b]) standard_normal((N, S, 1)) - so that model 0's numbers are the single-model draw's."""
    return _stack_model_draws(rng, N, D, F, S, ls, noise_plus_alpha)


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
    return _stack_model_draws(rng, m, D, F, S, ls, name="xi")


def check_path_shape(D, P, S, F):
    """The limits of the family (include/gpk.h, K10) as ValueErrors, before any launch."""
    if not 1 <= D <= DeviceGP.MAX_FEATURES:
        raise ValueError(f"D must be in [1, {DeviceGP.MAX_FEATURES}] (got {D})")
    if not 1 <= P <= _lib.GPK_MAX_P:
        raise ValueError(f"P must be in [1, {_lib.GPK_MAX_P}] (got {P})")
    if not 1 <= S <= MAX_PATHS:
        raise ValueError(f"the number of paths must be in [1, {MAX_PATHS}] (got {S})")
    if not 1 <= F <= MAX_FEATURES:
        raise ValueError(f"the number of features must be in [1, {MAX_FEATURES}] (got {F})")


def check_batch_path_shape(B, D, S, F):
    """The limits of the batch entries (include/gpk.h, K10, the per-axis batch) as ValueErrors, before any launch."""
    if not 1 <= B <= MAX_BATCH:
        raise ValueError(f"the number of models must be in [1, {MAX_BATCH}] (got {B})")
    check_path_shape(D, 1, S, F)


def check_randomness(n, D, P, omega, phase, weights, fourth, name, batch=None):
    """Shapes, limits and finiteness of a path set's randomness over n basis rows as ValueErrors, before any launch; `name`
    names the fourth array ("eps" or "xi", n rows).  Returns dict(omega, phase, weights, <name>) of contiguous float64 arrays,
    F and S.  batch=B: the batch layout (B leading, no output axis)."""
    omega = np.ascontiguousarray(omega, dtype=np.float64)
    phase = np.ascontiguousarray(phase, dtype=np.float64)
    weights = np.ascontiguousarray(weights, dtype=np.float64)
    fourth = np.ascontiguousarray(fourth, dtype=np.float64)
    if batch is None:
        if omega.ndim != 2 or omega.shape[1] != D:
            raise ValueError(f"omega must be (F, {D})")
        F = omega.shape[0]
        if phase.shape != (F,):
            raise ValueError(f"phase must be ({F},)")
        if weights.ndim == 2 and P == 1:
            weights = weights[:, :, None]
        if fourth.ndim == 2 and P == 1:
            fourth = fourth[:, :, None]
        if weights.ndim != 3 or weights.shape[0] != F or weights.shape[2] != P:
            raise ValueError(f"weights must be ({F}, S, {P})")
        S = weights.shape[1]
        if fourth.shape != (n, S, P):
            raise ValueError(f"{name} must be ({n}, {S}, {P})")
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
        if fourth.shape != (B, n, S):
            raise ValueError(f"{name} must be ({B}, {n}, {S})")
        check_batch_path_shape(B, D, S, F)
    if padded(n) + padded(F) > 65535:
        raise ValueError(f"gpk_padded({n}) + gpk_padded({F}) must not exceed 65535")
    r = {"omega": omega, "phase": phase, "weights": weights, name: fourth}
    for key, a in r.items():
        if not np.isfinite(a).all():
            raise ValueError(f"{key} contains NaN or infinity.")
    return r, F, S


def check_rollout_args(S, D, x0, U, lin, nx=None):
    """The arguments of a rollout as ValueErrors, before any launch: lin (nx, D) - nx, the state width, is lin's row count where
    the caller does not fix it - x0 (S, nx) or (nx,), U (H, D - nx) (1-D for one control).  Returns what goes to the library:
    x0, its row count (1 or S), U (None without controls), H, lin - contiguous float64."""
    lin = np.ascontiguousarray(lin, dtype=np.float64)
    if lin.ndim != 2 or lin.shape[1] != D or nx not in (None, lin.shape[0]):
        raise ValueError(f"lin must be ({'nx' if nx is None else nx}, {D})")
    nx = lin.shape[0]
    if nx > D:
        raise ValueError(f"rollout needs a state of at most D = {D} coordinates (got {nx})")
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    if x0.shape not in ((nx,), (S, nx)):
        raise ValueError(f"x0 must be ({S}, {nx}) or ({nx},)")
    U = np.ascontiguousarray(U, dtype=np.float64)
    if U.ndim == 1 and D - nx == 1:
        U = U[:, None]
    if U.ndim != 2 or U.shape[1] != D - nx:
        raise ValueError(f"U must be (H, {D - nx})")
    H = U.shape[0]
    if not 1 <= H <= MAX_HORIZON:
        raise ValueError(f"the horizon must be in [1, {MAX_HORIZON}] stages (got {H})")
    if not (np.isfinite(x0).all() and np.isfinite(U).all() and np.isfinite(lin).all()):
        raise ValueError("Input X contains NaN or infinity.")
    return x0, 1 if x0.ndim == 1 else S, U if D > nx else None, H, lin


def _dense_paths(be, X, ls, sf2, omega, phase, coef, q, M):
    """Every column of `coef` ((N + F, columns), a column block of a coefficient matrix) at the M uploaded queries q, in
    normalised units: the device block (M, columns).  Built from gpk_cross_gram_t over the basis points X (N, D),
    gpk_rff_features and two gpk_gemm_tiles products; not a hot path."""
    torch = _torch()
    (N, D), F, C = X.shape, omega.shape[0], coef.shape[1]
    Np, Fp, Mp, Cp = padded(N), padded(F), padded(M), padded(C)
    # the two row blocks of coef in the padded shape of the tile GEMM, zeros in the padding
    cv = torch.zeros((Np, Cp), dtype=torch.float64, device=be.device)
    cw = torch.zeros((Fp, Cp), dtype=torch.float64, device=be.device)
    cv[:N, :C] = coef[:N]
    cw[:F, :C] = coef[N:]
    kt = be.empty((Np, Mp), torch.float64)
    phi = be.empty((Mp, Fp), torch.float64)
    out = be.empty((Mp, Cp), torch.float64)
    with be.lock:
        be.call("gpk_cross_gram_t", _lib.GPK_F64, _p(X), N, _p(q), M, D, _hp(ls), sf2, _p(kt), Mp)
        be.call("gpk_rff_features", _p(q), M, D, _p(omega), _p(phase), F, 1.0, _p(phi), Fp)
        # out = K*^T V (kt is stored training-row major: ta = 1) + Phi(Xq) W~
        be.call("gpk_gemm_tiles", _lib.GPK_F64, 1, 1, _p(kt), Mp, _p(cv), Cp, _p(out), Cp, Mp, Cp, Np, 1.0, 0.0, 0)
        be.call("gpk_gemm_tiles", _lib.GPK_F64, 0, 1, _p(phi), Fp, _p(cw), Cp, _p(out), Cp, Mp, Cp, Fp, 1.0, 1.0, 0)
    return out[:M, :C]


class PosteriorPaths:
    """S posterior function draws of a fitted `GaussianProcessRegressor`, resident on its GPU.

    paths(X)                    all paths at the same M points: (M, S), or (M, P, S) for P > 1 (`sample_y`'s convention)
    paths.step(Xs)              Xs (S, D): path s at row s -> (S,) or (S, P); the hot path, two launches
    paths.rollout(x0, U, lin)   a closed-loop horizon in one call -> (H + 1, S, P)
                                both with return_jacobian=True: also the input Jacobian of every path, (S, D) / (S, P, D) and
                                (H, S, P, D), in the same two launches per stage; the values keep their bits
    paths.randomness            dict(omega, phase, weights, eps) it was built from
    paths.coef                  the device coefficient matrix (N + F, S P), column s P + p"""

    def __init__(self):
        raise TypeError("use GaussianProcessRegressor.sample_paths or PosteriorPaths.from_randomness")

    def _init_single(self, gp, dev, be, X, r, F, S, ls, sf2, y_mean, y_std):
        """The fields of a single-model path set over the device basis points X (N, D); uploads omega and phase and
        allocates coef.  Returns the device copies of the two (rows, S P) arrays the class's prepare call reads."""
        self.gp, self._dev, self.be, self._X = gp, dev, be, X
        (self.N, self.D), self.P, self.F, self.S = X.shape, len(y_mean), F, S
        self.randomness = r
        self._ls = np.ascontiguousarray(ls, dtype=np.float64).copy()
        self._sf2 = float(sf2)
        self._y_mean, self._y_std = y_mean, y_std
        self._omega = be.upload(r["omega"])
        self._phase = be.upload(r["phase"])
        self.coef = be.empty((self.N + F, S * self.P), _torch().float64)
        return [be.upload(a.reshape(a.shape[0], S * self.P)) for a in list(r.values())[2:]]

    @classmethod
    def from_randomness(cls, gp, omega, phase, weights, eps):
        """The path set of the fitted model `gp` from arrays of the caller's own: omega (F, D), phase (F,), weights (F, S, P)
        (or (F, S) for one output) = the w_s, eps (N, S, P) (or (N, S)) = the eps_s, already scaled by sqrt(noise + alpha)."""
        gp._ensure_device()
        dev = gp._dev
        if dev.replica:
            raise RuntimeError("a serving replica holds no fp64 inverse factor: paths are drawn on the rank that fitted the model")
        N, D, P = dev.N, dev.D, dev.P
        r, F, S = check_randomness(N, D, P, omega, phase, weights, eps, "eps")
        self = object.__new__(cls)
        be = dev.be
        w_d, e_d = self._init_single(gp, dev, be, dev.X, r, F, S, dev.ls, dev.sf2, _vec(gp._y_train_mean, P),
                                     _vec(gp._y_train_std, P))
        with be.lock:
            W = dev.inverse_factor(False)
            be.call("gpk_paths_prepare", _p(dev.X), N, D, _p(dev.Yn), P, _p(W), dev.Np, dev.Np, _p(self._omega), _p(self._phase),
                    F, self._sf2, _p(w_d), _p(e_d), S, _p(self.coef), S * P)
            be.sync()       # (w_d and e_d are released here: the set-up is not the hot path)
        return self

    # ---- the model's side of every call: X, N, D, ls, sf2, Omega, phase, F, Coef, ldc, S, P, y_mean, y_std
    def _model_args(self):
        return (_p(self._X), self.N, self.D, _hp(self._ls), self._sf2, _p(self._omega), _p(self._phase), self.F,
                _p(self.coef), self.S * self.P, self.S, self.P, _hp(self._y_mean), _hp(self._y_std))

    def _squeeze(self, a):
        return a[..., 0] if self.P == 1 else a

    def __call__(self, X):
        """Every path at the same M points: (M, S), or (M, P, S) for P > 1 (`_dense_paths`; not a hot path)."""
        X = check_queries(X, self.D)
        M = X.shape[0]
        if M == 0:
            return np.empty((0, self.S) if self.P == 1 else (0, self.P, self.S))
        out = _dense_paths(self.be, self._X, self._ls, self._sf2, self._omega, self._phase, self.coef, self.be.upload(X), M)
        f = out.reshape(M, self.S, self.P).cpu().numpy()
        f = self._y_mean + self._y_std * f
        return f[:, :, 0] if self.P == 1 else np.ascontiguousarray(f.transpose(0, 2, 1))

    def step(self, Xs, return_jacobian=False):
        """Path s at ITS OWN point Xs[s] (gpk_paths_step): Xs (S, D) -> (S,), or (S, P) for P > 1.  return_jacobian=True
        (gpk_paths_step_grad): (values, jac), jac[s, p, d] = d values[s, p] / d Xs[s, d], (S, D) or (S, P, D); the values
        have the bits of the call without it."""
        torch = _torch()
        Xs = check_queries(Xs, self.D)
        if Xs.shape[0] != self.S:
            raise ValueError(f"step takes one row per path: ({self.S}, {self.D})")
        be = self.be
        q = be.upload(Xs)
        out = be.empty((self.S, self.P), torch.float64)
        if return_jacobian:
            jac = be.empty((self.S, self.P, self.D), torch.float64)
            be.call("gpk_paths_step_grad", *self._model_args(), _p(q), _p(out), _p(jac))
            jac = jac.cpu().numpy()
            return self._squeeze(out.cpu().numpy()), jac[:, 0] if self.P == 1 else jac
        be.call("gpk_paths_step", *self._model_args(), _p(q), _p(out))
        return self._squeeze(out.cpu().numpy())

    def rollout(self, x0, U, lin, return_jacobian=False):
        """A closed-loop horizon in one call (gpk_paths_rollout).  The state has P coordinates - the model's outputs are its
        residuals - and the query of path s at stage h is q_s = [x_s, U[h]]:

            x_s <- x_s + lin q_s + path_s(q_s)

        x0 (S, P), or (P,) as the start of every path; U (H, D - P); lin (P, D).  Returns the trajectory (H + 1, S, P), stage
        0 = x0.  The next stage's queries never leave the device: 2 H launches, one synchronisation.

        return_jacobian=True (gpk_paths_rollout_grad): (traj, jac), jac (H, S, P, D): jac[h, s] is the Jacobian of path s at
        its stage-h query [traj[h, s], U[h]], so the sampled closed loop linearises as A_h = I + lin[:, :P] + jac[h, s][:, :P],
        B_h = lin[:, P:] + jac[h, s][:, P:]; traj has the bits of the call without it."""
        P, D, S = self.P, self.D, self.S
        if P > D:
            raise ValueError(f"rollout needs a state of P = {P} <= D = {D} coordinates")
        x0, rows, U, H, lin = check_rollout_args(S, D, x0, U, lin, nx=P)
        traj = np.empty((H + 1, S, P))
        if return_jacobian:
            jac = np.empty((H, S, P, D))
            self.be.call("gpk_paths_rollout_grad", *self._model_args(), _hp(x0), rows, _hp(U), H, _hp(lin), _hp(traj), _hp(jac))
            return traj, jac
        self.be.call("gpk_paths_rollout", *self._model_args(), _hp(x0), rows, _hp(U), H, _hp(lin), _hp(traj))
        return traj


# ---- the per-axis batch: B single-output models on shared inputs, each with its own kernel -------------------------------------
class BatchedPosteriorPaths:
    """S posterior function draws of every model of a fitted `BatchedARDGP` (B models on shared inputs), resident on its GPU.

    paths(X)                            all paths of all models at the same M points: (M, B, S)
    paths.step(Xs)                      Xs (S, D): path s of every model at row s -> (S, B); the hot path, two launches
    paths.rollout(x0, U, lin, ...)      a closed-loop horizon in one call -> (H + 1, S, nx)
                                        both with return_jacobian=True: also the input Jacobians, (S, B, D) and - in raw
                                        units - (H, S, B, D)
    paths.randomness                    dict(omega, phase, weights, eps) it was built from
    paths.coef                          the device coefficient matrix (N + F, B mstride), model-major: model b, path s is
                                        column b mstride + s, mstride = S rounded up to a multiple of 8 (`paths.mstride`)

    Column b of `step` and model b's column block of `coef` have the bits of `PosteriorPaths.from_randomness(models[b], ...)` on
    the same randomness.  The values are in the models' target units, y_mean_b + y_std_b f; `set_output_scaler` puts a further
    affine map per model behind them (a trainer's target scaler)."""

    _STEP, _ROLLOUT = "gpk_paths_step_multi", "gpk_paths_rollout_multi"
    _STEP_GRAD, _ROLLOUT_GRAD = "gpk_paths_step_multi_grad", "gpk_paths_rollout_multi_grad"

    def __init__(self):
        raise TypeError("use BatchedARDGP.sample_paths or BatchedPosteriorPaths.from_randomness")

    def _basis(self, b):
        """The device basis points model b's kernel rows are formed against (here: the shared training inputs)."""
        return self._X

    def _init_batch(self, bg, be, devs, N, D, r, F, S, ls, sf2, y_mean, y_std, X=None):
        """The fields of a batch path set over N basis rows per model, the models' values given per model; waits for the
        device, uploads omega and phase and allocates coef and - where no shared X is given - the basis points (B, N, D)."""
        torch = _torch()
        B = len(sf2)
        self.bg, self.be, self._devs = bg, be, devs
        self.N, self.D, self.B, self.F, self.S = N, D, B, F, S
        self.mstride = (S + 7) // 8 * 8          # every model's run of columns starts 64-byte aligned
        self.ldc = B * self.mstride
        self.randomness = r
        self._ls = np.ascontiguousarray(np.stack([np.asarray(v, dtype=np.float64) for v in ls]))
        self._sf2 = np.ascontiguousarray([float(v) for v in sf2], dtype=np.float64)
        self._y_mean = np.ascontiguousarray([float(np.ravel(v)[0]) for v in y_mean], dtype=np.float64)
        self._y_std = np.ascontiguousarray([float(np.ravel(v)[0]) for v in y_std], dtype=np.float64)
        self._shift, self._scale = self._y_mean.copy(), self._y_std.copy()
        with torch.cuda.device(be.device):
            torch.cuda.synchronize()              # the models may have been fitted or assembled on their own streams
            self._X = be.empty((B, N, D), torch.float64) if X is None else X.to(be.device)
            self._omega = be.upload(r["omega"])
            self._phase = be.upload(r["phase"])
            self.coef = be.empty((N + F, self.ldc), torch.float64)

    def _prepare_models(self, bes, prepare):
        """The set-up, model by model on that model's own backend: prepare(b, mb, w_d, e_d, block) is the class's one call,
        given the device copies of model b's two (rows, S) arrays and the address of its column block of coef."""
        torch = _torch()
        weights, fourth = list(self.randomness.values())[2:]
        with torch.cuda.device(self.be.device):
            for b, mb in enumerate(bes):
                with mb.lock:
                    w_d = mb.upload(weights[b])
                    e_d = mb.upload(fourth[b])
                    prepare(b, mb, w_d, e_d, C.c_void_p(self.coef.data_ptr() + 8 * b * self.mstride))
                    mb.sync()       # (w_d and e_d are released here: the set-up is not the hot path)
            torch.cuda.synchronize()

    @classmethod
    def from_randomness(cls, bg, omega, phase, weights, eps):
        """The path set of the fitted batch `bg` from arrays of the caller's own: omega (B, F, D), phase (B, F), weights (B, F, S)
        = the w_s of every model, eps (B, N, S) = the eps_s, already scaled by sqrt(noise_b + alpha).  The set-up is one
        `gpk_paths_prepare` (P = 1) per model on that model's own handle, pointed at its column block."""
        from .device import get_backend
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
        N, D = devs[0].N, devs[0].D
        r, F, S = check_randomness(N, D, 1, omega, phase, weights, eps, "eps", batch=B)
        self = object.__new__(cls)
        self._init_batch(bg, get_backend(bg.device), devs, N, D, r, F, S, [d.ls for d in devs], [d.sf2 for d in devs],
                         [m._y_train_mean for m in ms], [m._y_train_std for m in ms], X=devs[0].X)

        def prepare(b, mb, w_d, e_d, block):
            dev = devs[b]
            W = dev.inverse_factor(False)
            mb.call("gpk_paths_prepare", _p(dev.X), N, D, _p(dev.Yn), 1, _p(W), dev.Np, dev.Np, _p(self._omega[b]),
                    _p(self._phase[b]), F, float(self._sf2[b]), _p(w_d), _p(e_d), S, block, self.ldc)

        self._prepare_models([d.be for d in devs], prepare)
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
        """Every path of every model at the same M points: (M, B, S) (`_dense_paths` per model; not a hot path)."""
        X = check_queries(X, self.D)
        M, S = X.shape[0], self.S
        if M == 0:
            return np.empty((0, self.B, S))
        q = self.be.upload(X)
        res = np.empty((M, self.B, S))
        for b in range(self.B):
            out = _dense_paths(self.be, self._basis(b), self._ls[b], float(self._sf2[b]), self._omega[b], self._phase[b],
                               self.coef[:, b * self.mstride:b * self.mstride + S], q, M)
            res[:, b, :] = self._shift[b] + self._scale[b] * out.cpu().numpy()
        return res

    def step(self, Xs, return_jacobian=False):
        """Path s of every model at ITS OWN point Xs[s] (gpk_paths_step_multi): Xs (S, D) -> (S, B).  return_jacobian=True
        (gpk_paths_step_multi_grad): (values, jac), jac[s, b, d] = d values[s, b] / d Xs[s, d], (S, B, D); the values have the
        bits of the call without it, and column b of jac those of model b's own `PosteriorPaths.step`."""
        torch = _torch()
        Xs = check_queries(Xs, self.D)
        if Xs.shape[0] != self.S:
            raise ValueError(f"step takes one row per path: ({self.S}, {self.D})")
        be = self.be
        q = be.upload(Xs)
        out = be.empty((self.S, self.B), torch.float64)
        if return_jacobian:
            jac = be.empty((self.S, self.B, self.D), torch.float64)
            be.call(self._STEP_GRAD, *self._model_args(), _p(q), _p(out), _p(jac))
            return out.cpu().numpy(), jac.cpu().numpy()
        be.call(self._STEP, *self._model_args(), _p(q), _p(out))
        return out.cpu().numpy()

    def rollout(self, x0, U, lin, coord=None, in_scaler=None, return_jacobian=False):
        """A closed-loop horizon in one call (gpk_paths_rollout_multi), in raw units.  The state has nx = len(lin) coordinates,
        B <= nx <= D; model b's output is added to state coordinate coord[b] (default 0 .. B - 1; distinct); a coordinate
        without a model advances by `lin` alone.  The models read the scaled query: stage h, path s,

            q_s = [x_s, U[h]];   z_s = (q_s - in_shift) / in_scale;   x_s <- x_s + lin q_s + sum_b e_coord[b] path_{b,s}(z_s)

        x0 (S, nx), or (nx,) as the start of every path; U (H, D - nx); lin (nx, D); in_scaler: None (identity), a pair
        (shift (D,), scale (D,)) or an object with `mean_` / `scale_`.  Returns the trajectory (H + 1, S, nx), stage 0 = x0.
        The next stage's queries never leave the device: 2 H launches, one synchronisation.

        return_jacobian=True (gpk_paths_rollout_multi_grad): (traj, jac), jac (H, S, B, D): jac[h, s, b] is the gradient of
        model b's path s at stage h's query w.r.t. the RAW q_s = [traj[h, s], U[h]] (it includes 1 / in_scale); traj has the
        bits of the call without it."""
        B, D, S = self.B, self.D, self.S
        x0, rows, U, H, lin = check_rollout_args(S, D, x0, U, lin)
        nx = lin.shape[0]
        if nx < B:
            raise ValueError(f"rollout needs a state of {B} <= nx <= {D} coordinates (got {nx})")
        coord = np.arange(B) if coord is None else np.asarray(coord)
        if coord.shape != (B,) or not np.issubdtype(coord.dtype, np.integer):
            raise ValueError(f"coord must be {B} integers")
        if coord.min() < 0 or coord.max() >= nx:
            raise ValueError(f"coord must be in [0, {nx})")
        if len(set(coord.tolist())) != B:
            raise ValueError("coord must be distinct")
        coord = np.ascontiguousarray(coord, dtype=np.intc)
        in_shift = in_scale = None
        if in_scaler is not None:
            pair = (in_scaler.mean_, in_scaler.scale_) if hasattr(in_scaler, "mean_") else in_scaler
            in_shift, in_scale = _vec(pair[0], D), _vec(pair[1], D)
            if not (np.isfinite(in_shift).all() and np.isfinite(in_scale).all()):
                raise ValueError("the input scaler contains NaN or infinity.")
            if not in_scale.all():
                raise ValueError("in_scale must be non-zero")
        traj = np.empty((H + 1, S, nx))
        if return_jacobian:
            jac = np.empty((H, S, B, D))
            self.be.call(self._ROLLOUT_GRAD, *self._model_args(), nx, coord.ctypes.data_as(C.POINTER(C.c_int)),
                         _hp(in_shift), _hp(in_scale), _hp(x0), rows, _hp(U), H, _hp(lin), _hp(traj), _hp(jac))
            return traj, jac
        self.be.call(self._ROLLOUT, *self._model_args(), nx, coord.ctypes.data_as(C.POINTER(C.c_int)),
                     _hp(in_shift), _hp(in_scale), _hp(x0), rows, _hp(U), H, _hp(lin), _hp(traj))
        return traj


# ---- the sparse models: paths conditioned on the inducing variables --------------------------------------------------------------
#     f_s(x) = phi(x)^T w_s + k_u(x)^T v_s,   v_s = alpha_u + WS^T xi_s - Wuu^T (Wuu Phi_Z w_s),   xi_s ~ N(0, I_m),  w_s ~ N(0, I_F)
# (include/gpk.h, K10 "the sparse models"): the coefficient matrix of the exact model with N := m and X := Z, so `step`, `rollout`
# and `__call__` are the exact classes'; only the set-up (`gpk_sparse_paths_prepare`) and, for the batch, the basis points per
# model (`gpk_paths_step_multi_z`, `gpk_paths_rollout_multi_z`) differ.
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
        r, F, S = check_randomness(m, D, P, omega, phase, weights, xi, "xi")
        sp._ensure()
        comp = sp.kernel_.components()
        self = object.__new__(cls)
        be = sp._backend()
        w_d, x_d = self._init_single(sp, None, be, be.empty((m, D), _torch().float64), r, F, S, comp.ls_vector(D), comp.sf2,
                                     sp._ym.copy(), sp._ys.copy())
        with be.lock:
            be.call("gpk_sparse_paths_prepare", _p(self._omega), _p(self._phase), F, _p(w_d), _p(x_d), S, _p(self.coef), S * P,
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
    _STEP_GRAD, _ROLLOUT_GRAD = "gpk_paths_step_multi_grad_z", "gpk_paths_rollout_multi_grad_z"

    def __init__(self):
        raise TypeError("use BatchedSparseGP.sample_paths or BatchedSparsePosteriorPaths.from_randomness")

    def _basis(self, b):
        return self._X[b]

    @classmethod
    def from_randomness(cls, bg, omega, phase, weights, xi):
        """The path set of the sparse batch `bg` from arrays of the caller's own: omega (B, F, D), phase (B, F), weights
        (B, F, S), xi (B, m, S).  The set-up is one `gpk_sparse_paths_prepare` per model on that model's own handle, pointed at
        its column block and its slice of the basis points."""
        ms = list(bg.models)
        m, D = ms[0].inducing_.shape
        r, F, S = check_randomness(m, D, 1, omega, phase, weights, xi, "xi", batch=len(ms))
        bes, _ = bg._ensure()
        if any(b.device_index != bes[0].device_index for b in bes):
            raise RuntimeError("the models of a batch must be on one device")
        comps = [mm.kernel_.components() for mm in ms]
        self = object.__new__(cls)
        self._init_batch(bg, bes[0], None, m, D, r, F, S, [c.ls_vector(D) for c in comps], [c.sf2 for c in comps],
                         [mm._ym for mm in ms], [mm._ys for mm in ms])
        self._prepare_models(bes, lambda b, mb, w_d, x_d, block: mb.call(
            "gpk_sparse_paths_prepare", _p(self._omega[b]), _p(self._phase[b]), F, _p(w_d), _p(x_d), S, block, self.ldc,
            _p(self._X[b])))
        return self


# ---- the frame of a trainer's `sample_rollouts`: quadrotor state [p(3), v(3)], query [state(6), control(4)] ------------------------
def nominal_rollouts(dynamics, state, U_guess, dt, n_rollouts):
    """The nominal trajectory of `dynamics(x, u, dt)` from `state` under U_guess (4+, N), repeated n_rollouts times
    (R, 6, N + 1) - what a `sample_rollouts` returns when it cannot sample - and the 6 x 10 `lin` of a path set's rollout that
    is the same double integrator: x <- x + dt [v, a]."""
    N = U_guess.shape[1]
    nominal = np.empty((6, N + 1))
    nominal[:, 0] = state
    for k in range(N):
        nominal[:, k + 1] = dynamics(nominal[:, k], U_guess[:, k], dt)
    lin = np.zeros((6, 10))
    lin[0:3, 3:6] = dt * np.eye(3)
    lin[3:6, 6:9] = dt * np.eye(3)
    return np.repeat(nominal[None], max(int(n_rollouts), 0), axis=0), lin


def roll_paths(paths, state, U_guess, lin, return_jacobian=False, **how):
    """`paths.rollout` from `state` under U_guess (4+, N), as (R, 6, N + 1) - the layout of the trainers' X_guess.
    return_jacobian=True: (X, J), J (R, N, 6, 10) the Jacobian of the sampled residual of state coordinate i at stage k of
    rollout r w.r.t. [x_k, u_k]; a batch's models fill the rows of their `coord` (default 0 .. B - 1), the others stay zero."""
    U = np.ascontiguousarray(U_guess[:4].T)
    if not return_jacobian:
        traj = paths.rollout(state, U, lin, **how)      # (N + 1, R, 6)
        return np.ascontiguousarray(traj.transpose(1, 2, 0))
    traj, jac = paths.rollout(state, U, lin, return_jacobian=True, **how)      # (N + 1, R, 6), (N, R, outputs, 10)
    H, R, n_out, D = jac.shape
    rows = list(how.get("coord", range(n_out)))
    J = np.zeros((R, H, traj.shape[2], D))
    J[:, :, rows, :] = jac.transpose(1, 0, 2, 3)
    return np.ascontiguousarray(traj.transpose(1, 2, 0)), J


def cached_path_set(owner, attr, model, n_rollouts, n_features, random_state, finish=None):
    """The path set `model.sample_paths(n_rollouts, n_features, random_state)`, drawn once and kept on `owner` as
    `attr` = (key, paths) under the key (R, F, random_state, id(model), model.revision_) - a path set is a snapshot: a sparse
    model that has taken rows since it was drawn has a new revision.  `finish(paths)` runs once on a fresh set."""
    key = (int(n_rollouts), int(n_features), random_state if isinstance(random_state, (int, np.integer)) else id(random_state),
           id(model), getattr(model, "revision_", None))
    cached = getattr(owner, attr, None)      # (an object pickled before the attribute existed has none)
    if cached is None or cached[0] != key:
        paths = model.sample_paths(int(n_rollouts), n_features, random_state)
        if finish is not None:
            finish(paths)
        setattr(owner, attr, (key, paths))
    return getattr(owner, attr)[1]
