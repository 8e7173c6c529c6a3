"""Host-side checks of the horizon propagation; no device is touched.

`propagate_numpy_form` below is the expected value of every GPU test of the propagation: the recursion

    q = [x_h, U[r][h]],  z = (q - in_shift) / in_scale
    x_{h+1}     = x_h + lin q + sum_b e_coord[b] mu_b(z)
    A_h         = I + lin[:, :nx] + sum_b e_coord[b] J_b[:nx]
    Sigma_{h+1} = A_h Sigma_h A_h^T + sum_b v_b(z) e_coord[b] e_coord[b]^T + Q

on dense NumPy posteriors (`gp_numpy_form`: K = k(X, X) + (noise + alpha) I factored by LAPACK's Cholesky, the mean Jacobian and
the variance in closed form as in tests/test_gpu_jac.py).

1. Plumbing: both C entries are declared, bound and exported.
2. The form itself: A_h is the derivative of the mean recursion (central differences, 1e-6), and the Sigma recursion equals
   Hewing's block form [A B_d] [[Sx, Sx J^T], [J Sx, Sd + J Sx J^T]] [A B_d]^T (1e-12).
3. What the bar of the GPU tests rests on, printed and asserted for every fixture case: variance / prior along the horizon
   (> 1e-3: the clip at the floor is never active) and the growth of a 1e-12 relative perturbation of x0 (< 100).
4. The control-loop wrappers without a model, and the Python-side argument checks (before any device call)."""
import ctypes
import os

import numpy as np
import pytest
from scipy.linalg import cholesky, solve_triangular

from conftest import GOLDEN, ROOT

NEW_SYMBOLS = ("gpk_propagate_host", "gpk_propagate_host_multi")
SINGLE_CASES = ("a", "b", "csv", "one")
AXIS_CASES = ("a", "csv", "gap", "one")


def rbf(A, B, ls, sf2):
    d = (A / ls)[:, None, :] - (B / ls)[None, :, :]
    return sf2 * np.exp(-0.5 * np.sum(d * d, axis=2))


class gp_numpy_form:
    """One exact GP with P outputs on a shared kernel, normalize_y=True (normalize=False: y_mean = 0, y_std = 1):
    .stage(Z, noisy) -> mean (M, P), jac (M, P, D), var (M, P) in target units; noisy: the variance includes the WhiteKernel level
    (as predict(return_std=True)'s does)."""

    def __init__(self, X, Y, ls, sf2, noise, alpha, normalize=True):
        N = len(X)
        Y = Y.reshape(N, -1)
        self.X, self.ls, self.sf2, self.noise = X, np.broadcast_to(np.asarray(ls, dtype=float), (X.shape[1],)), sf2, noise
        self.ym, self.ys = (Y.mean(axis=0), Y.std(axis=0)) if normalize else (np.zeros(Y.shape[1]), np.ones(Y.shape[1]))
        self.L = cholesky(rbf(X, X, self.ls, sf2) + (noise + alpha) * np.eye(N), lower=True)
        Yn = (Y - self.ym) / self.ys
        self.alpha = solve_triangular(self.L, solve_triangular(self.L, Yn, lower=True), lower=True, trans="T")

    def stage(self, Z, noisy):
        k = rbf(Z, self.X, self.ls, self.sf2)                                      # (M, N)
        mean = self.ym + self.ys * (k @ self.alpha)
        u = (self.X[None, :, :] - Z[:, None, :]) / self.ls ** 2                    # (M, N, D)
        jac = self.ys[None, :, None] * np.einsum("mn,mnd,np->mpd", k, u, self.alpha)
        v = solve_triangular(self.L, k.T, lower=True)
        lat = np.maximum(self.sf2 + (self.noise if noisy else 0.0) - np.sum(v * v, axis=0), 0.0)
        return mean, jac, lat[:, None] * self.ys[None, :] ** 2


class propagate_numpy_form:
    """The recursion on a list of `gp_numpy_form`s whose outputs, one after the other, drive the state coordinates `coord`
    (default 0, 1, ...).  in_scaler = (shift, scale) or None; out = (mean, scale) per output behind the models' values or None.

    .run(x0 (R, nx), U (R, H, nu), lin, Sigma0 (R, nx, nx) / None, Q / None, noisy) -> traj (H + 1, R, nx), Sigma (H + 1, R, nx,
    nx), {"mean", "var" (H, R, NO), "jac" (H, R, NO, D) in RAW units}."""

    def __init__(self, gps, coord=None, in_scaler=None, out=None):
        self.gps = gps
        self.NO = sum(len(g.ym) for g in gps)
        self.coord = list(range(self.NO)) if coord is None else [int(c) for c in coord]
        self.in_scaler = in_scaler
        self.out = (np.zeros(self.NO), np.ones(self.NO)) if out is None else (np.asarray(out[0], float), np.asarray(out[1], float))

    def stage(self, q, noisy):
        D = q.shape[1]
        shift, scale = (np.zeros(D), np.ones(D)) if self.in_scaler is None else self.in_scaler
        parts = [g.stage((q - shift) / scale, noisy) for g in self.gps]
        mean, jac, var = (np.concatenate([p[i] for p in parts], axis=1) for i in range(3))
        om, os_ = self.out
        return om + os_ * mean, os_[None, :, None] * jac / scale[None, None, :], os_ ** 2 * var

    def step(self, x, u, lin, noisy):
        """one stage of the MEAN recursion: x (R, nx), u (R, nu) -> x_next, and the stage quantities"""
        q = np.concatenate([x, u], axis=1)
        mean, jac, var = self.stage(q, noisy)
        nxt = x + q @ lin.T
        nxt[:, self.coord] += mean
        return nxt, mean, jac, var

    def run(self, x0, U, lin, Sigma0=None, Q=None, noisy=False):
        nx, D = lin.shape
        R, H = U.shape[0], U.shape[1]
        traj, Sigma = np.zeros((H + 1, R, nx)), np.zeros((H + 1, R, nx, nx))
        st = {"mean": np.zeros((H, R, self.NO)), "var": np.zeros((H, R, self.NO)), "jac": np.zeros((H, R, self.NO, D)),
              "A": np.zeros((H, R, nx, nx))}
        traj[0] = x0
        if Sigma0 is not None:
            Sigma[0] = Sigma0
        for h in range(H):
            traj[h + 1], mean, jac, var = self.step(traj[h], U[:, h], lin, noisy)
            A = np.tile(np.eye(nx) + lin[:, :nx], (R, 1, 1))
            A[:, self.coord, :] += jac[:, :, :nx]
            S = A @ Sigma[h] @ A.transpose(0, 2, 1)
            S[:, self.coord, self.coord] += var
            if Q is not None:
                S = S + Q
            Sigma[h + 1] = S
            st["mean"][h], st["var"][h], st["jac"][h], st["A"][h] = mean, var, jac, A
        return traj, Sigma, st


def rollouts(x0_row, U, R):
    """The R rollouts of the GPU tests from a fixture's first start and its controls: x0 + 0.01 r and U (1 + 0.05 r)."""
    r = np.arange(R, dtype=float)
    return x0_row[None, :] + 0.01 * r[:, None], U[None, :, :] * (1.0 + 0.05 * r)[:, None, None]


def spd(nx, seed=3):
    """a fixed SPD Sigma0 and process noise Q, symmetric bit for bit"""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((nx, nx))
    S0 = 1e-2 * (G @ G.T + nx * np.eye(nx))
    Q = 1e-4 * np.diag(1.0 + np.arange(nx))
    return 0.5 * (S0 + S0.T), Q


_single, _axis = {}, {}


def single_form(name):
    """(the fixture's arrays, the NumPy form) of a single-model case of tests/golden/paths_ref.npz"""
    if name not in _single:
        d = np.load(os.path.join(GOLDEN, "paths_ref.npz"))
        c = {k[len(name) + 1:]: d[k] for k in d.files if k.startswith(name + "_")}
        sf2, noise, alpha = c["hyper"]
        _single[name] = (c, propagate_numpy_form([gp_numpy_form(c["X"], c["Y"], c["ls"], sf2, noise, alpha)]))
    return _single[name]


def axis_form(name, keep=None, coord=None, scaled=True):
    """(the fixture's arrays, the NumPy form) of a batch case of tests/golden/axis_paths_ref.npz: the models `keep` (default
    all) on the coordinates `coord` (default the fixture's) behind the fixture's input scaler (scaled) and output scaler."""
    key = (name, None if keep is None else tuple(keep), None if coord is None else tuple(coord), scaled)
    if key not in _axis:
        d = np.load(os.path.join(GOLDEN, "axis_paths_ref.npz"))
        c = {k[len(name) + 1:]: d[k].astype(np.float64) for k in d.files if k.startswith(name + "_")}
        c["coord"] = c["coord"].astype(int)
        ks = list(range(len(c["ls"]))) if keep is None else list(keep)
        gps = [gp_numpy_form(c["X"], c["Y"][:, b], c["ls"][b], *c["hyper"][b]) for b in ks]
        cd = [int(c["coord"][b]) for b in ks] if coord is None else list(coord)
        form = propagate_numpy_form(gps, cd, (c["in"][0], c["in"][1]) if scaled else None,
                                    (c["out"][0][ks], c["out"][1][ks]) if scaled else None)
        _axis[key] = (c, form)
    return _axis[key]


def eight_problem():
    """B = 8 models (the most a call takes) on D = 10 inputs, seeded: a state of nx = 8 coordinates, two controls, H = 6, an
    input scaler and an output scaler that are not the identity.  The arrays of a fixture case, and the NumPy form."""
    if "eight" not in _axis:
        rng = np.random.default_rng(808)
        N, D, B, H = 64, 10, 8, 6
        X = rng.standard_normal((N, D))
        Y = 0.2 * np.sin(X @ rng.standard_normal((D, B)) / 2.0) + 0.02 * rng.standard_normal((N, B))
        c = {"X": X, "Y": Y, "ls": 2.5 + 0.25 * np.arange(B)[:, None] + 0.05 * np.arange(D)[None, :],
             "hyper": np.stack([0.8 + 0.05 * np.arange(B), 0.01 * (1 + np.arange(B)), np.full(B, 1e-6)], axis=1),
             "x0": 0.3 * rng.standard_normal((1, B)), "U": 0.3 * rng.standard_normal((H, D - B)),
             "lin": 0.05 * rng.standard_normal((B, D)), "coord": np.array([7, 0, 3, 1, 6, 2, 5, 4]),
             "in": np.stack([0.1 * rng.standard_normal(D), 1.0 + 0.1 * np.arange(D)]),
             "out": np.stack([0.01 * rng.standard_normal(B), 0.5 + 0.1 * np.arange(B)])}
        gps = [gp_numpy_form(X, Y[:, b], c["ls"][b], *c["hyper"][b]) for b in range(B)]
        _axis["eight"] = (c, propagate_numpy_form(gps, c["coord"], (c["in"][0], c["in"][1]), (c["out"][0], c["out"][1])))
    return _axis["eight"]


class sparse_numpy_form:
    """`gp_numpy_form`'s interface on the dense form of one single-output sparse posterior (tests/test_gpu_sparse_batch.py:
    numpy_form, Sigma = Kuu + Kuf Kfu / s2); p: the model's inputs as `model_inputs` there builds them.  The dense form's variance
    carries the noise level; the latent one takes it off again."""

    def __init__(self, p, alpha):
        self.p, self.a = p, alpha
        self.ym, self.ys, self.sf2 = np.array([p["ym"]]), np.array([p["ys"]]), p["sf2"]

    def stage(self, Zq, noisy):
        from test_gpu_sparse_batch import numpy_form
        p = self.p
        mean, var, dmean, _, _ = numpy_form(p["X"], p["y"], p["Z"], Zq, p["ls"], p["sf2"], p["noise"], self.a, 1e-8 * p["sf2"],
                                            p["ym"], p["ys"])
        if not noisy:
            var = np.maximum(var - p["noise"] * p["ys"] ** 2, 0.0)
        return mean[:, None], dmean[:, None, :], var[:, None]


def sparse_batch_problem():
    """B = 2 sparse models (m = 60 inducing inputs, n = 400 rows, D = 10; the inputs of tests/test_gpu_sparse_batch.py's case
    (2, 60, 400, 10)) on coordinates (4, 1) of a state of nx = 6, H = 5, behind scalers: the arrays and the NumPy form."""
    if "sparse" not in _axis:
        from test_gpu_sparse_batch import ALPHA, model_inputs
        ps = [model_inputs(b, 60, 400, 10) for b in range(2)]
        rng = np.random.default_rng(909)
        lin = np.zeros((6, 10))
        lin[0:3, 3:6] = 0.05 * np.eye(3)
        lin[3:6, 6:9] = 0.05 * np.eye(3)
        c = {"ps": ps, "x0": 0.4 * rng.standard_normal((1, 6)), "U": 0.4 * rng.standard_normal((5, 4)), "lin": lin,
             "coord": np.array([4, 1]), "in": np.stack([0.05 * rng.standard_normal(10), 1.0 + 0.02 * np.arange(10)]),
             "out": np.array([[0.01, -0.02], [0.1, 0.2]])}
        form = propagate_numpy_form([sparse_numpy_form(p, ALPHA) for p in ps], c["coord"], (c["in"][0], c["in"][1]),
                                    (c["out"][0], c["out"][1]))
        _axis["sparse"] = (c, form)
    return _axis["sparse"]


def reference_models_form(tr):
    """The NumPy form of the six models of tests/golden/trainer_ref.npz as `PreTrainedGP` serves them in raw units: each model on
    its own scaled rows (normalize_y=False, alpha 1e-6), the shared input scaler and each model's target scaler around it."""
    names = [str(n) for n in tr["names"]]
    D = tr["X"].shape[1]
    gps = []
    for n in names:
        th = tr[f"{n}_theta"]
        gps.append(gp_numpy_form(tr[f"{n}_X_train"], tr[f"{n}_y_train"], np.exp(th[:D]), 1.0, float(np.exp(th[D])), 1e-6,
                                 normalize=False))
    sx = (tr[f"{names[0]}_sx_mean"], tr[f"{names[0]}_sx_scale"])
    out = (np.array([tr[f"{n}_sy_mean"][0] for n in names]), np.array([tr[f"{n}_sy_scale"][0] for n in names]))
    return propagate_numpy_form(gps, list(range(6)), sx, out)


def reference_horizon(tr, dt=0.05, H=8):
    """a start, controls (4, H) and the nominal `lin` for the reference models: a training row and small accelerations"""
    row = tr["X"][5]
    lin = np.zeros((6, 10))
    lin[0:3, 3:6] = dt * np.eye(3)
    lin[3:6, 6:9] = dt * np.eye(3)
    U = np.stack([tr["X"][5 + k, 6:10] for k in range(H)], axis=1)
    return row[:6].copy(), U, lin, dt


# ---- 1. plumbing -------------------------------------------------------------------------------------------------------------------
def test_libgpk_exports_the_propagation_entries():
    from unmanned_aerial_vehicles_amd import _build, _lib
    assert os.path.exists(_build.LIB_PATH), "libgpk.so must be built in-tree (python __graft_entry__.py)"
    _lib.load()
    lib = ctypes.CDLL(_build.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "gpk.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert f"GPK_API int {name}(" in header
        assert name in _lib.SIGNATURES
    assert "gpk_propagate.hip" in _build.SOURCES
    assert _lib.GPK_TIMED_PROPAGATE == 9 and "GPK_TIMED_PROPAGATE = 9" in header


def test_package_surface():
    import unmanned_aerial_vehicles_amd as pkg
    from unmanned_aerial_vehicles_amd.sparse import SparseGP
    from unmanned_aerial_vehicles_amd.trainer import PreTrainedGP
    from unmanned_aerial_vehicles_amd.sparse_batch import BatchedSparseGP
    for cls in (pkg.GaussianProcessRegressor, pkg.BatchedARDGP, SparseGP, BatchedSparseGP):
        assert callable(getattr(cls, "propagate", None)), cls
    assert callable(pkg.SimpleQuadrotorGP.propagate_horizon) and callable(PreTrainedGP.propagate_horizon)


# ---- 2. the form itself ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("b", "csv"))
def test_A_is_the_derivative_of_the_mean_recursion(name):
    c, form = single_form(name)
    x0, U = rollouts(c["x0"][0], c["U"], 2)
    lin = c["lin"]
    _, _, st = form.run(x0, U, lin)
    nx = lin.shape[0]
    worst = 0.0
    for h in (0, len(c["U"]) - 1):
        x = form.run(x0, U[:, :h], lin)[0][-1] if h else x0
        fd = np.zeros((2, nx, nx))
        eps = 1e-5
        for j in range(nx):
            e = np.zeros(nx)
            e[j] = eps
            fd[:, :, j] = (form.step(x + e, U[:, h], lin, False)[0] - form.step(x - e, U[:, h], lin, False)[0]) / (2 * eps)
        worst = max(worst, float(np.max(np.abs(fd - st["A"][h])) / np.max(np.abs(st["A"][h]))))
    print(f"case {name}: A_h against central differences of the mean recursion: {worst:.2e} (bar 1e-6)")
    assert worst < 1e-6


@pytest.mark.parametrize("name", SINGLE_CASES)
def test_sigma_recursion_equals_the_block_form(name):
    """Hewing, Kabzan, Zeilinger: with J the Jacobian of the residual d w.r.t. x, Sd = diag(var) and B_d the selector of the driven
    coordinates, Sigma+ = [A0 B_d] [[Sx, Sx J^T], [J Sx, Sd + J Sx J^T]] [A0 B_d]^T with A0 = I + lin_x - the model's share of A_h
    moved into the joint covariance of (x, d)."""
    c, form = single_form(name)
    x0, U = rollouts(c["x0"][0], c["U"], 3)
    lin = c["lin"]
    nx = lin.shape[0]
    S0, Q = spd(nx)
    traj, Sigma, st = form.run(x0, U, lin, np.tile(S0, (3, 1, 1)), Q)
    A0 = np.eye(nx) + lin[:, :nx]
    Bd = np.eye(nx)[:, form.coord]
    worst = 0.0
    for h in range(len(c["U"])):
        for r in range(3):
            Sx, J, Sd = Sigma[h, r], st["jac"][h, r][:, :nx], np.diag(st["var"][h, r])
            joint = np.block([[Sx, Sx @ J.T], [J @ Sx, Sd + J @ Sx @ J.T]])
            AB = np.concatenate([A0, Bd], axis=1)
            want = AB @ joint @ AB.T + Q
            worst = max(worst, float(np.max(np.abs(want - Sigma[h + 1, r])) / np.max(np.abs(want))))
    print(f"case {name}: Sigma recursion against the block form: {worst:.2e} (bar 1e-12)")
    assert worst < 1e-12


# ---- 3. what the bar of the GPU tests rests on ---------------------------------------------------------------------------------
def _room(tag, form, x0, U, lin, prior):
    traj, Sigma, st = form.run(x0, U, lin)
    ratio = float(np.min(st["var"] / prior))
    normA = float(max(np.linalg.norm(a, 2) for a in st["A"].reshape(-1, *st["A"].shape[2:])))
    t2, S2, _ = form.run(x0 * (1.0 + 1e-12), U, lin)
    gx = float(np.max(np.abs(t2 - traj)) / np.max(np.abs(traj)) / 1e-12)
    gs = float(np.max(np.abs(S2 - Sigma)) / np.max(np.abs(Sigma)) / 1e-12)
    print(f"{tag}: min variance / prior {ratio:.3e}, max |A_h|_2 {normA:.2f}, growth of a 1e-12 perturbation of x0: "
          f"{gx:.1f}x in x, {gs:.1f}x in Sigma")
    assert ratio > 1e-3 and gx < 100 and gs < 100, tag
    return gs


@pytest.mark.parametrize("name", SINGLE_CASES)
def test_single_model_cases_leave_room_under_the_bar(name):
    c, form = single_form(name)
    g = form.gps[0]
    for R in (1, 5):
        x0, U = rollouts(c["x0"][0], c["U"], R)
        _room(f"case {name}, R = {R}", form, x0, U, c["lin"], g.sf2 * g.ys[None, None, :] ** 2)


@pytest.mark.parametrize("name", AXIS_CASES)
def test_batch_cases_leave_room_under_the_bar(name):
    c, form = axis_form(name)
    prior = np.array([g.sf2 * g.ys[0] ** 2 for g in form.gps]) * form.out[1] ** 2
    for R in (1, 5):
        x0, U = rollouts(c["x0"][0], c["U"], R)
        _room(f"batch case {name}, R = {R}", form, x0, U, c["lin"], prior[None, None, :])


def test_eight_models_and_reference_models_leave_room_under_the_bar(trainer_ref):
    c, form = eight_problem()
    prior = np.array([g.sf2 * g.ys[0] ** 2 for g in form.gps]) * form.out[1] ** 2
    for R in (1, 5):
        x0, U = rollouts(c["x0"][0], c["U"], R)
        _room(f"eight models, R = {R}", form, x0, U, c["lin"], prior[None, None, :])
    c, form = sparse_batch_problem()
    prior = np.array([g.sf2 * g.ys[0] ** 2 for g in form.gps]) * form.out[1] ** 2
    for R in (1, 3):
        x0, U = rollouts(c["x0"][0], c["U"], R)
        _room(f"two sparse models, R = {R}", form, x0, U, c["lin"], prior[None, None, :])
    form = reference_models_form(trainer_ref)
    state, Ug, lin, _ = reference_horizon(trainer_ref)
    prior = np.array([g.sf2 for g in form.gps]) * form.out[1] ** 2
    _room("the reference trainer's six models", form, state[None], np.ascontiguousarray(Ug.T)[None], lin, prior[None, None, :])


def test_long_horizon_growth_on_case_one():
    """H = 256 on case `one` (controls repeated): the growth over the first 8 stages, the ones the GPU test compares."""
    c, form = single_form("one")
    U = np.tile(c["U"], (64, 1))[None]
    g = form.gps[0]
    _room("case one, first 8 of H = 256", form, c["x0"][:1], U[:, :8], c["lin"], g.sf2 * g.ys[None, None, :] ** 2)
    traj, Sigma, _ = form.run(c["x0"][:1], U, c["lin"])
    print(f"case one, H = 256: max |x| {np.max(np.abs(traj)):.3e}, max |Sigma| {np.max(np.abs(Sigma)):.3e}")


# ---- 4. the wrappers without a model, the argument checks -----------------------------------------------------------------------
def _nominal_sigma(lin, S0, Q, N):
    A = np.eye(6) + lin[:, :6]
    out = [S0]
    for _ in range(N):
        out.append(A @ out[-1] @ A.T + Q)
    return np.stack(out)


def test_untrained_wrappers_return_the_nominal_horizon(capsys):
    import unmanned_aerial_vehicles_amd as pkg
    from unmanned_aerial_vehicles_amd.paths import nominal_rollouts
    from unmanned_aerial_vehicles_amd.trainer import PreTrainedGP
    state, U, dt = np.arange(6.0) / 7.0, np.linspace(-1.0, 1.0, 12).reshape(4, 3), 0.1
    S0, Q = spd(6)
    sq = pkg.SimpleQuadrotorGP()
    pre = PreTrainedGP(os.path.join(ROOT, "no_such_model_file.pkl"))
    capsys.readouterr()
    for obj in (sq, pre):
        X, Sig = obj.propagate_horizon(state, U, dt, Sigma0=S0, process_noise=Q)
        said = capsys.readouterr().out
        assert "propagation" in said and ("not trained" in said or "no models are loaded" in said), said
        nominal, lin = nominal_rollouts(sq._nominal_dynamics, state, U, dt, 1)
        assert X.shape == (6, 4) and Sig.shape == (4, 6, 6)
        assert np.array_equal(X, nominal[0])
        assert np.allclose(Sig, _nominal_sigma(lin, S0, Q, 3), rtol=1e-14, atol=0)
        XR, SR = obj.propagate_horizon(state, np.stack([U, 2 * U]), dt)
        capsys.readouterr()
        assert XR.shape == (2, 6, 4) and SR.shape == (2, 4, 6, 6) and not SR.any()
        assert np.array_equal(XR[0], nominal[0]) and not np.array_equal(XR[1], nominal[0])
    assert sq.prediction_count == 0


def test_python_side_argument_checks():
    from unmanned_aerial_vehicles_amd.propagate import check_coord, check_horizon
    nx, D, H = 3, 5, 4
    x0, U, lin = np.zeros(nx), np.zeros((H, D - nx)), np.zeros((nx, D))
    S0, Q = spd(nx)
    out = check_horizon(x0, U, lin, nx, D, S0, Q)
    assert out[0].shape == (1, nx) and out[1].shape == (1, H, D - nx) and out[3].shape == (1, nx, nx) and out[5:] == (1, H)
    out = check_horizon(np.zeros((7, nx)), U, lin, nx, D)
    assert out[5:] == (7, H) and out[3] is None and out[4] is None
    out = check_horizon(x0, np.zeros((32, H, D - nx)), lin, nx, D, np.tile(S0, (32, 1, 1)))
    assert out[5:] == (32, H)
    bad = S0.copy()
    bad[0, 1] = np.nextafter(bad[0, 1], 1.0)
    nan = x0.copy()
    nan[1] = np.nan
    for what, args in (("asymmetric Sigma0", (x0, U, lin, nx, D, bad)),
                       ("asymmetric process noise", (x0, U, lin, nx, D, None, bad)),
                       ("x0 of the wrong width", (np.zeros(nx + 1), U, lin, nx, D)),
                       ("U of the wrong width", (x0, np.zeros((H, D - nx + 1)), lin, nx, D)),
                       ("lin of the wrong shape", (x0, U, np.zeros((nx, D + 1)), nx, D)),
                       ("Sigma0 of the wrong shape", (x0, U, lin, nx, D, np.zeros((nx, nx + 1)))),
                       ("rollout counts that disagree", (np.zeros((3, nx)), np.zeros((4, H, D - nx)), lin, nx, D)),
                       ("R = 33", (np.zeros((33, nx)), U, lin, nx, D)),
                       ("H = 0", (x0, np.zeros((0, D - nx)), lin, nx, D)),
                       ("H = 257", (x0, np.zeros((257, D - nx)), lin, nx, D)),
                       ("NaN in x0", (nan, U, lin, nx, D)),
                       ("infinity in U", (x0, np.full((H, D - nx), np.inf), lin, nx, D)),
                       ("NaN in lin", (x0, U, np.full((nx, D), np.nan), nx, D)),
                       ("nx above D", (np.zeros(6), np.zeros((H, 0)), np.zeros((6, 5)), 6, 5))):
        with pytest.raises(ValueError):
            check_horizon(*args)
            pytest.fail(what)
    assert check_coord(None, 2, 3) == [0, 1] and check_coord((2, 0), 2, 3) == [2, 0]
    for coord in ((0, 0), (0, 3), (0,), (-1, 1)):
        with pytest.raises(ValueError):
            check_coord(coord, 2, 3)
    # the estimators check before they touch the device: an unfitted model says so, whatever else is wrong
    import unmanned_aerial_vehicles_amd as pkg
    with pytest.raises(RuntimeError):
        pkg.GaussianProcessRegressor().propagate(x0, U, lin)
    with pytest.raises(RuntimeError):
        pkg.BatchedARDGP().propagate(x0, U, lin)
