"""Posterior function draws of the sparse models ("the sparse models"): what can be checked without a GPU.

1. The draw functions: shapes, order, seeding; model 0 of the batch draw is the single-model draw.
2. The method, in the dense NumPy form of tests/golden/make_golden_sparse_paths.py: xi = 0, w = 0 gives the sparse posterior
   mean exactly; B B^T is the + V1^T V1 term of the sparse covariance; the closed-form ensemble covariance A A^T + B B^T
   approaches the sparse posterior covariance as F grows.
3. tests/golden/sparse_paths_ref.npz holds what that form gives, and every case meets the fixture condition (two evaluations
   agree to 1e-10, cond(Kuu + jitter_uu I) <= 1e5).  Error growth of `rollout`, recorded in the fixture: a 1e-12 relative
   perturbation of x0 grows 7.6x (a), 80x (b), 5.7x (g), 4.9x (c, 25 stages), 3.7x (d), 1.9x (e) over the horizon in the NumPy
   form, so the 1e-8 bar of the device tests leaves room.
4. The public names exist, limits and shapes raise ValueError before any device is touched, and a `PreTrainedGP` with nothing
   loaded prints its reason and returns the nominal trajectory."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLDEN, relerr

SINGLE, BATCH = ("a", "b", "g"), ("c", "d", "e", "f")


@pytest.fixture(scope="module")
def G():
    spec = importlib.util.spec_from_file_location("make_golden_sparse_paths", os.path.join(GOLDEN, "make_golden_sparse_paths.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_case(name):
    d = np.load(os.path.join(GOLDEN, "sparse_paths_ref.npz"))
    return {k[len(name) + 1:]: d[k].astype(np.float64) for k in d.files if k.startswith(name + "_")}


def single_form(G, c, omega=None, phase=None, weights=None, xi=None, **kw):
    pick = lambda v, k: c[k] if v is None else v      # noqa: E731
    return G.SparseForm(c["Z"], c["X"], c["Y"], c["ls"], *c["hyper"], c["ynorm"][0], c["ynorm"][1], pick(omega, "omega"),
                        pick(phase, "phase"), pick(weights, "weights"), pick(xi, "xi"), **kw)


# ---- 1. the draws ----------------------------------------------------------------------------------------------------------------------
def test_draw_functions_shapes_order_and_seeding():
    from unmanned_aerial_vehicles_amd import draw_sparse_batch_path_randomness, draw_sparse_path_randomness
    m, D, F, S, P = 7, 3, 5, 4, 2
    ls = np.array([0.5, 1.0, 2.0])
    r = draw_sparse_path_randomness(np.random.RandomState(11), m, D, F, S, P, ls)
    assert sorted(r) == ["omega", "phase", "weights", "xi"]
    assert r["omega"].shape == (F, D) and r["phase"].shape == (F,) and r["weights"].shape == (F, S, P) and r["xi"].shape == (m, S, P)
    rng = np.random.RandomState(11)                  # the documented order, restated
    assert np.array_equal(r["omega"], rng.standard_normal((F, D)) / ls)
    assert np.array_equal(r["phase"], rng.uniform(0.0, 2.0 * np.pi, F))
    assert np.array_equal(r["weights"], rng.standard_normal((F, S, P)))
    assert np.array_equal(r["xi"], rng.standard_normal((m, S, P)))
    again = draw_sparse_path_randomness(np.random.RandomState(11), m, D, F, S, P, ls)
    other = draw_sparse_path_randomness(np.random.RandomState(12), m, D, F, S, P, ls)
    assert all(np.array_equal(r[k], again[k]) for k in r) and not np.array_equal(r["xi"], other["xi"])
    g = draw_sparse_path_randomness(np.random.default_rng(5), m, D, F, S, 1, 1.5)      # a Generator, a scalar length-scale
    assert g["xi"].shape == (m, S, 1) and (g["phase"] >= 0).all() and (g["phase"] < 2 * np.pi).all()
    # the batch: model by model from the one generator
    lsb = np.stack([ls, 2.0 * ls, 0.7 * ls])
    b = draw_sparse_batch_path_randomness(np.random.RandomState(11), m, D, F, S, lsb)
    assert b["omega"].shape == (3, F, D) and b["phase"].shape == (3, F) and b["weights"].shape == (3, F, S) and b["xi"].shape == (3, m, S)
    rng = np.random.RandomState(11)
    for k in range(3):
        one = draw_sparse_path_randomness(rng, m, D, F, S, 1, lsb[k])
        assert np.array_equal(b["omega"][k], one["omega"]) and np.array_equal(b["phase"][k], one["phase"])
        assert np.array_equal(b["weights"][k], one["weights"][:, :, 0]) and np.array_equal(b["xi"][k], one["xi"][:, :, 0])
    for bad in (dict(m=0), dict(F=0), dict(S=0)):
        a = dict(m=m, D=D, F=F, S=S)
        a.update(bad)
        with pytest.raises(ValueError):
            draw_sparse_path_randomness(np.random.RandomState(0), a["m"], a["D"], a["F"], a["S"], 1, ls)
    with pytest.raises(ValueError):
        draw_sparse_batch_path_randomness(np.random.RandomState(0), m, D, F, S, np.ones((9, D)))
    with pytest.raises(ValueError):
        draw_sparse_batch_path_randomness(np.random.RandomState(0), m, D, F, S, np.ones((2, D + 1)))


# ---- 2. the method ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SINGLE)
def test_zero_randomness_is_the_sparse_mean_exactly(G, name):
    c = load_case(name)
    f = single_form(G, c, weights=np.zeros_like(c["weights"]), xi=np.zeros_like(c["xi"]))
    got, mean = f.all(c["Xq"]), f.mean(c["Xq"])
    S = got.shape[1]
    # (exact in exact arithmetic - v = alpha_u and the cosine rows are zero; the two products only differ in BLAS's blocking)
    assert relerr(got, np.repeat(mean[:, None, :], S, axis=1)) < 1e-14, "xi = 0, w = 0: every path is the mean"
    # and that mean is the DTC predictor written the textbook way: sigma^-2 Kqu (Kuu + sigma^-2 Kuf Kfu)^-1 Kuf yn
    sf2, noise, alpha, jit = c["hyper"]
    Kuf = G.rbf(c["Z"], c["X"], c["ls"], sf2)
    Yn = (c["Y"] - c["ynorm"][0]) / c["ynorm"][1]
    A = G.rbf(c["Z"], c["Z"], c["ls"], sf2) + jit * np.eye(len(c["Z"])) + Kuf @ Kuf.T / (noise + alpha)
    want = c["ynorm"][0] + c["ynorm"][1] * (G.rbf(c["Xq"], c["Z"], c["ls"], sf2) @ np.linalg.solve(A, Kuf @ Yn) / (noise + alpha))
    assert relerr(mean, want) < 1e-10


@pytest.mark.parametrize("name", SINGLE)
def test_the_xi_term_is_the_v1_term_of_the_sparse_covariance(G, name):
    c = load_case(name)
    f = single_form(G, c)
    _, BB = f.ensemble_cov(c["Xq"])
    _, V1 = f.cov_terms(c["Xq"])
    assert relerr(BB, V1) < 1e-13
    # ... and V1^T V1 = Kqu (Kuu + sigma^-2 Kuf Kfu)^-1 Kuq, the textbook form
    sf2, noise, alpha, jit = c["hyper"]
    Kuf, Kqu = G.rbf(c["Z"], c["X"], c["ls"], sf2), G.rbf(c["Xq"], c["Z"], c["ls"], sf2)
    A = G.rbf(c["Z"], c["Z"], c["ls"], sf2) + jit * np.eye(len(c["Z"])) + Kuf @ Kuf.T / (noise + alpha)
    assert relerr(V1, Kqu @ np.linalg.solve(A, Kqu.T)) < 1e-10


def test_the_ensemble_covariance_approaches_the_sparse_posterior_covariance(G):
    """Case a, omega and phase drawn with RandomState(0) at each F: max |A A^T + B B^T - (K** - V0^T V0 + V1^T V1)| over the nine
    query rows, relative to the largest posterior variance, measured 1.16e-1 (F = 256), 5.34e-2 (1024), 3.60e-2 (4096),
    2.48e-2 (16 384) - the 1 / sqrt(F) error of random Fourier features (seeds 1 and 2: 1.3e-1 .. 1.5e-2, 1.2e-1 .. 2.0e-2;
    case g the same within 2x).  Asserted: monotone, and at most 5e-2 at F = 16 384 - twice the worst value seen over the seeds."""
    c = load_case("a")
    m, D = c["Z"].shape
    Q = c["Xq"]
    errs = []
    for F in (256, 1024, 4096, 16384):
        om, ph, w, xi = G.draw(np.random.RandomState(0), m, D, F, 1, 1, c["ls"])
        f = single_form(G, c, om, ph, w, xi)
        AA, BB = f.ensemble_cov(Q)
        V0, V1 = f.cov_terms(Q)
        post = G.rbf(Q, Q, c["ls"], c["hyper"][0]) - V0 + V1
        errs.append(float(np.max(np.abs(AA + BB - post)) / np.max(np.diag(post))))
        print(f"F = {F}: {errs[-1]:.3e}")
    assert all(a > b for a, b in zip(errs, errs[1:])), errs
    assert errs[-1] < 5e-2, errs


# ---- 3. the fixture --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SINGLE + BATCH)
def test_fixture_holds_the_numpy_form_and_is_well_determined(G, name):
    c = load_case(name)
    if name in SINGLE:
        forms = [single_form(G, c, explicit=e) for e in (True, False)]
        rolls = [f.rollout(c["x0"], c["U"], c["lin"]) for f in forms]
        conds = [forms[0].cond()]
    else:
        forms = [G.SparseBatchForm(c["Z"], c["X"], c["Y"], c["ls"], c["hyper"], c["ynorm"], c["omega"], c["phase"], c["weights"],
                                   c["xi"], c["out"], explicit=e) for e in (True, False)]
        rolls = [f.rollout(c["x0"], c["U"], c["lin"], c["coord"].astype(int), (c["in"][0], c["in"][1])) for f in forms] if "traj" in c else None
        conds = [f.cond() for f in forms[0].forms]
    assert max(conds) <= G.COND_MAX, conds
    for k, vals in (("all", [f.all(c["Xq"]) for f in forms]), ("step", [f.step(c["Xs"]) for f in forms]), ("traj", rolls)):
        if vals is None:
            assert name == "f"
            continue
        assert vals[0].shape == c[k].shape
        assert relerr(vals[0], c[k]) < 1e-11, (name, k, "the fixture is not what the form gives")
        assert relerr(vals[1], vals[0]) <= G.AGREE, (name, k, "the two evaluations differ")
    if "growth" in c:
        assert 1.0 <= float(np.ravel(c["growth"])[0]) < 100.0, "the rollout's own error growth must leave room under the 1e-8 bar"
    assert os.path.getsize(os.path.join(GOLDEN, "sparse_paths_ref.npz")) <= os.path.getsize(os.path.join(GOLDEN, "axis_paths_ref.npz"))


# ---- 4. the public surface, without a device ---------------------------------------------------------------------------------------------
def test_public_names_exist():
    import unmanned_aerial_vehicles_amd as pkg
    for name in ("draw_sparse_path_randomness", "draw_sparse_batch_path_randomness", "SparsePosteriorPaths", "BatchedSparsePosteriorPaths"):
        assert name in pkg.__all__ and callable(getattr(pkg, name)), name
    assert callable(pkg.SparseGP.sample_paths) and callable(pkg.BatchedSparseGP.sample_paths)
    for cls in (pkg.SparsePosteriorPaths, pkg.BatchedSparsePosteriorPaths):
        for attr in ("from_randomness", "step", "rollout", "__call__"):
            assert callable(getattr(cls, attr)), (cls, attr)
        with pytest.raises(TypeError):
            cls()
    assert callable(pkg.BatchedSparsePosteriorPaths.set_output_scaler)
    from unmanned_aerial_vehicles_amd import _lib
    for name in ("gpk_sparse_paths_prepare", "gpk_paths_step_multi_z", "gpk_paths_rollout_multi_z"):
        assert name in _lib.SIGNATURES
    assert _lib.SIGNATURES["gpk_paths_step_multi_z"] == _lib.SIGNATURES["gpk_paths_step_multi"]
    assert _lib.SIGNATURES["gpk_paths_rollout_multi_z"] == _lib.SIGNATURES["gpk_paths_rollout_multi"]


def test_limits_and_shapes_raise_value_errors_without_a_device():
    from unmanned_aerial_vehicles_amd import (RBF, BatchedSparseGP, BatchedSparsePosteriorPaths, SparseGP, SparsePosteriorPaths,
                                              WhiteKernel)
    rng = np.random.RandomState(3)
    m, D, F, S = 6, 3, 8, 4
    sp = SparseGP(RBF(1.0) + WhiteKernel(0.1), rng.standard_normal((m, D)), alpha=1e-4)
    for n_paths, n_features in ((0, 16), (4097, 16), (2, 0), (2, 16385)):
        with pytest.raises(ValueError):
            sp.sample_paths(n_paths, n_features=n_features)
    om, ph, w, x = rng.standard_normal((F, D)), rng.uniform(0, 6, F), rng.standard_normal((F, S, 1)), rng.standard_normal((m, S, 1))
    for bad in ((om[:, :2], ph, w, x), (om, ph[:-1], w, x), (om, ph, w[:-1], x), (om, ph, w, x[:-1]), (om, ph, w, x[:, :-1]),
                (om, ph, np.tile(w, (1, 1, 2)), x), (np.where(om == om[0, 0], np.nan, om), ph, w, x),
                (om, np.where(ph == ph[0], np.inf, ph), w, x), (om, ph, np.where(w == w[0, 0, 0], np.nan, w), x),
                (om, ph, w, np.where(x == x[0, 0, 0], np.inf, x))):
        with pytest.raises(ValueError):
            SparsePosteriorPaths.from_randomness(sp, *bad)
    # gpk_padded(m) + gpk_padded(F) > 65535: 50 048 + 16 384
    big = SparseGP(RBF(1.0) + WhiteKernel(0.1), np.arange(50000.0)[:, None], alpha=1e-4)
    with pytest.raises(ValueError, match="65535"):
        SparsePosteriorPaths.from_randomness(big, np.ones((16384, 1)), np.zeros(16384), np.zeros((16384, 1, 1)), np.zeros((50000, 1, 1)))
    bg = BatchedSparseGP([SparseGP(RBF(1.0 + 0.1 * b) + WhiteKernel(0.1), rng.standard_normal((m, D)), alpha=1e-4) for b in range(2)])
    for n_paths, n_features in ((0, 16), (4097, 16), (2, 0), (2, 16385)):
        with pytest.raises(ValueError):
            bg.sample_paths(n_paths, n_features=n_features)
    om, ph, w, x = (np.stack([a, a]) for a in (om, ph, w[:, :, 0], x[:, :, 0]))
    for bad in ((om[:, :, :2], ph, w, x), (om[:1], ph, w, x), (om, ph[:, :-1], w, x), (om, ph, w[:, :-1], x), (om, ph, w, x[:, :-1]),
                (om, ph, w, np.concatenate([x, x], axis=2)), (om, ph, np.where(w == w[0, 0, 0], np.nan, w), x)):
        with pytest.raises(ValueError):
            BatchedSparsePosteriorPaths.from_randomness(bg, *bad)
    # a model's revision moves with what a path set is a snapshot of (no device: nothing has been begun)
    assert sp.revision_ == 0 and bg.revision_ == (0, 0)


def test_pretrained_gp_with_nothing_loaded_returns_the_nominal_trajectory(capsys):
    from unmanned_aerial_vehicles_amd import PreTrainedGP
    from unmanned_aerial_vehicles_amd.trainer import GPTrainer
    pg = PreTrainedGP("/nonexistent/model.pkl")
    capsys.readouterr()
    state, U, dt = np.array([0.1, -0.2, 1.0, 0.3, 0.0, -0.1]), 0.2 * np.ones((4, 5)), 0.02
    out = pg.sample_rollouts(state, U, dt, n_rollouts=3, n_features=8)
    assert "GP rollout sampling failed: no models are loaded" in capsys.readouterr().out
    nominal = np.empty((6, 6))
    nominal[:, 0] = state
    for k in range(5):
        nominal[:, k + 1] = GPTrainer._nominal_dynamics(nominal[:, k], U[:, k], dt)
    assert out.shape == (3, 6, 6) and all(np.array_equal(out[r], nominal) for r in range(3))
