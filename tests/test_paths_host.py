"""Host-side checks of the posterior function draws; no device is touched.

1. Plumbing: the four C entries are declared, bound and exported; `draw_path_randomness` is seeded, shaped and ordered as
   documented.
2. The method, in the dense NumPy form (`paths_numpy_form` of tests/test_gpu_paths.py): with unit vectors for the weights and
   the noise draws the form's two linear maps are explicit, f = mean + A w + B z (w ~ N(0, I_F), z ~ N(0, I_N)), so the
   ensemble's mean and covariance are known in closed form: the mean must be the exact posterior mean, A A^T + B B^T must
   approach the exact posterior covariance as F grows.
3. tests/golden/make_golden_paths.py regenerates tests/golden/paths_ref.npz bit for bit."""
import ctypes
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
from scipy.linalg import cho_solve

from conftest import GOLDEN, ROOT
from test_gpu_paths import paths_numpy_form, rbf

NEW_SYMBOLS = ("gpk_rff_features", "gpk_paths_prepare", "gpk_paths_step", "gpk_paths_rollout")


def test_libgpk_exports_the_path_entries():
    from unmanned_aerial_vehicles_amd import _build, _lib
    assert os.path.exists(_build.LIB_PATH), "libgpk.so must be built in-tree (python __graft_entry__.py)"
    _lib.load()
    lib = ctypes.CDLL(_build.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "gpk.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert f"GPK_API int {name}(" in header
        assert name in _lib.SIGNATURES
    assert "gpk_paths.hip" in _build.SOURCES


def test_package_surface():
    import unmanned_aerial_vehicles_amd as pkg
    assert {"PosteriorPaths", "draw_path_randomness"} <= set(pkg.__all__)
    for name in ("from_randomness", "step", "rollout", "__call__"):
        assert callable(getattr(pkg.PosteriorPaths, name, None)), name
    assert callable(pkg.GaussianProcessRegressor.sample_paths) and callable(pkg.SimpleQuadrotorGP.sample_rollouts)
    sq = pkg.SimpleQuadrotorGP()
    out = sq.sample_rollouts(np.arange(6.0), np.ones((4, 3)), 0.1, n_rollouts=2)      # untrained: nominal, no device
    assert out.shape == (2, 6, 4) and (out[0] == out[1]).all()
    assert np.allclose(out[0][:, 1], sq._nominal_dynamics(np.arange(6.0), np.ones(4), 0.1))
    # the cached path set (device buffers) stays out of a pickle
    sq._paths = ("key", lambda: None)
    back = pickle.loads(pickle.dumps(sq))
    assert back._paths is None and back.max_data_points == sq.max_data_points


def test_draw_path_randomness():
    from unmanned_aerial_vehicles_amd import draw_path_randomness
    N, D, F, S, P = 7, 3, 5, 4, 2
    ls = np.array([0.5, 1.0, 2.0])
    a = draw_path_randomness(np.random.RandomState(11), N, D, F, S, P, ls, 0.25)
    b = draw_path_randomness(np.random.RandomState(11), N, D, F, S, P, ls, 0.25)
    assert set(a) == {"omega", "phase", "weights", "eps"}
    for k in a:
        assert a[k].dtype == np.float64 and np.array_equal(a[k], b[k]), k
    assert a["omega"].shape == (F, D) and a["phase"].shape == (F,) and a["weights"].shape == (F, S, P) and a["eps"].shape == (N, S, P)
    # the documented order: standard_normal((F, D)) / ls, uniform(0, 2 pi, F), standard_normal((F, S, P)), sqrt(.) standard_normal
    rng = np.random.RandomState(11)
    z = rng.standard_normal((F, D))
    assert np.allclose(a["omega"] * ls, z, rtol=1e-15, atol=0)
    assert np.array_equal(a["phase"], rng.uniform(0.0, 2.0 * np.pi, F)) and (a["phase"] >= 0).all() and (a["phase"] < 2 * np.pi).all()
    assert np.array_equal(a["weights"], rng.standard_normal((F, S, P)))
    assert np.array_equal(a["eps"], 0.5 * rng.standard_normal((N, S, P)))
    c = draw_path_randomness(np.random.RandomState(12), N, D, F, S, P, ls, 0.25)
    assert not np.array_equal(a["omega"], c["omega"])
    s = draw_path_randomness(np.random.RandomState(11), N, D, F, S, P, 2.0, 0.0)      # a scalar length-scale; no noise
    assert np.allclose(s["omega"] * 2.0, z, rtol=1e-15, atol=0) and not s["eps"].any()
    for bad in ((0, D, F, S, P), (N, D, 0, S, P), (N, D, F, 0, P)):
        with pytest.raises(ValueError):
            draw_path_randomness(np.random.RandomState(0), *bad, ls, 0.25)


def test_ensemble_moments_of_the_numpy_form(csv_data):
    """CSV fixture, N = 1000, D = 10, RBF(0.5) + White(0.1) and alpha = 1e-4 (train_gp's starting kernel), the first output,
    F = 4096, 25 rows of Xq10; omega and phase from draw_path_randomness(RandomState(0)).

    Measured on the CPU with this NumPy form alone: the ensemble mean differs from the exact posterior mean by 4.8e-14; the
    largest deviation of A A^T + B B^T from the exact posterior covariance (normalised-target units) is 3.78e-4, against
    posterior variances from 6.5e-3 to 4.1e-2.  Bound: twice that, 7.6e-4."""
    from unmanned_aerial_vehicles_amd import draw_path_randomness
    X, Y, Xq = csv_data["X10"], csv_data["Y6"][:, :1], csv_data["Xq10"][:25]
    N, D, F = 1000, 10, 4096
    ls, sf2, noise, alpha = np.full(D, 0.5), 1.0, 0.1, 1e-4
    s2 = noise + alpha
    r = draw_path_randomness(np.random.RandomState(0), N, D, F, 1, 1, ls, s2)
    # path 0: w = 0, eps = 0; paths 1 .. F: w = e_f; paths F + 1 .. F + N: eps = sqrt(s2) e_n
    S = 1 + F + N
    weights, eps = np.zeros((F, S, 1)), np.zeros((N, S, 1))
    weights[np.arange(F), 1 + np.arange(F), 0] = 1.0
    eps[np.arange(N), 1 + F + np.arange(N), 0] = np.sqrt(s2)
    form = paths_numpy_form(X, Y, ls, sf2, noise, alpha, r["omega"], r["phase"], weights, eps)
    f = (form.all(Xq)[:, :, 0] - form.ym[0]) / form.ys[0]         # normalised-target units
    mean, A, B = f[:, 0], f[:, 1:1 + F] - f[:, :1], f[:, 1 + F:] - f[:, :1]
    ks = rbf(Xq, X, ls, sf2)
    exact_mean = ks @ cho_solve(form.cK, form.Yn[:, 0])
    exact_cov = rbf(Xq, Xq, ls, sf2) - ks @ cho_solve(form.cK, ks.T)
    e_mean = np.max(np.abs(mean - exact_mean))
    e_cov = np.max(np.abs(A @ A.T + B @ B.T - exact_cov))
    var = np.diag(exact_cov)
    print(f"ensemble mean against the exact posterior mean: {e_mean:.2e} (bar 1e-10)")
    print(f"A A^T + B B^T against the exact posterior covariance: {e_cov:.3e} (bound 7.6e-04); variances {var.min():.2e} .. {var.max():.2e}")
    assert e_mean < 1e-10
    assert e_cov < 7.6e-4
    # the explicit maps are the documented ones: A = phi(x)^T - k_* K^-1 Phi, B = -sqrt(noise + alpha) k_* K^-1
    kik = cho_solve(form.cK, ks.T).T
    assert np.max(np.abs(A - (form.scale * np.cos(Xq @ r["omega"].T + r["phase"]) - kik @ form.Phi))) < 1e-12
    assert np.max(np.abs(B + np.sqrt(s2) * kik)) < 1e-12


def test_fixture_script_reproduces_the_file(tmp_path):
    committed = os.path.join(GOLDEN, "paths_ref.npz")
    # the script writes next to itself: run a copy from a directory that holds its input
    for name in ("make_golden_paths.py", "csv_170501.npz"):
        with open(os.path.join(GOLDEN, name), "rb") as src, open(tmp_path / name, "wb") as dst:
            dst.write(src.read())
    r = subprocess.run([sys.executable, str(tmp_path / "make_golden_paths.py")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True)
    assert r.returncode == 0, r.stdout
    print(r.stdout)
    with open(committed, "rb") as a, open(tmp_path / "paths_ref.npz", "rb") as b:
        assert a.read() == b.read(), "make_golden_paths.py no longer reproduces tests/golden/paths_ref.npz"


def test_fixture_holds_what_the_tests_read():
    d = np.load(os.path.join(GOLDEN, "paths_ref.npz"))
    for name, (N, D, F, S, P, H) in (("a", (120, 4, 48, 5, 1, 6)), ("b", (130, 4, 64, 70, 3, 5)), ("csv", (200, 10, 96, 7, 6, 25)),
                                     ("one", (128, 3, 16, 1, 2, 4))):
        g = lambda k: d[f"{name}_{k}"]      # noqa: E731
        assert g("X").shape == (N, D) and g("Y").shape == (N, P) and g("Xq").shape == (9, D) and g("ls").shape == (D,)
        assert g("omega").shape == (F, D) and g("phase").shape == (F,) and g("weights").shape == (F, S, P)
        assert g("eps").shape == (N, S, P) and g("Xs").shape == (S, D) and g("x0").shape == (S, P)
        assert g("U").shape == (H, D - P) and g("lin").shape == (P, D)
        assert g("all").shape == (9, S, P) and g("step").shape == (S, P) and g("traj").shape == (H + 1, S, P)
        assert all(np.isfinite(d[k]).all() for k in d.files if k.startswith(name + "_"))
        sf2, noise, alpha = g("hyper")
        form = paths_numpy_form(g("X"), g("Y"), g("ls"), sf2, noise, alpha, g("omega"), g("phase"), g("weights"), g("eps"))
        for what, mine in (("all", form.all(g("Xq"))), ("step", form.step(g("Xs"))), ("traj", form.rollout(g("x0"), g("U"), g("lin")))):
            assert np.max(np.abs(mine - g(what))) < 1e-11 * np.max(np.abs(g(what))), (name, what)
