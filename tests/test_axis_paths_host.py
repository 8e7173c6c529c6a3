"""Host-side checks of the posterior function draws of the per-axis batch ("the per-axis batch"); no device is
touched.

1. Plumbing: the two C entries are declared, bound and exported; the package surface; `draw_batch_path_randomness` is seeded,
   shaped and ordered as documented.
2. The dense NumPy batch form (`axis_paths_numpy_form` of tests/test_gpu_axis_paths.py) with one model and identity scalers is
   `paths_numpy_form` of tests/test_gpu_paths.py.
3. tests/golden/make_golden_axis_paths.py regenerates tests/golden/axis_paths_ref.npz bit for bit, and the file holds what the
   GPU tests read.
4. Error growth: on every rollout case a 1e-12 relative perturbation of x0 grows by less than 100x over the horizon in the NumPy
   form, so a kernel-value difference of 1e-12 stays two orders under the 1e-8 bar of the GPU tests; on the two generated
   problems without controls (three stages) by less than 1e3 - measured: at most 7.3x."""
import ctypes
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_gpu_axis_paths import (CASE_NAMES, NO_CONTROLS_KINDS, ROLLOUT_CASES, axis_paths_numpy_form, load_case,
                                 no_controls_problem)
from test_gpu_paths import paths_numpy_form

NEW_SYMBOLS = ("gpk_paths_step_multi", "gpk_paths_rollout_multi")
SHAPES = {"a": (120, 4, 48, 5, 2, 3, 6), "b": (130, 4, 64, 70, 3, 3, 5), "csv": (200, 10, 96, 7, 6, 6, 25),
          "gap": (96, 10, 32, 9, 4, 6, 5), "one": (128, 3, 16, 1, 1, 2, 4), "eight": (64, 2, 16, 65, 8, 0, 0)}


def test_libgpk_exports_the_batch_path_entries():
    from unmanned_aerial_vehicles_amd import _build, _lib
    assert os.path.exists(_build.LIB_PATH), "libgpk.so must be built in-tree (python __graft_entry__.py)"
    _lib.load()
    lib = ctypes.CDLL(_build.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "gpk.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert f"GPK_API int {name}(" in header
        assert name in _lib.SIGNATURES


def test_package_surface():
    import unmanned_aerial_vehicles_amd as pkg
    assert {"BatchedPosteriorPaths", "draw_batch_path_randomness"} <= set(pkg.__all__)
    for name in ("from_randomness", "step", "rollout", "__call__", "set_output_scaler"):
        assert callable(getattr(pkg.BatchedPosteriorPaths, name, None)), name
    assert callable(pkg.BatchedARDGP.sample_paths) and callable(pkg.PreTrainedGP.sample_rollouts)
    with pytest.raises(TypeError):
        pkg.BatchedPosteriorPaths()
    with pytest.raises(RuntimeError, match="not fitted"):
        pkg.BatchedARDGP(optimizer=None).sample_paths(4)


def test_pretrained_gp_falls_back_to_the_nominal_trajectory(capsys):
    from unmanned_aerial_vehicles_amd import GPTrainer, PreTrainedGP
    pg = PreTrainedGP("/nonexistent/model.pkl")
    capsys.readouterr()
    out = pg.sample_rollouts(np.arange(6.0), np.ones((4, 3)), 0.1, n_rollouts=2)      # nothing loaded: nominal, no device
    assert "GP rollout sampling failed: no models are loaded" in capsys.readouterr().out
    assert out.shape == (2, 6, 4) and (out[0] == out[1]).all() and (out[0][:, 0] == np.arange(6.0)).all()
    assert np.array_equal(out[0][:, 1], GPTrainer._nominal_dynamics(np.arange(6.0), np.ones(4), 0.1))
    assert np.array_equal(out[0][:, 3], GPTrainer._nominal_dynamics(out[0][:, 2], np.ones(4), 0.1))
    # the cached path set (device buffers) stays out of a pickle, and a new model file drops it
    pg._axis_paths = ("key", lambda: None)
    back = pickle.loads(pickle.dumps(pg))
    assert back._axis_paths is None and back.model_path == pg.model_path and back.is_loaded is False
    pg._axis_paths = ("key", None)
    assert pg.load_dict({"gp_models": {}, "scalers_X": {}, "scalers_y": {}}) and pg._axis_paths is None


def test_draw_batch_path_randomness():
    from unmanned_aerial_vehicles_amd import draw_batch_path_randomness, draw_path_randomness
    N, D, F, S, B = 7, 3, 5, 4, 3
    ls = np.array([[0.5, 1.0, 2.0], [1.5, 0.7, 0.9], [3.0, 2.0, 1.0]])
    s2 = np.array([0.25, 0.01, 1.0])
    a = draw_batch_path_randomness(np.random.RandomState(11), N, D, F, S, ls, s2)
    b = draw_batch_path_randomness(np.random.RandomState(11), N, D, F, S, ls, s2)
    assert set(a) == {"omega", "phase", "weights", "eps"}
    for k in a:
        assert a[k].dtype == np.float64 and np.array_equal(a[k], b[k]), k
    assert a["omega"].shape == (B, F, D) and a["phase"].shape == (B, F) and a["weights"].shape == (B, F, S) and a["eps"].shape == (B, N, S)
    # the documented order: model by model from the one generator, each the single-model draw with P = 1
    rng = np.random.RandomState(11)
    for m in range(B):
        r = draw_path_randomness(rng, N, D, F, S, 1, ls[m], s2[m])
        assert np.array_equal(a["omega"][m], r["omega"]) and np.array_equal(a["phase"][m], r["phase"])
        assert np.array_equal(a["weights"][m], r["weights"][:, :, 0]) and np.array_equal(a["eps"][m], r["eps"][:, :, 0])
    rng = np.random.RandomState(11)
    z = rng.standard_normal((F, D))
    assert np.allclose(a["omega"][0] * ls[0], z, rtol=1e-15, atol=0)
    assert np.array_equal(a["phase"][0], rng.uniform(0.0, 2.0 * np.pi, F))
    assert np.array_equal(a["weights"][0], rng.standard_normal((F, S, 1))[:, :, 0])
    assert np.array_equal(a["eps"][0], 0.5 * rng.standard_normal((N, S, 1))[:, :, 0])
    assert not np.array_equal(a["omega"], draw_batch_path_randomness(np.random.RandomState(12), N, D, F, S, ls, s2)["omega"])
    # one model: the single-model draw
    one = draw_batch_path_randomness(np.random.RandomState(5), N, D, F, S, ls[:1], s2[:1])
    r = draw_path_randomness(np.random.RandomState(5), N, D, F, S, 1, ls[0], s2[0])
    for k in ("omega", "phase"):
        assert np.array_equal(one[k][0], r[k]), k
    for k in ("weights", "eps"):
        assert np.array_equal(one[k][0], r[k][:, :, 0]), k
    for bad in ((ls[:, :2], s2), (ls, s2[:2]), (np.ones((9, D)), np.ones(9)), (ls, -s2)):
        with pytest.raises(ValueError):
            draw_batch_path_randomness(np.random.RandomState(0), N, D, F, S, *bad)
    with pytest.raises(ValueError):
        draw_batch_path_randomness(np.random.RandomState(0), N, D, 0, S, ls, s2)


def test_one_model_and_identity_scalers_is_the_single_model_form():
    rng = np.random.RandomState(21)
    N, D, F, S, H = 40, 3, 12, 4, 5
    X, Y = rng.standard_normal((N, D)), rng.standard_normal((N, 1)) + 2.0
    ls, sf2, noise, alpha = np.array([1.0, 1.5, 0.8]), 0.9, 0.1, 1e-4
    omega, phase = rng.standard_normal((F, D)) / ls, rng.uniform(0, 2 * np.pi, F)
    weights, eps = rng.standard_normal((F, S, 1)), 0.3 * rng.standard_normal((N, S, 1))
    single = paths_numpy_form(X, Y, ls, sf2, noise, alpha, omega, phase, weights, eps)
    batch = axis_paths_numpy_form(X, Y, ls[None], np.array([[sf2, noise, alpha]]), omega[None], phase[None], weights[None, :, :, 0],
                                  eps[None, :, :, 0])
    Q, Qs = rng.standard_normal((6, D)), rng.standard_normal((S, D))
    assert np.array_equal(batch.all(Q), single.all(Q).transpose(0, 2, 1))
    assert np.array_equal(batch.step(Qs), single.step(Qs))
    x0, U, lin = 0.5 * rng.standard_normal((S, 1)), 0.5 * rng.standard_normal((H, D - 1)), 0.1 * rng.standard_normal((1, D))
    assert np.array_equal(batch.rollout(x0, U, lin), single.rollout(x0, U, lin))
    assert np.array_equal(batch.rollout(x0, U, lin, coord=[0], in_scaler=(np.zeros(D), np.ones(D))), single.rollout(x0, U, lin))


def test_fixture_script_reproduces_the_file(tmp_path):
    committed = os.path.join(GOLDEN, "axis_paths_ref.npz")
    # the script writes next to itself: run a copy from a directory that holds its input
    for name in ("make_golden_axis_paths.py", "csv_170501.npz"):
        with open(os.path.join(GOLDEN, name), "rb") as src, open(tmp_path / name, "wb") as dst:
            dst.write(src.read())
    r = subprocess.run([sys.executable, str(tmp_path / "make_golden_axis_paths.py")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True)
    assert r.returncode == 0, r.stdout
    print(r.stdout)
    with open(committed, "rb") as a, open(tmp_path / "axis_paths_ref.npz", "rb") as b:
        assert a.read() == b.read(), "make_golden_axis_paths.py no longer reproduces tests/golden/axis_paths_ref.npz"
    assert os.path.getsize(committed) < (1 << 20)


def test_fixture_holds_what_the_tests_read():
    assert tuple(SHAPES) == CASE_NAMES
    for name, (N, D, F, S, B, nx, H) in SHAPES.items():
        c = load_case(name)
        assert c["X"].shape == (N, D) and c["Y"].shape == (N, B) and c["Xq"].shape == (9, D) and c["ls"].shape == (B, D)
        assert c["hyper"].shape == (B, 3) and c["omega"].shape == (B, F, D) and c["phase"].shape == (B, F)
        assert c["weights"].shape == (B, F, S) and c["eps"].shape == (B, N, S) and c["Xs"].shape == (S, D) and c["out"].shape == (2, B)
        assert c["all"].shape == (9, B, S) and c["step"].shape == (S, B)
        assert all(np.isfinite(v).all() for v in c.values())
        # distinct per model: length-scales, signal variance, noise
        for b in range(1, B):
            assert not np.array_equal(c["ls"][b], c["ls"][0]) and (c["hyper"][b, :2] != c["hyper"][0, :2]).all()
        form = axis_paths_numpy_form(c["X"], c["Y"], c["ls"], c["hyper"], c["omega"], c["phase"], c["weights"], c["eps"], c["out"])
        pairs = [("all", form.all(c["Xq"])), ("step", form.step(c["Xs"]))]
        assert (name in ROLLOUT_CASES) == ("traj" in c)
        if name in ROLLOUT_CASES:
            assert c["x0"].shape == (S, nx) and c["U"].shape == (H, D - nx) and c["lin"].shape == (nx, D)
            assert c["coord"].shape == (B,) and c["in"].shape == (2, D) and c["traj"].shape == (H + 1, S, nx)
            assert len(set(c["coord"].tolist())) == B and c["coord"].min() >= 0 and c["coord"].max() < nx
            pairs.append(("traj", form.rollout(c["x0"], c["U"], c["lin"], c["coord"], (c["in"][0], c["in"][1]))))
        for what, mine in pairs:
            assert np.max(np.abs(mine - c[what])) < 1e-11 * np.max(np.abs(c[what])), (name, what)
    assert tuple(load_case("gap")["coord"]) == (0, 2, 3, 5)
    assert not np.array_equal(load_case("csv")["in"][1], np.ones(10)) and not np.array_equal(load_case("csv")["out"][1], np.ones(6))


@pytest.mark.parametrize("name", ROLLOUT_CASES)
def test_rollout_error_growth_leaves_room(name):
    c = load_case(name)
    form = axis_paths_numpy_form(c["X"], c["Y"], c["ls"], c["hyper"], c["omega"], c["phase"], c["weights"], c["eps"], c["out"])
    sc = (c["in"][0], c["in"][1])
    base = form.rollout(c["x0"], c["U"], c["lin"], c["coord"], sc)
    pert = form.rollout(c["x0"] * (1.0 + 1e-12), c["U"], c["lin"], c["coord"], sc)
    growth = np.max(np.abs(pert[-1] - base[-1])) / np.max(np.abs(pert[0] - base[0]))
    print(f"case {name}, NumPy form: a 1e-12 relative perturbation of x0 grows {growth:.2f}x over {len(c['U'])} stages")
    assert growth < 100.0       # (two orders under what would bring a 1e-12 kernel-value difference near the 1e-8 bar)


@pytest.mark.parametrize("kind", NO_CONTROLS_KINDS)
def test_rollout_without_controls_error_growth_leaves_room(kind):
    """The problem of test_rollout_without_controls (tests/test_gpu_axis_paths.py): three stages, no controls."""
    p, form = no_controls_problem(kind)
    for tag, x0 in (("S rows", p["x0"]), ("one row", p["x0"][0])):
        base = form.rollout(x0, p["U"], p["lin"])
        pert = form.rollout(x0 * (1.0 + 1e-12), p["U"], p["lin"])
        growth = np.max(np.abs(pert[-1] - base[-1])) / np.max(np.abs(pert[0] - base[0]))
        print(f"{kind}, no controls, x0 as {tag}, NumPy form: a 1e-12 relative perturbation of x0 grows {growth:.2f}x over 3 stages")
        assert growth < 1e3     # (a 1e-12 kernel-value difference then stays an order under the 1e-8 bar)
