"""tests/golden/sparse_select_ref.npz (greedy conditional-variance selection of inducing inputs, written by
tests/golden/make_golden_sparse_select.py): the fixture regenerates, its cases are tie-free by the margin that makes an exact
index comparison legitimate, the recursion's trace agrees with the dense form tr(Kff - Kfu Kuu^-1 Kuf), `follow` along the
selection's own indices reproduces it, and the host side of the feature: the new C entries in the binding and the header, and the
argument checks that need no GPU.  NumPy / SciPy only."""
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

CASES = {"A": (600, 2, 64), "B": (1500, 3, 130), "C": (2100, 4, 200)}
GAP_GATE = 1e-8        # of sf2: largest minus second-largest d at every step after the first
DENSE_BAR = 1e-9       # of n sf2: the recursion's trace against the dense form


def load_select_writer():
    spec = importlib.util.spec_from_file_location("make_golden_sparse_select", os.path.join(GOLDEN, "make_golden_sparse_select.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def sref():
    d = np.load(os.path.join(GOLDEN, "sparse_select_ref.npz"))
    return {k: d[k] for k in d.files}


@pytest.fixture(scope="module")
def w():
    return load_select_writer()


def test_fixture_regenerates(sref, w):
    again = w.build()
    assert set(again) == set(sref)
    for k in sref:
        assert np.array_equal(np.asarray(again[k]), sref[k]), f"{k} differs from what the writer produces"
    assert w.CASES == {"A": (600, 2, 64, 0.0, 0.6), "B": (1500, 3, 130, 0.2, 0.8), "C": (2100, 4, 200, 0.4, 1.0)}
    assert float(sref["sf2"]) == 1.7 and w.GAP_GATE == GAP_GATE


@pytest.mark.parametrize("case", sorted(CASES))
def test_cases_are_tie_free_and_sound(sref, w, case):
    n, D, m = CASES[case]
    sf2 = float(sref["sf2"])
    X, ls, idx, trace, dmax = (sref[f"{case}_{k}"] for k in ("X", "ls", "idx", "trace", "dmax"))
    assert X.shape == (n, D) and ls.shape == (D,) and idx.shape == trace.shape == dmax.shape == (m,)
    assert idx.dtype == np.int64 and len(set(idx.tolist())) == m and idx.min() >= 0 and idx.max() < n
    assert idx[0] == 0 and dmax[0] == sf2, "every d equals sf2 at the first step: the lowest index wins"
    gap = float(sref[f"{case}_min_gap"])
    print(f"case {case}: smallest gap {gap / sf2:.2e} sf2")
    assert gap >= GAP_GATE * sf2
    assert np.all(np.diff(dmax) <= 0.0) and np.all(np.diff(trace) < 0.0) and trace[-1] > 0.0
    # the dense form, at the last step and at a few earlier ones
    for t in sorted({0, 1, m // 3, m - 1}):
        dense = w.dense_trace(X, ls, sf2, idx[:t + 1])
        assert abs(dense - trace[t]) <= DENSE_BAR * n * sf2, (t, dense, trace[t])
    # the recursion along its own indices reproduces it, and at every step the index taken is the first of the largest d
    d_before, tr = w.follow(X, ls, sf2, idx)
    assert np.array_equal(tr, trace)
    assert np.array_equal(d_before.argmax(axis=1), idx) and np.array_equal(d_before.max(axis=1), dmax)
    # the gaps, recomputed
    top = np.sort(d_before[1:], axis=1)[:, -2:]
    assert float(np.min(top[:, 1] - top[:, 0])) == gap


def test_stops(sref, w):
    X, ls, sf2 = sref["A_X"], sref["A_ls"], float(sref["sf2"])
    n = len(X)
    # tol between trace[19] and trace[20]: 21 rows; min_var between dmax[10] and dmax[11]: 11 rows; one row
    tol = float(np.sqrt(sref["A_trace"][19] * sref["A_trace"][20])) / (n * sf2)
    idx, trace, dmax = w.greedy_select(X, ls, sf2, 64, tol=tol)
    assert len(idx) == 21 and np.array_equal(idx, sref["A_idx"][:21]) and np.array_equal(trace, sref["A_trace"][:21])
    mv = float(np.sqrt(sref["A_dmax"][10] * sref["A_dmax"][11])) / sf2
    idx, trace, dmax = w.greedy_select(X, ls, sf2, 64, min_var=mv)
    assert len(idx) == 11 and np.array_equal(dmax, sref["A_dmax"][:11])
    idx, trace, dmax = w.greedy_select(X, ls, sf2, 1)
    assert idx.tolist() == [0] and dmax.tolist() == [sf2]
    # identical rows: one row explains everything
    idx, trace, dmax = w.greedy_select(np.tile(X[:1], (50, 1)), ls, sf2, 10)
    assert idx.tolist() == [0] and trace[0] <= 1e-10 * 50 * sf2


def test_reselect_then_train_raises_the_bound_on_the_training_case():
    """What tests/test_gpu_sparse_select.py asks of `train(select_inducing="greedy", selection_rounds=2)` on the training case of
    sparse_train_ref.npz holds for the NumPy recursion: every round finds all 64 rows, and the bound after the two rounds is above
    the bound of the model the case starts from (its random Z at the start kernel)."""
    from scipy.optimize import minimize
    from test_sparse_train_host import load_writer
    w, T = load_select_writer(), load_writer()
    t = np.load(os.path.join(GOLDEN, "sparse_train_ref.npz"))
    X, Yn = t["T_X"], (t["T_Y"] - t["T_y_mean"]) / t["T_y_std"]
    jitter, jit = t["T_hyper"]
    theta = np.log(t["T_start"])           # [sf2, ls_0, ls_1, noise]
    lo, hi = np.log(1e-5), np.log(1e5)
    start = float(t["T_bound_start"])
    for rnd in range(2):
        e = np.exp(theta)
        idx, _, _ = w.greedy_select(X, e[1:3], e[0], 64)
        assert len(idx) == 64, f"round {rnd}: only {len(idx)} usable rows"
        Z = X[idx]

        def obj(th):
            e = np.exp(th)
            try:
                b = T.bound_value(X, Yn, Z, e[1:3], e[0], e[3], jitter, jit)
                g, _, _ = T.grad_assembly(X, Yn, Z, e[1:3], e[0], e[3], jitter, jit)
            except np.linalg.LinAlgError:
                return np.inf, np.zeros_like(th)
            return -b, -np.array([g[3], g[0], g[1], g[2]])

        res = minimize(obj, theta, method="L-BFGS-B", jac=True, bounds=[(lo, hi)] * 4)
        theta = res.x
        print(f"round {rnd}: bound {-res.fun:.6f} in {res.nfev} evaluations (start {start:.6f})")
    assert -res.fun > start


def test_new_entries_in_binding_and_header():
    from unmanned_aerial_vehicles_amd import _lib
    new = {"gpk_greedy_select_bytes", "gpk_greedy_select", "gpk_sparse_select"}
    assert new <= set(_lib.SIGNATURES)
    header = open(os.path.join(ROOT, "include", "gpk.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(gpk_[a-z0-9_]+)\s*\(", code))
    assert new <= declared and declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    assert len(_lib.SIGNATURES["gpk_greedy_select"][1]) == 15 and len(_lib.SIGNATURES["gpk_sparse_select"][1]) == 10
    for name in new:     # documented in the header's style
        assert re.search(name + r":", header), f"{name} has no entry in the header's comments"
    assert "gpk_select.hip" in __import__("unmanned_aerial_vehicles_amd._build", fromlist=["SOURCES"]).SOURCES


def test_python_surface_and_argument_checks():
    """None of these touches a GPU: the checks come first."""
    from unmanned_aerial_vehicles_amd import RBF, SparseGP, WhiteKernel
    p = inspect.signature(SparseGP.from_exact).parameters
    assert p["selection"].default == "random"
    p = inspect.signature(SparseGP.train).parameters
    assert p["select_inducing"].default is None and p["selection_rounds"].default == 1
    p = inspect.signature(SparseGP.select_inducing).parameters
    assert [p[k].default for k in ("X", "m", "tol", "min_var")] == [None, None, 0.0, 1e-10]

    class Fitted:       # what from_exact reads of a fitted regressor
        X_train_ = np.arange(12.0).reshape(6, 2)
        kernel_ = RBF(1.0) + WhiteKernel(0.1)
        alpha, _y_train_mean, _y_train_std, device = 1e-10, np.zeros(1), np.ones(1), None

    with pytest.raises(ValueError, match="selection"):
        SparseGP.from_exact(Fitted(), inducing=3, selection="nope")
    with pytest.raises(ValueError, match="inducing must be"):
        SparseGP.from_exact(Fitted(), inducing=7, selection="greedy")
    # the default is the seeded permutation, as before
    gp = SparseGP.from_exact(Fitted(), inducing=3)
    assert np.array_equal(gp.inducing_, Fitted.X_train_[np.sort(np.random.default_rng(0).permutation(6)[:3])])
    with pytest.raises(ValueError, match="select_inducing"):
        gp.train(Fitted.X_train_, np.zeros(6), select_inducing="nope")
    with pytest.raises(ValueError, match="selection_rounds"):
        gp.train(Fitted.X_train_, np.zeros(6), select_inducing="greedy", selection_rounds=0)
    with pytest.raises(RuntimeError, match="held rows"):
        gp.select_inducing()
    with pytest.raises(ValueError, match=r"X must be \(n, 2\)"):
        gp.select_inducing(np.zeros((5, 3)))
    with pytest.raises(ValueError, match="NaN or infinity"):
        gp.select_inducing(np.full((5, 2), np.nan))
