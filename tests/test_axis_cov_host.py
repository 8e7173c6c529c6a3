"""CPU checks of the joint posterior of the per-axis GP batch: the built library exports its two C entries with the declared
arities, the fixture (tests/golden/axis_cov_ref.npz, tests/golden/make_golden_axis_cov.py) has the stated shapes, regenerates bit
for bit where scikit-learn is importable and records a closed form that agrees with scikit-learn's return_cov, the Cholesky-draw
helper reproduces the stored draws and handles every kind of random_state and a covariance that does not factorise, and an
unloaded PreTrainedGP serves the fallbacks without a GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

ARITY = {"gpk_predict_host_multi_cov": 18, "gpk_predict_batched_cov": 5}
DRAW_BAR = 1e-12         # the same NumPy on both sides: the helper is the fixture script's formula


@pytest.fixture(scope="module")
def cov_ref():
    d = np.load(os.path.join(GOLDEN, "axis_cov_ref.npz"))
    return {k: d[k] for k in d.files}


def test_libgpk_exports_the_per_axis_covariance_entries():
    from unmanned_aerial_vehicles_amd import _build, _lib
    assert os.path.exists(_build.LIB_PATH), "libgpk.so must be built in-tree (python __graft_entry__.py)"
    _lib.load()
    lib = ctypes.CDLL(_build.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "gpk.h")).read()
    for name, arity in ARITY.items():
        assert hasattr(lib, name), name
        m = re.search(r"GPK_API int " + name + r"\(([^;]*)\);", header)
        assert m, name
        assert len(m.group(1).split(",")) == arity, (name, m.group(1))
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == arity


def test_surfaces_exist():
    from unmanned_aerial_vehicles_amd.batched import BatchedARDGP
    from unmanned_aerial_vehicles_amd.trainer import PreTrainedGP
    for cls, names in ((BatchedARDGP, ("predict_host_cov", "sample_y")),
                       (PreTrainedGP, ("predict_residual_cov_batch", "sample_residuals"))):
        for n in names:
            assert callable(getattr(cls, n, None)), n


def test_fixture_shapes_and_its_own_error(cov_ref):
    r = cov_ref
    for case in ("ref", "csv"):
        assert r[f"{case}_Xq"].shape == (25, 10) and r[f"{case}_mean"].shape == (25, 6)
        assert r[f"{case}_cov"].shape == (25, 25, 6) and r[f"{case}_draws"].shape == (25, 6, 8)
        assert r[f"{case}_draw_shift"].shape == (6,) and r[f"{case}_draw_shift"].max() < 1e-10
    assert r["csv_Xq72"].shape == (72, 10) and r["csv_mean72"].shape == (72, 6) and r["csv_cov72"].shape == (72, 72, 6)
    assert r["csv_ls"].shape == (6, 10) and r["csv_noise"].shape == (6,)
    assert r["csv_sx_mean"].shape == (10,) and r["csv_sx_scale"].shape == (10,)
    assert r["csv_sy_mean"].shape == (6,) and r["csv_sy_scale"].shape == (6,)
    # the 25 rows are the first 17 and the last 8 of the 72
    assert np.array_equal(r["csv_Xq"], np.vstack([r["csv_Xq72"][:17], r["csv_Xq72"][64:]]))
    # the closed form that case `ref` uses, against scikit-learn's own return_cov on case `csv`
    print("closed form vs scikit-learn:", r["csv_closed_vs_sk"])
    assert r["csv_closed_vs_sk"].shape == (6,) and r["csv_closed_vs_sk"].max() < 1e-10


def test_make_golden_axis_cov_regenerates_fixture(tmp_path, cov_ref):
    pytest.importorskip("sklearn")
    out = str(tmp_path / "axis_cov_ref.npz")
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_axis_cov.py"), out], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    new = np.load(out)
    assert sorted(new.files) == sorted(cov_ref)
    for k in cov_ref:
        assert np.array_equal(new[k], cov_ref[k]), k


def test_cholesky_draws_reproduce_the_stored_draws(cov_ref):
    from unmanned_aerial_vehicles_amd.gpr import cholesky_draws
    for case in ("ref", "csv"):
        mean, cov, want = cov_ref[f"{case}_mean"], cov_ref[f"{case}_cov"], cov_ref[f"{case}_draws"]
        got = cholesky_draws(mean, cov, n_samples=8, random_state=0)
        e = np.max(np.abs(got - want)) / np.max(np.abs(want))
        print(case, e)
        assert got.shape == (25, 6, 8) and e < DRAW_BAR
        # a model's draw does not depend on which others are active; inactive ones are zeros
        act = np.array([True, False, True, True, False, True])
        part = cholesky_draws(mean, cov, n_samples=8, random_state=0, active=act)
        assert np.array_equal(part[:, act], got[:, act]) and not part[:, ~act].any()


def test_cholesky_draws_random_state(cov_ref):
    from unmanned_aerial_vehicles_amd.gpr import cholesky_draws
    mean, cov = cov_ref["ref_mean"], cov_ref["ref_cov"]
    a = cholesky_draws(mean, cov, 3, 7)
    assert np.array_equal(a, cholesky_draws(mean, cov, 3, np.int64(7)))
    rs = np.random.RandomState(7)
    b = cholesky_draws(mean, cov, 3, rs)
    c = cholesky_draws(mean, cov, 3, rs)                  # the instance's stream advances
    assert np.array_equal(a, b) and not np.array_equal(b, c)
    z = np.random.RandomState(7).standard_normal((2, 6, 25, 3))
    assert np.array_equal(c[:, 0, :], mean[:, 0, None] + np.linalg.cholesky(cov[..., 0]) @ z[1, 0])
    np.random.seed(7)                                     # None: NumPy's global stream
    assert np.array_equal(cholesky_draws(mean, cov, 3, None), a)
    assert cholesky_draws(mean, cov).shape == (25, 6, 1)


def test_cholesky_draws_retry_and_second_failure():
    from unmanned_aerial_vehicles_amd.gpr import cholesky_draws
    singular = np.ones((3, 3))                            # rank one: the second pivot is exactly zero
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(singular)
    mean = np.arange(3.0).reshape(3, 1)
    got = cholesky_draws(mean, singular[:, :, None], 4, 0)
    z = np.random.RandomState(0).standard_normal((1, 3, 4))
    L = np.linalg.cholesky(singular + 1e-10 * np.eye(3))
    assert np.isfinite(got).all() and np.array_equal(got[:, 0, :], mean + L @ z[0])
    indefinite = np.array([[1.0, 2.0], [2.0, 1.0]])       # eigenvalue -1: the shifted matrix fails as well
    with pytest.raises(np.linalg.LinAlgError):
        cholesky_draws(np.zeros((2, 1)), indefinite[:, :, None], 1, 0)


def test_not_loaded_returns_the_fallbacks(tmp_path):
    from unmanned_aerial_vehicles_amd.trainer import PreTrainedGP
    g = PreTrainedGP(str(tmp_path / "no_such_model.pkl"))
    assert not g.is_loaded
    X = np.random.default_rng(1).standard_normal((7, 10))
    mean, cov = g.predict_residual_cov_batch(X)
    assert mean.shape == (7, 6) and cov.shape == (7, 7, 6) and not mean.any()
    for i in range(6):
        assert np.array_equal(cov[..., i], 1e12 * np.eye(7))
    s = g.sample_residuals(X, n_samples=5, random_state=3)
    assert s.shape == (7, 6, 5) and not s.any()
    assert g.sample_residuals(X).shape == (7, 6, 1)
    # a malformed batch: never raises
    mean, cov = g.predict_residual_cov_batch(np.zeros((4, 7)))
    assert mean.shape == (4, 6) and cov.shape == (4, 4, 6)
    assert g.sample_residuals(np.zeros((4, 7)), 2).shape == (4, 6, 2)


# ---- PreTrainedGP's three batch surfaces and the draws, route by route, on fakes with closed forms ------------------------------
# Model k (its place in OUTPUT_NAMES) on scaled rows Z = (X - 0.5) / 2; the fused object answers differently from the models
# (mean + 100, std + 1, Jacobians x 3, covariance x 2), so every expected array says which route filled it.
def _own(k, Z):
    M = len(Z)
    mu, s = (k + 1) * Z.sum(axis=1), 0.25 * (k + 1) + np.abs(Z[:, 0])
    return {"mu": mu, "s": s, "dmu": (k + 1) * np.tile(np.arange(1.0, 11.0), (M, 1)), "var": s ** 2,
            "dvar": s[:, None] * np.arange(1.0, 11.0) / 10.0, "cov": (k + 1) * (np.eye(M) + 0.5 * np.outer(Z[:, 0], Z[:, 0]))}


def _via_fused(k, Z):
    o = _own(k, Z)
    return {"mu": o["mu"] + 100.0, "s": o["s"] + 1.0, "dmu": 3.0 * o["dmu"], "var": (o["s"] + 1.0) ** 2, "dvar": 3.0 * o["dvar"],
            "cov": 2.0 * o["cov"]}


class _FakeModel:
    def __init__(self, k):
        self.k, self.fail = k, False

    def _o(self, Z):
        if self.fail:
            raise RuntimeError(f"model {self.k} down")
        return _own(self.k, np.asarray(Z, dtype=np.float64))

    def predict(self, Z, return_std=False, return_cov=False):
        o = self._o(Z)
        return (o["mu"], o["cov"]) if return_cov else (o["mu"], o["s"]) if return_std else o["mu"]

    def predict_jacobian(self, Z, return_var=False):
        o = self._o(Z)
        return (o["mu"], o["dmu"], o["var"], o["dvar"]) if return_var else (o["mu"], o["dmu"])


class _FakeFused:
    def __init__(self, ks):
        self.ks, self.fail = ks, False

    def _o(self, Z, key, axis=1):
        if self.fail:
            raise RuntimeError("fused down")
        return np.stack([_via_fused(k, np.asarray(Z, dtype=np.float64))[key] for k in self.ks], axis=axis)

    def predict(self, Z, return_std=False, return_cov=False):
        if return_cov:
            return self._o(Z, "mu"), self._o(Z, "cov", 2)
        return (self._o(Z, "mu"), self._o(Z, "s")) if return_std else self._o(Z, "mu")

    def predict_jacobian(self, Z, return_var=False):
        out = (self._o(Z, "mu"), self._o(Z, "dmu"))
        return out + (self._o(Z, "var"), self._o(Z, "dvar")) if return_var else out


def _expected(X, routes):
    """What the four surfaces return when component i is filled by routes[i]: "fused", "own" or None (the fallbacks)."""
    M = len(X)
    Z = (X - 0.5) / 2.0 if X.shape[1] == 10 else None
    e = {"mean": np.zeros((M, 6)), "std": np.full((M, 6), 1e6), "J": np.zeros((M, 6, 10)), "dstd": np.zeros((M, 6, 10)),
         "jmean": np.zeros((M, 6)), "jstd": np.full((M, 6), 1e6), "cmean": np.zeros((M, 6)),
         "cov": np.repeat((1e12 * np.eye(M))[:, :, None], 6, axis=2), "draws": np.zeros((M, 6, 2))}
    z = np.random.RandomState(0).standard_normal((6, M, 2))
    for i, r in enumerate(routes):
        if r is None:
            continue
        o = (_via_fused if r == "fused" else _own)(i, Z)
        e["mean"][:, i] = e["jmean"][:, i] = e["cmean"][:, i] = 2.0 * o["mu"] + 0.5
        e["std"][:, i] = 2.0 * o["s"]
        sig = np.sqrt(o["var"])
        e["J"][:, i], e["jstd"][:, i] = 2.0 * o["dmu"] / 2.0, 2.0 * sig
        e["dstd"][:, i] = 2.0 * (o["dvar"] / (2.0 * sig[:, None])) / 2.0
        e["cov"][:, :, i] = 4.0 * o["cov"]
        e["draws"][:, i, :] = e["cmean"][:, i, None] + np.linalg.cholesky(e["cov"][:, :, i]) @ z[i]
    return e


def _fake_pretrained(tmp_path, present=range(6)):
    from unmanned_aerial_vehicles_amd.trainer import OUTPUT_NAMES, PreTrainedGP, StandardScaler
    g = PreTrainedGP(str(tmp_path / "no_such_model.pkl"))
    for k in present:
        n = OUTPUT_NAMES[k]
        g.gp_models[n] = _FakeModel(k)
        sx, sy = StandardScaler(), StandardScaler()
        sx.mean_, sx.scale_ = np.full(10, 0.5), np.full(10, 2.0)
        sy.mean_, sy.scale_ = np.full(1, 0.5), np.full(1, 2.0)
        g.scalers_X[n], g.scalers_y[n] = sx, sy
    g.is_loaded = True
    g._fused_bg = (_FakeFused(list(present)), [OUTPUT_NAMES[k] for k in present])
    return g


def _close(a, b):
    return a.shape == b.shape and np.allclose(a, b, rtol=1e-13, atol=0.0)


def _check_surfaces(g, X, e, capsys, batch_std=True, batch_routes_e=None, lines=None):
    """The four surfaces against `e`; `batch_routes_e`: predict_residual_batch's own expectation where it differs;
    `lines`: the set of lines the four calls print between them."""
    capsys.readouterr()
    eb = e if batch_routes_e is None else batch_routes_e
    mean, std = g.predict_residual_batch(X)
    assert _close(mean, eb["mean"]) and _close(std, eb["std"])
    out = g.predict_residual_jacobian_batch(X, return_std=True)
    assert len(out) == 4
    for got, key in zip(out, ("jmean", "J", "jstd", "dstd")):
        assert _close(got, e[key]), key
    mean2, J2 = g.predict_residual_jacobian_batch(X)
    assert _close(mean2, e["jmean"]) and _close(J2, e["J"])
    cmean, cov = g.predict_residual_cov_batch(X)
    assert _close(cmean, e["cmean"]) and _close(cov, e["cov"])
    draws = g.sample_residuals(X, n_samples=2)
    assert _close(draws, e["draws"])
    if lines is not None:
        assert set(capsys.readouterr().out.splitlines()) == set(lines)


def test_pretrained_batch_surfaces_route_by_route(tmp_path, capsys):
    from unmanned_aerial_vehicles_amd.trainer import OUTPUT_NAMES
    X = np.random.default_rng(5).standard_normal((3, 10))
    # the fused call serves everything
    g = _fake_pretrained(tmp_path)
    e = _expected(X, ["fused"] * 6)
    _check_surfaces(g, X, e, capsys, lines=[])
    mean, std = g.predict_residual_batch(X, return_std=False)
    assert _close(mean, e["mean"]) and std is None
    # the fused call raises: every model's own call serves; without return_std predict_residual_batch ends with zeros
    g._fused_bg[0].fail = True
    e = _expected(X, ["own"] * 6)
    _check_surfaces(g, X, e, capsys, lines=["GP prediction failed: fused down"])
    mean, std = g.predict_residual_batch(X, return_std=False)
    assert mean.shape == (3, 6) and not mean.any() and std is None
    assert capsys.readouterr().out.splitlines() == ["GP prediction failed: fused down"]
    # ... and one model's own call raises as well: that component is the fallback
    g.gp_models["z_residual"].fail = True
    e = _expected(X, ["own", "own", None, "own", "own", "own"])
    _check_surfaces(g, X, e, capsys, lines=["GP prediction failed: fused down", "GP prediction failed for z_residual: model 2 down"])
    # no fused object at all: the models' own calls, and predict_residual_batch hands back the stds it computed anyway
    g._fused_bg = False
    _check_surfaces(g, X, e, capsys, lines=["GP prediction failed for z_residual: model 2 down"])
    mean, std = g.predict_residual_batch(X, return_std=False)
    assert _close(mean, e["mean"]) and _close(std, e["std"])
    # one model missing, the fused call serving the other five; then failing
    g = _fake_pretrained(tmp_path, present=[0, 1, 2, 4, 5])
    _check_surfaces(g, X, _expected(X, ["fused", "fused", "fused", None, "fused", "fused"]), capsys, lines=[])
    g._fused_bg[0].fail = True
    _check_surfaces(g, X, _expected(X, ["own", "own", "own", None, "own", "own"]), capsys,
                    lines=["GP prediction failed: fused down"])
    # rows of width 7: the fallbacks everywhere, nothing raises
    g = _fake_pretrained(tmp_path)
    X7 = np.random.default_rng(6).standard_normal((3, 7))
    capsys.readouterr()
    _check_surfaces(g, X7, _expected(X7, [None] * 6), capsys)
    printed = capsys.readouterr().out.splitlines()
    assert printed and all(ln.startswith("GP prediction failed") for ln in printed)
    for n in OUTPUT_NAMES:      # (the Jacobian surface refuses the width before any call; the other two try every model)
        assert sum(ln.startswith(f"GP prediction failed for {n}: ") for ln in printed) == 3
    # nothing loaded
    g.is_loaded = False
    _check_surfaces(g, X, _expected(X, [None] * 6), capsys, lines=[])
    mean, std = g.predict_residual_batch(X, return_std=False)
    assert not mean.any() and np.array_equal(std, np.full((3, 6), 1e6))
