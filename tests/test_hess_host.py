"""CPU checks of the mean-Hessian feature (K8, second derivatives): the C entries are declared in include/gpk.h, exported by the
built library and listed in the signature table with the header's argument count; tests/golden/hess_ref.npz loads, is inside
its own cross-check bars and symmetric bit for bit, and its script regenerates it; the raw-unit conversion agrees with finite
differences of a NumPy model behind scalers; the wrappers serve the unloaded / untrained cases without a GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, relerr

NEW_ENTRIES = ("gpk_predict_mean_hess", "gpk_predict_mean_hess_multi", "gpk_predict_host_hess", "gpk_predict_host_multi_hess", "gpk_predict_model_hess",
               "gpk_predict_batched_hess", "gpk_sparse_predict_hess", "gpk_sparse_predict_multi_hess")
CASES = ("ka1", "train", "one", "ard", "pkg", "axis", "sparse")


@pytest.fixture(scope="module")
def hess_ref():
    d = np.load(os.path.join(GOLDEN, "hess_ref.npz"))
    return {k: d[k] for k in d.files}


def test_entries_are_declared_exported_and_listed():
    from unmanned_aerial_vehicles_amd import _build, _lib
    assert os.path.exists(_build.LIB_PATH), "libgpk.so must be built in-tree (python __graft_entry__.py)"
    _lib.load()
    lib = ctypes.CDLL(_build.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "gpk.h")).read()
    for name in NEW_ENTRIES:
        assert hasattr(lib, name), name
        m = re.search(r"GPK_API int " + name + r"\(([^;]*)\);", header)
        assert m, f"GPK_API int {name}( is missing from gpk.h"
        n_args = len(m.group(1).split(","))
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == n_args, (name, n_args)
        assert m.group(1).split(",")[-1].split()[-1].startswith("hess"), "the Hessian is the last argument"


def test_fixture_is_inside_its_bars_and_symmetric(hess_ref):
    shapes = {"ka1": (64, 6, 10, 10), "train": (25, 6, 10, 10), "one": (32, 10, 10), "ard": (32, 10, 10),
              "pkg": (16, 6, 10, 10), "axis": (25, 6, 10, 10), "sparse": (40, 2, 4, 4)}
    for case in CASES:
        H = hess_ref[case + "_hess"]
        assert H.shape == shapes[case] and H.dtype == np.float64 and np.isfinite(H).all(), case
        assert hess_ref[case + "_Xq"].shape == (H.shape[0], H.shape[-1]), case
        assert float(hess_ref[case + "_chk"]) < 1e-12 and float(hess_ref[case + "_fd"]) < 1e-9, case
        assert np.array_equal(H, H.swapaxes(-1, -2)), case
    Hs = hess_ref["axis_hess_scaled"]
    assert Hs.shape == (25, 6, 10, 10) and np.array_equal(Hs, Hs.swapaxes(-1, -2))


def test_make_golden_hess_regenerates_fixture(tmp_path):
    pytest.importorskip("sklearn")
    out = str(tmp_path / "hess_ref.npz")
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_hess.py"), out], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    assert open(out, "rb").read() == open(os.path.join(GOLDEN, "hess_ref.npz"), "rb").read(), "not regenerated bit for bit"


# ---- the raw-unit conversion ----------------------------------------------------------------------------------------------
def _numpy_model(seed=3, N=40, D=5):
    """f(z) = sum_j k(z, x_j) a_j with an ARD RBF kernel: value, gradient and Hessian in closed form."""
    rng = np.random.default_rng(seed)
    Xt, a, ls = rng.standard_normal((N, D)), rng.standard_normal(N), 0.8 + rng.random(D)

    def f(Z):
        delta = (Z[:, None, :] - Xt[None, :, :]) / ls
        return np.exp(-0.5 * np.sum(delta ** 2, axis=2)) @ a

    def hess(Z):
        delta = (Z[:, None, :] - Xt[None, :, :]) / ls
        w = np.exp(-0.5 * np.sum(delta ** 2, axis=2)) * a
        T = np.einsum("mj,mjd,mje->mde", w, delta, delta) - np.sum(w, axis=1)[:, None, None] * np.eye(D)
        return T / (ls[:, None] * ls[None, :])

    return f, hess, D


def test_hessian_to_raw_against_finite_differences():
    from unmanned_aerial_vehicles_amd.trainer import hessian_to_raw
    f, hess, D = _numpy_model()
    rng = np.random.default_rng(4)
    shift, scale_x = rng.standard_normal(D), np.array([0.5, 2.0, 30.0, 1e-3, 1.0])
    mean_y, scale_y = 0.3, -2.5                      # (a negative target scale: the sign goes through)
    X = shift + scale_x * rng.standard_normal((6, D))

    def raw(Xr):
        return mean_y + scale_y * f((Xr - shift) / scale_x)

    Hs = hess((X - shift) / scale_x)
    Hs = np.triu(Hs) + np.triu(Hs, 1).swapaxes(-1, -2)      # (einsum's two triangles differ in the last bit: mirror one)
    H = hessian_to_raw(Hs, scale_x, scale_y)
    assert H.shape == (6, D, D) and np.array_equal(H, H.swapaxes(-1, -2)), "a bit-symmetric input stays bit-symmetric"
    # second-order central differences of the raw function, step 1e-4 of each input's own scale; compared per (d, e) in units
    # of the inputs' scales (the raw entries span 12 orders of magnitude here).  Truncation ~h^2 f'''' / 12 ~ 1e-9 and
    # rounding ~4 eps |f| / h^2 ~ 1e-7 relative to entries of order one: bar 1e-5
    h = 1e-4 * scale_x
    fd = np.zeros_like(H)
    for d in range(D):
        for e in range(D):
            ed, ee = np.eye(D)[d] * h[d], np.eye(D)[e] * h[e]
            fd[:, d, e] = (raw(X + ed + ee) - raw(X + ed - ee) - raw(X - ed + ee) + raw(X - ed - ee)) / (4.0 * h[d] * h[e])
    unit = scale_x[:, None] * scale_x[None, :]
    err = relerr(fd * unit, H * unit)
    print(f"hessian_to_raw against central differences: {err:.2e}")
    assert err < 1e-5
    assert np.array_equal(hessian_to_raw(np.ones((D, D)), np.ones(D), 1.0), np.ones((D, D)))
    with pytest.raises(ValueError):
        hessian_to_raw(np.zeros((3, D, D + 1)), scale_x, 1.0)


# ---- surfaces and their fall-backs ------------------------------------------------------------------------------------
def test_surfaces_exist():
    from unmanned_aerial_vehicles_amd import GaussianProcessRegressor, SparseGP
    from unmanned_aerial_vehicles_amd.batched import BatchedARDGP
    from unmanned_aerial_vehicles_amd.device import DeviceGP
    from unmanned_aerial_vehicles_amd.package_gp import GaussianProcess
    from unmanned_aerial_vehicles_amd.simple_gp import SimpleQuadrotorGP
    from unmanned_aerial_vehicles_amd.sparse_batch import BatchedSparseGP
    from unmanned_aerial_vehicles_amd.trainer import PreTrainedGP
    for cls in (GaussianProcessRegressor, BatchedARDGP, SparseGP, BatchedSparseGP, GaussianProcess):
        assert callable(getattr(cls, "predict_hessian", None)), cls
    assert callable(getattr(DeviceGP, "predict_mean_hess_dev", None)) and callable(getattr(DeviceGP, "predict_hess_host", None))
    assert callable(getattr(PreTrainedGP, "predict_residual_hessian_batch", None))
    assert callable(getattr(PreTrainedGP, "predict_residual_hessian", None))
    assert callable(getattr(SimpleQuadrotorGP, "predict_residual_hessian", None))


def test_unfitted_estimator_returns_the_prior_and_zero_derivatives():
    from unmanned_aerial_vehicles_amd import RBF, GaussianProcessRegressor, WhiteKernel
    X = np.random.default_rng(0).standard_normal((7, 4))
    mean, dmean, hess = GaussianProcessRegressor(n_targets=3).predict_hessian(X)
    assert mean.shape == (7, 3) and dmean.shape == (7, 3, 4) and hess.shape == (7, 3, 4, 4)
    assert not mean.any() and not dmean.any() and not hess.any()
    gp = GaussianProcessRegressor(kernel=2.0 * RBF(0.7) + WhiteKernel(0.25))
    mean, dmean, hess = gp.predict_hessian(X)
    assert mean.shape == (7,) and dmean.shape == (7, 4) and hess.shape == (7, 4, 4) and not hess.any()
    assert not hasattr(gp, "X_train_") and getattr(gp, "_dev", None) is None
    with pytest.raises(ValueError, match="NaN or infinity"):
        gp.predict_hessian(np.array([[0.0, np.inf, 0.0, 0.0]]))


def test_unloaded_and_untrained_models_return_zeros(capsys):
    from unmanned_aerial_vehicles_amd.package_gp import GaussianProcess
    from unmanned_aerial_vehicles_amd.simple_gp import SimpleQuadrotorGP
    from unmanned_aerial_vehicles_amd.trainer import PreTrainedGP
    mean, J, H = SimpleQuadrotorGP().predict_residual_hessian(np.zeros(6), np.zeros(4))
    assert mean.shape == (6,) and J.shape == (6, 10) and H.shape == (6, 10, 10)
    assert not mean.any() and not J.any() and not H.any()
    assert "not trained" in capsys.readouterr().out
    pre = PreTrainedGP(os.path.join(GOLDEN, "no_such_model.pkl"))
    assert not pre.is_loaded
    mean, J, H = pre.predict_residual_hessian(np.zeros(6), np.zeros(4))
    assert mean.shape == (6,) and J.shape == (6, 10) and H.shape == (6, 10, 10)
    assert not mean.any() and not J.any() and not H.any()
    assert "no model loaded" in capsys.readouterr().out
    mean, J, H = pre.predict_residual_hessian_batch(np.zeros((5, 10)))
    assert mean.shape == (5, 6) and J.shape == (5, 6, 10) and H.shape == (5, 6, 10, 10) and not H.any()
    mean, J, H = pre.predict_residual_hessian("not a state", None)          # never raises
    assert mean.shape == (6,) and J.shape == (6, 10) and H.shape == (6, 10, 10) and not H.any()
    g = GaussianProcess(input_dim=5, output_dim=2)
    mean, dmean, hess = g.predict_hessian(np.zeros((3, 5)))
    assert mean.shape == (3, 2) and dmean.shape == (3, 2, 5) and hess.shape == (3, 2, 5, 5)
    assert not mean.any() and not dmean.any() and not hess.any()
