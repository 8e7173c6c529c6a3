"""CPU checks of the input-gradient feature (K8): the built library exports its C entries, the Python surfaces exist and
serve the unfitted / untrained cases without a GPU, and the fixture script regenerates tests/golden/jac_ref.npz bit for bit
where scikit-learn is importable."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

NEW_SYMBOLS = ("gpk_predict_mean_grad", "gpk_predict_var_grad_inv", "gpk_predict_host_grad", "gpk_predict_model_grad")


def test_libgpk_exports_the_gradient_entries():
    from unmanned_aerial_vehicles_amd import _build, _lib
    assert os.path.exists(_build.LIB_PATH), "libgpk.so must be built in-tree (python __graft_entry__.py)"
    _lib.load()
    lib = ctypes.CDLL(_build.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "gpk.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert f"GPK_API int {name}(" in header
        assert name in _lib.SIGNATURES


def test_surfaces_exist():
    from unmanned_aerial_vehicles_amd import GaussianProcessRegressor
    from unmanned_aerial_vehicles_amd.device import DeviceGP
    from unmanned_aerial_vehicles_amd.package_gp import GaussianProcess
    from unmanned_aerial_vehicles_amd.simple_gp import SimpleQuadrotorGP
    assert callable(getattr(GaussianProcessRegressor, "predict_jacobian", None))
    assert callable(getattr(SimpleQuadrotorGP, "predict_residual_jacobian", None))
    assert callable(getattr(SimpleQuadrotorGP, "linearize_gp_residuals", None))
    assert callable(getattr(GaussianProcess, "predict_jacobian", None))
    assert callable(getattr(DeviceGP, "predict_grad_dev", None)) and callable(getattr(DeviceGP, "predict_grad_host", None))


def test_unfitted_estimator_returns_the_prior_and_zero_gradients():
    from unmanned_aerial_vehicles_amd import RBF, GaussianProcessRegressor, WhiteKernel
    gp = GaussianProcessRegressor(n_targets=3)
    X = np.random.default_rng(0).standard_normal((7, 4))
    mean, dmean = gp.predict_jacobian(X)
    assert mean.shape == (7, 3) and dmean.shape == (7, 3, 4) and not mean.any() and not dmean.any()
    mean, dmean, var, dvar = gp.predict_jacobian(X, return_var=True)
    assert var.shape == (7, 3) and dvar.shape == (7, 3, 4) and np.all(var == 1.0) and not dvar.any()
    assert not hasattr(gp, "X_train_") and getattr(gp, "_dev", None) is None       # the GPU path's fitted state is untouched
    # one target: predict's squeezing; the prior variance carries the WhiteKernel level as predict(return_std=True) does
    gp = GaussianProcessRegressor(kernel=2.0 * RBF(0.7) + WhiteKernel(0.25))
    mean, dmean, var, dvar = gp.predict_jacobian(X, return_var=True)
    assert mean.shape == (7,) and dmean.shape == (7, 4) and var.shape == (7,) and dvar.shape == (7, 4)
    assert np.allclose(var, gp.predict(X, return_std=True)[1] ** 2, rtol=1e-15) and np.all(var == 2.25)
    with pytest.raises(ValueError, match="NaN or infinity"):
        gp.predict_jacobian(np.array([[0.0, np.inf, 0.0, 0.0]]))


def test_untrained_models_return_zeros():
    from unmanned_aerial_vehicles_amd.package_gp import GaussianProcess
    from unmanned_aerial_vehicles_amd.simple_gp import SimpleQuadrotorGP
    m = SimpleQuadrotorGP()
    mean, J = m.predict_residual_jacobian(np.zeros(6), np.zeros(4))
    assert mean.shape == (6,) and J.shape == (6, 10) and not mean.any() and not J.any()
    N = 25
    D, A, B = m.linearize_gp_residuals(np.ones((6, N + 1)), np.ones((4, N)), 0.05)
    assert D.shape == (6, N) and A.shape == (N, 6, 6) and B.shape == (N, 6, 4)
    assert not D.any() and not A.any() and not B.any()
    D, A, B = m.linearize_gp_residuals(np.ones((3, 6, N + 1)), np.ones((3, 4, N)), 0.05)
    assert D.shape == (3, 6, N) and A.shape == (3, N, 6, 6) and B.shape == (3, N, 6, 4)
    assert not D.any() and not A.any() and not B.any()
    g = GaussianProcess(input_dim=5, output_dim=2)
    mean, var, dmean, dvar = g.predict_jacobian(np.zeros((3, 5)))
    assert mean.shape == (3, 2) and var.shape == (3, 2) and dmean.shape == (3, 2, 5) and dvar.shape == (3, 5)
    assert not mean.any() and not dmean.any() and not dvar.any() and np.all(var == g.kernel.signal_variance)


def test_make_golden_jac_regenerates_fixture(tmp_path):
    pytest.importorskip("sklearn")
    out = str(tmp_path / "jac_ref.npz")
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_jac.py"), out], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    new, ref = np.load(out), np.load(os.path.join(GOLDEN, "jac_ref.npz"))
    assert sorted(new.files) == sorted(ref.files)
    for k in ref.files:
        assert np.array_equal(new[k], ref[k]), k
    # the reference's own error is far inside the 1e-8 bar it is used at: the closed forms through solve_triangular against
    # an explicit inverse of L_, and against fourth-order differences (h = 1e-3) of scikit-learn's predict
    for case in ("ka1", "train", "one", "ard", "pkg"):
        assert ref[case + "_chk"].max() < 1e-12 and ref[case + "_fd"].max() < 1e-9, case
