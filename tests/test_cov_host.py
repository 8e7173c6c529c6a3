"""CPU checks of the posterior-covariance feature: the built library exports its C entries, and the fixture script
regenerates tests/golden/cov_ref.npz bit for bit where scikit-learn is importable."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

NEW_SYMBOLS = ("gpk_predict_cov_inv", "gpk_predict_cov", "gpk_predict_host_cov", "gpk_predict_model_cov")


def test_libgpk_exports_the_covariance_entries():
    from unmanned_aerial_vehicles_amd import _build, _lib
    assert os.path.exists(_build.LIB_PATH), "libgpk.so must be built in-tree (python __graft_entry__.py)"
    _lib.load()
    lib = ctypes.CDLL(_build.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "gpk.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert f"GPK_API int {name}(" in header
        assert name in _lib.SIGNATURES


def test_estimator_has_the_covariance_surface():
    from unmanned_aerial_vehicles_amd import GaussianProcessRegressor
    assert callable(getattr(GaussianProcessRegressor, "sample_y", None))
    gp = GaussianProcessRegressor()
    with pytest.raises(RuntimeError, match="At most one of return_std or return_cov can be requested."):
        gp.predict(np.zeros((2, 3)), return_std=True, return_cov=True)


def test_make_golden_cov_regenerates_fixture(tmp_path):
    pytest.importorskip("sklearn")
    out = str(tmp_path / "cov_ref.npz")
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_cov.py"), out], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    new, ref = np.load(out), np.load(os.path.join(GOLDEN, "cov_ref.npz"))
    assert sorted(new.files) == sorted(ref.files)
    for k in ref.files:
        assert np.array_equal(new[k], ref[k]), k
