"""The FITC sparse GP ("FITC") without a GPU: the fixture regenerates bit for bit, the new C entries are
declared, bound and exported, `approximation=` is validated on every surface, the gradient surfaces and `train` refuse with
the named ValueError before any device is touched, and the pickle state carries the kind."""
import hashlib
import inspect
import os
import pickle
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

ENTRIES = ("gpk_sparse_accumulate_fitc", "gpk_sparse_set_approximation", "gpk_sparse_get_approximation",
           "gpk_sparse_restore_approximation")


def kernel():
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, WhiteKernel
    return ConstantKernel(1.3) * RBF([1.0, 1.1, 1.2]) + WhiteKernel(0.01)


def Z0():
    return np.random.default_rng(5).standard_normal((7, 3))


def test_fixture_regenerates_bit_for_bit(tmp_path):
    for name in ("make_golden_sparse_fitc.py", "sparse_ref.npz"):
        shutil.copy(os.path.join(GOLDEN, name), tmp_path / name)
    r = subprocess.run([sys.executable, str(tmp_path / "make_golden_sparse_fitc.py")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    digest = lambda p: hashlib.sha256(open(p, "rb").read()).hexdigest()  # noqa: E731
    assert digest(tmp_path / "sparse_fitc_ref.npz") == digest(os.path.join(GOLDEN, "sparse_fitc_ref.npz"))


def test_fixture_records_what_the_tests_rely_on():
    d = np.load(os.path.join(GOLDEN, "sparse_fitc_ref.npz"))
    for c in "ABC":
        assert d[c + "_forms"].shape == (3,) and d[c + "_forms"].max() < 1e-8       # the two CPU forms agree
        w = d[c + "_w"]
        assert np.isfinite(w).all() and w.min() > 0.0 and w.max() <= 1.0
    assert d["A_G"].shape == (130, 130)       # (G = (Kuf w) Kuf^T: symmetric up to rounding)
    assert np.max(np.abs(d["A_G"] - d["A_G"].T)) <= 1e-12 * np.max(np.abs(d["A_G"]))
    assert np.max(1.0 - d["C_w"][d["C_idx"]]) < 1e-6
    assert d["B_vs_dtc"].shape == (3,) and d["B_vs_exact"].shape == (3,) and np.isfinite(d["B_vs_dtc"]).all()
    # DTC and FITC are different models on case A
    ref = np.load(os.path.join(GOLDEN, "sparse_ref.npz"))
    assert np.max(np.abs((d["A_mean"] - ref["A_mean"]) / ref["A_y_std"])) > 0.1


def test_entries_declared_bound_and_exported():
    from unmanned_aerial_vehicles_amd import _lib
    header = open(os.path.join(ROOT, "include", "gpk.h")).read()
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(r"GPK_API int %s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert re.search(r"#define GPK_SPARSE_DTC 0\b", header) and re.search(r"#define GPK_SPARSE_FITC 1\b", header)
    assert "Replaces: GPflow's GPRFITC" in header
    # the building block: the operands of gpk_sparse_accumulate, then (Wuu, ldw, sigma2, log_lambda_sum, w)
    assert _lib.SIGNATURES["gpk_sparse_accumulate_fitc"][1][:12] == _lib.SIGNATURES["gpk_sparse_accumulate"][1]
    assert len(_lib.SIGNATURES["gpk_sparse_accumulate_fitc"][1]) == 17


def test_approximation_is_validated_on_every_surface():
    from unmanned_aerial_vehicles_amd import BatchedSparseGP, SparseGP
    from unmanned_aerial_vehicles_amd.trainer import GPTrainer
    assert SparseGP(kernel(), Z0()).approximation_ == "dtc"
    assert SparseGP(kernel(), Z0(), approximation="fitc").approximation_ == "fitc"
    for bad in ("FITC", "vfe", None, 1):
        with pytest.raises(ValueError, match="approximation must be 'dtc' or 'fitc'"):
            SparseGP(kernel(), Z0(), approximation=bad)
        with pytest.raises(ValueError, match="approximation must be 'dtc' or 'fitc'"):
            SparseGP.from_exact(object(), approximation=bad)          # (checked before the regressor is looked at)
        with pytest.raises(ValueError, match="approximation must be 'dtc' or 'fitc'"):
            BatchedSparseGP.from_exact([object()], approximation=bad)
        with pytest.raises(ValueError, match="approximation must be 'dtc' or 'fitc'"):
            GPTrainer().sparsify(np.zeros((1, 10)), np.zeros((1, 6)), 4, approximation=bad)
    for f in (SparseGP.__init__, SparseGP.from_exact, BatchedSparseGP.from_exact, GPTrainer.sparsify):
        assert inspect.signature(f).parameters["approximation"].default == "dtc"
    # a batch may mix the kinds
    b = BatchedSparseGP([SparseGP(kernel(), Z0(), approximation=a) for a in ("fitc", "dtc", "fitc")])
    assert b.approximations_ == ["fitc", "dtc", "fitc"]


def test_gradient_surfaces_refuse_without_a_device():
    from unmanned_aerial_vehicles_amd import SparseGP
    gp = SparseGP(kernel(), Z0(), approximation="fitc")
    theta = gp.kernel_.theta
    X, y = np.zeros((4, 3)), np.zeros(4)
    for call in (lambda: gp.log_bound(theta, eval_gradient=True),
                 lambda: gp.log_bound(theta, inducing=Z0(), eval_inducing_gradient=True),
                 lambda: gp.train(X, y),
                 lambda: gp.train(X, y, train_inducing=True, select_inducing="greedy")):
        with pytest.raises(ValueError, match="FITC") as e:
            call()
        assert "train as DTC" in str(e.value) and "approximation='fitc'" in str(e.value)
    assert gp._be is None and not gp._live, "no backend may have been created"
    # the DTC model's argument checks are what they were
    with pytest.raises(ValueError, match="Gradient can only be evaluated for theta!=None"):
        SparseGP(kernel(), Z0()).log_bound(None, eval_gradient=True)


def test_pickle_state_carries_the_kind():
    from unmanned_aerial_vehicles_amd import SparseGP
    gp = SparseGP(kernel(), Z0(), approximation="fitc")
    st = gp.__getstate__()
    assert st["approximation_"] == "fitc"
    back = pickle.loads(pickle.dumps(gp))
    assert back.approximation_ == "fitc" and back._fitc
    # statistics waiting to be imported travel with their scalar
    gp._state = {"G": np.eye(7), "g": np.ones((7, 1)), "yy": np.ones(1), "n_rows": 3, "log_lambda_sum": -1.25}
    back = pickle.loads(pickle.dumps(gp))
    assert back.statistics()["log_lambda_sum"] == -1.25 and back.n_rows_ == 3
    # a state written before the attribute existed loads as DTC
    old = SparseGP(kernel(), Z0()).__getstate__()
    del old["approximation_"]
    gp2 = SparseGP.__new__(SparseGP)
    gp2.__setstate__(old)
    assert gp2.approximation_ == "dtc" and not gp2._fitc
    assert "log_lambda_sum" not in (gp2.statistics() or {})
