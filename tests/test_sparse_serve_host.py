"""Host-side checks of the sparse GP's gradient / covariance serving: the fixture script reproduces
tests/golden/sparse_serve_ref.npz bit for bit, and the two new C entries are declared, bound and exported."""
import ctypes
import os
import subprocess
import sys

import numpy as np

from conftest import GOLDEN, ROOT

NEW_SYMBOLS = ("gpk_sparse_predict_grad", "gpk_sparse_predict_cov")


def test_fixture_script_reproduces_the_file(tmp_path):
    committed = os.path.join(GOLDEN, "sparse_serve_ref.npz")
    # the script writes next to itself: run a copy from a directory that holds its two inputs
    for name in ("make_golden_sparse_serve.py", "make_golden_sparse.py", "sparse_ref.npz"):
        with open(os.path.join(GOLDEN, name), "rb") as src, open(tmp_path / name, "wb") as dst:
            dst.write(src.read())
    r = subprocess.run([sys.executable, str(tmp_path / "make_golden_sparse_serve.py")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    print(r.stdout)
    with open(committed, "rb") as a, open(tmp_path / "sparse_serve_ref.npz", "rb") as b:
        assert a.read() == b.read(), "make_golden_sparse_serve.py no longer reproduces tests/golden/sparse_serve_ref.npz"


def test_fixture_holds_what_the_tests_read():
    d = np.load(os.path.join(GOLDEN, "sparse_serve_ref.npz"))
    src = np.load(os.path.join(GOLDEN, "sparse_ref.npz"))
    for case, (M, P, D) in (("A", (40, 2, 4)), ("B", (40, 1, 6))):
        assert src[case + "_Xq"].shape == (M, D)
        assert d[case + "_dmean"].shape == (M, P, D) and d[case + "_dvar"].shape == (M, D) and d[case + "_cov"].shape == (M, M)
        for what in ("dmean", "dvar", "cov"):
            assert 0.0 <= float(d[f"{case}_{what}_agree"]) < 1e-8
        assert np.allclose(d[case + "_cov"], d[case + "_cov"].T, rtol=0, atol=1e-14)
    assert d["B_exact_dmean"].shape == (40, 1, 6) and d["B_exact_cov"].shape == (40, 40) and float(d["B_exact_agree"].max()) < 1e-8
    # rows 3, 17 and 31 of case A's queries coincide with training rows
    assert all((src["A_X"] == src["A_Xq"][i]).all(axis=1).any() for i in (3, 17, 31))


def test_libgpk_exports_the_sparse_serving_entries():
    from unmanned_aerial_vehicles_amd import _build, _lib
    assert os.path.exists(_build.LIB_PATH), "libgpk.so must be built in-tree (python __graft_entry__.py)"
    _lib.load()
    lib = ctypes.CDLL(_build.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "gpk.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert f"GPK_API int {name}(" in header
        assert name in _lib.SIGNATURES


def test_sparse_gp_has_the_serving_surface():
    from unmanned_aerial_vehicles_amd import SparseGP
    for name in ("predict_jacobian", "sample_y"):
        assert callable(getattr(SparseGP, name, None)), name
    assert "return_cov" in SparseGP.predict.__code__.co_varnames
