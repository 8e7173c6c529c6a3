"""gpk_sparse_predict_multi / _multi_grad / _multi_cov from a plain C caller in its own process (tests/c_abi/sparse_batch.c):
three handles, each begin -> update -> finalize on case (3, 60, 120, 4) of tests/test_gpu_sparse_batch.py, then the three entries
at M = 25 (the two-factor small-batch kernels with the model dimension) and M = 40 (model by model through the panel routes).
The C program checks repeatability, every bad-argument status and that block b equals gpk_sparse_predict* on handle b bit for
bit; this side compares what it wrote with the dense NumPy form at the project's fp64 bar, 1e-8 of each array's largest
component."""
import subprocess

import numpy as np
import pytest

from conftest import relerr
from test_gpu_c_abi import _compile
from test_gpu_sparse_batch import ALPHA, model_inputs, numpy_form

pytestmark = pytest.mark.gpu


def test_sparse_batch_from_c(tmp_path):
    exe = _compile(tmp_path, "sparse_batch.c")
    B, m, n, D, M = 3, 60, 120, 4, 40
    ps = [model_inputs(b, m, n, D) for b in range(B)]
    Xq = ps[0]["Xq"][:M]
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    parts = [np.array([B, n, m, D, M], dtype=np.float64)]
    for p in ps:
        parts += [p["X"].ravel(), p["y"], p["Z"].ravel(), p["ls"],
                  np.array([p["sf2"], p["noise"], ALPHA, 1e-8 * p["sf2"], p["ym"], p["ys"]])]
    np.concatenate(parts + [Xq.ravel()]).tofile(src)
    r = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "sparse batch from C: OK" in r.stdout
    out = np.fromfile(dst)
    ref = [numpy_form(p["X"], p["y"], p["Z"], Xq, p["ls"], p["sf2"], p["noise"], ALPHA, 1e-8 * p["sf2"], p["ym"], p["ys"])
           for p in ps]
    at = 0
    for Mc in (25, 40):
        sizes = (Mc * B, Mc * B, Mc * B * D, Mc * B * D, B * Mc * Mc)
        mean, var, dmean, dvar, cov = (out[at + sum(sizes[:i]):at + sum(sizes[:i + 1])] for i in range(5))
        at += sum(sizes)
        errs = {"mean": relerr(mean.reshape(Mc, B), np.stack([r_[0][:Mc] for r_ in ref], axis=1)),
                "var": relerr(var.reshape(Mc, B), np.stack([r_[1][:Mc] for r_ in ref], axis=1)),
                "dmean": relerr(dmean.reshape(Mc, B, D), np.stack([r_[2][:Mc] for r_ in ref], axis=1)),
                "dvar": relerr(dvar.reshape(Mc, B, D), np.stack([r_[3][:Mc] for r_ in ref], axis=1)),
                "cov": relerr(cov.reshape(B, Mc, Mc), np.stack([r_[4][:Mc, :Mc] for r_ in ref], axis=0))}
        for k, e in errs.items():
            print(f"from C, M = {Mc}: {k} {e:.2e} (bar 1e-08)")
        for k, e in errs.items():
            assert e < 1e-8, (k, e)
    assert at == out.size
