"""gpk_sparse_predict_grad / gpk_sparse_predict_cov from a plain C caller in its own process (tests/c_abi/sparse_serve.c):
begin -> update -> finalize -> the two entries on case A of tests/golden/sparse_ref.npz at M = 25 (the two-factor small-batch
kernels) and M = 40 (the panel routes).  The C program checks repeatability, gpk_sparse_predict's bits and every
bad-argument status; this side compares what it wrote with tests/golden/sparse_serve_ref.npz at the fixture's bar,
max(1e-8, 10 x the stored two-form agreement) of each array's largest component."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, relerr
from test_gpu_c_abi import _compile

pytestmark = pytest.mark.gpu


def test_sparse_serving_from_c(tmp_path):
    exe = _compile(tmp_path, "sparse_serve.c")
    ref = np.load(os.path.join(GOLDEN, "sparse_ref.npz"))
    fix = np.load(os.path.join(GOLDEN, "sparse_serve_ref.npz"))
    X, Y, Z, Xq = ref["A_X"], ref["A_Y"], ref["A_Z"], ref["A_Xq"]
    (N, D), P, m, M = X.shape, Y.shape[1], Z.shape[0], Xq.shape[0]
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate([np.array([N, m, D, P, M], dtype=np.float64), X.ravel(), Y.ravel(), Z.ravel(), Xq.ravel(), ref["A_ls"],
                    ref["A_hyper"], ref["A_y_mean"], ref["A_y_std"]]).tofile(src)
    r = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "sparse serving from C: OK" in r.stdout
    out = np.fromfile(dst)
    ys2, noise = ref["A_y_std"] ** 2, ref["A_hyper"][1]
    at = 0
    for Mc in (25, 40):
        sizes = (Mc * P, Mc * P, Mc * P * D, Mc * P * D, P * Mc * Mc)
        mean, var, dmean, dvar, cov = (out[at + sum(sizes[:i]):at + sum(sizes[:i + 1])] for i in range(5))
        at += sum(sizes)
        bars = {k: max(1e-8, 10.0 * float(fix[f"A_{k}_agree"])) for k in ("dmean", "dvar", "cov")}
        errs = {"mean": (relerr(mean.reshape(Mc, P), ref["A_mean"][:Mc]), 1e-8),
                "var": (relerr(var.reshape(Mc, P), np.maximum(ref["A_var"][:Mc] + noise, 0.0)[:, None] * ys2), 1e-8),
                "dmean": (relerr(dmean.reshape(Mc, P, D), fix["A_dmean"][:Mc]), bars["dmean"]),
                "dvar": (relerr(dvar.reshape(Mc, P, D), fix["A_dvar"][:Mc, None, :] * ys2[None, :, None]), bars["dvar"]),
                "cov": (relerr(cov.reshape(P, Mc, Mc), fix["A_cov"][None, :Mc, :Mc] * ys2[:, None, None]), bars["cov"])}
        for k, (e, b) in errs.items():
            print(f"from C, M = {Mc}: {k} {e:.2e} (bar {b:.1e})")
        for k, (e, b) in errs.items():
            assert e < b, (k, e, b)
    assert at == out.size
