"""Posterior function draws of the sparse models (K10, "the sparse models") from a plain C caller in its own process
(tests/c_abi/sparse_paths.c): case b of tests/test_gpu_sparse_paths.py - one model, (m, D, F, S, P, n) = (50, 4, 64, 70, 3, 130) -
through gpk_sparse_begin -> update -> finalize -> gpk_sparse_paths_prepare -> gpk_paths_step, and case d - four models without rows,
(m, D, F, S, B) = (33, 10, 32, 9, 4), nx = 6, coord = (0, 2, 3, 5) - through a handle and a gpk_sparse_paths_prepare per model, then
gpk_paths_step_multi_z -> gpk_paths_rollout_multi_z, with the randomness of tests/golden/sparse_paths_ref.npz written to files.
The C program allocates both coefficient matrices pitched (three guard columns) and checks that the padding between the blocks
and the guard columns stay NaN, repeatability, the copies of the inducing inputs and a bad-argument status of each new entry;
this side compares what it wrote with the dense NumPy form at the project's fp64 bar, 1e-8 of each array's largest component."""
import subprocess

import numpy as np
import pytest

from conftest import relerr
from test_gpu_c_abi import _compile
from test_gpu_sparse_paths import G, load_case

pytestmark = pytest.mark.gpu


def test_sparse_paths_from_c(tmp_path):
    exe = _compile(tmp_path, "sparse_paths.c")
    b = load_case("b")
    m, D, F, S, P, n = 50, 4, 64, 70, 3, 130
    fb = G.SparseForm(b["Z"], b["X"], b["Y"], b["ls"], *b["hyper"], b["ynorm"][0], b["ynorm"][1], b["omega"], b["phase"], b["weights"],
                      b["xi"])
    d = load_case("d")
    m2, D2, F2, S2, B, nx, H = 33, 10, 32, 9, 4, 6, len(d["U"])
    fd = G.SparseBatchForm(d["Z"], d["X"], d["Y"], d["ls"], d["hyper"], d["ynorm"], d["omega"], d["phase"], d["weights"], d["xi"],
                           d["out"])
    shift, scale = d["out"][0] + d["out"][1] * d["ynorm"][0], d["out"][1] * d["ynorm"][1]      # the target scaler folded on the host
    src1, src2, dst = str(tmp_path / "single.bin"), str(tmp_path / "batch.bin"), str(tmp_path / "out.bin")
    parts1 = [np.array([m, D, F, S, P, n]), b["hyper"], b["ynorm"][0], b["ynorm"][1], b["ls"], b["Z"], b["X"], b["Y"], b["omega"],
              b["phase"], b["weights"], b["xi"], b["Xs"]]
    parts2 = [np.array([m2, D2, F2, S2, B, H, nx]), d["hyper"], d["ynorm"][0], d["ynorm"][1], shift, scale, d["ls"], d["Z"], d["omega"],
              d["phase"], d["weights"], d["xi"], d["Xs"], d["x0"], d["U"], d["lin"], d["coord"], d["in"][0], d["in"][1]]
    for path, parts in ((src1, parts1), (src2, parts2)):
        np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in parts]).tofile(path)
    r = subprocess.run([exe, src1, src2, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "sparse paths from C: OK" in r.stdout
    out = np.fromfile(dst)
    sizes = ((m + F) * S * P, S * P, (m2 + F2) * B * S2, B * m2 * D2, S2 * B, (H + 1) * S2 * nx)
    assert out.size == sum(sizes)
    coef1, step1, coef2, zs, step2, traj = (out[sum(sizes[:i]):sum(sizes[:i + 1])] for i in range(6))
    assert np.array_equal(zs.reshape(B, m2, D2), d["Z"])
    want1 = np.concatenate([fb.V.reshape(m, S * P), fb.Ww.reshape(F, S * P)])
    want2 = np.stack([np.concatenate([f.V[:, :, 0], f.Ww[:, :, 0]]) for f in fd.forms], axis=1)       # (m + F, B, S)
    errs = {"single Coef": relerr(coef1.reshape(m + F, S * P), want1),
            "single step": relerr(step1.reshape(S, P), b["step"]),
            "batch Coef": relerr(coef2.reshape(m2 + F2, B, S2), want2),
            "batch step": relerr(step2.reshape(S2, B), d["step"]),
            "batch traj": relerr(traj.reshape(H + 1, S2, nx), d["traj"])}
    for k, e in errs.items():
        print(f"from C: {k} {e:.2e} (bar 1e-08)")
    for k, e in errs.items():
        assert e < 1e-8, (k, e)
