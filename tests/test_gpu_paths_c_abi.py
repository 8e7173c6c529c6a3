"""Posterior function draws (K10) from a plain C caller in its own process (tests/c_abi/paths.c): the fit building blocks, then
gpk_rff_features -> gpk_paths_prepare -> gpk_paths_step -> gpk_paths_rollout on case b of tests/test_gpu_paths.py, (N, D, F, S,
P) = (130, 4, 64, 70, 3), with the randomness of tests/golden/paths_ref.npz written to a file.  The C program checks the zeros
in the padding of the feature block, that a pitched Coef keeps its pitch columns, repeatability and every bad-argument status;
this side compares what it wrote with the dense NumPy form at the project's fp64 bar, 1e-8 of each array's largest component."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, relerr
from test_gpu_c_abi import _compile
from test_gpu_paths import paths_numpy_form

pytestmark = pytest.mark.gpu


def test_paths_from_c(tmp_path):
    exe = _compile(tmp_path, "paths.c")
    d = np.load(os.path.join(GOLDEN, "paths_ref.npz"))
    c = {k[2:]: d[k] for k in d.files if k.startswith("b_")}
    N, D, F, S, P, H, M = 130, 4, 64, 70, 3, len(c["U"]), len(c["Xq"])
    C = S * P
    sf2, noise, alpha = c["hyper"]
    form = paths_numpy_form(c["X"], c["Y"], c["ls"], sf2, noise, alpha, c["omega"], c["phase"], c["weights"], c["eps"])
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    parts = [np.array([N, D, F, S, P, H, M, sf2, noise + alpha]), c["ls"], form.ym, form.ys, c["X"], form.Yn, c["omega"], c["phase"],
             c["weights"].reshape(F, C), c["eps"].reshape(N, C), c["Xs"], c["x0"], c["U"], c["lin"], c["Xq"]]
    np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in parts]).tofile(src)
    r = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "paths from C: OK" in r.stdout
    out = np.fromfile(dst)
    sizes = (M * F, (N + F) * C, C, (H + 1) * C)
    assert out.size == sum(sizes)
    phi, coef, step, traj = (out[sum(sizes[:i]):sum(sizes[:i + 1])] for i in range(4))
    want_coef = np.concatenate([form.V.reshape(N, C), form.Ww.reshape(F, C)])
    errs = {"Phi": relerr(phi.reshape(M, F), 0.7 * np.cos(c["Xq"] @ c["omega"].T + c["phase"])),
            "Coef": relerr(coef.reshape(N + F, C), want_coef),
            "step": relerr(step.reshape(S, P), form.step(c["Xs"])),
            "traj": relerr(traj.reshape(H + 1, S, P), form.rollout(c["x0"], c["U"], c["lin"]))}
    for k, e in errs.items():
        print(f"from C: {k} {e:.2e} (bar 1e-08)")
    for k, e in errs.items():
        assert e < 1e-8, (k, e)
