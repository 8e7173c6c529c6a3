"""Posterior function draws of the per-axis batch (K10) from a plain C caller in its own process (tests/c_abi/axis_paths.c): per
model the fit building blocks and gpk_paths_prepare (P = 1) into its column block, then gpk_paths_step_multi ->
gpk_paths_rollout_multi on case b of tests/test_gpu_axis_paths.py, (N, D, F, S, B) = (130, 4, 64, 70, 3), nx = 3, with the
randomness of tests/golden/axis_paths_ref.npz written to a file.  The C program allocates the coefficient matrix with
ldc = B mstride + 3 and checks that the padding between the blocks and the pitch columns stay NaN, repeatability, stage 1 of the
rollout against the step, and a bad-argument status of each entry; this side compares what it wrote with the dense NumPy form at
the project's fp64 bar, 1e-8 of each array's largest component."""
import subprocess

import numpy as np
import pytest

from conftest import relerr
from test_gpu_axis_paths import axis_paths_numpy_form, load_case
from test_gpu_c_abi import _compile

pytestmark = pytest.mark.gpu


def test_axis_paths_from_c(tmp_path):
    exe = _compile(tmp_path, "axis_paths.c")
    c = load_case("b")
    N, D, F, S, B, nx, H = 130, 4, 64, 70, 3, 3, len(c["U"])
    form = axis_paths_numpy_form(c["X"], c["Y"], c["ls"], c["hyper"], c["omega"], c["phase"], c["weights"], c["eps"], c["out"])
    ym, ys = np.array([f.ym[0] for f in form.forms]), np.array([f.ys[0] for f in form.forms])
    shift, scale = c["out"][0] + c["out"][1] * ym, c["out"][1] * ys        # the target scaler folded on the host
    Yn = np.stack([f.Yn[:, 0] for f in form.forms])
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    parts = [np.array([N, D, F, S, B, H, nx]), c["hyper"][:, 0], c["hyper"][:, 1] + c["hyper"][:, 2], shift, scale, c["ls"], c["X"],
             Yn, c["omega"], c["phase"], c["weights"], c["eps"], c["Xs"], c["x0"], c["U"], c["lin"], c["coord"], c["in"][0],
             c["in"][1]]
    np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in parts]).tofile(src)
    r = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "axis paths from C: OK" in r.stdout
    out = np.fromfile(dst)
    sizes = ((N + F) * B * S, S * B, (H + 1) * S * nx)
    assert out.size == sum(sizes)
    coef, step, traj = (out[sum(sizes[:i]):sum(sizes[:i + 1])] for i in range(3))
    want_coef = np.stack([np.concatenate([f.V[:, :, 0], f.Ww[:, :, 0]]) for f in form.forms], axis=1)       # (N + F, B, S)
    errs = {"Coef": relerr(coef.reshape(N + F, B, S), want_coef),
            "step": relerr(step.reshape(S, B), form.step(c["Xs"])),
            "traj": relerr(traj.reshape(H + 1, S, nx), form.rollout(c["x0"], c["U"], c["lin"], c["coord"], (c["in"][0], c["in"][1])))}
    for k, e in errs.items():
        print(f"from C: {k} {e:.2e} (bar 1e-08)")
    for k, e in errs.items():
        assert e < 1e-8, (k, e)
