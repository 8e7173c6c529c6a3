"""Path gradients (K10) from a plain C caller in its own process (tests/c_abi/paths_grad.c): gpk_paths_prepare ->
gpk_paths_step_grad -> gpk_paths_rollout_grad on case b of tests/test_gpu_paths.py, (N, D, F, S, P) = (130, 4, 64, 70, 3), and
gpk_paths_step_multi_grad on case b of tests/test_gpu_axis_paths.py, (N, D, F, S, B) = (130, 4, 64, 70, 3), whose model-major
Coef - written here from the dense NumPy form, mstride = 72, ldc = 3 * 72 + 3, NaN in the padding and pitch columns - is pitched.
The C program checks the statuses, that out / traj have the bytes of the plain entries, repeatability and the refusal of a null
jac; this side compares the Jacobians it wrote with the closed form in NumPy at the fp64 bar, 1e-8 of the largest component."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, relerr
from test_gpu_axis_paths import axis_paths_numpy_form, load_case
from test_gpu_c_abi import _compile
from test_gpu_paths import paths_numpy_form
from test_gpu_paths_grad import axis_jac_numpy_form, jac_numpy_form, rollout_jac_numpy_form

pytestmark = pytest.mark.gpu


def test_path_gradients_from_c(tmp_path):
    exe = _compile(tmp_path, "paths_grad.c")
    d = np.load(os.path.join(GOLDEN, "paths_ref.npz"))
    c = {k[2:]: d[k] for k in d.files if k.startswith("b_")}
    N, D, F, S, P, H = 130, 4, 64, 70, 3, len(c["U"])
    C = S * P
    sf2, noise, alpha = c["hyper"]
    form = paths_numpy_form(c["X"], c["Y"], c["ls"], sf2, noise, alpha, c["omega"], c["phase"], c["weights"], c["eps"])
    parts = [np.array([N, D, F, S, P, H, sf2, noise + alpha]), c["ls"], form.ym, form.ys, c["X"], form.Yn, c["omega"], c["phase"],
             c["weights"].reshape(F, C), c["eps"].reshape(N, C), c["Xs"], c["x0"], c["U"], c["lin"]]
    # the batch: its coefficient matrix from the NumPy form, model-major and pitched
    a = load_case("b")
    B, N2, D2, F2, S2 = len(a["ls"]), len(a["X"]), a["X"].shape[1], a["omega"].shape[1], a["weights"].shape[2]
    aform = axis_paths_numpy_form(a["X"], a["Y"], a["ls"], a["hyper"], a["omega"], a["phase"], a["weights"], a["eps"], a["out"])
    mstride = (S2 + 7) // 8 * 8
    ldc2 = B * mstride + 3
    assert mstride > S2
    coef = np.full((N2 + F2, ldc2), np.nan)
    for b, fb in enumerate(aform.forms):
        coef[:N2, b * mstride:b * mstride + S2] = fb.V[:, :, 0]
        coef[N2:, b * mstride:b * mstride + S2] = fb.Ww[:, :, 0]
    shift = np.array([aform.out_mean[b] + aform.out_scale[b] * fb.ym[0] for b, fb in enumerate(aform.forms)])
    scale = np.array([aform.out_scale[b] * fb.ys[0] for b, fb in enumerate(aform.forms)])
    parts += [np.array([N2, D2, F2, S2, B, mstride, ldc2]), a["ls"], a["hyper"][:, 0], shift, scale, a["X"], a["omega"], a["phase"],
              coef, a["Xs"]]
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in parts]).tofile(src)
    r = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "path gradients from C: OK" in r.stdout
    out = np.fromfile(dst)
    sizes = (C * D, H * C * D, S2 * B * D2)
    assert out.size == sum(sizes)
    jac, rjac, mjac = (out[sum(sizes[:i]):sum(sizes[:i + 1])] for i in range(3))
    traj = form.rollout(c["x0"], c["U"], c["lin"])
    errs = {"step jac": relerr(jac.reshape(S, P, D), jac_numpy_form(form, c["Xs"])),
            "rollout jac": relerr(rjac.reshape(H, S, P, D), rollout_jac_numpy_form(form, traj, c["U"])),
            "batch step jac": relerr(mjac.reshape(S2, B, D2), axis_jac_numpy_form(aform, a["Xs"]))}
    for k, e in errs.items():
        print(f"from C: {k} {e:.2e} (bar 1e-08)")
    for k, e in errs.items():
        assert e < 1e-8, (k, e)
