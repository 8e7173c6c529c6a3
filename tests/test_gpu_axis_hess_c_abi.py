"""The per-axis Hessian composite from a plain C caller: tests/c_abi/axis_hess.c (gcc, linked with libgpk.so and the HIP runtime,
its own process) drives gpk_fit_batched -> gpk_predict_batched_hess on case `axis` of tests/golden/hess_ref.npz - the scaled inputs
and targets go in - at M = 25 (one call: gpk_predict_host_multi_hess) and M = 40 (the panel route: the fused mean, Jacobian and
Hessian launches), against the fixture's Hessians on the scaled inputs at the fp64 bar."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, relerr
from test_gpu_c_abi import _compile

pytestmark = pytest.mark.gpu

FP64_BAR = 1e-8
ROUTE_BAR = 1e-11


def test_batched_hess_from_c(tmp_path, csv_data):
    d = np.load(os.path.join(GOLDEN, "hess_ref.npz"))
    ref = {k: d[k] for k in d.files}
    exe = _compile(tmp_path, "axis_hess.c")
    X, Y = csv_data["X10"], csv_data["Y6"]
    Xq = np.vstack([ref["axis_Xq"], X[100:115]])          # the fixture's 25 rows, then 15 training rows: M = 40
    N, D, B, M, Ms = len(X), X.shape[1], Y.shape[1], len(Xq), 25
    Xs = (X - ref["axis_sx_mean"]) / ref["axis_sx_scale"]
    Ys = (Y - ref["axis_sy_mean"]) / ref["axis_sy_scale"]
    Z = (Xq - ref["axis_sx_mean"]) / ref["axis_sx_scale"]
    src, dst = str(tmp_path / "problem.bin"), str(tmp_path / "result.bin")
    np.concatenate([np.array([N, D, B, M, Ms, 1e-6]), Xs.ravel(), Ys.ravel(), ref["axis_ls"].ravel(), ref["axis_noise"].ravel(),
                    Z.ravel()]).tofile(src)
    env = dict(os.environ, GPK_DEBUG_FILL="nan")
    r = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout
    assert "C ABI axis hess: OK" in r.stdout
    out = np.fromfile(dst)
    per = B + B * D + B * D * D
    assert out.size == (M + Ms) * per and np.isfinite(out).all()
    large = out[M * (B + B * D):M * per].reshape(M, B, D, D)
    small = out[M * per + Ms * (B + B * D):].reshape(Ms, B, D, D)
    for name, H in (("M = 40", large), ("M = 25", small)):
        assert np.array_equal(H, H.swapaxes(-1, -2)), name
        e = relerr(H[:Ms], ref["axis_hess_scaled"])
        print(name, e)
        assert e < FP64_BAR
    assert relerr(large[:Ms], small) < ROUTE_BAR
