"""The composite Hessian call from a plain C caller: tests/c_abi/hess.c (gcc, linked with libgpk.so and the HIP runtime, its own
process) drives gpk_fit -> gpk_predict_model_hess on test_gpu_jac_c_abi.py's deterministic problem (N = 300, D = 4, P = 2,
M = 40, and again the first 7 rows) and writes mean / dmean / hess, which are compared with the Python route
(GaussianProcessRegressor.predict_hessian) to 1e-12."""
import os
import subprocess

import numpy as np
import pytest

from conftest import relerr
from test_gpu_c_abi import _compile

pytestmark = pytest.mark.gpu


def test_model_hess_from_c(tmp_path):
    from unmanned_aerial_vehicles_amd import RBF, GaussianProcessRegressor, WhiteKernel
    exe = _compile(tmp_path, "hess.c")
    N, D, P, M, MS = 300, 4, 2, 40, 7
    i = np.arange(N, dtype=np.float64)[:, None]
    X = np.sin(0.37 * i + 1.3 * np.arange(D)[None, :]) * (1.0 + 0.1 * np.arange(D)[None, :])
    Y = np.stack([np.cos(X @ np.array([0.7, -0.4, 0.2, 0.5])), np.sin(X[:, 0] * X[:, 1]) + 3.0], axis=1)
    j = np.arange(M, dtype=np.float64)[:, None]
    Xq = 0.9 * np.cos(0.53 * j + 0.9 * np.arange(D)[None, :])
    Xq[:3] = X[:3]
    ls, noise, jitter = 0.9, 0.03, 1e-6
    src, dst = str(tmp_path / "problem.bin"), str(tmp_path / "result.bin")
    np.concatenate([np.array([N, D, P, M, ls, noise, jitter]), X.ravel(), Y.ravel(), Xq.ravel()]).tofile(src)
    env = dict(os.environ, GPK_DEBUG_FILL="nan")
    r = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout
    assert "C ABI hess: OK" in r.stdout
    out = np.fromfile(dst)
    per = P + P * D + P * D * D
    assert out.size == (M + MS) * per and np.isfinite(out).all()
    gp = GaussianProcessRegressor(kernel=RBF(ls) + WhiteKernel(noise), alpha=jitter, normalize_y=True, optimizer=None,
                                  device=0).fit(X, Y)
    at = 0
    for rows in (M, MS):
        mean = out[at:at + rows * P].reshape(rows, P)
        dmean = out[at + rows * P:at + rows * (P + P * D)].reshape(rows, P, D)
        hess = out[at + rows * (P + P * D):at + rows * per].reshape(rows, P, D, D)
        at += rows * per
        pm, pdm, ph = gp.predict_hessian(Xq[:rows])
        errs = (relerr(mean, pm), relerr(dmean, pdm), relerr(hess, ph))
        print(rows, errs)
        assert max(errs) < 1e-12
        assert np.array_equal(hess, hess.swapaxes(-1, -2))
