"""The composite gradient call from a plain C caller: tests/c_abi/jac.c (gcc, linked with libgpk.so and the HIP runtime, its
own process) drives gpk_fit -> gpk_predict_model_grad on a small deterministic problem and writes mean / var / dmean / dvar,
which are compared with the Python route (GaussianProcessRegressor.predict_jacobian) to 1e-12."""
import os
import subprocess

import numpy as np
import pytest

from conftest import relerr
from test_gpu_c_abi import _compile

pytestmark = pytest.mark.gpu


def test_model_grad_from_c(tmp_path):
    from unmanned_aerial_vehicles_amd import RBF, GaussianProcessRegressor, WhiteKernel
    exe = _compile(tmp_path, "jac.c")
    N, D, P, M = 300, 4, 2, 40
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
    assert "C ABI jac: OK" in r.stdout
    out = np.fromfile(dst)
    nm, nj = M * P, M * P * D
    assert out.size == 3 * nm + 3 * nj and np.isfinite(out).all()
    mean, var = out[:nm].reshape(M, P), out[nm:2 * nm].reshape(M, P)
    dmean, dvar = out[2 * nm:2 * nm + nj].reshape(M, P, D), out[2 * nm + nj:2 * nm + 2 * nj].reshape(M, P, D)
    mean2, dmean2 = out[2 * nm + 2 * nj:3 * nm + 2 * nj].reshape(M, P), out[3 * nm + 2 * nj:].reshape(M, P, D)
    gp = GaussianProcessRegressor(kernel=RBF(ls) + WhiteKernel(noise), alpha=jitter, normalize_y=True, optimizer=None,
                                  device=0).fit(X, Y)
    pm, pdm, pv, pdv = gp.predict_jacobian(Xq, return_var=True)
    errs = (relerr(mean, pm), relerr(var, pv), relerr(dmean, pdm), relerr(dvar, pdv), relerr(mean2, pm), relerr(dmean2, pdm))
    print(errs)
    assert max(errs) < 1e-12
