"""The per-axis covariance composite from a plain C caller: tests/c_abi/axis_cov.c (gcc, linked with libgpk.so and the HIP
runtime, its own process) drives gpk_fit_batched -> gpk_predict_batched_cov on case `csv` of tests/golden/axis_cov_ref.npz - the
scaled inputs and targets go in, the target scalers are applied here - at 25 rows (one call: gpk_predict_host_multi_cov) and 72
rows (the fused mean + one gpk_predict_cov_inv per model), against scikit-learn's return_cov at the fp64 bar.  The C program
itself checks the bit-for-bit symmetry, the repeatability and the refusals of both entries."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN
from test_gpu_c_abi import _compile

pytestmark = pytest.mark.gpu

FP64_BAR = 1e-8


def blockrel(a, b):
    ax = tuple(range(b.ndim - 1))
    return float(np.max(np.max(np.abs(a - b), axis=ax) / np.max(np.abs(b), axis=ax)))


def test_batched_cov_from_c(tmp_path, csv_data):
    d = np.load(os.path.join(GOLDEN, "axis_cov_ref.npz"))
    ref = {k: d[k] for k in d.files}
    exe = _compile(tmp_path, "axis_cov.c")
    X, Y = csv_data["X10"], csv_data["Y6"]
    N, D, B, M, Ms = len(X), X.shape[1], Y.shape[1], 72, 25
    Xs = (X - ref["csv_sx_mean"]) / ref["csv_sx_scale"]
    Ys = (Y - ref["csv_sy_mean"]) / ref["csv_sy_scale"]
    Z72 = (ref["csv_Xq72"] - ref["csv_sx_mean"]) / ref["csv_sx_scale"]
    Z25 = (ref["csv_Xq"] - ref["csv_sx_mean"]) / ref["csv_sx_scale"]
    src, dst = str(tmp_path / "problem.bin"), str(tmp_path / "result.bin")
    np.concatenate([np.array([N, D, B, M, Ms, 1e-6]), Xs.ravel(), Ys.ravel(), ref["csv_ls"].ravel(), ref["csv_noise"].ravel(),
                    Z72.ravel(), Z25.ravel()]).tofile(src)
    env = dict(os.environ, GPK_DEBUG_FILL="nan")
    r = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout
    assert "C ABI axis cov: OK" in r.stdout
    out = np.fromfile(dst)
    assert np.isfinite(out).all() and out.size == M * B + B * M * M + Ms * B + B * Ms * Ms
    o = 0
    for rows, name in ((M, "72"), (Ms, "")):
        mean = out[o:o + rows * B].reshape(rows, B)
        o += rows * B
        cov = out[o:o + B * rows * rows].reshape(B, rows, rows).transpose(1, 2, 0)
        o += B * rows * rows
        mean = mean * ref["csv_sy_scale"] + ref["csv_sy_mean"]
        cov = cov * ref["csv_sy_scale"] ** 2
        e = (blockrel(mean, ref["csv_mean" + name]), blockrel(cov, ref["csv_cov" + name]))
        print(f"{rows} rows: mean {e[0]:.2e} cov {e[1]:.2e}")
        assert max(e) < FP64_BAR
        for b in range(B):
            assert np.array_equal(cov[..., b], cov[..., b].T)
