"""The per-axis gradient composite from a plain C caller: tests/c_abi/axis_jac.c (gcc, linked with libgpk.so and the HIP runtime,
its own process) drives gpk_fit_batched -> gpk_predict_batched_grad on case `csv` of tests/golden/axis_jac_ref.npz - the scaled
inputs and targets go in, the scalers' chain rule is applied here - at M = 25 (one call: gpk_predict_host_multi_grad) and M = 72
(the panel route: gpk_predict_mean_grad_multi + one variance-gradient chain per model), against the fixture at the fp64 bar,
per input column."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, relerr
from test_gpu_c_abi import _compile

pytestmark = pytest.mark.gpu

FP64_BAR = 1e-8


def colrel(a, b):
    D = b.shape[-1]
    a, b = np.asarray(a).reshape(-1, D), np.asarray(b).reshape(-1, D)
    return float(np.max(np.max(np.abs(a - b), axis=0) / np.maximum(np.max(np.abs(b), axis=0), 1e-300)))


def _raw(mean, var, dmean, dvar, ref):
    """The chain rule through the scalers: mean, std, J, dstd in raw units from the composite's target-unit outputs."""
    sxs, sym, sys_ = ref["csv_sx_scale"], ref["csv_sy_mean"], ref["csv_sy_scale"]
    m = mean * sys_[None, :] + sym[None, :]
    J = dmean * sys_[None, :, None] / sxs[None, None, :]
    if var is None:
        return m, J
    sig = np.sqrt(var)
    assert (sig > 0).all()
    std = np.abs(sig * sys_[None, :])
    dstd = np.abs(sys_)[None, :, None] * dvar / (2.0 * sig[:, :, None]) / sxs[None, None, :]
    return m, J, std, dstd


def test_batched_grad_from_c(tmp_path, csv_data):
    d = np.load(os.path.join(GOLDEN, "axis_jac_ref.npz"))
    ref = {k: d[k] for k in d.files}
    exe = _compile(tmp_path, "axis_jac.c")
    X, Y, Xq = csv_data["X10"], csv_data["Y6"], ref["csv_Xq"]
    N, D, B, M, Ms = len(X), X.shape[1], Y.shape[1], len(Xq), 25
    Xs = (X - ref["csv_sx_mean"]) / ref["csv_sx_scale"]
    Ys = (Y - ref["csv_sy_mean"]) / ref["csv_sy_scale"]
    Z = (Xq - ref["csv_sx_mean"]) / ref["csv_sx_scale"]
    src, dst = str(tmp_path / "problem.bin"), str(tmp_path / "result.bin")
    np.concatenate([np.array([N, D, B, M, Ms, 1e-6]), Xs.ravel(), Ys.ravel(), ref["csv_ls"].ravel(), ref["csv_noise"].ravel(),
                    Z.ravel()]).tofile(src)
    env = dict(os.environ, GPK_DEBUG_FILL="nan")
    r = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout
    assert "C ABI axis jac: OK" in r.stdout
    out = np.fromfile(dst)
    assert np.isfinite(out).all()

    def take(o, rows, with_var):
        nm, nj = rows * B, rows * B * D
        mean = out[o:o + nm].reshape(rows, B)
        o += nm
        var = None
        if with_var:
            var = out[o:o + nm].reshape(rows, B)
            o += nm
        dmean = out[o:o + nj].reshape(rows, B, D)
        o += nj
        dvar = None
        if with_var:
            dvar = out[o:o + nj].reshape(rows, B, D)
            o += nj
        return o, (mean, var, dmean, dvar)

    o, large = take(0, M, True)
    o, small = take(o, Ms, True)
    o, small_mean = take(o, Ms, False)
    assert o == out.size
    for name, got, rows in (("M = 72", large, slice(None)), ("M = 25", small, slice(0, Ms))):
        m, J, std, dstd = _raw(*got, ref)
        e = (relerr(m, ref["csv_mean"][rows]), relerr(std, ref["csv_std"][rows]), colrel(J, ref["csv_J"][rows]),
             colrel(dstd, ref["csv_dstd"][rows]), colrel(got[3], ref["csv_dvar"][rows]))
        print(name, e)
        assert max(e) < FP64_BAR
    m, J = _raw(small_mean[0], None, small_mean[2], None, ref)
    assert relerr(m, ref["csv_mean"][:Ms]) < FP64_BAR and colrel(J, ref["csv_J"][:Ms]) < FP64_BAR
