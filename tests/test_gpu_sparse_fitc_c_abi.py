"""The FITC sparse GP from a plain C caller: tests/c_abi/sparse_fitc.c (gcc, linked with libgpk.so and the HIP runtime, its own
process) runs gpk_sparse_begin -> set_approximation -> update x 2 -> finalize -> predict -> bound -> export / get_approximation and
imports the statistics and the kind into a second handle, on case A of tests/golden/sparse_fitc_ref.npz (inputs: sparse_ref.npz);
the results are compared here with the fixture at the fp64 bar.  The C program itself checks that the importing handle reproduces
the bits, and the refusals of the new entries."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, relerr
from test_gpu_c_abi import _compile

pytestmark = pytest.mark.gpu

FP64_BAR = 1e-8


def test_sparse_fitc_from_c(tmp_path):
    d = np.load(os.path.join(GOLDEN, "sparse_ref.npz"))
    ref = {k: d[k] for k in d.files}
    d = np.load(os.path.join(GOLDEN, "sparse_fitc_ref.npz"))
    fit = {k: d[k] for k in d.files}
    exe = _compile(tmp_path, "sparse_fitc.c")
    X, Y, Z, Xq = ref["A_X"], ref["A_Y"], ref["A_Z"], ref["A_Xq"]
    sf2, noise, alpha, jit = ref["A_hyper"]
    N, D, P, m, M, Ms = len(X), X.shape[1], Y.shape[1], len(Z), len(Xq), 25
    src, dst = str(tmp_path / "problem.bin"), str(tmp_path / "result.bin")
    np.concatenate([np.array([N, m, D, P, M, Ms, 300, sf2, noise, alpha, jit]), X.ravel(), Y.ravel(), Z.ravel(), Xq.ravel(),
                    ref["A_ls"], ref["A_y_mean"], ref["A_y_std"]]).tofile(src)
    env = dict(os.environ, GPK_DEBUG_FILL="nan")
    r = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout
    assert "C ABI sparse FITC: OK" in r.stdout
    out = np.fromfile(dst)
    assert np.isfinite(out).all() and out.size == 2 * M * P + 2 * Ms * P + 2 + m * m + m * P + P
    o = 0

    def take(*shape):
        nonlocal o
        n = int(np.prod(shape))
        a = out[o:o + n].reshape(shape)
        o += n
        return a

    mean, var, smean, svar = take(M, P), take(M, P), take(Ms, P), take(Ms, P)
    lik, loglam, G, g, yy = take(1)[0], take(1)[0], take(m, m), take(m, P), take(P)
    # var_includes_noise = 0: the latent variance (floored at 1e-10) times y_std^2
    want_var = fit["A_var"][:, None] * ref["A_y_std"][None, :] ** 2
    e = (relerr(mean, fit["A_mean"]), relerr(var, want_var), relerr(smean, fit["A_mean"][:Ms]), relerr(svar, want_var[:Ms]),
         abs(lik - float(fit["A_lik"])) / abs(float(fit["A_lik"])))
    print("mean %.2e var %.2e small mean %.2e small var %.2e likelihood %.2e" % e)
    assert max(e) < FP64_BAR
    e = (relerr(G, fit["A_G"]), relerr(g, fit["A_g"]), relerr(yy, fit["A_yy"]), abs(loglam - float(fit["A_loglam"])) / abs(float(fit["A_loglam"])))
    print("G %.2e g %.2e yy %.2e sum log lambda %.2e" % e)
    assert max(e) < FP64_BAR
