"""The inducing-input entries of the sparse GP's training from a plain C caller: tests/c_abi/sparse_z.c (gcc, linked with
libgpk.so and the HIP runtime, its own process) runs gpk_sparse_begin -> gpk_sparse_hold -> gpk_sparse_eval_z on case A; bound
and gradient are compared here with tests/golden/sparse_train_ref.npz at the fp64 bar and dL/dZ with
tests/golden/sparse_z_ref.npz at the bar of tests/test_gpu_sparse_z.py.  The C program itself checks that evaluations reproduce
their bits, that Z == NULL is gpk_sparse_eval bit for bit, that gpk_sparse_export returns the Z given, and the status of every
bad-argument call (a Z that is not finite, no held rows)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, relerr
from test_gpu_c_abi import _compile

pytestmark = pytest.mark.gpu

FP64_BAR = 1e-8


def test_sparse_z_from_c(tmp_path):
    d = np.load(os.path.join(GOLDEN, "sparse_train_ref.npz"))
    ref = {k: d[k] for k in d.files}
    zref = np.load(os.path.join(GOLDEN, "sparse_z_ref.npz"))
    exe = _compile(tmp_path, "sparse_z.c")
    X, Y, Z = ref["A_X"], ref["A_Y"], ref["A_Z"]
    sf2, noise, alpha, jit = ref["A_hyper"]
    N, D, P, m = len(X), X.shape[1], Y.shape[1], len(Z)
    src, dst = str(tmp_path / "problem.bin"), str(tmp_path / "result.bin")
    np.concatenate([np.array([N, m, D, P, sf2, noise, alpha, jit]), X.ravel(), Y.ravel(), Z.ravel(), ref["A_ls"], ref["A_y_mean"],
                    ref["A_y_std"]]).tofile(src)
    env = dict(os.environ, GPK_DEBUG_FILL="nan")
    r = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout
    assert "C ABI sparse Z: OK" in r.stdout
    out = np.fromfile(dst)
    assert out.size == D + 3 + m * D and np.isfinite(out).all()
    gZ = out[D + 3:].reshape(m, D)
    bar = max(FP64_BAR, 10.0 * float(zref["A_gradZ_agree"][0]))
    e = (abs(out[0] - float(ref["A_bound"])) / abs(float(ref["A_bound"])), relerr(out[1:D + 3], ref["A_grad"]), relerr(gZ, zref["A_gradZ"]))
    print("bound %.2e gradient %.2e dL/dZ %.2e of its largest component (bar %.1e)" % (e + (bar,)))
    assert max(e[:2]) < FP64_BAR and e[2] < bar
