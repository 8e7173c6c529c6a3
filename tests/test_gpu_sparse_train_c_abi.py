"""The training entries of the sparse inducing-point GP from a plain C caller: tests/c_abi/sparse_train.c (gcc, linked with
libgpk.so and the HIP runtime, its own process) runs gpk_sparse_begin -> gpk_sparse_hold -> gpk_sparse_eval on case A of
tests/golden/sparse_train_ref.npz; bound and gradient are compared here with the fixture at the fp64 bar.  The C program itself
checks that evaluations reproduce their bits, that gpk_sparse_update releases the held rows (the next gpk_sparse_eval is
refused with a message) and the status of every bad-argument call."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, relerr
from test_gpu_c_abi import _compile

pytestmark = pytest.mark.gpu

FP64_BAR = 1e-8


def test_sparse_train_from_c(tmp_path):
    d = np.load(os.path.join(GOLDEN, "sparse_train_ref.npz"))
    ref = {k: d[k] for k in d.files}
    exe = _compile(tmp_path, "sparse_train.c")
    X, Y, Z = ref["A_X"], ref["A_Y"], ref["A_Z"]
    sf2, noise, alpha, jit = ref["A_hyper"]
    N, D, P, m = len(X), X.shape[1], Y.shape[1], len(Z)
    src, dst = str(tmp_path / "problem.bin"), str(tmp_path / "result.bin")
    np.concatenate([np.array([N, m, D, P, sf2, noise, alpha, jit]), X.ravel(), Y.ravel(), Z.ravel(), ref["A_ls"], ref["A_y_mean"],
                    ref["A_y_std"]]).tofile(src)
    env = dict(os.environ, GPK_DEBUG_FILL="nan")
    r = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout
    assert "C ABI sparse train: OK" in r.stdout
    out = np.fromfile(dst)
    assert out.size == D + 3 and np.isfinite(out).all()
    e = (abs(out[0] - float(ref["A_bound"])) / abs(float(ref["A_bound"])), relerr(out[1:], ref["A_grad"]))
    print("bound %.2e gradient %.2e of its largest component" % e)
    assert max(e) < FP64_BAR
