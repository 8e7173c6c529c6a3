"""Greedy selection of inducing inputs from a plain C caller: tests/c_abi/sparse_select.c (gcc, linked with libgpk.so and the
HIP runtime, its own process) runs gpk_sparse_begin -> gpk_sparse_hold -> gpk_sparse_select(X = NULL) on the (600, 2) case of
tests/golden/sparse_select_ref.npz; indices and trace are compared here with the fixture as tests/test_gpu_sparse_select.py
compares them.  The C program itself checks that a second call and host rows give the same bits, and the status of every bad call
(no held rows, m_max > n, a non-finite row, batched mode)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN
from test_gpu_c_abi import _compile

pytestmark = pytest.mark.gpu

TRACE_BAR, DMAX_BAR = 1e-10, 1e-10      # of n sf2 / of sf2: two orders over the recursion's rounding bound (the fixture's writer)


def test_sparse_select_from_c(tmp_path):
    d = np.load(os.path.join(GOLDEN, "sparse_select_ref.npz"))
    X, ls, sf2 = d["A_X"], d["A_ls"], float(d["sf2"])
    n, D, m = X.shape[0], X.shape[1], len(d["A_idx"])
    exe = _compile(tmp_path, "sparse_select.c")
    src, dst = str(tmp_path / "problem.bin"), str(tmp_path / "result.bin")
    np.concatenate([np.array([n, D, m, sf2]), X.ravel(), ls]).tofile(src)
    env = dict(os.environ, GPK_DEBUG_FILL="nan")
    r = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout
    assert "C ABI sparse select: OK" in r.stdout
    out = np.fromfile(dst)
    assert out.size == 1 + 3 * m and np.isfinite(out).all()
    assert int(out[0]) == m
    idx, trace, dmax = out[1:1 + m].astype(np.int64), out[1 + m:1 + 2 * m], out[1 + 2 * m:]
    assert np.array_equal(idx, d["A_idx"])
    e = (np.max(np.abs(trace - d["A_trace"])) / (n * sf2), np.max(np.abs(dmax - d["A_dmax"])) / sf2)
    print("trace %.2e of n sf2, dmax %.2e of sf2" % e)
    assert e[0] < TRACE_BAR and e[1] < DMAX_BAR
