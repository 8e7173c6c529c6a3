"""gpk_sparse_propagate / gpk_sparse_propagate_multi from a plain C caller in its own process (tests/c_abi/sparse_propagate.c):
two handles, each begin -> update -> finalize on the models of `sparse_batch_problem` (tests/test_propagate_host.py: B = 2, m = 60,
n = 400, D = 10, coordinates (4, 1) of nx = 6, both scalers), then the batch entry with latent variances on R = 3 rollouts over
H = 5 stages with an SPD Sigma0 and a process noise, and the single entry on handle 0 - a state of one coordinate, nine controls, the
noise level included.  The C program checks repeatability, NULL stage outputs, the symmetry of Sigma, stage 0 against
gpk_sparse_predict_grad bit for bit and every bad-argument status; this side compares what it wrote with the dense NumPy form
(`propagate_numpy_form`) at the project's fp64 bar, 1e-8 of each array's largest component (the room under it:
tests/test_sparse_propagate_host.py, problem batch2; the single horizon carries the noise level, so no clip is near)."""
import subprocess

import numpy as np
import pytest

from conftest import relerr
from test_gpu_c_abi import _compile
from test_propagate_host import propagate_numpy_form, rollouts, spd, sparse_batch_problem, sparse_numpy_form

pytestmark = pytest.mark.gpu


def test_sparse_propagate_from_c(tmp_path):
    from test_gpu_sparse_batch import ALPHA
    exe = _compile(tmp_path, "sparse_propagate.c")
    c, form = sparse_batch_problem()
    ps = c["ps"]
    B, n, m, D, R, H, nx = 2, 400, 60, 10, 3, 5, 6
    x0, U = rollouts(c["x0"][0], c["U"], R)
    S0, Q = spd(nx)
    rng = np.random.default_rng(4711)
    x0s, Us = rollouts(0.3 * rng.standard_normal(1), 0.4 * rng.standard_normal((H, D - 1)), R)
    lins = 0.05 * rng.standard_normal((1, D))
    S0s, Qs = spd(1)
    parts = [np.array([B, n, m, D, R, H, nx], dtype=np.float64)]
    for p in ps:
        parts += [p["X"].ravel(), p["y"], p["Z"].ravel(), p["ls"],
                  np.array([p["sf2"], p["noise"], ALPHA, 1e-8 * p["sf2"], p["ym"], p["ys"]])]
    parts += [c["coord"].astype(np.float64), c["in"][0], c["in"][1], c["out"][0], c["out"][1], x0, U, c["lin"], S0, Q, x0s, Us, lins,
              S0s, Qs]
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate([np.ascontiguousarray(p, dtype=np.float64).ravel() for p in parts]).tofile(src)
    r = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "sparse propagate from C: OK" in r.stdout
    out = np.fromfile(dst)
    single = propagate_numpy_form([sparse_numpy_form(ps[0], ALPHA)])
    at = 0
    for tag, (nxx, NO), want in (("gpk_sparse_propagate_multi", (nx, B), form.run(x0, U, c["lin"], np.tile(S0, (R, 1, 1)), Q, noisy=False)),
                                 ("gpk_sparse_propagate", (1, 1), single.run(x0s, Us, lins, np.tile(S0s, (R, 1, 1)), Qs, noisy=True))):
        shapes = ((H + 1, R, nxx), (H + 1, R, nxx, nxx), (H, R, NO), (H, R, NO), (H, R, NO, D))
        wants = (want[0], want[1], want[2]["mean"], want[2]["var"], want[2]["jac"])
        for name, shape, b in zip(("traj", "Sigma", "mean", "var", "jac"), shapes, wants):
            size = int(np.prod(shape))
            a = out[at:at + size].reshape(shape)
            at += size
            e = relerr(a, b)
            print(f"from C, {tag}: {name} {e:.2e} (bar 1e-08)")
            assert e < 1e-8, (tag, name, e)
    assert at == out.size
