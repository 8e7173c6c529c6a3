"""Horizon propagation (K11) from a plain C caller in its own process (tests/c_abi/propagate.c): the fit building blocks, then
gpk_propagate_host on case b of tests/test_gpu_paths.py, (N, D, P) = (130, 4, 3), R = 5 rollouts over H = 5 stages with an SPD
Sigma0 and a process noise, and gpk_propagate_host_multi on the same three outputs as single-output models behind an input scaler,
the noise level added through var_includes_noise.  The C program checks repeatability, NULL stage outputs, the symmetry of Sigma
and every bad-argument status; this side compares what it wrote with the dense NumPy form (`propagate_numpy_form`,
tests/test_propagate_host.py) at the project's fp64 bar, 1e-8 of each array's largest component."""
import subprocess

import numpy as np
import pytest

from conftest import relerr
from test_gpu_c_abi import _compile
from test_propagate_host import gp_numpy_form, propagate_numpy_form, rollouts, single_form, spd

pytestmark = pytest.mark.gpu


def test_propagate_from_c(tmp_path):
    exe = _compile(tmp_path, "propagate.c")
    c, form = single_form("b")
    g = form.gps[0]
    N, D, P, R, H = 130, 4, 3, 5, len(c["U"])
    sf2, noise, alpha = c["hyper"]
    x0, U = rollouts(c["x0"][0], c["U"], R)
    S0, Q = spd(P)
    in_scaler = (np.array([0.05, -0.1, 0.2, 0.0]), np.array([1.1, 0.9, 1.25, 0.8]))
    Yn = (c["Y"] - g.ym) / g.ys
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    parts = [np.array([N, D, P, R, H, sf2, noise, alpha]), c["ls"], g.ym, g.ys, c["X"], Yn, Yn.T, x0, U, c["lin"], S0, Q, *in_scaler]
    np.concatenate([np.ascontiguousarray(p, dtype=np.float64).ravel() for p in parts]).tofile(src)
    r = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "propagate from C: OK" in r.stdout
    out = np.fromfile(dst)
    shapes = ((H + 1, R, P), (H + 1, R, P, P), (H, R, P), (H, R, P), (H, R, P, D))
    sizes = [int(np.prod(s)) for s in shapes]
    assert out.size == 2 * sum(sizes)
    # the batch form reads every model through the scaled query: the same three outputs as models on the inputs X, queried at z
    multi = propagate_numpy_form([gp_numpy_form(c["X"], c["Y"][:, b], c["ls"], sf2, noise, alpha) for b in range(P)], None, in_scaler)
    S0R = np.tile(S0, (R, 1, 1))
    for tag, block, want in (("gpk_propagate_host", out[:sum(sizes)], form.run(x0, U, c["lin"], S0R, Q, noisy=True)),
                             ("gpk_propagate_host_multi", out[sum(sizes):], multi.run(x0, U, c["lin"], S0R, Q, noisy=True))):
        got = [block[sum(sizes[:i]):sum(sizes[:i + 1])].reshape(shapes[i]) for i in range(5)]
        wants = (want[0], want[1], want[2]["mean"], want[2]["var"], want[2]["jac"])
        for name, a, b in zip(("traj", "Sigma", "mean", "var", "jac"), got, wants):
            e = relerr(a, b)
            print(f"from C, {tag}: {name} {e:.2e} (bar 1e-08)")
            assert e < 1e-8, (tag, name, e)
