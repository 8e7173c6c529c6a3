"""Second-order horizon propagation (K11, order = 2) from a plain C caller in its own process (tests/c_abi/propagate2.c): the four
entries gpk_propagate2_host, gpk_propagate2_host_multi, gpk_sparse_propagate2 and gpk_sparse_propagate2_multi on the problems of
tests/test_gpu_propagate_c_abi.py (case b: (N, D, P) = (130, 4, 3), R = 5, H = 5; the same outputs as three models behind an input
scaler) and tests/test_gpu_sparse_propagate_c_abi.py (`sparse_batch_problem`: B = 2, m = 60, n = 400, D = 10, coordinates (4, 1)
of nx = 6, both scalers, R = 3, H = 5; handle 0 alone on a state of one coordinate).  The C program checks, per entry, that
order = 1 has the bits of the first-order sibling and leaves corr zero, repeatability, NULL outputs, the symmetry of Sigma, the
bits of a one-stage horizon and the refusals; this side compares what it wrote with `propagate2_numpy_form`
(tests/test_propagate2_host.py) at the project's fp64 bar, 1e-8 of each array's largest component."""
import subprocess

import numpy as np
import pytest

from conftest import relerr
from test_gpu_c_abi import _compile
from test_propagate2_host import propagate2_numpy_form, second
from test_propagate_host import gp_numpy_form, rollouts, single_form, spd, sparse_batch_problem, sparse_numpy_form

pytestmark = pytest.mark.gpu


def test_propagate2_from_c(tmp_path):
    from test_gpu_sparse_batch import ALPHA
    exe = _compile(tmp_path, "propagate2.c")
    # the exact part: tests/test_gpu_propagate_c_abi.py's file
    c, form = single_form("b")
    g = form.gps[0]
    N, D, P, R, H = 130, 4, 3, 5, len(c["U"])
    sf2, noise, alpha = c["hyper"]
    x0, U = rollouts(c["x0"][0], c["U"], R)
    S0, Q = spd(P)
    in_scaler = (np.array([0.05, -0.1, 0.2, 0.0]), np.array([1.1, 0.9, 1.25, 0.8]))
    Yn = (c["Y"] - g.ym) / g.ys
    exact = [np.array([N, D, P, R, H, sf2, noise, alpha]), c["ls"], g.ym, g.ys, c["X"], Yn, Yn.T, x0, U, c["lin"], S0, Q, *in_scaler]
    exact = np.concatenate([np.ascontiguousarray(p, dtype=np.float64).ravel() for p in exact])
    # the sparse part: tests/test_gpu_sparse_propagate_c_abi.py's file
    cs, sform = sparse_batch_problem()
    ps = cs["ps"]
    B, n, m, Ds, Rs, Hs, nx = 2, 400, 60, 10, 3, 5, 6
    sx0, sU = rollouts(cs["x0"][0], cs["U"], Rs)
    sS0, sQ = spd(nx)
    rng = np.random.default_rng(4711)
    x0s, Us = rollouts(0.3 * rng.standard_normal(1), 0.4 * rng.standard_normal((Hs, Ds - 1)), Rs)
    lins = 0.05 * rng.standard_normal((1, Ds))
    S0s, Qs = spd(1)
    sparse = [np.array([B, n, m, Ds, Rs, Hs, nx], dtype=np.float64)]
    for p in ps:
        sparse += [p["X"].ravel(), p["y"], p["Z"].ravel(), p["ls"], np.array([p["sf2"], p["noise"], ALPHA, 1e-8 * p["sf2"], p["ym"], p["ys"]])]
    sparse += [cs["coord"].astype(np.float64), cs["in"][0], cs["in"][1], cs["out"][0], cs["out"][1], sx0, sU, cs["lin"], sS0, sQ, x0s, Us,
               lins, S0s, Qs]
    sparse = np.concatenate([np.ascontiguousarray(p, dtype=np.float64).ravel() for p in sparse])
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate([np.array([float(exact.size)]), exact, sparse]).tofile(src)
    r = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=180)
    assert r.returncode == 0, r.stdout
    assert "propagate2 from C: OK" in r.stdout
    out = np.fromfile(dst)
    multi = propagate2_numpy_form([gp_numpy_form(c["X"], c["Y"][:, b], c["ls"], sf2, noise, alpha) for b in range(P)], None, in_scaler)
    single = propagate2_numpy_form([sparse_numpy_form(ps[0], ALPHA)])
    at = 0
    for tag, (HH, RR, nxx, NO, DD), want in (
            ("gpk_propagate2_host", (H, R, P, P, D), second(form).run2(x0, U, c["lin"], np.tile(S0, (R, 1, 1)), Q, noisy=True)),
            ("gpk_propagate2_host_multi", (H, R, P, P, D), multi.run2(x0, U, c["lin"], np.tile(S0, (R, 1, 1)), Q, noisy=True)),
            ("gpk_sparse_propagate2", (Hs, Rs, 1, 1, Ds), single.run2(x0s, Us, lins, np.tile(S0s, (Rs, 1, 1)), Qs, noisy=True)),
            ("gpk_sparse_propagate2_multi", (Hs, Rs, nx, B, Ds),
             second(sform).run2(sx0, sU, cs["lin"], np.tile(sS0, (Rs, 1, 1)), sQ, noisy=False))):
        shapes = ((HH + 1, RR, nxx), (HH + 1, RR, nxx, nxx), (HH, RR, NO), (HH, RR, NO), (HH, RR, NO, DD), (HH, RR, NO))
        wants = (want[0], want[1], want[2]["mean"], want[2]["var"], want[2]["jac"], want[2]["corr"])
        for name, shape, b in zip(("traj", "Sigma", "mean", "var", "jac", "corr"), shapes, wants):
            size = int(np.prod(shape))
            a = out[at:at + size].reshape(shape)
            at += size
            e = relerr(a, b)
            print(f"from C, {tag}: {name} {e:.2e} (bar 1e-08)")
            assert e < 1e-8, (tag, name, e)
    assert at == out.size
