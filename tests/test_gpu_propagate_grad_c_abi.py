"""Gradient of a horizon cost through the propagation (K11) from a plain C caller in its own process
(tests/c_abi/propagate_grad.c): the four entries gpk_propagate_grad_host, gpk_propagate_grad_host_multi,
gpk_sparse_propagate_grad and gpk_sparse_propagate_grad_multi.  The exact pair runs on case b ((N, D, P) = (130, 4, 3), H = 5) and
on case csv ((200, 10, 6), H = 25) of tests/golden/paths_ref.npz with R = 5 - the single model, and the same outputs as P models
behind an input scaler; the sparse pair on `sparse_batch_problem` (B = 2, m = 60, n = 400, D = 10, coordinates (4, 1) of nx = 6,
both scalers, R = 3, H = 5; handle 0 alone on a state of one coordinate).  The C program checks, per entry, the bits of the
first-order sibling, repeatability, the NULL-able arguments, the symmetry of dSigma0 and that every refusal is GPK_BAD_ARG with
a message and leaves the outputs untouched; this side compares what it wrote with `adjoint_numpy_form`
(tests/test_propagate_grad_host.py) at the project's fp64 bar, 1e-8 of each array's largest component (measured <= 1.4e-13)."""
import subprocess

import numpy as np
import pytest

from conftest import relerr
from test_gpu_c_abi import _compile
from test_propagate_grad_host import adjoint_numpy_form, seeds
from test_propagate_host import gp_numpy_form, propagate_numpy_form, rollouts, single_form, spd, sparse_batch_problem, sparse_numpy_form

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ("b", "csv"))
def test_propagate_grad_from_c(tmp_path, name):
    from test_gpu_sparse_batch import ALPHA
    exe = _compile(tmp_path, "propagate_grad.c")
    c, form = single_form(name)
    g = form.gps[0]
    (N, D), P, R, H = c["X"].shape, c["Y"].shape[1], 5, len(c["U"])
    sf2, noise, alpha = c["hyper"]
    x0, U = rollouts(c["x0"][0], c["U"], R)
    S0, Q = spd(P)
    in_scaler = (0.05 * np.cos(np.arange(D)), 1.0 + 0.1 * np.sin(1.0 + np.arange(D)))
    Yn = (c["Y"] - g.ym) / g.ys
    exact = [np.array([N, D, P, R, H, sf2, noise, alpha]), np.broadcast_to(c["ls"], (D,)), g.ym, g.ys, c["X"], Yn, Yn.T, x0, U, c["lin"],
             S0, Q, *in_scaler]
    exact = np.concatenate([np.ascontiguousarray(p, dtype=np.float64).ravel() for p in exact])
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
    (gxe, gSe), (gxb, gSb), (gxs, gSs) = seeds(R, H, P), seeds(Rs, Hs, nx), seeds(Rs, Hs, 1)
    sparse += [gxe, gSe, gxb, gSb, gxs, gSs]
    sparse = np.concatenate([np.ascontiguousarray(p, dtype=np.float64).ravel() for p in sparse])
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate([np.array([float(exact.size)]), exact, sparse]).tofile(src)
    r = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=180)
    assert r.returncode == 0, r.stdout
    assert "propagate_grad from C: OK" in r.stdout
    out = np.fromfile(dst)
    multi = propagate_numpy_form([gp_numpy_form(c["X"], c["Y"][:, b], c["ls"], sf2, noise, alpha) for b in range(P)], None, in_scaler)
    single = propagate_numpy_form([sparse_numpy_form(ps[0], ALPHA)])
    at = 0
    for tag, (HH, RR, nxx, DD), want in (
            ("gpk_propagate_grad_host", (H, R, P, D), adjoint_numpy_form(form, x0, U, c["lin"], np.tile(S0, (R, 1, 1)), Q, True, gxe, gSe)),
            ("gpk_propagate_grad_host_multi", (H, R, P, D),
             adjoint_numpy_form(multi, x0, U, c["lin"], np.tile(S0, (R, 1, 1)), Q, True, gxe, gSe)),
            ("gpk_sparse_propagate_grad", (Hs, Rs, 1, Ds),
             adjoint_numpy_form(single, x0s, Us, lins, np.tile(S0s, (Rs, 1, 1)), Qs, True, gxs, gSs)),
            ("gpk_sparse_propagate_grad_multi", (Hs, Rs, nx, Ds),
             adjoint_numpy_form(sform, sx0, sU, cs["lin"], np.tile(sS0, (Rs, 1, 1)), sQ, False, gxb, gSb))):
        shapes = ((HH + 1, RR, nxx), (HH + 1, RR, nxx, nxx), (RR, HH, DD - nxx), (RR, nxx), (RR, nxx, nxx))
        for what, shape, b in zip(("traj", "Sigma", "dU", "dx0", "dSigma0"), shapes, want):
            size = int(np.prod(shape))
            a = out[at:at + size].reshape(shape)
            at += size
            e = relerr(a, b)
            print(f"from C, case {name}, {tag}: {what} {e:.2e} (bar 1e-08)")
            assert e < 1e-8, (tag, what, e)
    assert at == out.size
