"""gpk_sparse_moments_vjp[_multi] and gpk_sparse_propagate_mm_grad[_multi] from a plain C caller in its own process
(tests/c_abi/sparse_moments_grad.c): two handles, each begin -> update -> finalize on the models of `sparse_batch_problem`
(tests/test_propagate_host.py: B = 2, m = 60, n = 400, D = 10, coordinates (4, 1) of nx = 6, both scalers), then the batch entries
with latent variances on R = 5 Gaussian queries / rollouts over H = 4 stages with an SPD Sigma0 and a process noise, and the single
entries on handle 0 - a state of one coordinate, nine controls, the noise level included.  The C program checks the bits of the
forward entries, repeatability, NULL seeds and optional outputs, the sweep without the tape, and every bad-argument status with its
outputs untouched; this side compares what it wrote with the dense NumPy adjoint (`moments_vjp_numpy_form` on
`sparse_moments_numpy_form`) at the project's fp64 bar, 1e-8 of each array's largest component (the room under it:
tests/test_sparse_moments_grad_host.py, problem batch2)."""
import subprocess

import numpy as np
import pytest

from conftest import relerr
from test_gpu_c_abi import _compile
from test_moments_grad_host import horizon_seeds, moments_vjp_numpy_form, seeds
from test_propagate_host import rollouts, spd, sparse_batch_problem
from test_sparse_moments_host import model_defs, sparse_form, sparse_moments_numpy_form

pytestmark = pytest.mark.gpu


def test_sparse_moments_gradient_from_c(tmp_path):
    from test_gpu_sparse_batch import ALPHA
    exe = _compile(tmp_path, "sparse_moments_grad.c")
    c, _ = sparse_batch_problem()
    ps = c["ps"]
    B, n, m, D, R, H, nx = 2, 400, 60, 10, 5, 4, 6
    x0, U = rollouts(c["x0"][0], c["U"][:H], R)
    S0, Q = spd(nx)
    S0 = 0.05 * S0
    rng = np.random.default_rng(4711)
    x0s, Us = rollouts(0.3 * rng.standard_normal(1), 0.4 * rng.standard_normal((H, D - 1)), R)
    lins = 0.05 * rng.standard_normal((1, D))
    S0s, Qs = spd(1)
    gm, gc, gxc = seeds(R, B, D)
    gx, gS = horizon_seeds(H, R, nx)
    gms, gcs, gxcs = seeds(R, 1, D, seed=11)
    gxs, gSs = horizon_seeds(H, R, 1, seed=13)
    parts = [np.array([B, n, m, D, R, H, nx], dtype=np.float64)]
    for p in ps:
        parts += [p["X"].ravel(), p["y"], p["Z"].ravel(), p["ls"],
                  np.array([p["sf2"], p["noise"], ALPHA, 1e-8 * p["sf2"], p["ym"], p["ys"]])]
    parts += [c["coord"].astype(np.float64), c["in"][0], c["in"][1], c["out"][0], c["out"][1], x0, U, c["lin"], S0, Q, x0s, Us, lins,
              S0s, Qs, gm, gc, gxc, gx, gS, gms, gcs, gxcs, gxs, gSs]
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate([np.ascontiguousarray(p, dtype=np.float64).ravel() for p in parts]).tofile(src)
    r = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "sparse moments gradient from C: OK" in r.stdout
    out = np.fromfile(dst)
    multi = sparse_form("batch2")
    single = sparse_moments_numpy_form(model_defs("batch2")[0][:1])
    at = 0
    for tag, form, nxx, coord, q0, u, l, s0, qn, noisy, sd, hsd in (
            ("the batch entries", multi, nx, list(c["coord"]), x0, U, c["lin"], S0, Q, False, (gm, gc, gxc), (gx, gS)),
            ("the single entries", single, 1, [0], x0s, Us, lins, S0s, Qs, True, (gms, gcs, gxcs), (gxs, gSs))):
        v = moments_vjp_numpy_form(form)
        SR = np.tile(s0, (R, 1, 1))
        Xq = np.concatenate([q0, u[:, 0]], axis=1)
        wants = v.batch(Xq, SR, noisy, *sd) + tuple(v.horizon(coord, q0, u, l, SR, qn, *hsd, noisy))
        shapes = ((R, D), (R, nxx, nxx), (H + 1, R, nxx), (H + 1, R, nxx, nxx), (R, H, D - nxx), (R, nxx), (R, nxx, nxx))
        names = ("dXq", "dSq", "traj", "Sigma", "dU", "dx0", "dSigma0")
        for name, shape, b in zip(names, shapes, wants):
            size = int(np.prod(shape))
            a = out[at:at + size].reshape(shape)
            at += size
            e = relerr(a, np.asarray(b, dtype=np.float64))
            print(f"from C, {tag}: {name} {e:.2e} (bar 1e-08)")
            assert e < 1e-8, (tag, name, e)
    assert at == out.size
