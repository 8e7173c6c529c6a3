"""The gradient through exact moment matching (K11) from a plain C caller in its own process (tests/c_abi/moments_grad.c): the fit
building blocks and gpk_wtw, then gpk_moments_vjp_host and gpk_propagate_mm_grad_host on case b of tests/test_gpu_paths.py, (N, D, P)
= (130, 4, 3), R = 5 Gaussian queries / rollouts over H = 4 stages with an SPD Sigma0 and a process noise, and
gpk_moments_vjp_host_multi and gpk_propagate_mm_grad_host_multi on the same three outputs as single-output models behind an input
scaler, the noise level added through var_includes_noise.  The C program checks the bits of the forward entries, repeatability,
NULL seeds, the symmetry of dSq and dSigma0, and every bad-argument status with its outputs untouched; this side compares what it
wrote with the dense NumPy adjoint (`moments_vjp_numpy_form`, tests/test_moments_grad_host.py) at the project's fp64 bar, 1e-8 of
each array's largest component, and with the Python route."""
import subprocess

import numpy as np
import pytest

from conftest import relerr
from test_gpu_c_abi import _compile
from test_gpu_paths import case
from test_moments_grad_host import horizon_seeds, moments_vjp_numpy_form, seeds
from test_moments_host import form_of, moments_numpy_form
from test_propagate_host import gp_numpy_form, rollouts, spd

pytestmark = pytest.mark.gpu


def test_moments_gradient_from_c(tmp_path):
    exe = _compile(tmp_path, "moments_grad.c")
    c, pform, mform = form_of("b")
    g = pform.gps[0]
    N, D, P, R, H = 130, 4, 3, 5, 4
    sf2, noise, alpha = c["hyper"]
    x0, U = rollouts(c["x0"][0], c["U"][:H], R)
    S0, Q = spd(P)
    S0 = 0.05 * S0
    in_scaler = (np.array([0.05, -0.1, 0.2, 0.0]), np.array([1.1, 0.9, 1.25, 0.8]))
    Yn = (c["Y"] - g.ym) / g.ys
    gm, gc, gxc = seeds(R, P, D)
    gx, gS = horizon_seeds(H, R, P)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    parts = [np.array([N, D, P, R, H, sf2, noise, alpha]), c["ls"], g.ym, g.ys, c["X"], Yn, Yn.T, x0, U, c["lin"], S0, Q, *in_scaler,
             gm, gc, gxc, gx, gS]
    np.concatenate([np.ascontiguousarray(p, dtype=np.float64).ravel() for p in parts]).tofile(src)
    r = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "moments gradient from C: OK" in r.stdout
    out = np.fromfile(dst)
    shapes = ((R, P), (R, P, P), (R, P, D), (R, D), (R, P, P), (H + 1, R, P), (H + 1, R, P, P), (R, H, D - P), (R, P), (R, P, P))
    names = ("mean", "cov", "xcov", "dXq", "dSq", "traj", "Sigma", "dU", "dx0", "dSigma0")
    sizes = [int(np.prod(s)) for s in shapes]
    assert out.size == 2 * sum(sizes)
    Xq = np.concatenate([x0, U[:, 0]], axis=1)
    S0R = np.tile(S0, (R, 1, 1))
    multi = moments_numpy_form([gp_numpy_form(c["X"], c["Y"][:, b], c["ls"], sf2, noise, alpha) for b in range(P)], in_scaler)
    blocks = {}
    for tag, block, form, noisy in (("single", out[:sum(sizes)], mform, False), ("multi", out[sum(sizes):], multi, True)):
        got = [block[sum(sizes[:i]):sum(sizes[:i + 1])].reshape(shapes[i]) for i in range(10)]
        v = moments_vjp_numpy_form(form)
        wants = form.batch(Xq, S0R, noisy) + v.batch(Xq, S0R, noisy, gm, gc, gxc) + v.horizon(range(P), x0, U, c["lin"], S0R, Q, gx, gS,
                                                                                              noisy)
        for name, a, b in zip(names, got, wants):
            e = relerr(a, b)
            print(f"from C, {tag}: {name} {e:.2e} (bar 1e-08)")
            assert e < 1e-8, (tag, name, e)
        blocks[tag] = got
    # the Python route on the same model: the same kernels on the package's own factorisation
    gp = case("b")[1]
    pv = gp.predict_moments_vjp(Xq, S0R, gm, gc, gxc)
    pg = gp.propagate_moments_gradient(x0, U, c["lin"], gx, gS, Sigma0=S0, process_noise=Q)
    for name, a, b in zip(names, blocks["single"], pv + pg):
        e = relerr(a, b)
        print(f"from C against the Python route: {name} {e:.2e} (bar 1e-08)")
        assert e < 1e-8, (name, e)
