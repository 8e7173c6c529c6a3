"""Gradient of a horizon cost through the propagation on the sparse posteriors as ONE C call ("gradient of a horizon
cost") on the GPU: `SparseGP.propagate_gradient(route="chain")` (`gpk_sparse_propagate_grad`),
`BatchedSparseGP.propagate_gradient(route="chain")` (`gpk_sparse_propagate_grad_multi`) and their host routes.  Buffers start out as NaN (conftest: GPK_DEBUG_FILL).

Expected values: `adjoint_numpy_form` (tests/test_propagate_grad_host.py) on the dense form of the sparse posteriors: the mean's
model is (Z, alpha_u), the variance's gradient the dense form's own.  Bar: the project's fp64 bar, 1e-8 of each array's largest
component; tests/test_sparse_propagate_host.py asserts for every problem here that the variance stays above 2.5 % of the prior
along the horizon, so neither clip is active and the variance's gradient is the unclipped one.  Measured: <= 1.6e-12 against the
NumPy form, <= 2.9e-15 against the host route, 1.5e-10 for the device finite difference.

Problems (tests/test_sparse_propagate_host.py): single3 (P = 3, m = 26, D = 4), batch2 (B = 2, m = 60, coordinates (4, 1) of nx =
6, both scalers), batch8 (B = 8, m = 60, nx = 8), one200 (P = 1, m = 200 -> mp = 256); H = 5."""
import numpy as np
import pytest

from test_gpu_propagate_grad import NAMES, check_five, worst
from test_gpu_sparse_propagate import served
from test_propagate_grad_host import FD_BAR, FD_STEP, adjoint_numpy_form, cost, seeds
from test_propagate_host import rollouts, spd
from test_sparse_propagate_host import PROBLEMS, problem

pytestmark = pytest.mark.gpu


# ---- 1. parity with the NumPy form, and with the host route ----------------------------------------------------------------------
@pytest.mark.parametrize("name", PROBLEMS)
def test_parity_with_the_numpy_form_and_the_host_route(name):
    c, form, kw, _ = problem(name)
    gp = served(name)
    assert gp.propagate_ok()
    lin = c["lin"]
    nx = lin.shape[0]
    S0, Q = spd(nx)
    top = top_host = 0.0
    for R in (1, 5):
        x0, U = rollouts(c["x0"][0], c["U"], R)
        gx, gS = seeds(R, U.shape[1], nx)
        for noisy in (False, True):
            for seedS in (None, gS):
                for extra, want_args in (({}, (None, None)), (dict(Sigma0=S0, process_noise=Q), (np.tile(S0, (R, 1, 1)), Q))):
                    args = dict(var_includes_noise=noisy, **kw, **extra)
                    got = gp.propagate_gradient(x0, U, lin, gx, seedS, route="chain", **args)
                    want = adjoint_numpy_form(form, x0, U, lin, *want_args, noisy, gx, seedS)
                    tag = f"{name}, R = {R}, noise {noisy}, gS {seedS is not None}, SPD {bool(extra)}"
                    check_five(tag, got, want)
                    top = max(top, worst(got, want))
        # the class's own host route: host_adjoint over the device's predict_jacobian / predict_hessian; with the noise level
        # in the variances the two routes serve the same variance (without it they differ in where the level is taken off)
        args = dict(var_includes_noise=True, Sigma0=S0, process_noise=Q, **kw)
        chain = gp.propagate_gradient(x0, U, lin, gx, gS, route="chain", **args)
        host = gp.propagate_gradient(x0, U, lin, gx, gS, route="host", **args)
        check_five(f"{name}, R = {R}: chain against route = host", chain, host, 1e-10)
        top_host = max(top_host, worst(chain, host))
        auto = gp.propagate_gradient(x0, U, lin, gx, gS, **args)
        for i in range(5):
            assert np.array_equal(auto[i], host[i]), f"{name}: auto is the host route ({NAMES[i]})"
    print(f"{name}: chain against the NumPy form {top:.2e} (bar 1e-8), against route = host {top_host:.2e} (bar 1e-10)")


# ---- 2. the forward results have the bits of propagate(route="chain") ----------------------------------------------------------------
@pytest.mark.parametrize("R", (1, 16, 17, 32))
@pytest.mark.parametrize("name", ("single3", "batch2"))
def test_forward_results_have_the_bits_of_propagate(name, R):
    c, _, kw, _ = problem(name)
    gp = served(name)
    lin = c["lin"]
    nx = lin.shape[0]
    x0, U = rollouts(c["x0"][0], c["U"], R)
    gx, gS = seeds(R, U.shape[1], nx)
    S0, Q = spd(nx)
    for extra in ({}, dict(Sigma0=S0, process_noise=Q, var_includes_noise=True)):
        traj, Sigma = gp.propagate(x0, U, lin, route="chain", **kw, **extra)
        got = gp.propagate_gradient(x0, U, lin, gx, gS, route="chain", **kw, **extra)
        assert np.array_equal(got[0], traj), (name, R, "traj")
        assert np.array_equal(got[1], Sigma), (name, R, "Sigma")


# ---- 3. one stage, rebuilt from one predict_jacobian and one predict_hessian call --------------------------------------------------
def test_one_stage_rebuilt_from_predict_jacobian_and_predict_hessian():
    c = problem("single3")[0]
    gp = served("single3")
    lin = c["lin"]
    nx, D = lin.shape
    R = 3
    x0, U = rollouts(c["x0"][0], c["U"][:1], R)
    gx, gS = seeds(R, 1, nx)
    S0, _ = spd(nx)
    q = np.ascontiguousarray(np.concatenate([x0, U[:, 0]], axis=1))
    _, dmean, _, dvar = gp.predict_jacobian(q, return_var=True)
    hess = gp.predict_hessian(q)[2]
    dmean, dvar, hess = dmean.reshape(R, nx, D), dvar.reshape(R, nx, D), hess.reshape(R, nx, D, D)
    F = np.concatenate([np.eye(nx), np.zeros((nx, D - nx))], axis=1) + lin + dmean
    A = F[:, :, :nx]
    Lam = 0.5 * (gS[1] + gS[1].transpose(0, 2, 1))
    G = Lam @ A @ S0
    gq = np.einsum("rid,ri->rd", F, gx[1]) + np.einsum("rc,rcd->rd", np.diagonal(Lam, axis1=1, axis2=2), dvar) \
        + 2.0 * np.einsum("rcde,rce->rd", hess[:, :, :, :nx], G)
    got = gp.propagate_gradient(x0, U, lin, gx, gS, Sigma0=S0, route="chain")
    check_five("single3, one stage", got[2:], (gq[:, None, nx:], gx[0] + gq[:, :nx],
                                               0.5 * (gS[0] + gS[0].transpose(0, 2, 1)) + A.transpose(0, 2, 1) @ Lam @ A))


# ---- 4. linear in the seeds; symmetric; the same bits every call -------------------------------------------------------------------
@pytest.mark.parametrize("name", PROBLEMS)
def test_linearity_symmetry_and_repeatability(name):
    c, _, kw, _ = problem(name)
    gp = served(name)
    lin = c["lin"]
    nx = lin.shape[0]
    R = 5
    x0, U = rollouts(c["x0"][0], c["U"], R)
    H = U.shape[1]
    S0, Q = spd(nx)
    kw = dict(Sigma0=S0, process_noise=Q, route="chain", **kw)
    zero = gp.propagate_gradient(x0, U, lin, np.zeros((H + 1, R, nx)), np.zeros((H + 1, R, nx, nx)), **kw)
    assert not zero[2].any() and not zero[3].any() and not zero[4].any(), "zero seeds give exact zeros"
    (gx1, gS1), (gx2, gS2) = seeds(R, H, nx, 11), seeds(R, H, nx, 12)
    a = gp.propagate_gradient(x0, U, lin, gx1, gS1, **kw)
    b = gp.propagate_gradient(x0, U, lin, gx2, gS2, **kw)
    s = gp.propagate_gradient(x0, U, lin, gx1 + gx2, gS1 + gS2, **kw)
    err = max(float(np.max(np.abs(s[i] - (a[i] + b[i]))) / np.max(np.abs(s[i]))) for i in (2, 3, 4) if s[i].size)
    print(f"{name}: gradient of the sum of two seed sets against the sum of the gradients {err:.2e} (bar 1e-12)")
    assert err < 1e-12
    again = gp.propagate_gradient(x0, U, lin, gx1, gS1, **kw)
    for i in range(5):
        assert np.array_equal(a[i], again[i]), (name, NAMES[i])
    assert np.array_equal(a[4], a[4].transpose(0, 2, 1)), "dSigma0 equals its transpose bit for bit"


# ---- 5. a one-model batch against the single model -----------------------------------------------------------------------------------
def test_one_model_batch_has_the_bits_of_the_single_model_chain():
    from unmanned_aerial_vehicles_amd import BatchedSparseGP
    c = problem("one200")[0]
    gp = served("one200")
    bg = BatchedSparseGP([gp])
    S0, Q = spd(1)
    x0, U = rollouts(c["x0"][0], c["U"], 5)
    gx, gS = seeds(5, U.shape[1], 1)
    for noisy in (False, True):
        args = dict(Sigma0=S0, process_noise=Q, var_includes_noise=noisy, route="chain")
        a = bg.propagate_gradient(x0, U, c["lin"], gx, gS, coord=[0], **args)
        b = gp.propagate_gradient(x0, U, c["lin"], gx, gS, **args)
        for i in range(5):
            assert np.array_equal(a[i], b[i]), (NAMES[i], noisy)


# ---- 6. the device's own finite difference ---------------------------------------------------------------------------------------------
def test_directional_central_difference_of_the_device_propagate():
    c, _, kw, _ = problem("batch2")
    gp = served("batch2")
    lin = c["lin"]
    nx, D = lin.shape
    R = 2
    x0, U = rollouts(c["x0"][0], c["U"], R)
    H = U.shape[1]
    S0, Q = spd(nx)
    S0 = np.tile(S0, (R, 1, 1))
    gx, gS = seeds(R, H, nx)
    kw = dict(process_noise=Q, route="chain", **kw)
    _, _, dU, dx0, dS0 = gp.propagate_gradient(x0, U, lin, gx, gS, Sigma0=S0, **kw)
    rng = np.random.default_rng(23)
    a, b, s = rng.standard_normal((R, H, D - nx)), rng.standard_normal((R, nx)), rng.standard_normal((R, nx, nx))
    s = 1e-2 * 0.5 * (s + s.transpose(0, 2, 1))
    want = float(np.sum(dU * a) + np.sum(dx0 * b) + np.sum(dS0 * s))
    up = gp.propagate(x0 + FD_STEP * b, U + FD_STEP * a, lin, Sigma0=S0 + FD_STEP * s, **kw)
    dn = gp.propagate(x0 - FD_STEP * b, U - FD_STEP * a, lin, Sigma0=S0 - FD_STEP * s, **kw)
    fd = (cost(*up, gx, gS) - cost(*dn, gx, gS)) / (2 * FD_STEP)
    gap = abs(fd - want) / abs(want)
    print(f"batch2: directional derivative {want:.6e}, central difference of the device's chain {fd:.6e}, gap {gap:.2e} "
          f"(step {FD_STEP:g}, bar {FD_BAR:.2e})")
    assert gap < FD_BAR


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_model_serving():
    c = problem("single3")[0]
    gp = served("single3")
    lin = c["lin"]
    x0, U = rollouts(c["x0"][0], c["U"], 1)
    gx, gS = seeds(1, U.shape[1], 3)
    with pytest.raises(ValueError, match="order must be 1"):
        gp.propagate_gradient(x0, U, lin, gx, route="chain", order=2)
    with pytest.raises(ValueError, match="route must be"):
        gp.propagate_gradient(x0, U, lin, gx, route="device")
    be = gp._backend()
    be.set_options(small_path=0)
    try:
        with pytest.raises(ValueError, match="small_path"):
            gp.propagate_gradient(x0, U, lin, gx, route="chain")
    finally:
        be.set_options(small_path=1)
    want = gp.propagate_gradient(x0, U, lin, gx, gS, route="chain")
    assert all(np.isfinite(a).all() for a in want)
