"""Gradient of a horizon cost through the propagation of a single model ("gradient of a horizon cost") on the GPU:
`GaussianProcessRegressor.propagate_gradient` (one C call, `gpk_propagate_grad_host`), its host route and
`SimpleQuadrotorGP.horizon_gradient`.  Buffers start out as NaN (conftest: GPK_DEBUG_FILL), so a sweep that read an unwritten
share, query padding or a stage buffer of another stage would show.

Expected values: `adjoint_numpy_form` of tests/test_propagate_grad_host.py (the backward sweep on dense NumPy posteriors, itself
checked there against central differences of the forward form).  Bar: the project's fp64 bar, 1e-8 of each array's largest
component; the variance clip is inactive along every horizon here (asserted there), so the variance's gradient is the unclipped
one.  Measured: <= 1.4e-14 against the NumPy form, <= 8.2e-16 against the host route, 1.1e-10 for the device finite
difference.  Bit identity is asserted with np.array_equal.  The device finite difference uses the step and the bar found on the CPU
(FD_STEP, FD_BAR there).

Inputs: the models and horizons of tests/golden/paths_ref.npz, cases (N, D, P, H) = a (120, 4, 1, 6), b (130, 4, 3, 5), csv (200, 10,
6, 25), one (128, 3, 2, 4); R = 1 is the fixture's first start and its controls, R > 1 the rollouts x0 + 0.01 r, U (1 + 0.05 r)."""
import numpy as np
import pytest

from test_gpu_paths import case, check
from test_propagate_grad_host import FD_BAR, FD_STEP, adjoint_numpy_form, cost, seeds
from test_propagate_host import rollouts, single_form, spd

pytestmark = pytest.mark.gpu

CASE_NAMES = ("a", "b", "csv", "one")
NAMES = ("traj", "Sigma", "dU", "dx0", "dSigma0")


def worst(got, want, skip=()):
    """the largest difference of two results, each array relative to its largest component"""
    return max(float(np.max(np.abs(g - w)) / max(np.max(np.abs(w)), 1e-300)) for n, g, w in zip(NAMES, got, want)
               if n not in skip and w.size)


def check_five(tag, got, want, bar=1e-8):
    for n, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape, (tag, n, g.shape, w.shape)
        if w.size:
            err = float(np.max(np.abs(g - w)) / max(np.max(np.abs(w)), 1e-300))
            assert err < bar, f"{tag}: {n} differs by {err:.3e} (bar {bar:.0e})"


# ---- 1. parity with the NumPy form ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_parity_with_the_numpy_form(name):
    c, gp, _, _ = case(name)
    _, form = single_form(name)
    lin = c["lin"]
    nx, H = lin.shape[0], len(c["U"])
    S0, Q = spd(nx)
    top = 0.0
    for R in (1, 5):
        x0, U = rollouts(c["x0"][0], c["U"], R)
        gx, gS = seeds(R, H, nx)
        for noisy in (False, True):
            for seedS in (None, gS):
                for kw, want_args in (({}, (None, None)), (dict(Sigma0=S0, process_noise=Q), (np.tile(S0, (R, 1, 1)), Q))):
                    got = gp.propagate_gradient(x0, U, lin, gx, seedS, var_includes_noise=noisy, **kw)
                    want = adjoint_numpy_form(form, x0, U, lin, *want_args, noisy, gx, seedS)
                    tag = f"case {name}, R = {R}, noise {noisy}, gS {seedS is not None}, SPD {bool(kw)}"
                    check_five(tag, got, want)
                    top = max(top, worst(got, want))
    print(f"case {name}: propagate_gradient against the NumPy form, worst over every variant {top:.2e} (bar 1e-8)")
    # the shorthand shapes: x0 (P,), U (H, nu), seeds without the rollout axis
    gx, gS = seeds(1, H, nx)
    one = gp.propagate_gradient(c["x0"][0], c["U"], lin, gx[:, 0], gS[:, 0])
    assert one[2].shape == (1, H, lin.shape[1] - nx) and one[3].shape == (1, nx) and one[4].shape == (1, nx, nx)


# ---- 2. the forward results have the bits of propagate ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,R", [("b", 1), ("b", 16), ("b", 17), ("b", 32), ("csv", 17)])
def test_forward_results_have_the_bits_of_propagate(name, R):
    c, gp, _, _ = case(name)
    lin = c["lin"]
    nx = lin.shape[0]
    x0, U = rollouts(c["x0"][0], c["U"], R)
    gx, gS = seeds(R, U.shape[1], nx)
    S0, Q = spd(nx)
    for kw in ({}, dict(Sigma0=S0, process_noise=Q, var_includes_noise=True)):
        traj, Sigma = gp.propagate(x0, U, lin, **kw)
        got = gp.propagate_gradient(x0, U, lin, gx, gS, **kw)
        assert np.array_equal(got[0], traj), (name, R, "traj")
        assert np.array_equal(got[1], Sigma), (name, R, "Sigma")


# ---- 3. the host route --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("b", "csv"))
def test_host_route_agrees(name):
    c, gp, _, _ = case(name)
    lin = c["lin"]
    nx = lin.shape[0]
    x0, U = rollouts(c["x0"][0], c["U"], 5)
    gx, gS = seeds(5, U.shape[1], nx)
    S0, Q = spd(nx)
    for noisy in (False, True):
        kw = dict(Sigma0=S0, process_noise=Q, var_includes_noise=noisy)
        one_call = gp.propagate_gradient(x0, U, lin, gx, gS, **kw)
        host = gp.propagate_gradient(x0, U, lin, gx, gS, route="host", **kw)
        print(f"case {name}, noise {noisy}: one call against route = host {worst(one_call, host):.2e} (bar 1e-10)")
        check_five(f"case {name}: route = host, noise {noisy}", one_call, host, 1e-10)
    be = gp._dev.be
    be.set_options(small_path=0)
    try:
        loop = gp.propagate_gradient(x0, U, lin, gx, gS, **kw)
    finally:
        be.set_options(small_path=1)
    check_five(f"case {name}: option small_path = 0", loop, one_call, 1e-10)


# ---- 4. one stage, rebuilt from one predict_jacobian and one predict_hessian call --------------------------------------------------
@pytest.mark.parametrize("name", ("b", "csv"))
def test_one_stage_rebuilt_from_predict_jacobian_and_predict_hessian(name):
    c, gp, _, _ = case(name)
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
    got = gp.propagate_gradient(x0, U, lin, gx, gS, Sigma0=S0)
    check(f"case {name}: dU of one stage", got[2][:, 0], gq[:, nx:])
    check(f"case {name}: dx0 of one stage", got[3], gx[0] + gq[:, :nx])
    check(f"case {name}: dSigma0 of one stage", got[4], 0.5 * (gS[0] + gS[0].transpose(0, 2, 1)) + A.transpose(0, 2, 1) @ Lam @ A)


# ---- 5. linear in the seeds; symmetric; the same bits every call -------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_linearity_symmetry_and_repeatability(name):
    c, gp, _, _ = case(name)
    lin = c["lin"]
    nx = lin.shape[0]
    R = 5
    x0, U = rollouts(c["x0"][0], c["U"], R)
    H = U.shape[1]
    S0, Q = spd(nx)
    kw = dict(Sigma0=S0, process_noise=Q)
    zero = gp.propagate_gradient(x0, U, lin, np.zeros((H + 1, R, nx)), np.zeros((H + 1, R, nx, nx)), **kw)
    assert not zero[2].any() and not zero[3].any() and not zero[4].any(), "zero seeds give exact zeros"
    zero = gp.propagate_gradient(x0, U, lin, np.zeros((H + 1, R, nx)), **kw)
    assert not zero[2].any() and not zero[3].any() and not zero[4].any()
    (gx1, gS1), (gx2, gS2) = seeds(R, H, nx, 11), seeds(R, H, nx, 12)
    a = gp.propagate_gradient(x0, U, lin, gx1, gS1, **kw)
    b = gp.propagate_gradient(x0, U, lin, gx2, gS2, **kw)
    s = gp.propagate_gradient(x0, U, lin, gx1 + gx2, gS1 + gS2, **kw)
    err = max(float(np.max(np.abs(s[i] - (a[i] + b[i]))) / np.max(np.abs(s[i]))) for i in (2, 3, 4) if s[i].size)
    print(f"case {name}: gradient of the sum of two seed sets against the sum of the gradients {err:.2e} (bar 1e-12)")
    assert err < 1e-12
    again = gp.propagate_gradient(x0, U, lin, gx1, gS1, **kw)
    for i in range(5):
        assert np.array_equal(a[i], again[i]), (name, NAMES[i])
    assert np.array_equal(a[4], a[4].transpose(0, 2, 1)), "dSigma0 equals its transpose bit for bit"
    # an asymmetric gS enters through its symmetric part
    rng = np.random.default_rng(4)
    skew = rng.standard_normal((H + 1, R, nx, nx))
    skew = skew - skew.transpose(0, 1, 3, 2)
    c2 = gp.propagate_gradient(x0, U, lin, gx1, gS1 + skew, **kw)
    check_five(f"case {name}: gS + a skew part", c2, a, 1e-12)


# ---- 6. the device's own finite difference ---------------------------------------------------------------------------------------------
def test_directional_central_difference_of_the_device_propagate():
    c, gp, _, _ = case("b")
    lin = c["lin"]
    nx, D = lin.shape
    R = 2
    x0, U = rollouts(c["x0"][0], c["U"], R)
    H = U.shape[1]
    S0, Q = spd(nx)
    S0 = np.tile(S0, (R, 1, 1))
    gx, gS = seeds(R, H, nx)
    _, _, dU, dx0, dS0 = gp.propagate_gradient(x0, U, lin, gx, gS, Sigma0=S0, process_noise=Q)
    rng = np.random.default_rng(23)
    a, b, s = rng.standard_normal((R, H, D - nx)), rng.standard_normal((R, nx)), rng.standard_normal((R, nx, nx))
    s = 1e-2 * 0.5 * (s + s.transpose(0, 2, 1))
    want = float(np.sum(dU * a) + np.sum(dx0 * b) + np.sum(dS0 * s))
    up = gp.propagate(x0 + FD_STEP * b, U + FD_STEP * a, lin, Sigma0=S0 + FD_STEP * s, process_noise=Q)
    dn = gp.propagate(x0 - FD_STEP * b, U - FD_STEP * a, lin, Sigma0=S0 - FD_STEP * s, process_noise=Q)
    fd = (cost(*up, gx, gS) - cost(*dn, gx, gS)) / (2 * FD_STEP)
    gap = abs(fd - want) / abs(want)
    print(f"case b: directional derivative {want:.6e}, central difference of the device's propagate {fd:.6e}, gap {gap:.2e} "
          f"(step {FD_STEP:g}, bar {FD_BAR:.2e})")
    assert gap < FD_BAR


# ---- 7. the largest small-path size: every workgroup count of the Hessian-vector launch, two output slices -------------------------
def test_largest_shapes_against_the_host_route():
    """Np = 4096 (64 workgroups of 64 rows), D = P = 16 (nu = 0: dU is empty), R = 32: two output slices of the Hessian-vector
    launch, the widest state, against the host route."""
    from unmanned_aerial_vehicles_amd import RBF, GaussianProcessRegressor, WhiteKernel
    N, D = 4000, 16
    rng = np.random.default_rng(N)
    X = rng.standard_normal((N, D))
    Y = 0.3 * np.sin(X @ rng.standard_normal((D, D)) / 4.0) + 0.1 * rng.standard_normal((N, D))
    gp = GaussianProcessRegressor(RBF(3.0) + WhiteKernel(0.05), alpha=1e-6, normalize_y=True, optimizer=None).fit(X, Y)
    assert gp._dev.Np == 4096 and gp._dev.propagate_ok()
    x0 = 0.5 * rng.standard_normal((32, D))
    lin = 0.05 * rng.standard_normal((D, D))
    U = np.zeros((2, 0))
    S0, Q = spd(D)
    gx, gS = seeds(32, 2, D)
    got = gp.propagate_gradient(x0, U, lin, gx, gS, Sigma0=S0, process_noise=Q)
    want = gp.propagate_gradient(x0, U, lin, gx, gS, Sigma0=S0, process_noise=Q, route="host")
    assert got[2].shape == (32, 2, 0) and got[3].shape == (32, 16) and got[4].shape == (32, 16, 16)
    print(f"Np = 4096, D = P = 16, R = 32, H = 2: one call against route = host {worst(got, want):.2e} (bar 1e-10)")
    check_five("Np = 4096, D = P = 16, R = 32", got, want, 1e-10)


# ---- 8. the control-loop wrapper ---------------------------------------------------------------------------------------------------
def test_simple_quadrotor_gp_horizon_gradient(capsys):
    from unmanned_aerial_vehicles_amd import SimpleQuadrotorGP
    from unmanned_aerial_vehicles_amd.paths import nominal_rollouts
    from unmanned_aerial_vehicles_amd.propagate import nominal_adjoint
    c, gp, _, _ = case("csv")
    _, form = single_form("csv")
    sq = SimpleQuadrotorGP()
    sq.gp_model, sq.is_trained = gp, True
    state, Ug, dt = c["x0"][0], np.ascontiguousarray(c["U"].T), 0.1
    N = Ug.shape[1]
    nominal, lin = nominal_rollouts(sq._nominal_dynamics, state, Ug, dt, 1)
    gx, gS = seeds(1, N, 6)
    X, Sig, dU, dx0 = sq.horizon_gradient(state, Ug, dt, gx[:, 0], gS[:, 0])
    assert X.shape == (6, N + 1) and Sig.shape == (N + 1, 6, 6) and dU.shape == (N, 4) and dx0.shape == (6,)
    assert sq.prediction_count == N
    want = adjoint_numpy_form(form, state[None], c["U"][None], lin, None, None, False, gx, gS)
    check("horizon_gradient: X", X, want[0][:, 0].T)
    check("horizon_gradient: Sigma", Sig, want[1][:, 0])
    check("horizon_gradient: dU", dU, want[2][0])
    check("horizon_gradient: dx0", dx0, want[3][0])
    # a model that refuses: the nominal horizon and sweep, with the reason printed

    class refusing:
        def propagate_gradient(self, *a, **k):
            raise ValueError("this model refuses")

    sq.gp_model = refusing()
    capsys.readouterr()
    X, Sig, dU, dx0 = sq.horizon_gradient(state, Ug, dt, gx[:, 0], gS[:, 0])
    assert "this model refuses" in capsys.readouterr().out
    wU, wx = nominal_adjoint(lin, 1, N, gx, None)
    assert np.array_equal(X, nominal[0]) and not Sig.any() and np.array_equal(dU, wU[0]) and np.array_equal(dx0, wx[0])


# ---- 9. the limits -------------------------------------------------------------------------------------------------------------------
def test_refusals_raise_with_the_library_message():
    c, gp, _, _ = case("b")
    dev, lin = gp._dev, c["lin"]
    ym, ys = gp._y_train_mean, gp._y_train_std
    x1, U1 = rollouts(c["x0"][0], c["U"], 1)
    H = U1.shape[1]
    gx, gS = seeds(1, H, 3)
    nan = gx.copy()
    nan[2, 0, 1] = np.nan
    inf = gS.copy()
    inf[0, 0, 1, 1] = np.inf
    for what, msg, args in (("NaN in gx", "seeds gx and gS must not contain NaN", (nan, gS)),
                            ("infinity in gS", "seeds gx and gS must not contain NaN", (gx, inf)),
                            ("no gx", "null seed gx", (None, gS))):
        with pytest.raises(ValueError, match=msg):
            dev.propagate_grad_host(ym, ys, 1.0, x1, U1, np.ascontiguousarray(lin), None, None, 1, H, *args)
            pytest.fail(what)
    x33, U33 = rollouts(c["x0"][0], c["U"], 33)
    with pytest.raises(ValueError, match="R must be in"):
        gp.propagate_gradient(x33, U33, lin, np.zeros((H + 1, 33, 3)))
    with pytest.raises(ValueError, match="order must be 1"):
        gp.propagate_gradient(x1, U1, lin, gx, order=2)
    # a refused call leaves the handle serving
    want = adjoint_numpy_form(single_form("b")[1], x1, U1, lin, None, None, False, gx, gS)
    check_five("after the refusals", gp.propagate_gradient(x1, U1, lin, gx, gS), want)
