"""Exact moment matching of a single model (DESIGN.md, K11 "moment matching") on the GPU: `GaussianProcessRegressor.predict_moments`
(one C call, `gpk_moments_host`) and `propagate(method="moment")` (`gpk_propagate_mm_host`), its host route and the wrapper.
Buffers start out as NaN (conftest: GPK_DEBUG_FILL), so a pair tile that read K^-1's padding, a row beyond N or an unwritten slot
would show.

Expected values: `moments_numpy_form` of tests/test_moments_host.py (dense NumPy, L built explicitly from R^-1 S, LAPACK's
factorisation), checked there against Gauss-Hermite quadrature.  Bar: the project's fp64 bar, 1e-8 of each array's largest
component; that file prints and asserts what it rests on (E[v] >= 1.8 % of the prior on every case: the clip is inactive; float64
against longdouble <= 7.2e-13).  Bit identity is asserted with np.array_equal.

Inputs: tests/golden/paths_ref.npz, cases (N, D, P, H) = a (120, 4, 1, 6), b (130, 4, 3, 5), csv (200, 10, 6, 25), one (128 = two
full tiles, 3, 2, 4), a model fitted here with (N, D, P) = (333, 5, 2): six tile rows of the pair pass, diagonal and off-diagonal
tiles and a ragged edge of 13 rows, and one with (N, D, P) = (70, 12, 10): a state of ten coordinates, ten outputs, 55 output pairs
in one pass - the finishing launch's sums past one wave of threads, and the pair kernel's second chunk of sums."""
import numpy as np
import pytest

from test_gpu_paths import case, check
from test_moments_host import form_of, moments_numpy_form
from test_propagate_host import gp_numpy_form, rollouts, spd

pytestmark = pytest.mark.gpu

CASE_NAMES = ("a", "b", "csv", "one")
_big = {}


def big():
    """(arrays, fitted model, moments form) of the N = 333 model: built once, shared, left unchanged"""
    if "v" not in _big:
        from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, GaussianProcessRegressor, WhiteKernel
        rng = np.random.default_rng(333)
        N, D, P, H = 333, 5, 2, 3
        X = rng.standard_normal((N, D))
        Y = np.stack([0.3 * np.sin(X[:, 0] + X[:, 2]) + 0.1 * X[:, 4], 0.2 * np.cos(X[:, 1]) * X[:, 3]], axis=1)
        Y += 0.05 * rng.standard_normal((N, P))
        ls, sf2, noise, alpha = 1.5 + 0.2 * np.arange(D), 0.9, 0.02, 1e-8
        lin = 0.05 * rng.standard_normal((P, D))
        c = {"X": X, "Y": Y, "lin": lin, "x0": 0.3 * rng.standard_normal((1, P)), "U": 0.3 * rng.standard_normal((H, D - P))}
        gp = GaussianProcessRegressor(ConstantKernel(sf2) * RBF(ls) + WhiteKernel(noise), alpha=alpha, normalize_y=True,
                                      optimizer=None).fit(X, Y)
        _big["v"] = (c, gp, moments_numpy_form([gp_numpy_form(X, Y, ls, sf2, noise, alpha)]))
    return _big["v"]


def wide():
    """(arrays, fitted model, moments form) of the nx = P = 10 model: built once, shared, left unchanged"""
    if "w" not in _big:
        from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, GaussianProcessRegressor, WhiteKernel
        rng = np.random.default_rng(1210)
        N, D, P, H = 70, 12, 10, 3
        X = rng.standard_normal((N, D))
        Y = 0.2 * np.sin(X @ rng.standard_normal((D, P)) / 2.0) + 0.03 * rng.standard_normal((N, P))
        ls, sf2, noise, alpha = 2.5 + 0.1 * np.arange(D), 0.8, 0.03, 1e-8
        c = {"X": X, "Y": Y, "lin": 0.03 * rng.standard_normal((P, D)), "x0": 0.3 * rng.standard_normal((1, P)),
             "U": 0.3 * rng.standard_normal((H, D - P))}
        gp = GaussianProcessRegressor(ConstantKernel(sf2) * RBF(ls) + WhiteKernel(noise), alpha=alpha, normalize_y=True,
                                      optimizer=None).fit(X, Y)
        _big["w"] = (c, gp, moments_numpy_form([gp_numpy_form(X, Y, ls, sf2, noise, alpha)]))
    return _big["w"]


def problem(name):
    if name == "big":
        return big()
    if name == "wide":
        return wide()
    c, _, mform = form_of(name)
    return c, case(name)[1], mform


def check_moments(tag, got, want):
    for what, g, w in zip(("mean", "cov", "xcov"), got, want):
        check(f"{tag}: {what}", np.asarray(g), np.asarray(w))


def check_run(tag, got, want):
    for what, g, w in (("traj", got[0], want[0]), ("Sigma", got[1], want[1])) + tuple((k, got[2][k], want[2][k])
                                                                                       for k in ("mean", "cov", "xcov")):
        check(f"{tag}: {what}", g, w)


# ---- 1. parity with the NumPy form ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", (1, 5, 17, 32))
@pytest.mark.parametrize("name", CASE_NAMES + ("big", "wide"))
def test_predict_moments_parity(name, R):
    c, gp, mform = problem(name)
    nx = c["lin"].shape[0]
    S0, _ = spd(nx)
    x0, U = rollouts(c["x0"][0], c["U"], R)
    Q = np.ascontiguousarray(np.concatenate([x0, U[:, 0]], axis=1))
    S = np.stack([S0 * (0.05 + 0.01 * r) for r in range(R)])
    for noisy in (False, True):
        got = gp.predict_moments(Q, S, var_includes_noise=noisy)
        assert got[0].shape == (R, nx) and got[1].shape == (R, nx, nx) and got[2].shape == (R, nx, Q.shape[1])
        check_moments(f"case {name}, R = {R}, noise {noisy}", got, mform.batch(Q, S, noisy))
        assert np.array_equal(got[1], got[1].transpose(0, 2, 1)), "every V block equals its transpose bit for bit"
        assert not got[2][:, :, nx:].any(), "the controls are certain"


@pytest.mark.parametrize("name", CASE_NAMES + ("big", "wide"))
def test_propagate_parity(name):
    c, gp, mform = problem(name)
    lin = c["lin"]
    nx = lin.shape[0]
    S0, Q = spd(nx)
    S0 = 0.05 * S0
    for R in (1, 5, 17, 32):
        # (the whole horizon at R = 1 and 5; its first four stages at 17 and 32, where the NumPy form is what takes the time)
        Uc = c["U"] if R <= 5 else c["U"][:4]
        H = len(Uc)
        x0, U = rollouts(c["x0"][0], Uc, R)
        for noisy in ((False, True) if R <= 5 else ()):
            got = gp.propagate(x0, U, lin, var_includes_noise=noisy, return_stages=True, method="moment")
            assert got[0].shape == (H + 1, R, nx) and got[1].shape == (H + 1, R, nx, nx)
            assert np.array_equal(got[0][0], x0) and not got[1][0].any()
            check_run(f"case {name}, R = {R}, noise {noisy}, Sigma0 = 0", got, mform.run(range(nx), x0, U, lin, None, None, noisy))
        got = gp.propagate(x0, U, lin, Sigma0=S0, process_noise=Q, return_stages=True, method="moment")
        check_run(f"case {name}, R = {R}, SPD Sigma0 and Q", got, mform.run(range(nx), x0, U, lin, np.tile(S0, (R, 1, 1)), Q))
        assert np.array_equal(got[1], got[1].transpose(0, 1, 3, 2)), "every Sigma[h, r] equals its transpose bit for bit"
        assert np.array_equal(got[2]["cov"], got[2]["cov"].transpose(0, 1, 3, 2))


# ---- 2. independent device checks ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("b", "csv", "big"))
def test_zero_covariance_is_predict_and_the_linear_stage(name):
    c, gp, _ = problem(name)
    lin = c["lin"]
    nx = lin.shape[0]
    x0, U = rollouts(c["x0"][0], c["U"][:1], 5)
    q = np.ascontiguousarray(np.concatenate([x0, U[:, 0]], axis=1))
    mean, cov, xcov = gp.predict_moments(q, np.zeros((nx, nx)), var_includes_noise=True)
    pm, ps = gp.predict(q, return_std=True)
    check(f"case {name}: mean at Sigma = 0 against predict", mean, pm.reshape(5, nx))
    check(f"case {name}: variance at Sigma = 0 against predict", cov[:, np.arange(nx), np.arange(nx)], ps.reshape(5, nx) ** 2)
    off = cov - cov * np.eye(nx)
    assert np.max(np.abs(off)) <= 1e-8 * np.max(np.abs(cov)) and not xcov.any()
    _, Q = spd(nx)
    lt, lS = gp.propagate(x0, U, lin, process_noise=Q)
    mt, mS = gp.propagate(x0, U, lin, process_noise=Q, method="moment")
    check(f"case {name}: H = 1, Sigma0 = 0, traj against the linear chain", mt, lt)
    check(f"case {name}: H = 1, Sigma0 = 0, Sigma against the linear chain", mS, lS)


@pytest.mark.parametrize("name", ("b", "csv"))
def test_host_route_and_stage_bits(name):
    c, gp, _ = problem(name)
    lin = c["lin"]
    nx = lin.shape[0]
    S0, Q = spd(nx)
    x0, U = rollouts(c["x0"][0], c["U"][:4], 17)
    chain = gp.propagate(x0, U, lin, Sigma0=0.05 * S0, process_noise=Q, return_stages=True, method="moment")
    host = gp.propagate(x0, U, lin, Sigma0=0.05 * S0, process_noise=Q, return_stages=True, method="moment", route="host")
    check_run(f"case {name}: the host route against the chain", host, chain)
    traj, Sigma, st = chain
    for h in range(U.shape[1]):
        q = np.ascontiguousarray(np.concatenate([traj[h], U[:, h]], axis=1))
        mean, cov, xcov = gp.predict_moments(q, Sigma[h])
        assert np.array_equal(st["mean"][h], mean), (name, h, "mean")
        assert np.array_equal(st["cov"][h], cov), (name, h, "cov")
        assert np.array_equal(st["xcov"][h], xcov), (name, h, "xcov")


# ---- 3. bits ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("b", "big"))
def test_repeatable_and_independent_of_the_batch(name):
    c, gp, _ = problem(name)
    lin = c["lin"]
    nx = lin.shape[0]
    S0, Q = spd(nx)
    x0, U = rollouts(c["x0"][0], c["U"], 17)
    kw = dict(Sigma0=0.05 * S0, process_noise=Q, return_stages=True, method="moment")
    one, two = gp.propagate(x0, U, lin, **kw), gp.propagate(x0, U, lin, **kw)
    for a, b in zip(one[:2] + tuple(one[2].values()), two[:2] + tuple(two[2].values())):
        assert np.array_equal(a, b), "two calls return the same bits"
    for r in (0, 9, 16):
        alone = gp.propagate(x0[r], U[r], lin, **kw)
        assert np.array_equal(alone[0][:, 0], one[0][:, r]) and np.array_equal(alone[1][:, 0], one[1][:, r]), r
        assert np.array_equal(alone[2]["xcov"][:, 0], one[2]["xcov"][:, r]), r


def test_linear_is_untouched():
    c, gp, _ = problem("b")
    S0, Q = spd(3)
    x0, U = rollouts(c["x0"][0], c["U"], 5)
    a = gp.propagate(x0, U, c["lin"], Sigma0=S0, process_noise=Q, return_stages=True)
    b = gp.propagate(x0, U, c["lin"], Sigma0=S0, process_noise=Q, return_stages=True, method="linear")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert all(np.array_equal(a[2][k], b[2][k]) for k in ("mean", "var", "jac"))


def test_inverse_gram_is_cached_and_dropped_with_the_factor():
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, GaussianProcessRegressor, WhiteKernel
    c, _, _ = problem("a")

    def fit(sf2, scale, noise):
        return GaussianProcessRegressor(ConstantKernel(sf2) * RBF(scale * c["ls"]) + WhiteKernel(noise), alpha=1e-8, normalize_y=True,
                                        optimizer=None).fit(c["X"], c["Y"][:, 0])

    gp, other = fit(1.1, 1.0, 0.02), fit(0.7, 1.5, 0.05)
    q, S = np.concatenate([c["x0"][0], c["U"][0]])[None], np.array([[0.01]])
    first = gp.predict_moments(q, S)
    dev = gp._dev
    assert dev.moments_ok() and dev.inverse_gram() is dev.inverse_gram() and "kinv" in dev._Winv
    # a new factorisation of the same device model at other hyper-parameters drops K^-1 with the inverse factor
    gp.kernel_.theta = other.kernel_.theta
    gp._refactor()
    gp._alpha_host = gp._L_host = None
    assert gp._dev is dev and "kinv" not in dev._Winv
    again = gp.predict_moments(q, S)
    assert all(np.array_equal(a, b) for a, b in zip(again, other.predict_moments(q, S))) and not np.array_equal(again[1], first[1])
    with pytest.raises(ValueError, match="positive semi-definite"):
        gp.predict_moments(q, np.array([[-0.01]]))


# ---- 4. refusals and the wrapper -------------------------------------------------------------------------------------------------
def test_refusals():
    from unmanned_aerial_vehicles_amd.sparse import SparseGP
    c, gp, _ = problem("b")
    x0, U = rollouts(c["x0"][0], c["U"], 33)
    with pytest.raises(ValueError, match="R must be"):
        gp.propagate(x0, U, c["lin"], method="moment")
    with pytest.raises(ValueError, match="order=1"):
        gp.propagate(x0[:2], U[:2], c["lin"], method="moment", order=2)
    with pytest.raises(ValueError, match="propagate_gradient"):
        gp.propagate_gradient(x0[:1], U[:1], c["lin"], np.zeros((len(c["U"]) + 1, 1, 3)), method="moment")
    with pytest.raises(ValueError, match="M must be"):
        gp.predict_moments(np.zeros((33, 4)), np.eye(3))
    with pytest.raises(ValueError, match="SparseGP"):
        SparseGP.propagate(SparseGP.__new__(SparseGP), x0[:1], U[:1], c["lin"], method="moment")


def test_wrapper_runs_the_chain_and_falls_back(capsys):
    from unmanned_aerial_vehicles_amd import SimpleQuadrotorGP
    from unmanned_aerial_vehicles_amd.paths import nominal_rollouts
    c, gp, mform = problem("csv")
    sq = SimpleQuadrotorGP()
    sq.gp_model, sq.is_trained = gp, True
    state, Ug, dt = c["x0"][0], np.ascontiguousarray(c["U"][:6].T), 0.1
    _, lin = nominal_rollouts(sq._nominal_dynamics, state, Ug, dt, 1)
    S0, Q = spd(6)
    X, Sig = sq.propagate_horizon(state, Ug, dt, Sigma0=0.05 * S0, process_noise=Q, method="moment")
    assert "failed" not in capsys.readouterr().out
    wt, wS, _ = mform.run(range(6), state[None], c["U"][None, :6], lin, 0.05 * S0[None], Q)
    check("propagate_horizon(method='moment'): X", X, wt[:, 0].T)
    check("propagate_horizon(method='moment'): Sigma", Sig, wS[:, 0])
    X, Sig = sq.propagate_horizon(state, Ug, dt, Sigma0=np.full((6, 6), np.nan), method="moment")
    assert "failed" in capsys.readouterr().out and X.shape == (6, 7) and np.isfinite(Sig).all()
