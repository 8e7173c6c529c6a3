"""Input gradients of the posterior on the GPU (K8): GaussianProcessRegressor.predict_jacobian, the model seams
(SimpleQuadrotorGP, the package GaussianProcess) and the DeviceGP routes behind them (gpk_predict_host_grad: small path and
large route; gpk_predict_mean_grad / gpk_predict_var_grad_inv) against the closed forms evaluated from scikit-learn's fitted
attributes (tests/golden/jac_ref.npz, tests/golden/make_golden_jac.py), against finite differences of the existing predict,
and against each other."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, relerr

pytestmark = pytest.mark.gpu

FP64_BAR = 1e-8          # the project's fp64 parity bar, relative to the largest entry
ROUTE_BAR = 1e-11        # routes differ in summation order only


@pytest.fixture(scope="module")
def jac_ref():
    d = np.load(os.path.join(GOLDEN, "jac_ref.npz"))
    return {k: d[k] for k in d.files}


def _gp(kernel, **kw):
    from unmanned_aerial_vehicles_amd import GaussianProcessRegressor
    return GaussianProcessRegressor(kernel=kernel, optimizer=None, device=0, **kw)


def _ka1(csv_data, y=None, **kw):
    from unmanned_aerial_vehicles_amd import RBF, WhiteKernel
    y = csv_data["Y6"] if y is None else y
    return _gp(RBF(0.5) + WhiteKernel(0.1), alpha=1e-4, **kw).fit(csv_data["X10"], y)


def _synthetic(N, D=6, P=2, seed=0, **kw):
    """test_gpu_cov._synthetic's recipe."""
    from unmanned_aerial_vehicles_amd import RBF, WhiteKernel
    rng = np.random.default_rng(seed + N)
    X = rng.standard_normal((N, D))
    Y = np.sin(X @ rng.standard_normal((D, P))) + 0.1 * rng.standard_normal((N, P))
    gp = _gp(RBF(1.6) + WhiteKernel(0.05), alpha=1e-6, normalize_y=True, **kw).fit(X, Y)
    return gp, rng


def _check_case(out, ref, name, shapes):
    mean, dmean, var, dvar = out
    assert mean.shape == shapes[0] and dmean.shape == shapes[1] and var.shape == shapes[0] and dvar.shape == shapes[1]
    errs = {"mean": relerr(mean, ref[name + "_mean"]), "var": relerr(var, ref[name + "_var"]),
            "dmean": relerr(dmean, ref[name + "_dmean"]), "dvar": relerr(dvar, ref[name + "_dvar"])}
    print(name, {k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < FP64_BAR, (name, k, v)


# ---- 1: parity with the fixture, shapes -----------------------------------------------------------------------------------
def test_ka1_and_train_match_fixture(csv_data, jac_ref):
    gp = _ka1(csv_data, normalize_y=True)
    _check_case(gp.predict_jacobian(csv_data["Xq10"], return_var=True), jac_ref, "ka1", ((64, 6), (64, 6, 10)))
    # 8 training rows + 17 queries (the small path: 25 rows), variances at the noise level
    _check_case(gp.predict_jacobian(jac_ref["train_Xq"], return_var=True), jac_ref, "train", ((25, 6), (25, 6, 10)))
    mean, dmean = gp.predict_jacobian(jac_ref["train_Xq"])
    assert relerr(mean, jac_ref["train_mean"]) < FP64_BAR and relerr(dmean, jac_ref["train_dmean"]) < FP64_BAR


def test_one_target_unnormalised_matches_fixture(csv_data, jac_ref):
    gp = _ka1(csv_data, y=csv_data["Y6"][:, 0], normalize_y=False)
    _check_case(gp.predict_jacobian(csv_data["Xq10"], return_var=True), jac_ref, "one", ((64,), (64, 10)))


def test_ard_constant_kernel_matches_fixture(csv_data, jac_ref):
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, WhiteKernel
    gp = _gp(ConstantKernel(2.0) * RBF(jac_ref["ard_ls"]) + WhiteKernel(0.05), alpha=1e-5, normalize_y=True)
    gp.fit(csv_data["X10"], csv_data["Y6"][:, [2]])
    _check_case(gp.predict_jacobian(csv_data["Xq10"], return_var=True), jac_ref, "ard", ((64,), (64, 10)))


def _package_gp(csv_data, jac_ref):
    from unmanned_aerial_vehicles_amd.package_gp import GaussianProcess
    g = GaussianProcess(input_dim=10, output_dim=6, device=0)
    g.kernel.length_scale, g.kernel.signal_variance, g.noise_variance = (float(v) for v in jac_ref["pkg_hyper"])
    g.add_training_data(csv_data["X10"], csv_data["Y6"])
    g.fit()
    return g


def test_package_gp_matches_fixture(csv_data, jac_ref):
    g = _package_gp(csv_data, jac_ref)
    mean, var, dmean, dvar = g.predict_jacobian(csv_data["Xq10"])
    assert mean.shape == (64, 6) and var.shape == (64, 6) and dmean.shape == (64, 6, 10) and dvar.shape == (64, 10)
    errs = (relerr(mean, jac_ref["pkg_mean"]), relerr(var[:, 0], jac_ref["pkg_var"]), relerr(dmean, jac_ref["pkg_dmean"]),
            relerr(dvar, jac_ref["pkg_dvar"]))
    print("pkg", errs)
    assert max(errs) < FP64_BAR
    assert np.array_equal(var, np.tile(var[:, :1], (1, 6)))
    # a failed fit (the reference's except branch): the prior and zeros, never raising
    g._model = None
    mean, var, dmean, dvar = g.predict_jacobian(csv_data["Xq10"][:5])
    assert not mean.any() and not dmean.any() and not dvar.any() and np.all(var == g.kernel.signal_variance)
    assert dmean.shape == (5, 6, 10) and dvar.shape == (5, 10)


# ---- 2: finite differences of the existing predict --------------------------------------------------------------------
def _fd4(f, X, h):
    """Fourth-order central differences of f (rows -> (M, K)) along every input: (M, K, D)."""
    M, D = X.shape
    out = None
    for d in range(D):
        acc = 0.0
        for w, s in zip((1.0, -8.0, 8.0, -1.0), (-2, -1, 1, 2)):
            Xs = X.copy()
            Xs[:, d] += s * h
            acc = acc + w * f(Xs)
        acc = acc / (12.0 * h)
        if out is None:
            out = np.zeros((M, acc.shape[1], D))
        out[:, :, d] = acc
    return out


@pytest.mark.parametrize("N", [1000, 3000, 20000])
def test_finite_differences_of_predict(N):
    gp, rng = _synthetic(N)
    X = 1.1 * rng.standard_normal((16, 6))
    X[:3] = gp.X_train_[:3]

    def both(Xs):
        mean, std = gp.predict(Xs, return_std=True)
        return np.concatenate([mean, std ** 2], axis=1)

    fd = _fd4(both, X, 1e-3)
    mean, dmean, var, dvar = gp.predict_jacobian(X, return_var=True)
    e1, e2 = relerr(dmean, fd[:, :2]), relerr(dvar, fd[:, 2:])
    print(f"N = {N}: dmean vs FD {e1:.2e}, dvar vs FD {e2:.2e}")
    assert e1 < FP64_BAR and e2 < FP64_BAR


# ---- 3: the routes agree --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1000, 3000, 20000])
def test_routes_agree(N):
    gp, rng = _synthetic(N)
    gp.predict(gp.X_train_[:1])
    dev = gp._dev
    comp = gp.kernel_.components()
    kss = comp.sf2 + comp.noise
    prior = kss * gp._y_train_std ** 2
    for M in (1, 25, 32, 33, 64, 200, 1000, 5000):
        X = 1.1 * rng.standard_normal((M, 6))
        if M >= 5:
            X[:5] = gp.X_train_[:5]            # queries at training points: variances near the noise level
        dm_d, v_d, dv_d = (t.cpu().numpy() for t in dev.predict_grad_dev(X, gp._y_train_std, kss, 0.0))
        assert dm_d.shape == (M, 2, 6) and dv_d.shape == (M, 6) and v_d.shape == (M,)
        assert np.isfinite(dm_d).all() and np.isfinite(dv_d).all()
        routes = {}
        if M <= 4096:
            routes["host"] = dev.predict_grad_host(X, gp._y_train_mean, gp._y_train_std, kss, 0.0)
            dev.be.set_options(small_path=0)
            try:
                routes["host_large"] = dev.predict_grad_host(X, gp._y_train_mean, gp._y_train_std, kss, 0.0)
            finally:
                dev.be.set_options(small_path=1)
            m_only = dev.predict_grad_host(X, gp._y_train_mean, gp._y_train_std)
            assert m_only[1] is None and m_only[3] is None
            assert relerr(m_only[2], dm_d) < ROUTE_BAR and relerr(m_only[0], routes["host"][0]) < 1e-12
        for name, (mean, var, dmean, dvar) in routes.items():
            e = (relerr(dmean, dm_d), relerr(dvar, dv_d), float(np.max(np.abs(var - v_d))) / kss)
            print(f"N = {N}, M = {M}, {name}: dmean {e[0]:.2e} dvar {e[1]:.2e} var {e[2]:.2e}")
            assert e[0] < ROUTE_BAR and e[1] < ROUTE_BAR and e[2] < 1e-12, (N, M, name, e)
        # the estimator's surface: its mean is predict's, its variance predict's std squared
        mean, dmean, y_var, dvar = gp.predict_jacobian(X, return_var=True)
        pm, ps = gp.predict(X, return_std=True)
        assert relerr(mean, pm) < 1e-12
        unclipped = ps > 0
        assert float(np.max(np.abs(y_var - ps ** 2)[unclipped] / np.broadcast_to(prior, y_var.shape)[unclipped])) < 1e-12
        assert relerr(dmean, dm_d) < ROUTE_BAR
        assert relerr(dvar, dv_d[:, None, :] * (gp._y_train_std ** 2)[None, :, None]) < ROUTE_BAR
        m2, d2 = gp.predict_jacobian(X)
        assert relerr(m2, pm) < 1e-12 and relerr(d2, dm_d) < ROUTE_BAR


# ---- 4: run to run -------------------------------------------------------------------------------------------------
# (M <= 256: the host call - small path up to 32 rows; M = 500: the device route, one panel; M = 70 000: the device route with two
# launches of the mean Jacobian and five variance-gradient panels)
@pytest.mark.parametrize("N,M", [(1000, 25), (1000, 32), (3000, 7), (16000, 25), (3000, 500), (3000, 100), (3000, 70000)])
def test_repeatable(N, M):
    gp, rng = _synthetic(N)
    X = rng.standard_normal((M, 6))
    a = gp.predict_jacobian(X, return_var=True)
    b = gp.predict_jacobian(X, return_var=True)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    c = gp.predict_jacobian(X)
    d = gp.predict_jacobian(X)
    assert np.array_equal(c[0], d[0]) and np.array_equal(c[1], d[1])
    # the device route itself, whatever the batch size
    comp = gp.kernel_.components()
    e = gp._dev.predict_grad_dev(X, gp._y_train_std, comp.sf2 + comp.noise, 0.0)
    f = gp._dev.predict_grad_dev(X, gp._y_train_std, comp.sf2 + comp.noise, 0.0)
    for u, v in zip(e, f):
        assert np.array_equal(u.cpu().numpy(), v.cpu().numpy())


# ---- 5: structure --------------------------------------------------------------------------------------------------
def test_variance_gradient_vanishes_at_training_rows():
    from unmanned_aerial_vehicles_amd import RBF, WhiteKernel
    rng = np.random.default_rng(5)
    N, D = 1000, 6
    Xt = rng.standard_normal((N, D))
    Y = np.sin(Xt @ rng.standard_normal((D, 2))) + 0.01 * rng.standard_normal((N, 2))
    gp = _gp(RBF(1.6) + WhiteKernel(1e-4), alpha=1e-6, normalize_y=True).fit(Xt, Y)
    X = 1.1 * rng.standard_normal((64, D))
    X[:5] = Xt[:5]
    _, _, _, dvar = gp.predict_jacobian(X, return_var=True)
    norms = np.linalg.norm(dvar[:, 0, :], axis=1)
    ratio = float(norms[:5].max() / norms.max())
    print(f"|dvar| at training rows / largest over the batch: {ratio:.2e}")
    assert ratio <= 1e-2


def test_ard_feature_scaling(csv_data, jac_ref):
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, WhiteKernel
    X, y, Xq, ls = csv_data["X10"], csv_data["Y6"][:, [2]], csv_data["Xq10"], jac_ref["ard_ls"].copy()

    def run(X, Xq, ls):
        gp = _gp(ConstantKernel(2.0) * RBF(ls) + WhiteKernel(0.05), alpha=1e-5, normalize_y=True).fit(X, y)
        return gp.predict_jacobian(Xq, return_var=True)

    a = run(X, Xq, ls)
    d = 3
    s = np.ones(10)
    s[d] = 3.0
    b = run(X * s, Xq * s, ls * s)
    for u, v in ((a[1], b[1]), (a[3], b[3])):       # column d divided by 3, the others unchanged
        e = relerr(v * s, u)
        print(f"feature scaling: {e:.2e}")
        assert e < 1e-10


# ---- 6: model seams ------------------------------------------------------------------------------------------------
def _flight_model(csv_data):
    from unmanned_aerial_vehicles_amd.simple_gp import SimpleQuadrotorGP
    m = SimpleQuadrotorGP(device=0)
    m.gp_model = _ka1(csv_data, normalize_y=True)
    m.is_trained = True
    return m


def test_predict_residual_jacobian(csv_data, jac_ref):
    from unmanned_aerial_vehicles_amd.simple_gp import SimpleQuadrotorGP
    m = _flight_model(csv_data)
    Xq = csv_data["Xq10"]
    for i in (0, 7, 40):
        mean, J = m.predict_residual_jacobian(Xq[i, :6], Xq[i, 6:])
        assert mean.shape == (6,) and J.shape == (6, 10)
        assert relerr(mean, jac_ref["ka1_mean"][i]) < FP64_BAR and relerr(J, jac_ref["ka1_dmean"][i]) < FP64_BAR
    mean, J = SimpleQuadrotorGP(device=0).predict_residual_jacobian(Xq[0, :6], Xq[0, 6:])
    assert mean.shape == (6,) and J.shape == (6, 10) and not mean.any() and not J.any()


def test_linearize_gp_residuals(csv_data, jac_ref):
    m = _flight_model(csv_data)
    Xq = csv_data["Xq10"]
    N, dt, gain = 20, 0.05, 0.1
    Xg = np.zeros((6, N + 1))
    Xg[:, :N] = Xq[:N, :6].T
    Ug = Xq[:N, 6:].T.copy()
    D, A, B = m.linearize_gp_residuals(Xg, Ug, dt, gain)
    assert D.shape == (6, N) and A.shape == (N, 6, 6) and B.shape == (N, 6, 4)
    assert relerr(D, m.build_gp_residuals(Xg, Ug, dt, gain)) < 1e-12
    J = jac_ref["ka1_dmean"][:N]
    assert relerr(A[:, 3:6, :], gain / dt * J[:, 3:6, :6]) < FP64_BAR
    assert relerr(B[:, 3:6, :], gain / dt * J[:, 3:6, 6:10]) < FP64_BAR
    assert not A[:, :3].any() and not B[:, :3].any() and not D[:3].any()
    # R = 3 rollouts
    Xr = np.stack([Xg, np.roll(Xg, 1, axis=1), np.roll(Xg, 2, axis=1)])
    Ur = np.stack([Ug, np.roll(Ug, 1, axis=1), np.roll(Ug, 2, axis=1)])
    D3, A3, B3 = m.linearize_gp_residuals(Xr, Ur, dt, gain)
    assert D3.shape == (3, 6, N) and A3.shape == (3, N, 6, 6) and B3.shape == (3, N, 6, 4)
    assert relerr(D3, m.build_gp_residuals(Xr, Ur, dt, gain)) < 1e-12
    assert relerr(A3[0], A) < ROUTE_BAR and relerr(B3[0], B) < ROUTE_BAR
    D1, A1, B1 = m.linearize_gp_residuals(Xr[1], Ur[1], dt, gain)
    assert relerr(A3[1], A1) < ROUTE_BAR and relerr(B3[1], B1) < ROUTE_BAR and relerr(D3[1], D1) < ROUTE_BAR


# ---- 7: fp32-serving models and replicas ------------------------------------------------------------------------------
def test_fp32_serving_model_and_replica(csv_data):
    from unmanned_aerial_vehicles_amd.device import DeviceGP
    Xq = csv_data["Xq10"]
    a = _ka1(csv_data, normalize_y=True).predict_jacobian(Xq, return_var=True)
    gp32 = _ka1(csv_data, normalize_y=True, predict_dtype="float32")
    b = gp32.predict_jacobian(Xq, return_var=True)
    for u, v in zip(a, b):
        assert v.dtype == np.float64 and relerr(v, u) < 1e-12
    gp32.predict(Xq[:2])
    dev = gp32._dev
    meta, tensors = dev.serving_state()
    rep = DeviceGP.from_serving_state(meta, tensors, dev.be)
    comp = gp32.kernel_.components()
    with pytest.raises(RuntimeError, match="replica"):
        rep.predict_grad_dev(Xq, gp32._y_train_std, comp.sf2 + comp.noise)
    with pytest.raises(RuntimeError, match="replica"):
        rep.predict_grad_host(Xq, gp32._y_train_mean, gp32._y_train_std, comp.sf2 + comp.noise)
    dm, var, dv = rep.predict_grad_dev(Xq, gp32._y_train_std)
    assert var is None and dv is None and relerr(dm.cpu().numpy(), a[1]) < 1e-12
    mean, var, dm, dv = rep.predict_grad_host(Xq[:25], gp32._y_train_mean, gp32._y_train_std)
    assert var is None and dv is None and relerr(dm, a[1][:25]) < 1e-12 and relerr(mean, a[0][:25]) < 1e-12


def test_input_validation_and_prior(csv_data):
    from unmanned_aerial_vehicles_amd import GaussianProcessRegressor
    gp = _ka1(csv_data, normalize_y=True)
    bad = csv_data["Xq10"][:3].copy()
    bad[1, 2] = np.nan
    with pytest.raises(ValueError, match="NaN or infinity"):
        gp.predict_jacobian(bad)
    mean, dmean, var, dvar = GaussianProcessRegressor(n_targets=3).predict_jacobian(np.zeros((4, 5)), return_var=True)
    assert mean.shape == (4, 3) and dmean.shape == (4, 3, 5) and var.shape == (4, 3) and dvar.shape == (4, 3, 5)
    assert not dmean.any() and not dvar.any() and np.all(var == 1.0)


# ---- 8: the headline size ---------------------------------------------------------------------------------------------
def test_headline_size_directional_difference():
    """N = 65 536, D = 9, P = 3 (test_baseline_size_properties' problem), M = 256: finite results, and a directional
    fourth-order difference of the existing fp64 predict(return_std=True) along one random direction against dmean . v and
    dvar . v.  The stencil's own error at this size is estimated from its values at h = 1e-3 and 2e-3; the bar is
    max(1e-6, 10 x that difference) - 1e-6 being what test_gpu_c5.py uses for its finite-difference check at size, the factor
    10 covering that the estimate is itself first-order.
    Measured on MI355X: dmean . v - h / 2h difference of the stencil 1.57e-10, agreement with it 1.44e-10; dvar . v - 6.80e-11 and
    6.10e-11: ten times the stencil's own error is far below 1e-6, so the bar that applied is the 1e-6 floor (margin ~7000x).
    HBM reserved at the peak of the call, sampled every millisecond: 82.8 GiB - and as much before it: the 32 GiB inverse factor
    and its scratch went into blocks the caching allocator had kept from the fit and the solve-route predict calls above."""
    import torch
    from oracle import gp_oracle as O
    from unmanned_aerial_vehicles_amd import RBF, WhiteKernel
    N, M = 65536, 256
    X, Y, _ = O.synthetic_problem(N, 1)
    gp = _gp(RBF(2.0) + WhiteKernel(0.1), alpha=1e-4, normalize_y=True).fit(X, Y)
    rng = np.random.default_rng(8)
    Xq = rng.standard_normal((M, X.shape[1]))
    Xq[:4] = X[[7, 4099, 30000, N - 1]]
    v = rng.standard_normal(X.shape[1])
    v /= np.linalg.norm(v)

    def quotient(h):
        acc = 0.0
        for w, s in zip((1.0, -8.0, 8.0, -1.0), (-2, -1, 1, 2)):
            mean, std = gp.predict(Xq + s * h * v, return_std=True)
            acc = acc + w * np.concatenate([mean, std ** 2], axis=1)
        return acc / (12.0 * h)

    q1, q2 = quotient(1e-3), quotient(2e-3)
    P = Y.shape[1]
    # peak HBM of the call: free memory sampled every millisecond from a host thread while it runs (it sees torch's allocator
    # and the library's own allocations alike: the inverse factor and the scratch of its formation, the three panels)
    import threading
    import time
    total = torch.cuda.mem_get_info(0)[1]
    low, stop = [torch.cuda.mem_get_info(0)[0]], threading.Event()

    def sample():
        while not stop.is_set():
            low[0] = min(low[0], torch.cuda.mem_get_info(0)[0])
            time.sleep(1e-3)

    before = total - low[0]
    th = threading.Thread(target=sample, daemon=True)
    th.start()
    mean, dmean, var, dvar = gp.predict_jacobian(Xq, return_var=True)
    stop.set()
    th.join()
    assert all(np.isfinite(a).all() for a in (mean, dmean, var, dvar))
    assert dmean.shape == (M, P, X.shape[1]) and dvar.shape == (M, P, X.shape[1])
    for name, g, a, b in (("dmean.v", dmean @ v, q1[:, :P], q2[:, :P]), ("dvar.v", dvar @ v, q1[:, P:], q2[:, P:])):
        stencil = relerr(a, b)
        err = relerr(g, a)
        bar = max(1e-6, 10.0 * stencil)
        print(f"N = 65536 {name}: stencil h / 2h difference {stencil:.2e}, agreement {err:.2e}, bar {bar:.2e}")
        assert err < bar
    print(f"HBM in use before the call {before / 2**30:.1f} GiB, peak during it {(total - low[0]) / 2**30:.1f} GiB")
