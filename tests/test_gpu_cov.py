"""Joint posterior on the GPU: GaussianProcessRegressor.predict(X, return_cov=True), sample_y and the C entries behind them
(gpk_predict_cov_inv / gpk_predict_cov / gpk_predict_host_cov / gpk_predict_model_cov) against scikit-learn's recorded
answers (tests/golden/cov_ref.npz, tests/golden/make_golden_cov.py) and against each other."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest

from conftest import GOLDEN, relerr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cov_ref():
    d = np.load(os.path.join(GOLDEN, "cov_ref.npz"))
    return {k: d[k] for k in d.files}


def _gp(kernel, **kw):
    from unmanned_aerial_vehicles_amd import GaussianProcessRegressor
    return GaussianProcessRegressor(kernel=kernel, optimizer=None, device=0, **kw)


def _ka1(csv_data, y=None, **kw):
    from unmanned_aerial_vehicles_amd import RBF, WhiteKernel
    y = csv_data["Y6"] if y is None else y
    return _gp(RBF(0.5) + WhiteKernel(0.1), alpha=1e-4, **kw).fit(csv_data["X10"], y)


def _synthetic(N, D=6, P=2, seed=0, **kw):
    from unmanned_aerial_vehicles_amd import RBF, WhiteKernel
    rng = np.random.default_rng(seed + N)
    X = rng.standard_normal((N, D))
    Y = np.sin(X @ rng.standard_normal((D, P))) + 0.1 * rng.standard_normal((N, P))
    gp = _gp(RBF(1.6) + WhiteKernel(0.05), alpha=1e-6, normalize_y=True, **kw).fit(X, Y)
    return gp, rng


def _symmetric(cov):
    c = cov if cov.ndim == 3 else cov[:, :, None]
    return all(np.array_equal(c[..., p], c[..., p].T) for p in range(c.shape[2]))


# ---- 1, 2: parity with scikit-learn and shapes ----------------------------------------------------------------------
def test_ka1_cov_matches_sklearn(csv_data, cov_ref):
    gp = _ka1(csv_data, normalize_y=True)
    mean, cov = gp.predict(csv_data["Xq10"], return_cov=True)
    assert mean.shape == (64, 6) and cov.shape == (64, 64, 6)
    assert relerr(cov, cov_ref["ka1_cov"]) < 1e-8
    assert relerr(mean, cov_ref["ka1_mean"]) < 1e-8
    for p in range(6):
        assert relerr(cov[..., p], cov_ref["ka1_cov"][..., p]) < 1e-8
    assert _symmetric(cov)


def test_one_target_unnormalised_matches_sklearn(csv_data, cov_ref):
    gp = _ka1(csv_data, y=csv_data["Y6"][:, 0], normalize_y=False)
    mean, cov = gp.predict(csv_data["Xq10"], return_cov=True)
    assert mean.shape == (64,) and cov.shape == (64, 64)
    assert relerr(cov, cov_ref["one_cov"]) < 1e-8 and relerr(mean, cov_ref["one_mean"]) < 1e-8
    assert _symmetric(cov)


def test_ard_constant_kernel_matches_sklearn(csv_data, cov_ref):
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, WhiteKernel
    gp = _gp(ConstantKernel(2.0) * RBF(cov_ref["ard_ls"]) + WhiteKernel(0.05), alpha=1e-5, normalize_y=True)
    gp.fit(csv_data["X10"], csv_data["Y6"][:, [2]])          # 2-D y with one column: sklearn squeezes to (M,) / (M, M)
    mean, cov = gp.predict(csv_data["Xq10"], return_cov=True)
    assert mean.shape == (64,) and cov.shape == (64, 64)
    assert relerr(cov, cov_ref["ard_cov"]) < 1e-8 and relerr(mean, cov_ref["ard_mean"]) < 1e-8


def test_prior_cov_matches_sklearn(csv_data, cov_ref):
    from unmanned_aerial_vehicles_amd import RBF, GaussianProcessRegressor, WhiteKernel
    gp = GaussianProcessRegressor(kernel=RBF(0.5) + WhiteKernel(0.1), alpha=1e-4, normalize_y=True, device=0)
    mean, cov = gp.predict(csv_data["Xq10"][:25], return_cov=True)
    assert mean.shape == cov_ref["prior_mean"].shape and cov.shape == (25, 25)
    assert relerr(cov, cov_ref["prior_cov"]) < 1e-8 and np.array_equal(mean, cov_ref["prior_mean"])
    assert _symmetric(cov)
    # noise on the diagonal only: a duplicated query row gets the prior variance off the diagonal, not + noise
    Xd = np.vstack([csv_data["Xq10"][:3], csv_data["Xq10"][:1]])
    _, cd = gp.predict(Xd, return_cov=True)
    assert abs(cd[0, 3] - 1.0) < 1e-15 and cd[0, 0] == 1.1 and cd[3, 3] == 1.1
    gp3 = GaussianProcessRegressor(kernel=RBF(0.5) + WhiteKernel(0.1), n_targets=3, device=0)
    m3, c3 = gp3.predict(csv_data["Xq10"][:25], return_cov=True)
    assert m3.shape == (25, 3) and c3.shape == (25, 25, 3)
    assert all(np.array_equal(c3[..., p], cov) for p in range(3))


# ---- 3, 4, 5: consistency with the variance path, symmetry, the two routes --------------------------------------------
def _check_diag(gp, X, cov):
    _, std = gp.predict(X, return_std=True)
    comp = gp.kernel_.components()
    prior = (comp.sf2 + (comp.noise or 0.0)) * gp._y_train_std ** 2
    var = std ** 2
    c = cov if cov.ndim == 3 else cov[:, :, None]
    v = var if var.ndim == 2 else var[:, None]
    for p in range(c.shape[2]):
        d = np.diag(c[..., p])
        keep = v[:, p] > 0
        assert np.max(np.abs(d[keep] - v[keep, p])) <= 1e-12 * prior[p]


@pytest.mark.parametrize("N", [1000, 3000, 20000])
def test_routes_agree(N):
    from oracle import gp_oracle as O
    gp, rng = _synthetic(N)
    st = None
    for M in (1, 25, 32, 33, 64, 200, 1000):
        X = rng.standard_normal((M, 6)) * 1.1
        if M >= 25:
            X[:5] = gp.X_train_[:5]            # queries at training points: variances near the noise level
        gp.var_method = "auto"
        m1, c1 = gp.predict(X, return_cov=True)
        gp.var_method = "solve"
        m2, c2 = gp.predict(X, return_cov=True)
        gp.var_method = "auto"
        assert c1.shape == (M, M, 2)
        assert _symmetric(c1) and _symmetric(c2)
        assert relerr(c2, c1) < 1e-12, (N, M)
        assert relerr(m2, m1) < 1e-12
        _check_diag(gp, X, c1)
        if N == 1000 and M in (33, 200, 1000):
            # both routes end in the same launch: an answer that shares none of it (NumPy, oracle.gp_oracle.predict_cov)
            if st is None:
                st = O.fit_fixed(gp.X_train_, np.zeros((N, 1)), 1.6, 1.0, 0.05, 1e-6, normalize_y=False)
            want = O.predict_cov(st, X, 0.05)[:, :, None] * gp._y_train_std ** 2
            e = relerr(c1, want)
            print(f"N {N} M {M}: covariance against the oracle {e:.2e} of its largest entry")
            assert e < 1e-8


def test_solve_route_default_at_40000():
    gp, rng = _synthetic(40000, P=1)
    assert gp._dev._fp64_var_method() == "solve"
    X = rng.standard_normal((300, 6))
    X[:3] = gp.X_train_[:3]
    mean, cov = gp.predict(X, return_cov=True)
    assert cov.shape == (300, 300) and mean.shape == (300,)
    assert _symmetric(cov)
    assert "f64" not in gp._dev._Winv          # no inverse factor was formed for it
    _check_diag(gp, X, cov)


# ---- 6: repeatability ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M", [(1000, 25), (1000, 32), (3000, 7), (16000, 25), (3000, 500)])
def test_repeatable(N, M):
    gp, rng = _synthetic(N)
    X = rng.standard_normal((M, 6))
    m1, c1 = gp.predict(X, return_cov=True)
    m2, c2 = gp.predict(X, return_cov=True)
    assert np.array_equal(c1, c2) and np.array_equal(m1, m2)


# ---- 7: other model sources ----------------------------------------------------------------------------------------
def test_imported_pickled_and_fp32_models(csv_data):
    from sklearn.gaussian_process import GaussianProcessRegressor as SkGPR
    from sklearn.gaussian_process.kernels import RBF as SkRBF, WhiteKernel as SkWhite
    from unmanned_aerial_vehicles_amd import GaussianProcessRegressor
    X, Y, Xq = csv_data["X10"], csv_data["Y6"], csv_data["Xq10"]
    gp = _ka1(csv_data, normalize_y=True)
    m0, c0 = gp.predict(Xq, return_cov=True)
    skl = SkGPR(kernel=SkRBF(0.5) + SkWhite(0.1), alpha=1e-4, normalize_y=True, optimizer=None).fit(X, Y)
    imp = GaussianProcessRegressor.from_sklearn(skl, device=0)
    m1, c1 = imp.predict(Xq, return_cov=True)
    assert relerr(c1, c0) < 1e-10 and relerr(m1, m0) < 1e-10
    back = pickle.loads(pickle.dumps(gp))
    m2, c2 = back.predict(Xq, return_cov=True)
    assert np.array_equal(c2, c0) and np.array_equal(m2, m0)
    f32 = _ka1(csv_data, normalize_y=True, predict_dtype="float32")
    m3, c3 = f32.predict(Xq, return_cov=True)
    assert c3.dtype == np.float64 and relerr(c3, c0) < 1e-12 and relerr(m3, m0) < 1e-12


# ---- 8: sample_y --------------------------------------------------------------------------------------------------
def test_sample_y(csv_data, cov_ref):
    Xq = csv_data["Xq10"][:25]
    gp = _ka1(csv_data, y=csv_data["Y6"][:, 0], normalize_y=False)
    s = gp.sample_y(Xq, 8, random_state=0)
    mean, cov = gp.predict(Xq, return_cov=True)
    assert np.array_equal(s, np.random.RandomState(0).multivariate_normal(mean, cov, 8).T)
    assert s.shape == cov_ref["one_samples"].shape == (25, 8)
    # multivariate_normal draws through an SVD: the singular vectors follow the covariance's entries (here ~1e-13 apart)
    # to ~1e-13 / gap - the comparison is meaningful where that is far below the bar
    if cov_ref["one_gap"][0] > 1e-5:
        assert np.max(np.abs(s - cov_ref["one_samples"])) < 1e-6 * np.max(np.abs(cov_ref["one_samples"]))
    g6 = _ka1(csv_data, normalize_y=True)
    s6 = g6.sample_y(Xq, 8, random_state=0)
    assert s6.shape == cov_ref["ka1_samples"].shape == (25, 6, 8)
    m6, c6 = g6.predict(Xq, return_cov=True)
    rng = np.random.RandomState(0)
    for p in range(6):
        assert np.array_equal(s6[:, p, :], rng.multivariate_normal(m6[:, p], c6[..., p], 8).T)
        if cov_ref["ka1_gap"][p] > 1e-5:
            ref = cov_ref["ka1_samples"][:, p, :]
            assert np.max(np.abs(s6[:, p, :] - ref)) < 1e-6 * np.max(np.abs(ref))
    # random_state semantics (check_random_state): a RandomState instance is used as it is
    r = np.random.RandomState(5)
    a = g6.sample_y(Xq, 2, random_state=r)
    assert not np.array_equal(a, g6.sample_y(Xq, 2, random_state=r))


# ---- 9: the C entries ---------------------------------------------------------------------------------------------
def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_model_cov_after_fit_agrees_with_estimator(csv_data):
    from unmanned_aerial_vehicles_amd import _lib
    lib = _lib.load()
    X, Y = np.ascontiguousarray(csv_data["X10"]), np.ascontiguousarray(csv_data["Y6"])
    Xq = np.ascontiguousarray(csv_data["Xq10"])
    gp = _ka1(csv_data, normalize_y=True)
    h = C.c_void_p()
    assert lib.gpk_create(C.byref(h), 0) == _lib.GPK_OK
    try:
        def ok(rc):
            assert rc == _lib.GPK_OK, lib.gpk_last_error(h).decode()
        ok(lib.gpk_set_stream(h, C.c_void_p(-1)))
        ls = np.array([0.5])
        ok(lib.gpk_fit(h, _dp(X), X.shape[0], 10, _dp(Y), 6, _dp(ls), 1, 1.0, 0.1, 1e-4, 1))
        for M in (25, 64):
            mean, cov = np.empty((M, 6)), np.empty((6, M, M))
            ok(lib.gpk_predict_model_cov(h, _dp(np.ascontiguousarray(Xq[:M])), M, _dp(mean), _dp(cov)))
            em, ec = gp.predict(Xq[:M], return_cov=True)
            assert relerr(mean, em) < 1e-12
            assert relerr(np.moveaxis(cov, 0, -1), ec) < 1e-12
    finally:
        lib.gpk_destroy(h)


def test_host_cov_agrees_with_building_block():
    import torch
    gp, rng = _synthetic(3000)
    dev = gp._dev
    be = dev.be
    for M in (5, 25, 32, 40, 200):
        X = rng.standard_normal((M, 6))
        _, ch = dev.predict_cov_host(X, gp._y_train_mean, gp._y_train_std, 0.05)
        q = dev._as_queries(X, torch.float64)
        Mp = (M + 127) // 128 * 128
        W = dev.inverse_factor(False)
        work = be.empty((dev.Np * Mp,), torch.float64)
        cov = be.empty((Mp, Mp), torch.float64)
        with be.lock:
            be.bind_stream()
            be.check(be.lib.gpk_predict_cov_inv(be.h, 1, dev.X.data_ptr(), dev.N, dev.D, dev.ls.ctypes.data_as(C.POINTER(C.c_double)),
                                                dev.sf2, W.data_ptr(), dev.Np, dev.Np, q.data_ptr(), M, 0.05, work.data_ptr(),
                                                cov.data_ptr(), Mp))
            be.sync()
        full = cov.cpu().numpy()
        assert np.all(np.isfinite(full))                       # the padding is written too (the buffers start as NaN)
        assert np.all(full[M:, :] == 0.0) and np.all(full[:, M:] == 0.0)
        assert relerr(ch, full[:M, :M]) < 1e-12, M
        assert np.array_equal(ch, ch.T)


def test_building_blocks_reject_fp32():
    import torch
    gp, rng = _synthetic(1000)
    dev = gp._dev
    be = dev.be
    q = dev._as_queries(rng.standard_normal((4, 6)), torch.float64)
    work = be.empty((dev.Np * 128,), torch.float64)
    cov = be.empty((128, 128), torch.float64)
    W = dev.inverse_factor(False)
    rc = be.lib.gpk_predict_cov_inv(be.h, 0, dev.X.data_ptr(), dev.N, dev.D, dev.ls.ctypes.data_as(C.POINTER(C.c_double)),
                                    dev.sf2, W.data_ptr(), dev.Np, dev.Np, q.data_ptr(), 4, 0.05, work.data_ptr(),
                                    cov.data_ptr(), 128)
    assert rc == 2 and b"fp64 only" in be.lib.gpk_last_error(be.h)


# ---- 10: errors ---------------------------------------------------------------------------------------------------
def test_errors(csv_data):
    gp = _ka1(csv_data, normalize_y=True)
    with pytest.raises(RuntimeError, match="At most one of return_std or return_cov"):
        gp.predict(csv_data["Xq10"], return_std=True, return_cov=True)
    with pytest.raises(ValueError, match="VAR_PANEL_MAX"):
        gp.predict(np.zeros((16385, 10)), return_cov=True)
    big, _ = _synthetic(1000, P=1)
    big._dev.VAR_PANEL_BYTES = big._dev.Np * 128 * 8   # (an instance-level limit: V of 129 queries no longer fits)
    with pytest.raises(ValueError, match="VAR_PANEL_BYTES"):
        big.predict(np.zeros((129, 6)), return_cov=True)
    assert big.predict(np.zeros((128, 6)), return_cov=True)[1].shape == (128, 128)
