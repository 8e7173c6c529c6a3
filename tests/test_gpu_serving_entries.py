"""The five one-call serving entries (gpk_predict_host, _host_multi, _host_cov, _host_grad, _host_multi_grad) agree with one
another on what they share: with the small-batch kernels (small_path = 1, up to 32 rows) a mean, a variance or a Jacobian is
the same bits whichever entry, and whichever request, returned it - the kernels add the workgroups' shares in an order that
depends on the shape only.  The covariance's diagonal comes from a different summation (V_r^T V_r per workgroup instead of
squares), so it agrees with the variance to rounding, not to the bit."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS = (1, 16, 17, 32)      # one and two 16-query blocks of the variance kernels, full and ragged


def _fit(P, seed=0):
    """N = 200 (Np = 256: the first row blocks of W have fewer 64-wide k-chunks than the variance kernel has waves), D = 3."""
    from unmanned_aerial_vehicles_amd import RBF, GaussianProcessRegressor, WhiteKernel
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((200, 3))
    Y = np.sin(X @ rng.standard_normal((3, P))) + 0.1 * rng.standard_normal((200, P))
    gp = GaussianProcessRegressor(kernel=RBF(1.6) + WhiteKernel(0.05), alpha=1e-6, normalize_y=True, optimizer=None, device=0)
    gp.fit(X, Y)
    gp.predict(X[:1])
    comp = gp.kernel_.components()
    Q = 1.1 * rng.standard_normal((32, 3))
    Q[:3] = X[:3]               # queries at training points: variances near the noise level
    return gp, comp.sf2 + comp.noise, comp.noise, Q


@pytest.fixture(scope="module")
def two_outputs():
    return _fit(2)


@pytest.fixture(scope="module")
def one_output():
    return _fit(1, seed=1)


@pytest.mark.parametrize("M", ROWS)
def test_single_model_entries_share_bits(two_outputs, M):
    gp, kss, noise, Q = two_outputs
    dev, ym, ys, X = gp._dev, gp._y_train_mean, gp._y_train_std, Q[:M]
    mean_only, none = dev.predict_host(X, ym, ys)
    mean_var, var = dev.predict_host(X, ym, ys, kss, 0.0)
    mean_cov, cov = dev.predict_cov_host(X, ym, ys, noise)
    mean_jac, none_v, jac, none_dv = dev.predict_grad_host(X, ym, ys)
    mean_all, var_all, jac_all, dvar = dev.predict_grad_host(X, ym, ys, kss, 0.0)
    assert none is None and none_v is None and none_dv is None
    assert mean_only.shape == (M, 2) and var.shape == (M,) and cov.shape == (M, M) and jac.shape == (M, 2, 3) and dvar.shape == (M, 3)
    for name, other in (("with variance", mean_var), ("cov", mean_cov), ("mean + Jacobian", mean_jac), ("grad, all four", mean_all)):
        assert np.array_equal(mean_only, other), (M, name, float(np.max(np.abs(mean_only - other))))
    assert np.array_equal(var, var_all), (M, float(np.max(np.abs(var - var_all))))
    assert np.array_equal(jac, jac_all), (M, float(np.max(np.abs(jac - jac_all))))
    # diag(cov) = kss - sum_r V_rm^2 unclipped; var = max(kss - sum_r V_rm^2, floor = 0)
    unclipped = var > 0.0
    assert unclipped.any()
    e = float(np.max(np.abs(np.diag(cov) - var)[unclipped])) / kss
    print(f"M = {M}: |diag(cov) - var| / kss = {e:.2e}")
    assert e < 1e-12


@pytest.mark.parametrize("M", ROWS)
def test_per_axis_entry_with_one_model_is_the_single_model_entry(one_output, M):
    gp, kss, noise, Q = one_output
    dev, X = gp._dev, Q[:M]
    want_mean, want_var = dev.predict_host(X, gp._y_train_mean, gp._y_train_std, kss, 0.0)
    want_only, _ = dev.predict_host(X, gp._y_train_mean, gp._y_train_std)
    W = dev.inverse_factor(False)
    one = C.c_void_p * 1
    ym, ys = (np.ascontiguousarray(v, dtype=np.float64).reshape(1) for v in (gp._y_train_mean, gp._y_train_std))
    ls, sf2, k = np.ascontiguousarray(dev.ls, dtype=np.float64), np.array([dev.sf2]), np.array([kss])
    be = dev.be
    for with_var in (False, True):
        mean, var = np.empty((1, M)), np.empty((1, M))
        with be.lock:
            be.bind_stream()
            be.check(be.lib.gpk_predict_host_multi(
                be.h, 1, one(dev.X.data_ptr()), one(dev.alpha.data_ptr()), dev.N, dev.D, ls.ctypes.data, sf2.ctypes.data,
                ym.ctypes.data, ys.ctypes.data, one(W.data_ptr()) if with_var else None, dev.Np, dev.Np, k.ctypes.data, 0.0,
                X.ctypes.data, M, mean.ctypes.data, var.ctypes.data if with_var else None))
        assert np.array_equal(mean[0], (want_mean if with_var else want_only)[:, 0]), (M, with_var)
        if with_var:
            assert np.array_equal(var[0], want_var), M
