"""Mean Hessians of the per-axis GP batch on the GPU: BatchedARDGP.predict_hessian / predict_host_hess
(gpk_predict_host_multi_hess) and PreTrainedGP.predict_residual_hessian_batch in raw units, against the closed forms of
tests/golden/hess_ref.npz (case `axis`, tests/golden/make_golden_hess.py), against finite differences of the batch's own
predict_jacobian, and model by model against the single-model call.

Raw Hessian entries of the yaw-rate column are ~1e32 and more (its scaler's scale is ~1e-21), so the raw-unit comparison is made
twice: relative to the largest entry, and entry by entry in units of the inputs' scales (the Hessian on the scaled inputs)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, relerr

pytestmark = pytest.mark.gpu

FP64_BAR = 1e-8
ROUTE_BAR = 1e-11


@pytest.fixture(scope="module")
def hess_ref():
    d = np.load(os.path.join(GOLDEN, "hess_ref.npz"))
    return {k: d[k] for k in d.files}


def _axis_models(X, Y, B, ls_of, noise_of):
    """test_gpu_axis_jac._axis_models: B scalar models on shared inputs, C(1, fixed) * RBF(ls_b) + White(noise_b), alpha 1e-6."""
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, GaussianProcessRegressor, WhiteKernel
    ms = []
    for b in range(B):
        k = ConstantKernel(1.0, constant_value_bounds="fixed") * RBF(ls_of(b)) + WhiteKernel(noise_of(b))
        ms.append(GaussianProcessRegressor(kernel=k, alpha=1e-6, normalize_y=False, optimizer=None, device=0)
                  .fit(X, Y[:, b % Y.shape[1]]))
    return ms


def _batch(models):
    from unmanned_aerial_vehicles_amd.batched import BatchedARDGP
    bg = BatchedARDGP(optimizer=None, device=0)
    bg.models = list(models)
    return bg


@pytest.fixture(scope="module")
def csv_pre(csv_data, hess_ref):
    """Case `axis` served by this package: PreTrainedGP around six models fitted here with the fixture's hyper-parameters."""
    from unmanned_aerial_vehicles_amd.trainer import OUTPUT_NAMES, PreTrainedGP, StandardScaler
    X, Y = csv_data["X10"], csv_data["Y6"]
    sx = StandardScaler().fit(X)
    assert relerr(sx.scale_, hess_ref["axis_sx_scale"]) < 1e-13 and relerr(sx.mean_, hess_ref["axis_sx_mean"]) < 1e-13
    sys_ = [StandardScaler().fit(Y[:, [b]]) for b in range(6)]
    Ys = np.concatenate([sys_[b].transform(Y[:, [b]]) for b in range(6)], axis=1)
    ms = _axis_models(sx.transform(X), Ys, 6, lambda b: hess_ref["axis_ls"][b], lambda b: float(hess_ref["axis_noise"][b]))
    pre = PreTrainedGP(os.path.join(GOLDEN, "no_such_model.pkl"))
    for b in range(6):
        n = OUTPUT_NAMES[b]
        pre.gp_models[n], pre.scalers_X[n], pre.scalers_y[n] = ms[b], sx, sys_[b]
    pre.is_loaded = True
    return pre


@pytest.fixture(scope="module")
def small_batches():
    """B = 8 scalar models at N = 129, D = 10 (two row blocks of the triangle; 32-row chunks and a tail)."""
    rng = np.random.default_rng(21)
    N, D = 129, 10
    X = rng.standard_normal((N, D))
    Y = np.sin(X @ rng.standard_normal((D, 8))) + 0.05 * rng.standard_normal((N, 8))
    ms = _axis_models(X, Y, 8, lambda b: np.roll(np.linspace(1.2, 3.0, D), b), lambda b: 0.02 * (b + 1))
    return ms, rng


# ---- 1, 7: the fixture in raw units ---------------------------------------------------------------------------------------
def test_raw_units_match_fixture(csv_pre, hess_ref):
    pre = csv_pre
    Xq = hess_ref["axis_Xq"]
    mean, J, H = pre.predict_residual_hessian_batch(Xq)
    assert pre._fused_bg, "the six models share inputs and scaler: the fused path must have served them"
    assert mean.shape == (25, 6) and J.shape == (25, 6, 10) and H.shape == (25, 6, 10, 10)
    assert np.isfinite(H).all() and np.array_equal(H, H.swapaxes(-1, -2))
    m2, J2 = pre.predict_residual_jacobian_batch(Xq)
    assert np.array_equal(mean, m2) and np.array_equal(J, J2)
    sxs, sys_ = hess_ref["axis_sx_scale"], hess_ref["axis_sy_scale"]
    unit = (sxs[:, None] * sxs[None, :])[None, None] / sys_[None, :, None, None]
    e_raw, e_scaled = relerr(H, hess_ref["axis_hess"]), relerr(H * unit, hess_ref["axis_hess_scaled"])
    print(f"axis: raw {e_raw:.2e}, in units of the scalers {e_scaled:.2e}")
    assert e_raw < FP64_BAR and e_scaled < FP64_BAR
    # the batch on the scaled inputs, and one row through the controller-facing wrapper
    bg, names = pre._fused_bg
    Z = pre.scalers_X[names[0]].transform(Xq)
    assert relerr(bg.predict_hessian(Z)[2], hess_ref["axis_hess_scaled"]) < FP64_BAR
    for i in (0, 9):
        m1, J1, H1 = pre.predict_residual_hessian(Xq[i, :6], Xq[i, 6:])
        assert m1.shape == (6,) and J1.shape == (6, 10) and H1.shape == (6, 10, 10)
        assert relerr(H1 * unit[0], hess_ref["axis_hess_scaled"][i]) < FP64_BAR and relerr(m1, mean[i]) < 1e-12


# ---- 2, 3, 7: bits of predict_jacobian, symmetry, column b = model b alone ---------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 6, 8])
def test_columns_have_the_bits_of_the_models_served_alone(small_batches, B):
    ms, rng = small_batches
    bg = _batch(ms[:B])
    alone = [_batch([m]) for m in ms[:B]]
    for M in (1, 17, 32):
        Z = 0.9 * rng.standard_normal((M, 10))
        mean, dmean, hess = bg.predict_hessian(Z)
        assert mean.shape == (M, B) and dmean.shape == (M, B, 10) and hess.shape == (M, B, 10, 10)
        assert np.isfinite(hess).all() and np.array_equal(hess, hess.swapaxes(-1, -2))
        jac = bg.predict_jacobian(Z)
        assert np.array_equal(mean, jac[0]) and np.array_equal(dmean, jac[1])
        for b in range(B):
            m1, d1, h1 = alone[b].predict_host_hess(Z)          # gpk_predict_host_multi_hess with B = 1
            assert np.array_equal(hess[:, b], h1[:, 0]) and np.array_equal(dmean[:, b], d1[:, 0])
            assert np.array_equal(mean[:, b], m1[:, 0])
            # ... and the single-model estimator agrees to the routes' bar
            assert relerr(hess[:, b], ms[b].predict_hessian(Z)[2]) < ROUTE_BAR


# ---- 4, 5: finite differences and the routes --------------------------------------------------------------------------------
def test_finite_differences_and_routes(small_batches):
    ms, rng = small_batches
    bg = _batch(ms[:6])
    for M in (25, 33, 300):          # the one-call path; the fused large route with one Hessian launch pair per model
        Z = 0.9 * rng.standard_normal((M, 10))
        Z[:2] = ms[0].X_train_[:2]
        mean, dmean, hess = bg.predict_hessian(Z)
        assert hess.shape == (M, 6, 10, 10) and np.isfinite(hess).all() and np.array_equal(hess, hess.swapaxes(-1, -2))
        jac = bg.predict_jacobian(Z)
        assert np.array_equal(mean, jac[0]) and np.array_equal(dmean, jac[1])
        single = np.stack([m.predict_hessian(Z)[2] for m in ms[:6]], axis=1)
        assert relerr(hess, single) < ROUTE_BAR
        if M <= 32:
            d0 = ms[0]._dev
            d0.be.set_options(small_path=0)
            try:
                general = bg.predict_host_hess(Z)
            finally:
                d0.be.set_options(small_path=1)
            assert relerr(general[2], hess) < ROUTE_BAR and relerr(general[1], dmean) < ROUTE_BAR
            assert relerr(general[0], mean) < ROUTE_BAR
        if M == 25:
            fd = np.zeros_like(hess)
            for e in range(10):
                acc = 0.0
                for w, s in zip((1.0, -8.0, 8.0, -1.0), (-2, -1, 1, 2)):
                    Zs = Z.copy()
                    Zs[:, e] += s * 1e-3
                    acc = acc + w * bg.predict_jacobian(Zs)[1]
                fd[..., e] = acc / 12e-3
            err = relerr(hess, fd)
            print(f"batch hess vs FD of predict_jacobian {err:.2e}")
            assert err < FP64_BAR


# ---- the fused launch itself: every model grouping and every row-block form of the triangle ------------------------------------
# D = 1, 3 (one block, groups of up to four models), 6 (two blocks), 10 (three), 16 (five); B = 1, 3 (an odd last group), 6, 8;
# N = 1, 33 (a ragged staging round), 129 (32-row chunks and a tail); M = 300: more than one workgroup of queries
@pytest.mark.parametrize("N,D,B", [(1, 1, 1), (33, 3, 6), (129, 3, 3), (33, 6, 3), (129, 10, 6), (33, 16, 8), (129, 16, 1),
                                   (129, 10, 8)])
def test_fused_launch_against_the_single_model_launch(N, D, B):
    rng = np.random.default_rng(100 * N + 10 * D + B)
    X = rng.standard_normal((N, D))
    Y = np.sin(X @ rng.standard_normal((D, B))) + 0.05 * rng.standard_normal((N, B))
    ms = _axis_models(X, Y, B, lambda b: np.roll(np.linspace(1.2, 3.0, D), b), lambda b: 0.02 * (b + 1))
    bg = _batch(ms)
    for M in (7, 33, 300):
        Z = 0.9 * rng.standard_normal((M, D))
        Z[:1] = X[:1]
        mean, dmean, hess = bg._predict_hessian_large(Z)
        assert hess.shape == (M, B, D, D) and np.isfinite(hess).all() and np.array_equal(hess, hess.swapaxes(-1, -2))
        single = np.stack([m._dev.predict_mean_hess_dev(Z, m._y_train_std).cpu().numpy()[:, 0] for m in ms], axis=1)
        e = relerr(hess, single)
        print(f"N = {N}, D = {D}, B = {B}, M = {M}: fused against single-model launches {e:.2e}")
        assert e < ROUTE_BAR
        again = bg._predict_hessian_large(Z)
        assert np.array_equal(again[2], hess)


def test_repeatable(small_batches):
    ms, rng = small_batches
    bg = _batch(ms[:6])
    for M in (25, 300):
        Z = rng.standard_normal((M, 10))
        a, b = bg.predict_hessian(Z), bg.predict_hessian(Z)
        for u, v in zip(a, b):
            assert np.array_equal(u, v)
