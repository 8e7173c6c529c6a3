"""Input gradients of the per-axis GP batch on the GPU: PreTrainedGP.predict_residual_jacobian_batch / linearize_residuals and
BatchedARDGP.predict_jacobian / predict_host_grad behind them (gpk_predict_host_multi_grad: mean + Jacobian of all models in one
launch, all four results in three; gpk_predict_mean_grad_multi for large batches) against the closed forms in raw units of
tests/golden/axis_jac_ref.npz (tests/golden/make_golden_axis_jac.py), against finite differences of the existing predict,
against the existing calls and against each other.

Raw Jacobian entries of the yaw-rate column are ~1e16 (its scaler's scale is ~1e-21), so every comparison of a gradient is
relative to the largest entry of the same input column (`colrel`)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, reference_pickle_dict, relerr

pytestmark = pytest.mark.gpu

FP64_BAR = 1e-8          # the project's fp64 parity bar
ROUTE_BAR = 1e-11        # routes differ in summation order only (test_gpu_jac.py)


@pytest.fixture(scope="module")
def axis_ref():
    d = np.load(os.path.join(GOLDEN, "axis_jac_ref.npz"))
    return {k: d[k] for k in d.files}


def colrel(a, b):
    D = b.shape[-1]
    a, b = np.asarray(a).reshape(-1, D), np.asarray(b).reshape(-1, D)
    return float(np.max(np.max(np.abs(a - b), axis=0) / np.maximum(np.max(np.abs(b), axis=0), 1e-300)))


def _axis_models(X, Y, B, ls_of, noise_of, **kw):
    """B scalar models of this package on shared inputs: C(1, fixed) * RBF(ls_b) + White(noise_b), alpha 1e-6."""
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, GaussianProcessRegressor, WhiteKernel
    ms = []
    for b in range(B):
        k = ConstantKernel(1.0, constant_value_bounds="fixed") * RBF(ls_of(b)) + WhiteKernel(noise_of(b))
        ms.append(GaussianProcessRegressor(kernel=k, alpha=1e-6, normalize_y=False, optimizer=None, device=0, **kw)
                  .fit(X, Y[:, b % Y.shape[1]]))
    return ms


def _batch(models, **kw):
    from unmanned_aerial_vehicles_amd.batched import BatchedARDGP
    bg = BatchedARDGP(optimizer=None, device=0, **kw)
    bg.models = list(models)
    return bg


def _csv_pre(csv_data, axis_ref, B=6, **kw):
    """Case `csv` served by this package: PreTrainedGP around six models fitted here with the fixture's hyper-parameters."""
    from unmanned_aerial_vehicles_amd.trainer import OUTPUT_NAMES, PreTrainedGP, StandardScaler
    X, Y = csv_data["X10"], csv_data["Y6"]
    sx = StandardScaler().fit(X)
    assert relerr(sx.scale_, axis_ref["csv_sx_scale"]) < 1e-13 and relerr(sx.mean_, axis_ref["csv_sx_mean"]) < 1e-13
    sys_ = [StandardScaler().fit(Y[:, [b]]) for b in range(6)]
    Ys = np.concatenate([sys_[b].transform(Y[:, [b]]) for b in range(6)], axis=1)
    ms = _axis_models(sx.transform(X), Ys, B, lambda b: axis_ref["csv_ls"][b], lambda b: float(axis_ref["csv_noise"][b]), **kw)
    pre = PreTrainedGP(os.path.join(GOLDEN, "no_such_model.pkl"))
    for b in range(B):
        n = OUTPUT_NAMES[b]
        pre.gp_models[n], pre.scalers_X[n], pre.scalers_y[n] = ms[b], sx, sys_[b]
    pre.is_loaded = True
    return pre


def _ref_pre(trainer_ref):
    from unmanned_aerial_vehicles_amd.trainer import PreTrainedGP
    pre = PreTrainedGP(os.path.join(GOLDEN, "no_such_model.pkl"))
    assert pre.load_dict(reference_pickle_dict(trainer_ref), device=0)
    return pre


def _check_raw(out, ref, name, rows=slice(None)):
    mean, J, std, dstd = out
    e = {"mean": relerr(mean, ref[name + "_mean"][rows]), "std": relerr(std, ref[name + "_std"][rows]),
         "J": colrel(J, ref[name + "_J"][rows]), "dstd": colrel(dstd, ref[name + "_dstd"][rows])}
    print(name, {k: f"{v:.2e}" for k, v in e.items()})
    for k, v in e.items():
        assert v < FP64_BAR, (name, k, v)


# ---- 1: parity with the fixture -------------------------------------------------------------------------------------------
def test_reference_models_match_fixture(trainer_ref, axis_ref):
    """The reference trainer's own six models (N = 240, Np = 256): 25 rows, the one-call path."""
    pre = _ref_pre(trainer_ref)
    Xq = axis_ref["ref_Xq"]
    out = pre.predict_residual_jacobian_batch(Xq, return_std=True)
    assert pre._fused_bg, "the six models share inputs and scaler: the fused path must have served them"
    assert out[0].shape == (25, 6) and out[1].shape == (25, 6, 10) and out[2].shape == (25, 6) and out[3].shape == (25, 6, 10)
    _check_raw(out, axis_ref, "ref")
    mean, J = pre.predict_residual_jacobian_batch(Xq)
    assert relerr(mean, axis_ref["ref_mean"]) < FP64_BAR and colrel(J, axis_ref["ref_J"]) < FP64_BAR
    # the normalised-target variance gradient of the one-call path itself
    bg, names = pre._fused_bg
    Z = pre.scalers_X[names[0]].transform(Xq)
    _, _, _, dvar = bg.predict_host_grad(Z, return_var=True)
    assert colrel(dvar, axis_ref["ref_dvar"]) < FP64_BAR
    for i in (0, 9):
        m1, J1 = pre.predict_residual_jacobian(Xq[i, :6], Xq[i, 6:])
        assert m1.shape == (6,) and J1.shape == (6, 10)
        assert relerr(m1, axis_ref["ref_mean"][i]) < FP64_BAR and colrel(J1, axis_ref["ref_J"][i]) < FP64_BAR


def test_csv_models_match_fixture(csv_data, axis_ref):
    """Six models fitted here (Np = 1024): the first 25 rows on the one-call path, all 72 on the large route."""
    pre = _csv_pre(csv_data, axis_ref)
    Xq = axis_ref["csv_Xq"]
    _check_raw(pre.predict_residual_jacobian_batch(Xq[:25], return_std=True), axis_ref, "csv", slice(0, 25))
    assert pre._fused_bg
    _check_raw(pre.predict_residual_jacobian_batch(Xq, return_std=True), axis_ref, "csv")
    bg, names = pre._fused_bg
    Z = pre.scalers_X[names[0]].transform(Xq)
    assert colrel(bg.predict_jacobian(Z, return_var=True)[3], axis_ref["csv_dvar"]) < FP64_BAR
    assert colrel(bg.predict_host_grad(Z[47:72], return_var=True)[3], axis_ref["csv_dvar"][47:72]) < FP64_BAR


# ---- 2: the routes agree --------------------------------------------------------------------------------------------------
def _single_model_route(bg, Z):
    """Six single-model predict_jacobian calls, stacked: (mean (M, B), dmean (M, B, D), var (M, B), dvar (M, B, D))."""
    outs = [m.predict_jacobian(Z, return_var=True) for m in bg.models]
    return tuple(np.stack([o[i] for o in outs], axis=1) for i in range(4))


def _agree(name, got, want, prior):
    e = (relerr(got[0], want[0]), colrel(got[1], want[1]), float(np.max(np.abs(got[2] - want[2]) / prior)),
         colrel(got[3], want[3]))
    print(f"{name}: mean {e[0]:.2e} dmean {e[1]:.2e} var {e[2]:.2e} dvar {e[3]:.2e}")
    assert max(e) < ROUTE_BAR, (name, e)


def test_routes_agree(csv_data, axis_ref):
    pre = _csv_pre(csv_data, axis_ref)
    pre.predict_residual_jacobian_batch(axis_ref["csv_Xq"][:2])
    bg, names = pre._fused_bg
    sx = pre.scalers_X[names[0]]
    Zt = sx.transform(csv_data["X10"])
    prior = np.array([1.0 + float(v) for v in axis_ref["csv_noise"]])[None, :]
    rng = np.random.default_rng(11)
    for M in (1, 25, 32, 33, 200, 5000):
        Z = 0.9 * rng.standard_normal((M, 10))
        if M >= 5:
            Z[:5] = Zt[:5]                  # queries at training points: variances near the noise level
        want = _single_model_route(bg, Z)
        _agree(f"M = {M} large route", bg._predict_jacobian_large(Z, True), want, prior)
        _agree(f"M = {M} predict_jacobian", bg.predict_jacobian(Z, return_var=True), want, prior)
        m_only = bg.predict_jacobian(Z)
        assert len(m_only) == 2 and relerr(m_only[0], want[0]) < 1e-12 and colrel(m_only[1], want[1]) < ROUTE_BAR
        if M <= 32:
            host = bg.predict_host_grad(Z, return_var=True)
            assert host is not None
            _agree(f"M = {M} one call", host, want, prior)
            be = bg._serve["dev0"].be
            be.set_options(small_path=0)
            try:
                _agree(f"M = {M} one call, small_path = 0", bg.predict_host_grad(Z, return_var=True), want, prior)
                mo = bg.predict_host_grad(Z)
            finally:
                be.set_options(small_path=1)
            assert mo[2] is None and mo[3] is None and colrel(mo[1], want[1]) < ROUTE_BAR
            mo = bg.predict_host_grad(Z)
            assert mo[2] is None and mo[3] is None and colrel(mo[1], want[1]) < ROUTE_BAR and relerr(mo[0], want[0]) < 1e-12
        else:
            assert bg.predict_host_grad(Z, return_var=True) is None
        # the loader's two routes in raw units: the fused one and the per-model one with the host chain rule
        Xr = sx.inverse_transform(Z)
        a = pre.predict_residual_jacobian_batch(Xr, return_std=True)
        pre._fused_bg = False
        try:
            b = pre.predict_residual_jacobian_batch(Xr, return_std=True)
        finally:
            pre._fused_bg = (bg, names)
        e = (relerr(a[0], b[0]), colrel(a[1], b[1]), relerr(a[2], b[2]), colrel(a[3], b[3]))
        print(f"M = {M} loader fused / per model: {e}")
        assert e[0] < 1e-12 and e[1] < ROUTE_BAR and e[2] < 1e-12 and e[3] < ROUTE_BAR


# ---- 3: one model through the multi entry ---------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 16, 25, 32])
def test_single_model_is_bit_equal_to_the_single_model_call(csv_data, axis_ref, M):
    pre = _csv_pre(csv_data, axis_ref, B=1)
    g = pre.gp_models["x_residual"]
    bg = _batch([g])
    Z = pre.scalers_X["x_residual"].transform(axis_ref["csv_Xq"][40:40 + M])
    comp = g.kernel_.components()
    g._ensure_device()
    for want_var in (True, False):
        mean, var, dmean, dvar = g._dev.predict_grad_host(Z, g._y_train_mean, g._y_train_std,
                                                          comp.sf2 + comp.noise if want_var else None, 0.0)
        out = bg.predict_host_grad(Z, return_var=want_var)
        assert out is not None and np.array_equal(out[0], mean) and np.array_equal(out[1], dmean)
        if want_var:
            assert float(g._y_train_std[0]) == 1.0          # (normalize_y=False: the un-normalisation multiplies by one)
            assert np.array_equal(out[2][:, 0], var) and np.array_equal(out[3][:, 0], dvar)
        else:
            assert out[2] is None and out[3] is None


# ---- 4: consistency with the existing calls -------------------------------------------------------------------------------
def test_mean_and_std_equal_predict_residual_batch(trainer_ref, csv_data, axis_ref):
    for pre, Xq in ((_ref_pre(trainer_ref), axis_ref["ref_Xq"]), (_csv_pre(csv_data, axis_ref), axis_ref["csv_Xq"])):
        for rows in (slice(0, 1), slice(0, 25), slice(None)):
            mean, J, std, dstd = pre.predict_residual_jacobian_batch(Xq[rows], return_std=True)
            m0, s0 = pre.predict_residual_batch(Xq[rows])
            assert relerr(mean, m0) < 1e-12 and relerr(std, s0) < 1e-12
        bg, names = pre._fused_bg
        Z = pre.scalers_X[names[0]].transform(Xq)
        for rows in (slice(0, 25), slice(None)):
            mean, dmean, var, dvar = bg.predict_jacobian(Z[rows], return_var=True)
            pm, ps = bg.predict(Z[rows], return_std=True)
            assert relerr(mean, pm) < 1e-12 and relerr(var, ps ** 2) < 1e-12


# ---- 5: run to run ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [2, 6, 8])
def test_repeatable(csv_data, B):
    X = csv_data["X10"]
    Xs = (X - X.mean(axis=0)) / np.where(X.std(axis=0) > 1e-12, X.std(axis=0), 1.0)
    Xs[:, 9] = np.sin(np.arange(len(X)))                     # (the yaw-rate column is constant: any bounded stand-in)
    Y = csv_data["Y6"] / csv_data["Y6"].std(axis=0)
    bg = _batch(_axis_models(Xs, Y, B, lambda b: np.roll(np.linspace(0.6, 3.0, 10), b), lambda b: 0.02 * (b + 1)))
    rng = np.random.default_rng(B)
    for M in (25, 200):                                      # the one-call path, the large route
        Z = rng.standard_normal((M, 10))
        a = bg.predict_jacobian(Z, return_var=True)
        b = bg.predict_jacobian(Z, return_var=True)
        assert a[0].shape == (M, B) and a[1].shape == (M, B, 10) and a[2].shape == (M, B) and a[3].shape == (M, B, 10)
        for u, v in zip(a, b):
            assert np.isfinite(u).all() and np.array_equal(u, v)
        c, d = bg.predict_jacobian(Z), bg.predict_jacobian(Z)
        assert np.array_equal(c[0], d[0]) and np.array_equal(c[1], d[1])
    assert bg.predict_host_grad(rng.standard_normal((25, 10)), True) is not None


# ---- 6: boundary sizes --------------------------------------------------------------------------------------------------
def _fd4(f, X, h):
    """Fourth-order central differences of f (rows -> (M, K)) along every input: (M, K, D) (test_gpu_jac.py)."""
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


def test_largest_small_path_size():
    """Np = 16 384, B = 3 (test_gpu_jac._synthetic's recipe): M = 25 on the one-call path against the large route; M = 200 on the
    large route against fourth-order differences of predict, at test_finite_differences_of_predict's bar."""
    N, D, B = 16384, 6, 3
    rng = np.random.default_rng(N)
    X = rng.standard_normal((N, D))
    Y = np.sin(X @ rng.standard_normal((D, B))) + 0.1 * rng.standard_normal((N, B))
    bg = _batch(_axis_models(X, Y, B, lambda b: 1.6 + 0.2 * b, lambda b: 0.05))
    Z = 1.1 * rng.standard_normal((200, D))
    Z[:3] = X[:3]
    small = bg.predict_host_grad(Z[:25], return_var=True)
    assert small is not None and bg._serve["dev0"].Np == 16384
    prior = 1.05
    _agree("Np = 16384, M = 25", small, bg._predict_jacobian_large(Z[:25], True), prior)
    a, b = bg.predict_host_grad(Z[:25], return_var=True), bg.predict_host_grad(Z[:25], return_var=True)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    mean, dmean, var, dvar = bg.predict_jacobian(Z, return_var=True)

    def both(Q):
        m, s = bg.predict(Q, return_std=True)
        return np.concatenate([m, s ** 2], axis=1)

    fd = _fd4(both, Z, 1e-3)
    e1, e2 = relerr(dmean, fd[:, :B]), relerr(dvar, fd[:, B:])
    print(f"Np = 16384, M = 200: dmean vs FD {e1:.2e}, dvar vs FD {e2:.2e}")
    assert e1 < FP64_BAR and e2 < FP64_BAR


# ---- 7: models that do not qualify, fp32 serving --------------------------------------------------------------------------
def test_models_that_do_not_share_inputs_take_the_fallback(csv_data, axis_ref):
    from unmanned_aerial_vehicles_amd.trainer import StandardScaler
    pre = _csv_pre(csv_data, axis_ref)
    # the same model behind an input scaler of its own (equal numbers, one bit off in one mean): not fusable
    sx = StandardScaler()
    sx.mean_, sx.scale_ = pre.scalers_X["y_residual"].mean_.copy(), pre.scalers_X["y_residual"].scale_.copy()
    sx.mean_[0] = np.nextafter(sx.mean_[0], np.inf)
    pre.scalers_X["y_residual"] = sx
    out = pre.predict_residual_jacobian_batch(axis_ref["csv_Xq"], return_std=True)
    assert pre._fused_bg is False
    _check_raw(out, axis_ref, "csv")
    # a broken component never raises: its fallback row, the others served
    pre.gp_models["z_residual"] = object()
    mean, J, std, dstd = pre.predict_residual_jacobian_batch(axis_ref["csv_Xq"][:25], return_std=True)
    assert not mean[:, 2].any() and not J[:, 2].any() and np.all(std[:, 2] == 1e6) and not dstd[:, 2].any()
    keep = [0, 1, 3, 4, 5]
    assert colrel(J[:, keep], axis_ref["csv_J"][:25, keep]) < FP64_BAR


def test_fp32_serving_batch_returns_fp64_gradients(csv_data, axis_ref):
    pre64 = _csv_pre(csv_data, axis_ref)
    pre32 = _csv_pre(csv_data, axis_ref, predict_dtype="float32")
    pre64.predict_residual_jacobian_batch(axis_ref["csv_Xq"][:2])
    pre32.predict_residual_jacobian_batch(axis_ref["csv_Xq"][:2])
    bg64, names = pre64._fused_bg
    bg32 = _batch(pre32._fused_bg[0].models, predict_dtype="float32")
    Z = pre64.scalers_X[names[0]].transform(axis_ref["csv_Xq"])
    assert bg32.predict_host(Z[:25]) is None                  # fp32 serving: the existing one-call path does not apply
    for rows in (slice(0, 25), slice(None)):
        a, b = bg64.predict_jacobian(Z[rows], return_var=True), bg32.predict_jacobian(Z[rows], return_var=True)
        for u, v in zip(a, b):
            assert v.dtype == np.float64 and colrel(v, u) < 1e-12
    assert bg32.predict_host_grad(Z[:25], True) is not None


# ---- 8: the linearisation ----------------------------------------------------------------------------------------------
def test_linearize_residuals(csv_data, axis_ref):
    pre = _csv_pre(csv_data, axis_ref)
    Xq = axis_ref["csv_Xq"]
    N, dt, gain = 20, 0.05, 0.1
    Xg = np.zeros((6, N + 1))
    Xg[:, :N] = Xq[:N, :6].T
    Ug = Xq[:N, 6:].T.copy()
    D, A, B = pre.linearize_residuals(Xg, Ug, dt, gain)
    assert D.shape == (6, N) and A.shape == (N, 6, 6) and B.shape == (N, 6, 4)
    assert relerr(D[3:6], gain / dt * axis_ref["csv_mean"][:N, 3:6].T) < FP64_BAR
    J = axis_ref["csv_J"][:N]
    assert colrel(A[:, 3:6, :], gain / dt * J[:, 3:6, :6]) < FP64_BAR
    assert colrel(B[:, 3:6, :], gain / dt * J[:, 3:6, 6:10]) < FP64_BAR
    assert not A[:, :3].any() and not B[:, :3].any() and not D[:3].any()
    # R = 3 rollouts
    Xr = np.stack([Xg, np.roll(Xg, 1, axis=1), np.roll(Xg, 2, axis=1)])
    Ur = np.stack([Ug, np.roll(Ug, 1, axis=1), np.roll(Ug, 2, axis=1)])
    D3, A3, B3 = pre.linearize_residuals(Xr, Ur, dt, gain)
    assert D3.shape == (3, 6, N) and A3.shape == (3, N, 6, 6) and B3.shape == (3, N, 6, 4)
    assert relerr(D3[0], D) < ROUTE_BAR and colrel(A3[0], A) < ROUTE_BAR and colrel(B3[0], B) < ROUTE_BAR
    D1, A1, B1 = pre.linearize_residuals(Xr[1], Ur[1], dt, gain)
    assert colrel(A3[1], A1) < ROUTE_BAR and colrel(B3[1], B1) < ROUTE_BAR and relerr(D3[1], D1) < ROUTE_BAR


# ---- 9: a failing fused call, models on different inputs --------------------------------------------------------------------
def test_fused_failure_is_served_model_by_model(csv_data, axis_ref):
    """As predict_residual_batch: when the fused call raises, the per-model loop still serves every component."""
    pre = _csv_pre(csv_data, axis_ref)
    pre.predict_residual_jacobian_batch(axis_ref["csv_Xq"][:2])
    bg, names = pre._fused_bg

    def broken(*a, **k):
        raise RuntimeError("fused call unavailable")

    bg.predict_jacobian = broken
    _check_raw(pre.predict_residual_jacobian_batch(axis_ref["csv_Xq"], return_std=True), axis_ref, "csv")
    _check_raw(pre.predict_residual_jacobian_batch(axis_ref["csv_Xq"][:25], return_std=True), axis_ref, "csv", slice(0, 25))


def test_models_on_different_inputs_agree_on_both_sides_of_32_rows():
    """A BatchedARDGP whose models were fitted on different inputs (same size): the one-call path takes each model's own X,
    and the large route must not fuse them on model 0's."""
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, GaussianProcessRegressor, WhiteKernel
    rng = np.random.default_rng(21)
    N, D, B = 700, 5, 3
    ms = []
    for b in range(B):
        X = rng.standard_normal((N, D))
        y = np.sin(X @ rng.standard_normal(D)) + 0.05 * rng.standard_normal(N)
        k = ConstantKernel(1.0, constant_value_bounds="fixed") * RBF(1.0 + 0.3 * b) + WhiteKernel(0.03)
        ms.append(GaussianProcessRegressor(kernel=k, alpha=1e-6, normalize_y=False, optimizer=None, device=0).fit(X, y))
    bg = _batch(ms)
    for M in (25, 40):
        Z = rng.standard_normal((M, D))
        _agree(f"different inputs, M = {M}", bg.predict_jacobian(Z, return_var=True), _single_model_route(bg, Z), 1.03)
        mo = bg.predict_jacobian(Z)
        assert len(mo) == 2 and colrel(mo[1], _single_model_route(bg, Z)[1]) < ROUTE_BAR
    assert bg.predict_host_grad(rng.standard_normal((25, D)), True) is not None
