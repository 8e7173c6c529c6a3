"""Joint posterior of the per-axis GP batch on the GPU: gpk_predict_host_multi_cov (small_cov_kernel with the model as a grid
dimension: B covariances in two launches), BatchedARDGP.predict(return_cov=True) / sample_y and
PreTrainedGP.predict_residual_cov_batch / sample_residuals behind it, against scikit-learn's return_cov and the closed form of
tests/golden/axis_cov_ref.npz (tests/golden/make_golden_axis_cov.py), bit for bit against gpk_predict_host_cov on each model
alone, and against the existing calls."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, relerr
from test_gpu_axis_jac import _axis_models, _batch, _csv_pre, _ref_pre

pytestmark = pytest.mark.gpu

FP64_BAR = 1e-8          # the project's fp64 parity bar
ROUTE_BAR = 1e-12        # routes differ in summation order only


@pytest.fixture(scope="module")
def cov_ref():
    d = np.load(os.path.join(GOLDEN, "axis_cov_ref.npz"))
    return {k: d[k] for k in d.files}


@pytest.fixture(scope="module")
def csv_pre(csv_data, cov_ref):
    pre = _csv_pre(csv_data, cov_ref)
    assert pre._fused(), "the six models share inputs and scaler"
    return pre


def blockrel(a, b):
    """max |a - b| per model block (last axis), relative to the block's largest entry."""
    a, b = np.asarray(a), np.asarray(b)
    ax = tuple(range(b.ndim - 1))
    return float(np.max(np.max(np.abs(a - b), axis=ax) / np.max(np.abs(b), axis=ax)))


def _raw(mean, cov, ref):
    return mean * ref["csv_sy_scale"] + ref["csv_sy_mean"], cov * ref["csv_sy_scale"] ** 2


# ---- the C entries, called directly ------------------------------------------------------------------------------------
class _Models:
    """Seeded single-output ARD models on shared inputs (distinct length-scales and noise levels) and the argument block of
    the per-axis entries."""

    def __init__(self, N, B, D=6):
        rng = np.random.default_rng(N)
        X = rng.standard_normal((N, D))
        Y = np.sin(X @ rng.standard_normal((D, B))) + 0.1 * rng.standard_normal((N, B))
        self.X, self.D = X, D
        self.gps = _axis_models(X, Y, B, lambda b: 1.2 + 0.1 * b + 0.05 * np.arange(D), lambda b: 0.02 * (b + 1))
        self.noise = np.array([0.02 * (b + 1) for b in range(B)])
        Q = 1.1 * rng.standard_normal((32, D))
        Q[:3] = X[:3]                       # queries at training points: the covariance is what cancellation leaves
        self.Q = Q
        for g in self.gps:
            g._ensure_device()
        self.devs = [g._dev for g in self.gps]
        self.Ws = [d.inverse_factor(False) for d in self.devs]
        import torch
        torch.cuda.synchronize()

    def block(self, B):
        devs = self.devs[:B]
        vp = C.c_void_p * B
        return {"B": B, "d0": devs[0], "X": vp(*[d.X.data_ptr() for d in devs]), "alpha": vp(*[d.alpha.data_ptr() for d in devs]),
                "W": vp(*[w.data_ptr() for w in self.Ws[:B]]), "ls": np.ascontiguousarray(np.stack([d.ls for d in devs])),
                "sf2": np.ascontiguousarray([d.sf2 for d in devs]), "ym": np.zeros(B), "ys": np.ones(B),
                "noise": np.ascontiguousarray(self.noise[:B]), "kss": np.ascontiguousarray(1.0 + self.noise[:B])}

    def single(self, b, Xq):
        g = self.gps[b]
        mean, cov = self.devs[b].predict_cov_host(Xq, g._y_train_mean, g._y_train_std, float(self.noise[b]))
        return mean[:, 0], cov


def _multi_cov_rc(a, Xq, be=None, **over):
    """gpk_predict_host_multi_cov with the block's arguments (some overridden): (rc, mean (B, M), cov (B, M, M))."""
    B, d0 = over.get("B", a["B"]), a["d0"]
    M = over.get("M", Xq.shape[0])
    be = be or d0.be
    mean, cov = np.full((max(B, 1), max(M, 1)), np.nan), np.full((max(B, 1), max(M, 1), max(M, 1)), np.nan)
    with be.lock:
        be.bind_stream()
        rc = be.lib.gpk_predict_host_multi_cov(
            be.h, B, over.get("X", a["X"]), a["alpha"], d0.N, d0.D, a["ls"].ctypes.data, a["sf2"].ctypes.data, a["ym"].ctypes.data,
            a["ys"].ctypes.data, a["W"], over.get("Np", d0.Np), d0.Np, a["noise"].ctypes.data, Xq.ctypes.data, M,
            mean.ctypes.data, cov.ctypes.data)
        msg = be.lib.gpk_last_error(be.h).decode()
    return rc, msg, mean, cov


def _multi_cov(a, Xq, be=None):
    rc, msg, mean, cov = _multi_cov_rc(a, np.ascontiguousarray(Xq), be)
    assert rc == 0, msg
    return mean, cov


def _multi_grad(a, Xq, be=None):
    B, d0 = a["B"], a["d0"]
    M, D = Xq.shape
    be = be or d0.be
    mean, var, dmean, dvar = np.empty((B, M)), np.empty((B, M)), np.empty((B, M, D)), np.empty((B, M, D))
    with be.lock:
        be.bind_stream()
        be.check(be.lib.gpk_predict_host_multi_grad(
            be.h, B, a["X"], a["alpha"], d0.N, D, a["ls"].ctypes.data, a["sf2"].ctypes.data, a["ym"].ctypes.data,
            a["ys"].ctypes.data, a["W"], d0.Np, d0.Np, a["kss"].ctypes.data, 0.0, Xq.ctypes.data, M, mean.ctypes.data,
            var.ctypes.data, dmean.ctypes.data, dvar.ctypes.data))
    return mean, var, dmean, dvar


# ---- 1: parity with the fixtures -------------------------------------------------------------------------------------------
def test_csv_models_match_scikit_learn(csv_pre, cov_ref):
    """Case `csv` (Np = 1024): 25 rows through BatchedARDGP.predict(return_cov=True) - the one call - against scikit-learn's
    own return_cov, and the draws against the stored Cholesky draws."""
    bg, names = csv_pre._fused()
    Z = csv_pre.scalers_X[names[0]].transform(cov_ref["csv_Xq"])
    mean, cov = bg.predict(Z, return_cov=True)
    assert mean.shape == (25, 6) and cov.shape == (25, 25, 6)
    assert bg.predict_host_cov(Z) is not None
    mean, cov = _raw(mean, cov, cov_ref)
    e = (blockrel(mean, cov_ref["csv_mean"]), blockrel(cov, cov_ref["csv_cov"]))
    print("csv, 25 rows: mean %.2e cov %.2e" % e)
    assert max(e) < FP64_BAR
    draws = bg.sample_y(Z, n_samples=8, random_state=0)
    assert draws.shape == (25, 6, 8)
    draws = draws * cov_ref["csv_sy_scale"][None, :, None] + cov_ref["csv_sy_mean"][None, :, None]
    e = relerr(draws, cov_ref["csv_draws"])
    print("csv draws %.2e" % e)
    assert e < FP64_BAR
    # the loader's surface in raw units
    m2, c2 = csv_pre.predict_residual_cov_batch(cov_ref["csv_Xq"])
    assert blockrel(m2, cov_ref["csv_mean"]) < FP64_BAR and blockrel(c2, cov_ref["csv_cov"]) < FP64_BAR
    assert relerr(csv_pre.sample_residuals(cov_ref["csv_Xq"], 8, 0), cov_ref["csv_draws"]) < FP64_BAR


def test_reference_models_match_the_closed_form(trainer_ref, cov_ref):
    """Case `ref`: the reference trainer's own six models (N = 240, Np = 256: exactly one full reduction group) through
    PreTrainedGP.load_dict + predict_residual_cov_batch in raw units."""
    pre = _ref_pre(trainer_ref)
    mean, cov = pre.predict_residual_cov_batch(cov_ref["ref_Xq"])
    assert pre._fused_bg, "the six models share inputs and scaler: the fused path must have served them"
    assert mean.shape == (25, 6) and cov.shape == (25, 25, 6)
    e = (blockrel(mean, cov_ref["ref_mean"]), blockrel(cov, cov_ref["ref_cov"]))
    print("ref: mean %.2e cov %.2e" % e)
    assert max(e) < FP64_BAR
    draws = pre.sample_residuals(cov_ref["ref_Xq"], n_samples=8, random_state=0)
    assert draws.shape == (25, 6, 8)
    e = relerr(draws, cov_ref["ref_draws"])
    print("ref draws %.2e" % e)
    assert e < FP64_BAR
    # a missing component: its fallback, zeros for its draws; the others' draws unchanged
    del pre.gp_models["y_residual"]
    pre._fused_bg = None
    m2, c2 = pre.predict_residual_cov_batch(cov_ref["ref_Xq"])
    assert not m2[:, 1].any() and np.array_equal(c2[..., 1], 1e12 * np.eye(25))
    d2 = pre.sample_residuals(cov_ref["ref_Xq"], n_samples=8, random_state=0)
    keep = [0, 2, 3, 4, 5]
    assert not d2[:, 1].any() and relerr(d2[:, keep], cov_ref["ref_draws"][:, keep]) < FP64_BAR


# ---- 2: bits ------------------------------------------------------------------------------------------------------------
_MODELS = {}


def _models(N, B=8):
    if (N, B) not in _MODELS:
        _MODELS[(N, B)] = _Models(N, B)
    return _MODELS[(N, B)]


@pytest.mark.parametrize("N", [100, 300, 1000])
def test_a_models_block_has_the_bits_of_that_model_alone(N):
    """N = 100: Np = 128, 8 workgroups, less than one group; 300: Np = 384, one full group and half of a second; 1000: four
    groups.  M = 16 / 17 straddle the NMB switch."""
    ms = _models(N)
    be = ms.devs[0].be
    for M in (1, 2, 16, 17, 25, 32):
        Xq = np.ascontiguousarray(ms.Q[:M])
        alone = [ms.single(b, Xq) for b in range(8)]
        for B in (1, 3, 8):
            a = ms.block(B)
            mean, cov = _multi_cov(a, Xq)
            assert np.isfinite(mean).all() and np.isfinite(cov).all()
            for b in range(B):
                assert np.array_equal(mean[b], alone[b][0]), (N, M, B, b)
                assert np.array_equal(cov[b], alone[b][1]), (N, M, B, b)
                assert np.array_equal(cov[b], cov[b].T), (N, M, B, b)
            mean2, cov2 = _multi_cov(a, Xq)
            assert np.array_equal(mean2, mean) and np.array_equal(cov2, cov)
            be.set_options(small_path=0)
            try:
                mean0, cov0 = _multi_cov(a, Xq)
            finally:
                be.set_options(small_path=1)
            e = (relerr(mean0, mean), blockrel(np.moveaxis(cov0, 0, -1), np.moveaxis(cov, 0, -1)))
            assert max(e) < ROUTE_BAR, (N, M, B, e)
            for b in range(B):
                assert np.array_equal(cov0[b], cov0[b].T)


# ---- 3: the counter budget -------------------------------------------------------------------------------------------------
def test_eight_models_at_4096_rows_and_the_shared_counter_block():
    """B = 8 at N = 4096, M = 32: 8 x (1 + 16) = 136 tickets, more than the block of 128 held before it was resized; then the
    single-model covariance, the gradient call with variances (its counters share the block) and the batch again."""
    from unmanned_aerial_vehicles_amd.device import Backend
    ms = _Models(4096, 8)
    a = ms.block(8)
    Xq = np.ascontiguousarray(ms.Q[:32])
    mean, cov = _multi_cov(a, Xq)
    alone = [ms.single(b, Xq) for b in range(8)]                   # (1: gpk_predict_host_cov on the same handle)
    for b in range(8):
        assert np.array_equal(mean[b], alone[b][0]) and np.array_equal(cov[b], alone[b][1]), b
        assert np.array_equal(cov[b], cov[b].T)
    grad = _multi_grad(a, Xq)                                      # (2)
    mean2, cov2 = _multi_cov(a, Xq)                                # (3)
    assert np.array_equal(mean2, mean) and np.array_equal(cov2, cov)
    fresh = Backend(0)
    grad_fresh = _multi_grad(a, Xq, be=fresh)
    for u, v in zip(grad, grad_fresh):
        assert np.isfinite(u).all() and np.array_equal(u, v)
    mean3, cov3 = _multi_cov(a, Xq, be=fresh)
    assert np.array_equal(mean3, mean) and np.array_equal(cov3, cov)


# ---- 4: consistency with the existing calls --------------------------------------------------------------------------------
def test_diagonal_equals_the_variance(csv_pre, cov_ref, csv_data):
    bg, names = csv_pre._fused()
    sx = csv_pre.scalers_X[names[0]]
    prior = 1.0 + cov_ref["csv_noise"]
    for Z in (sx.transform(cov_ref["csv_Xq"]), sx.transform(cov_ref["csv_Xq72"][:32]), sx.transform(cov_ref["csv_Xq72"][:1])):
        mean, cov = bg.predict(Z, return_cov=True)
        pm, ps = bg.predict(Z, return_std=True)
        assert relerr(mean, pm) < 1e-12
        diag = np.stack([np.diag(cov[..., b]) for b in range(6)], axis=1)
        ok = ps > 0.0                                            # (where the variance is not clipped)
        assert ok.any()
        e = float(np.max((np.abs(diag - ps ** 2) / prior[None, :])[ok]))
        print("diag vs variance %.2e" % e)
        assert e < 1e-12


def test_fp32_serving_batch_returns_the_fp64_covariance(csv_data, cov_ref, csv_pre):
    pre32 = _csv_pre(csv_data, cov_ref, predict_dtype="float32")
    bg32 = _batch([pre32.gp_models[n] for n in csv_pre._fused()[1]], predict_dtype="float32")
    bg64, names = csv_pre._fused()
    sx = csv_pre.scalers_X[names[0]]
    assert bg32.predict_host(sx.transform(cov_ref["csv_Xq"])) is None      # fp32 serving: the mean / std one-call path does not apply
    for Z in (sx.transform(cov_ref["csv_Xq"]), sx.transform(cov_ref["csv_Xq72"])):
        a, b = bg64.predict(Z, return_cov=True), bg32.predict(Z, return_cov=True)
        assert b[0].dtype == np.float64 and b[1].dtype == np.float64
        assert blockrel(b[0], a[0]) < ROUTE_BAR and blockrel(b[1], a[1]) < ROUTE_BAR
    assert bg32.predict_host_cov(sx.transform(cov_ref["csv_Xq"])) is not None


# ---- 5: the large route ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [33, 72])
def test_large_route(csv_pre, cov_ref, M):
    """N = 1000, B = 6: the fused mean launch plus each model's predict_cov_dev."""
    bg, names = csv_pre._fused()
    Z = csv_pre.scalers_X[names[0]].transform(cov_ref["csv_Xq72"][:M])
    mean, cov = bg.predict(Z, return_cov=True)
    assert mean.shape == (M, 6) and cov.shape == (M, M, 6) and bg.predict_host_cov(Z) is None
    outs = [m.predict(Z, return_cov=True) for m in bg.models]
    want = np.stack([o[0] for o in outs], axis=1), np.stack([o[1] for o in outs], axis=2)
    e = (blockrel(mean, want[0]), blockrel(cov, want[1]))
    print(f"M = {M}: against the estimators {e}")
    assert max(e) < ROUTE_BAR
    for b in range(6):
        assert np.array_equal(cov[..., b], cov[..., b].T)
    small = bg.predict(Z[:32], return_cov=True)
    e = (blockrel(mean[:32], small[0]), blockrel(cov[:32, :32], small[1]))
    print(f"M = {M}: leading 32 x 32 block against the small route {e}")
    assert max(e) < ROUTE_BAR
    if M == 72:
        rm, rc = _raw(mean, cov, cov_ref)
        e = (blockrel(rm, cov_ref["csv_mean72"]), blockrel(rc, cov_ref["csv_cov72"]))
        print(f"M = 72 against scikit-learn {e}")
        assert max(e) < FP64_BAR
        m2, c2 = csv_pre.predict_residual_cov_batch(cov_ref["csv_Xq72"])
        assert blockrel(m2, cov_ref["csv_mean72"]) < FP64_BAR and blockrel(c2, cov_ref["csv_cov72"]) < FP64_BAR


# ---- 6: batches that do not qualify ----------------------------------------------------------------------------------------
def test_batches_that_do_not_qualify_take_the_per_model_path():
    rng = np.random.default_rng(5)
    D = 4
    X = rng.standard_normal((260, D))
    Y = np.sin(X @ rng.standard_normal((D, 9))) + 0.05 * rng.standard_normal((260, 9))
    nine = _axis_models(X, Y, 9, lambda b: 1.0 + 0.1 * b, lambda b: 0.03)
    other = _axis_models(X[:200], Y[:200], 1, lambda b: 1.3, lambda b: 0.05)
    for models in (nine, nine[:2] + other):
        bg = _batch(models)
        for M in (25, 40):
            Z = rng.standard_normal((M, D))
            assert bg.predict_host_cov(Z) is None
            mean, cov = bg.predict(Z, return_cov=True)
            assert mean.shape == (M, len(models)) and cov.shape == (M, M, len(models))
            outs = [m.predict(Z, return_cov=True) for m in models]
            assert blockrel(mean, np.stack([o[0] for o in outs], axis=1)) < ROUTE_BAR
            assert blockrel(cov, np.stack([o[1] for o in outs], axis=2)) < ROUTE_BAR
            assert bg.sample_y(Z, 2).shape == (M, len(models), 2)


# ---- 7: errors -------------------------------------------------------------------------------------------------------------
def test_refusals(csv_pre, cov_ref):
    from unmanned_aerial_vehicles_amd import _lib
    from unmanned_aerial_vehicles_amd.device import Backend
    ms = _models(100)
    a = ms.block(3)
    Xq = np.ascontiguousarray(ms.Q[:4])
    Q33 = np.zeros((33, ms.D))
    B9 = ms.block(8)
    vp9 = (C.c_void_p * 9)(*([ms.devs[0].X.data_ptr()] * 9))
    null = (C.c_void_p * 3)(ms.devs[0].X.data_ptr(), None, ms.devs[2].X.data_ptr())
    for name, kw, q in (("M = 0", {"M": 0}, Xq), ("M = 33", {}, Q33), ("B = 9", {"B": 9, "X": vp9}, Xq),
                        ("null model pointer", {"X": null}, Xq), ("Np != gpk_padded(N)", {"Np": 256}, Xq)):
        rc, msg, _, _ = _multi_cov_rc(B9 if name == "B = 9" else a, q, **kw)
        print(name, rc, msg)
        assert rc == _lib.GPK_BAD_ARG and "predict_host_multi_cov" in msg, (name, rc, msg)
    assert _multi_cov_rc(a, Xq)[0] == _lib.GPK_OK
    bg, names = csv_pre._fused()
    Z = csv_pre.scalers_X[names[0]].transform(cov_ref["csv_Xq"])
    for bad in (np.nan, np.inf):
        Zb = Z.copy()
        Zb[3, 2] = bad
        with pytest.raises(ValueError):
            bg.predict(Zb, return_cov=True)
    with pytest.raises(RuntimeError):
        bg.predict(Z, return_std=True, return_cov=True)
    # the composite before gpk_fit_batched
    fresh = Backend(0)
    mean, cov = np.empty((4, 3)), np.empty((3, 4, 4))
    dp = _lib._dp
    rc = fresh.lib.gpk_predict_batched_cov(fresh.h, Xq.ctypes.data_as(dp), 4, mean.ctypes.data_as(dp), cov.ctypes.data_as(dp))
    msg = fresh.lib.gpk_last_error(fresh.h).decode()
    assert rc == _lib.GPK_BAD_ARG and "gpk_fit_batched" in msg, (rc, msg)
