"""Mean Hessians of the sparse models on the GPU: SparseGP.predict_hessian (gpk_sparse_predict_hess) and
BatchedSparseGP.predict_hessian (gpk_sparse_predict_multi_hess) against the dense NumPy form of tests/golden/hess_ref.npz (case
`sparse`: the Titsias posterior over 64 inducing rows, tests/golden/make_golden_hess.py), against finite differences of the
models' own predict_jacobian, model by model, and after partial_fit.  Buffers start out as NaN (conftest: GPK_DEBUG_FILL)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, relerr

pytestmark = pytest.mark.gpu

FP64_BAR = 1e-8
ROUTE_BAR = 1e-11


def _load(name):
    d = np.load(os.path.join(GOLDEN, name))
    return {k: d[k] for k in d.files}


@pytest.fixture(scope="module")
def ref():
    out = _load("sparse_ref.npz")
    out.update({"H_" + k: v for k, v in _load("hess_ref.npz").items()})
    return out


def _fd4_jac(model, X, h=1e-3):
    """Fourth-order central differences of predict_jacobian: [..., d, e] = d dmean[..., d] / dx_e."""
    D = X.shape[1]
    cols = []
    for e in range(D):
        acc = 0.0
        for w, s in zip((1.0, -8.0, 8.0, -1.0), (-2, -1, 1, 2)):
            Xs = X.copy()
            Xs[:, e] += s * h
            acc = acc + w * model.predict_jacobian(Xs)[1]
        cols.append(acc / (12.0 * h))
    return np.stack(cols, axis=-1)


def _checked(model, X, shape):
    """predict_hessian with the checks every call gets: shapes, finite, symmetric, mean / dmean the bits of predict_jacobian"""
    mean, dmean, hess = model.predict_hessian(X)
    assert hess.shape == shape and dmean.shape == shape[:-1] and mean.shape == shape[:-2]
    assert np.isfinite(hess).all() and np.array_equal(hess, hess.swapaxes(-1, -2))
    jac = model.predict_jacobian(X)
    assert np.array_equal(mean, jac[0]) and np.array_equal(dmean, jac[1])
    return mean, dmean, hess


def test_fixture_and_finite_differences(ref):
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, SparseGP, WhiteKernel
    sf2, noise, alpha, jit = (float(v) for v in ref["A_hyper"])
    kern = ConstantKernel(sf2) * RBF(ref["A_ls"]) + WhiteKernel(noise)
    gp = SparseGP(kern, ref["H_sparse_Z"], alpha=alpha, jitter_uu=jit, y_mean=ref["A_y_mean"], y_std=ref["A_y_std"])
    gp.partial_fit(ref["A_X"], ref["A_Y"])
    Xq = ref["H_sparse_Xq"]
    for M in (40, 25, 1):          # the panel route; the one-call route
        mean, dmean, hess = _checked(gp, Xq[:M], (M, 2, 4, 4))
        e = (relerr(hess, ref["H_sparse_hess"][:M]), relerr(dmean, ref["H_sparse_dmean"][:M]), relerr(mean, ref["H_sparse_mean"][:M]))
        print(f"sparse fixture, M = {M}: hess {e[0]:.2e} dmean {e[1]:.2e} mean {e[2]:.2e}")
        assert max(e) < FP64_BAR
    h40, h25 = gp.predict_hessian(Xq)[2], gp.predict_hessian(Xq[:25])[2]
    assert relerr(h25, h40[:25]) < ROUTE_BAR
    fd = _fd4_jac(gp, Xq[:25])
    e = relerr(h25, fd)
    print(f"sparse hess vs FD of predict_jacobian {e:.2e}")
    assert e < FP64_BAR
    a, b = gp.predict_hessian(Xq), gp.predict_hessian(Xq)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    # small_path = 0: the panel route for a control-loop batch
    be = gp._backend()
    be.set_options(small_path=0)
    try:
        general = gp.predict_hessian(Xq[:25])
    finally:
        be.set_options(small_path=1)
    assert relerr(general[2], h25) < ROUTE_BAR and relerr(general[1], gp.predict_jacobian(Xq[:25])[1]) < ROUTE_BAR


def _model(b, m, n, D, rows):
    """Single-output model b of a batch: test_gpu_sparse_batch.model_inputs' recipe at small sizes."""
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, SparseGP, WhiteKernel
    rng = np.random.default_rng(2300 + 97 * b + 31 * m + n)
    X = rng.standard_normal((n, D))
    Z = X[rng.permutation(n)[:m]] + 0.05 * rng.standard_normal((m, D))
    y = np.sin(X @ rng.standard_normal(D)) + 0.1 * rng.standard_normal(n)
    ls = (3.0 if D == 16 else 1.5) * (1.0 + 0.05 * np.arange(D)) * (1.0 + 0.1 * b)
    gp = SparseGP(ConstantKernel(0.9 + 0.1 * b) * RBF(ls) + WhiteKernel(0.02 * (1 + b)), Z, alpha=1e-6, y_mean=float(y.mean()),
                  y_std=float(y.std()))
    return gp.partial_fit(X[:rows], y[:rows]), X, y


@pytest.mark.parametrize("B,m,D", [(6, 33, 10), (3, 129, 16), (8, 64, 4)])
def test_batch_columns_have_the_bits_of_the_models_alone(B, m, D):
    from unmanned_aerial_vehicles_amd import BatchedSparseGP
    models = [_model(b, m, 300, D, 300)[0] for b in range(B)]
    bg = BatchedSparseGP(models)
    rng = np.random.default_rng(5)
    for M in (1, 25, 32, 40):
        X = rng.standard_normal((M, D))
        mean, dmean, hess = _checked(bg, X, (M, B, D, D))
        for b in range(B):
            m1, d1, h1 = models[b].predict_hessian(X)
            assert np.array_equal(hess[:, b], h1) and np.array_equal(dmean[:, b], d1) and np.array_equal(mean[:, b], m1)
    X = rng.standard_normal((25, D))
    e = relerr(bg.predict_hessian(X)[2], _fd4_jac(bg, X))
    print(f"sparse batch (B = {B}, m = {m}, D = {D}) hess vs FD of predict_jacobian {e:.2e}")
    assert e < FP64_BAR


def test_partial_fit_changes_the_hessian_and_still_matches_finite_differences():
    gp, X, y = _model(0, 64, 400, 6, 200)
    Xq = np.random.default_rng(9).standard_normal((25, 6))
    before = _checked(gp, Xq, (25, 6, 6))[2]
    assert relerr(before, _fd4_jac(gp, Xq)) < FP64_BAR
    gp.partial_fit(X[200:], y[200:])
    after = _checked(gp, Xq, (25, 6, 6))[2]
    assert relerr(after, before) > 1e-3, "200 more rows must move the posterior mean"
    e = relerr(after, _fd4_jac(gp, Xq))
    print(f"after partial_fit: hess vs FD {e:.2e}, moved by {relerr(after, before):.2e}")
    assert e < FP64_BAR


def test_pretrained_gp_serves_a_sparsified_model_file(tmp_path):
    """A model file written by `GPTrainer.sparsify`: PreTrainedGP serves its Hessians through BatchedSparseGP, in raw units."""
    from unmanned_aerial_vehicles_amd import BatchedSparseGP, GPTrainer, PreTrainedGP
    from unmanned_aerial_vehicles_amd.trainer import OUTPUT_NAMES, hessian_to_raw
    rng = np.random.default_rng(77)
    X = rng.standard_normal((300, 10)) * (1.0 + 0.3 * np.arange(10))
    W = rng.standard_normal((10, 6)) / (1.0 + 0.3 * np.arange(10))[:, None]
    y = np.sin(0.5 * X @ W) * (1.0 + np.arange(6)) + 0.05 * rng.standard_normal((300, 6))
    tr = GPTrainer(model_dir=str(tmp_path))
    tr.train_gp_models(X[:100], y[:100], optimizer=None)
    tr.sparsify(X, y, inducing=40)
    pt = PreTrainedGP(tr.save_models("sparse"))
    assert pt.is_loaded and isinstance(pt._fused()[0], BatchedSparseGP)
    rows = X[:25] + 0.1
    mean, J, H = pt.predict_residual_hessian_batch(rows)
    assert H.shape == (25, 6, 10, 10) and np.isfinite(H).all() and H.any() and np.array_equal(H, H.swapaxes(-1, -2))
    m2, J2 = pt.predict_residual_jacobian_batch(rows)
    assert np.array_equal(mean, m2) and np.array_equal(J, J2)
    # the batch itself on the scaled rows, through the scalers
    sx = pt.scalers_X[OUTPUT_NAMES[0]]
    hs = pt._fused()[0].predict_hessian(sx.transform(rows))[2]
    for j, n in enumerate(OUTPUT_NAMES):
        assert np.array_equal(H[:, j], hessian_to_raw(hs[:, j], sx.scale_, float(pt.scalers_y[n].scale_[0])))
    # fourth-order differences of the raw Jacobian, step 1e-3 of each input's scale, compared in units of the scalers
    fd = np.zeros_like(H)
    for e in range(10):
        h = 1e-3 * sx.scale_[e]
        for w, s in zip((1.0, -8.0, 8.0, -1.0), (-2, -1, 1, 2)):
            Xs = rows.copy()
            Xs[:, e] += s * h
            fd[..., e] += w * pt.predict_residual_jacobian_batch(Xs)[1] / (12.0 * h)
    unit = (sx.scale_[:, None] * sx.scale_[None, :])[None, None]
    err = relerr(H * unit, fd * unit)
    print(f"sparsified model file: raw Hessian vs FD of the raw Jacobian {err:.2e}")
    assert err < FP64_BAR
    one = pt.predict_residual_hessian(rows[3, :6], rows[3, 6:])
    assert one[2].shape == (6, 10, 10) and relerr(one[2] * unit[0], H[3] * unit[0]) < ROUTE_BAR


def test_prior_without_rows_has_zero_derivatives():
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, SparseGP, WhiteKernel
    rng = np.random.default_rng(1)
    gp = SparseGP(ConstantKernel(1.0) * RBF(np.ones(4)) + WhiteKernel(0.01), rng.standard_normal((20, 4)), alpha=1e-6,
                  y_mean=np.array([0.7]), y_std=np.array([2.0]))
    mean, dmean, hess = gp.predict_hessian(rng.standard_normal((7, 4)))
    assert hess.shape == (7, 4, 4) and not hess.any() and not dmean.any() and np.array_equal(mean, np.full(7, 0.7))
