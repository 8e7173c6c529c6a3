"""The per-axis batch of sparse GPs ("the per-axis batch") on the GPU: `BatchedSparseGP` and
`gpk_sparse_predict_multi[_grad|_cov]` - B <= 8 single-output sparse models, each with its own kernel, noise, normalisation and
inducing inputs, served for one query batch in one call - then `PreTrainedGP` and `GPTrainer.sparsify` on top of it.  Buffers
start out as NaN (conftest: GPK_DEBUG_FILL).

Expected values: the dense NumPy form of tests/test_gpu_sparse_serve.py (Sigma = Kuu + Kuf Kfu / s2, Cholesky solves), restated
here, per model.  Bars: the project's fp64 bar 1e-8 on each array's largest component; 1e-12 between routes that differ in
summation order only.

Inputs.  Model b of a case (B, m, n, D): rng seed 1700 + 97 b + 31 m + n; X (n, D) and Xq (40, D) standard normal; Z = m
permuted rows of X + 0.05 normal noise (m <= n) or standard normal (m > n); ls_b = (3.0 if D == 16 else 1.5) (1 + 0.05 d)
(1 + 0.1 b), sf2_b = 0.9 + 0.1 b, noise_b = 0.02 (1 + b), alpha = 1e-6, the default jitter_uu; y = sin(X w) + 0.1 normal,
normalised by its own mean / std.  The batch is served at model 0's queries.  On these inputs the dense form and the library's
factor form (Wuu, LB, WSigma) agree to <= 1e-10 on all five results in NumPy, cond(Kuu) <= 5e4 and the smallest variance (in
normalised-target units) is >= 0.04: the bar has two orders of margin and no clip is active."""
import ctypes as C
import pickle

import numpy as np
import pytest
from scipy.linalg import cho_solve, cholesky

from conftest import relerr

pytestmark = pytest.mark.gpu

ROUTE_BAR = 1e-12
FP64_BAR = 1e-8
ALPHA = 1e-6
MQ = 40


def rbf(A, B, ls, sf2):
    d = (A / ls)[:, None, :] - (B / ls)[None, :, :]
    return sf2 * np.exp(-0.5 * np.sum(d * d, axis=2))


def numpy_form(X, Y, Z, Xq, ls, sf2, noise, alpha, jit, ym, ys):
    """The dense form for one single-output model: mean (M,), y_var (M,) with the noise level, dmean (M, D), dvar (M, D),
    cov (M, M) as SparseGP returns them.  No rows: X of shape (0, D)."""
    s2, m = noise + alpha, len(Z)
    Yn = (Y - ym) / ys
    Kuu = rbf(Z, Z, ls, sf2) + jit * np.eye(m)
    Kuf = rbf(Z, X, ls, sf2)
    cS, cU = (cholesky(Kuu + Kuf @ Kuf.T / s2, lower=True), True), (cholesky(Kuu, lower=True), True)
    ku = rbf(Z, Xq, ls, sf2)
    au = cho_solve(cS, Kuf @ Yn) / s2
    c0, c1 = cho_solve(cU, ku), cho_solve(cS, ku)
    U = ((Z / ls)[None, :, :] - (Xq / ls)[:, None, :]) / ls
    ys2 = ys ** 2
    mean = ym + ys * (ku.T @ au)
    var = sf2 + noise - np.sum(ku * c0, axis=0) + np.sum(ku * c1, axis=0)
    dmean = np.einsum("jm,mjd,j->md", ku, U, au) * ys
    dvar = -2.0 * np.einsum("jm,mjd,jm->md", ku, U, c0 - c1)
    cov = rbf(Xq, Xq, ls, sf2) + noise * np.eye(len(Xq)) - ku.T @ c0 + ku.T @ c1
    return mean, np.maximum(var, 0.0) * ys2, dmean, dvar * ys2, cov * ys2


def model_inputs(b, m, n, D):
    rng = np.random.default_rng(1700 + 97 * b + 31 * m + n)
    X = rng.standard_normal((n, D))
    Xq = rng.standard_normal((MQ, D))
    if m <= n:
        Z = X[rng.permutation(n)[:m]] + 0.05 * rng.standard_normal((m, D))
    else:
        Z = rng.standard_normal((m, D))
    y = np.sin(X @ rng.standard_normal(D)) + 0.1 * rng.standard_normal(n)
    ls = (3.0 if D == 16 else 1.5) * (1.0 + 0.05 * np.arange(D)) * (1.0 + 0.1 * b)
    return {"X": X, "Xq": Xq, "Z": Z, "y": y, "ls": ls, "sf2": 0.9 + 0.1 * b, "noise": 0.02 * (1 + b),
            "ym": float(y.mean()), "ys": float(y.std())}


def build_model(p, rows=True):
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, SparseGP, WhiteKernel
    gp = SparseGP(ConstantKernel(p["sf2"]) * RBF(p["ls"]) + WhiteKernel(p["noise"]), p["Z"], alpha=ALPHA, y_mean=p["ym"],
                  y_std=p["ys"])
    return gp.partial_fit(p["X"], p["y"]) if rows else gp


_cases = {}


def case(B, m, n, D):
    """(inputs per model, the SparseGP models, the batch, the shared queries, the dense form per model at all MQ queries):
    built once, shared by the tests and left unchanged."""
    key = (B, m, n, D)
    if key not in _cases:
        from unmanned_aerial_vehicles_amd import BatchedSparseGP
        ps = [model_inputs(b, m, n, D) for b in range(B)]
        models = [build_model(p) for p in ps]
        Xq = ps[0]["Xq"]
        ref = [numpy_form(p["X"], p["y"], p["Z"], Xq, p["ls"], p["sf2"], p["noise"], ALPHA, 1e-8 * p["sf2"], p["ym"], p["ys"])
               for p in ps]
        _cases[key] = (ps, models, BatchedSparseGP(models), Xq, ref)
    return _cases[key]


def expected(ref, M):
    """the dense form of every model at the first M queries in the batch's shapes"""
    return (np.stack([r[0][:M] for r in ref], axis=1), np.stack([r[1][:M] for r in ref], axis=1),
            np.stack([r[2][:M] for r in ref], axis=1), np.stack([r[3][:M] for r in ref], axis=1),
            np.stack([r[4][:M, :M] for r in ref], axis=2))


def serve(bg, Xq):
    mean_s, std = bg.predict(Xq, return_std=True)
    mean_c, cov = bg.predict(Xq, return_cov=True)
    mean, dmean, var, dvar = bg.predict_jacobian(Xq, return_var=True)
    return mean, dmean, var, dvar, mean_s, std, mean_c, cov


NAMES = ("mean", "dmean", "var", "dvar", "mean (std call)", "std", "mean (cov call)", "cov")


def check_against_numpy(tag, got, ref, M):
    mean, dmean, var, dvar, mean_s, std, mean_c, cov = got
    e_mean, e_var, e_dmean, e_dvar, e_cov = expected(ref, M)
    errs = {"mean": relerr(mean, e_mean), "mean (std call)": relerr(mean_s, e_mean), "mean (cov call)": relerr(mean_c, e_mean),
            "var": relerr(var, e_var), "std": relerr(std, np.sqrt(e_var)), "dmean": relerr(dmean, e_dmean),
            "dvar": relerr(dvar, e_dvar), "cov": relerr(cov, e_cov)}
    for k, e in errs.items():
        print(f"{tag}: {k} {e:.2e} (bar {FP64_BAR:.1e})")
    for k, e in errs.items():
        assert e < FP64_BAR, (tag, k, e)


# ---- 1. parity and the bit rule ---------------------------------------------------------------------------------------------
CASES = [(6, 1, 17, 3), (8, 128, 40, 16), (6, 300, 400, 10), (2, 60, 400, 10), (1, 200, 300, 10)]


@pytest.mark.parametrize("M", [1, 16, 17, 25, 32])
@pytest.mark.parametrize("shape", CASES, ids=lambda s: "B%d-m%d-n%d-D%d" % s)
def test_parity_and_bit_rule(shape, M):
    B, m, n, D = shape
    ps, models, bg, Xq_all, ref = case(*shape)
    Xq = Xq_all[:M]
    got = serve(bg, Xq)
    mean, dmean, var, dvar, mean_s, std, mean_c, cov = got
    assert mean.shape == (M, B) and dmean.shape == (M, B, D) and var.shape == (M, B) and dvar.shape == (M, B, D)
    assert std.shape == (M, B) and cov.shape == (M, M, B)
    check_against_numpy(f"case {shape}, M = {M}", got, ref, M)
    # block b: the bits of model b served alone
    for b, gp in enumerate(models):
        a_mean, a_dmean, a_var, a_dvar = gp.predict_jacobian(Xq, return_var=True)
        a_mean_s, a_std = gp.predict(Xq, return_std=True)
        a_mean_c, a_cov = gp.predict(Xq, return_cov=True)
        alone = (a_mean, a_dmean, a_var, a_dvar, a_mean_s, a_std, a_mean_c, a_cov)
        block = (mean[:, b], dmean[:, b], var[:, b], dvar[:, b], mean_s[:, b], std[:, b], mean_c[:, b], cov[:, :, b])
        for name, x, y in zip(NAMES, block, alone):
            assert x.shape == y.shape, (name, x.shape, y.shape)
            assert np.array_equal(x, y), f"model {b}: {name} differs from the model served alone"
    again = serve(bg, Xq)
    for name, x, y in zip(NAMES, got, again):
        assert np.array_equal(x, y), f"two calls differ in {name}"
    for b in range(B):
        assert np.array_equal(cov[:, :, b], cov[:, :, b].T), "every covariance block must be symmetric bit for bit"
    e_diag = relerr(np.einsum("iib->ib", cov), var)
    print(f"case {shape}, M = {M}: diag(cov) against var {e_diag:.2e} (bar {ROUTE_BAR:.1e})")
    assert e_diag < ROUTE_BAR
    assert np.array_equal(mean, mean_s) and np.array_equal(mean, mean_c), "the means of all three calls must agree bit for bit"
    assert np.array_equal(std, np.sqrt(var))
    # mean + Jacobian alone: one launch
    mean_j, dmean_j = bg.predict_jacobian(Xq)
    assert np.array_equal(mean_j, mean) and relerr(dmean_j, dmean) < ROUTE_BAR
    assert np.array_equal(bg.predict(Xq), mean)


# ---- 2. routes ------------------------------------------------------------------------------------------------------------------
def test_routes():
    shape = (6, 300, 400, 10)
    ps, models, bg, Xq_all, ref = case(*shape)
    check_against_numpy("panel route, M = 40", serve(bg, Xq_all[:40]), ref, 40)
    Xq = Xq_all[:25]
    small = serve(bg, Xq)
    bes = [gp._backend() for gp in models]
    for be in bes:
        be.set_options(small_path=0)
    try:
        panel = serve(bg, Xq)
    finally:
        for be in bes:
            be.set_options(small_path=1)
    for name, a, b in zip(NAMES, small, panel):
        e = relerr(a, b)
        print(f"M = 25: small path against small_path=0, {name} {e:.2e} (bar {ROUTE_BAR:.1e})")
        assert e < ROUTE_BAR, (name, e)


# ---- 3. different Z, same m -------------------------------------------------------------------------------------------------------
def test_disjoint_inducing_inputs():
    from unmanned_aerial_vehicles_amd import BatchedSparseGP
    p0 = model_inputs(0, 60, 400, 10)
    p1 = dict(model_inputs(1, 60, 400, 10), X=p0["X"], y=p0["y"], ym=p0["ym"], ys=p0["ys"])
    perm = np.random.default_rng(5).permutation(400)
    p0, p1 = dict(p0, Z=p0["X"][perm[:60]].copy()), dict(p1, Z=p0["X"][perm[60:120]].copy())
    models = [build_model(p0), build_model(p1)]
    bg = BatchedSparseGP(models)
    Xq = p0["Xq"][:25]
    mean, dmean, var, dvar, mean_s, std, mean_c, cov = serve(bg, Xq)
    for b, (gp, p) in enumerate(zip(models, (p0, p1))):
        a_mean, a_dmean, a_var, a_dvar = gp.predict_jacobian(Xq, return_var=True)
        a_cov = gp.predict(Xq, return_cov=True)[1]
        for name, x, y in (("mean", mean[:, b], a_mean), ("dmean", dmean[:, b], a_dmean), ("var", var[:, b], a_var),
                           ("dvar", dvar[:, b], a_dvar), ("cov", cov[:, :, b], a_cov)):
            assert np.array_equal(x, y), f"model {b}: {name} differs from the model served alone"
        r = numpy_form(p["X"], p["y"], p["Z"], Xq, p["ls"], p["sf2"], p["noise"], ALPHA, 1e-8 * p["sf2"], p["ym"], p["ys"])
        for name, x, y in (("mean", mean[:, b], r[0]), ("var", var[:, b], r[1]), ("dmean", dmean[:, b], r[2]),
                           ("dvar", dvar[:, b], r[3]), ("cov", cov[:, :, b], r[4])):
            e = relerr(x, y)
            print(f"disjoint Z, model {b}: {name} {e:.2e} (bar {FP64_BAR:.1e})")
            assert e < FP64_BAR, (b, name, e)
    assert not np.array_equal(mean[:, 0], mean[:, 1])


# ---- 4. the prior -----------------------------------------------------------------------------------------------------------------
def test_prior():
    from unmanned_aerial_vehicles_amd import BatchedSparseGP
    ps = [model_inputs(b, 60, 400, 10) for b in range(3)]
    bg = BatchedSparseGP([build_model(p, rows=False) for p in ps])
    Xq = ps[0]["Xq"][:25]
    mean, dmean, var, dvar, mean_s, std, mean_c, cov = serve(bg, Xq)
    for b, p in enumerate(ps):
        assert np.array_equal(mean[:, b], np.full(25, p["ym"])) and np.array_equal(mean_c[:, b], mean[:, b])
        assert np.array_equal(dmean[:, b], np.zeros((25, 10)))
        want = p["ys"] ** 2 * (rbf(Xq, Xq, p["ls"], p["sf2"]) + p["noise"] * np.eye(25))
        e = relerr(cov[:, :, b], want)
        print(f"prior, model {b}: cov {e:.2e} (bar 1e-14)")
        assert e < 1e-14
        assert relerr(var[:, b], np.diag(want)) < 1e-14


# ---- 5. refusals, never a fault -----------------------------------------------------------------------------------------------------
def test_python_refusals():
    from unmanned_aerial_vehicles_amd import RBF, BatchedSparseGP, SparseGP, WhiteKernel
    ps, models, bg, Xq_all, ref = case(2, 60, 400, 10)
    bad = Xq_all[:5].copy()
    bad[2, 3] = np.nan
    for call in (bg.predict, bg.predict_jacobian, lambda q: bg.predict(q, return_cov=True), bg.sample_y):
        with pytest.raises(ValueError):
            call(bad)
        with pytest.raises(ValueError):
            call(Xq_all[:5, :9])
    bad[2, 3] = np.inf
    with pytest.raises(ValueError):
        bg.predict(bad, return_std=True)
    with pytest.raises(RuntimeError, match="At most one of return_std"):
        bg.predict(Xq_all[:5], return_std=True, return_cov=True)
    kern = RBF(np.ones(10)) + WhiteKernel(0.1)
    with pytest.raises(ValueError):
        BatchedSparseGP([models[0], SparseGP(kern, np.zeros((61, 10)))])
    with pytest.raises(ValueError):
        BatchedSparseGP([models[0], SparseGP(RBF(np.ones(9)) + WhiteKernel(0.1), np.zeros((60, 9)))])
    with pytest.raises(ValueError):
        BatchedSparseGP([SparseGP(kern, np.zeros((60, 10)), y_mean=[0.0, 0.0], y_std=[1.0, 1.0]), models[0]])
    with pytest.raises(ValueError):
        BatchedSparseGP([SparseGP(kern, np.zeros((60, 10))) for _ in range(9)])
    with pytest.raises(ValueError):
        BatchedSparseGP([])
    # the batch still serves, with the earlier bits
    assert np.array_equal(bg.predict(Xq_all[:5]), np.stack([gp.predict(Xq_all[:5]) for gp in models], axis=1))


def test_c_refusals():
    from unmanned_aerial_vehicles_amd import _lib
    ps, models, bg, Xq_all, ref = case(2, 60, 400, 10)
    other = case(6, 1, 17, 3)[1][0]                   # another m and D
    raw = build_model(model_inputs(1, 60, 400, 10))   # rows, but never finalised
    for gp in models + [other]:
        gp._ensure()
    be = models[0]._backend()
    lib = be.lib
    dp = _lib._dp
    M, D = 25, 10
    Xq = np.ascontiguousarray(Xq_all[:M])
    big = np.zeros((16385, D))
    mean, var = np.full((M, 2), np.nan), np.full((M, 2), np.nan)
    dmean, dvar = np.full((M, 2, D), np.nan), np.full((M, 2, D), np.nan)
    cov = np.full((2, M, M), np.nan)
    p = lambda a: a.ctypes.data_as(dp)      # noqa: E731

    def handles(*gps):
        return (C.c_void_p * max(len(gps), 1))(*[None if g is None else g._backend().h.value for g in gps])

    good = handles(*models)
    nine = (C.c_void_p * 9)(*[models[i % 2]._backend().h.value for i in range(9)])
    with be.lock:
        be.bind_stream()
        assert lib.gpk_sparse_predict_multi(be.h, 2, good, p(Xq), M, p(mean), p(var), 1) == _lib.GPK_OK
        first = (mean.copy(), var.copy())
        BAD = _lib.GPK_BAD_ARG
        assert lib.gpk_sparse_predict_multi(be.h, 0, good, p(Xq), M, p(mean), p(var), 1) == BAD
        assert lib.gpk_sparse_predict_multi(be.h, 9, nine, p(Xq), M, p(mean), p(var), 1) == BAD
        assert lib.gpk_sparse_predict_multi(be.h, 2, handles(models[0], None), p(Xq), M, p(mean), p(var), 1) == BAD
        assert lib.gpk_sparse_predict_multi(be.h, 2, handles(models[0], raw), p(Xq), M, p(mean), p(var), 1) == BAD
        assert b"finalised" in lib.gpk_last_error(be.h)
        assert lib.gpk_sparse_predict_multi(be.h, 2, handles(models[0], other), p(Xq), M, p(mean), p(var), 1) == BAD
        assert b"m and D" in lib.gpk_last_error(be.h)
        assert lib.gpk_sparse_predict_multi_cov(be.h, 2, handles(models[0], other), p(Xq), M, p(mean), p(cov)) == BAD
        assert lib.gpk_sparse_predict_multi_grad(be.h, 2, handles(models[0], other), p(Xq), M, p(mean), p(var), p(dmean), p(dvar),
                                                 1) == BAD
        assert lib.gpk_sparse_predict_multi_grad(be.h, 2, good, p(Xq), M, p(mean), p(var), p(dmean), None, 1) == BAD
        assert lib.gpk_sparse_predict_multi_grad(be.h, 2, good, p(Xq), M, p(mean), None, p(dmean), p(dvar), 1) == BAD
        assert lib.gpk_sparse_predict_multi(be.h, 2, good, p(Xq), 0, p(mean), p(var), 1) == BAD
        assert lib.gpk_sparse_predict_multi_grad(be.h, 2, good, p(Xq), 0, p(mean), p(var), p(dmean), p(dvar), 1) == BAD
        assert lib.gpk_sparse_predict_multi_cov(be.h, 2, good, p(Xq), 0, p(mean), p(cov)) == BAD
        assert lib.gpk_sparse_predict_multi_cov(be.h, 2, good, p(big), 16385, p(mean), p(cov)) == BAD
        assert lib.gpk_sparse_predict_multi(be.h, 2, None, p(Xq), M, p(mean), p(var), 1) == BAD
        assert lib.gpk_sparse_predict_multi(None, 2, good, p(Xq), M, p(mean), p(var), 1) == BAD
        nanq = Xq.copy()
        nanq[3, 1] = np.nan
        assert lib.gpk_sparse_predict_multi(be.h, 2, good, p(nanq), M, p(mean), p(var), 1) == BAD
        assert b"NaN or infinity" in lib.gpk_last_error(be.h)
        assert lib.gpk_batch_begin(be.h, 2) == _lib.GPK_OK
        try:
            assert lib.gpk_sparse_predict_multi(be.h, 2, good, p(Xq), M, p(mean), p(var), 1) == BAD
        finally:
            assert lib.gpk_batch_end(be.h) == _lib.GPK_OK
        # a good call: GPK_OK and the earlier bits
        mean[:], var[:] = np.nan, np.nan
        assert lib.gpk_sparse_predict_multi(be.h, 2, good, p(Xq), M, p(mean), p(var), 1) == _lib.GPK_OK
        assert np.array_equal(mean, first[0]) and np.array_equal(var, first[1])
        assert lib.gpk_sparse_predict_multi_grad(be.h, 2, good, p(Xq), M, p(mean), p(var), p(dmean), p(dvar), 1) == _lib.GPK_OK
        assert np.array_equal(mean, first[0]) and np.array_equal(var, first[1])
        assert lib.gpk_sparse_predict_multi_cov(be.h, 2, good, p(Xq), M, p(mean), p(cov)) == _lib.GPK_OK
        assert np.array_equal(mean, first[0]) and np.isfinite(cov).all() and np.isfinite(dvar).all()


# ---- 6. PreTrainedGP ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_dict():
    from unmanned_aerial_vehicles_amd.trainer import OUTPUT_NAMES, StandardScaler
    rng = np.random.default_rng(66)
    Xraw = rng.standard_normal((400, 10)) * (1.0 + np.arange(10)) + np.arange(10)
    sx = StandardScaler().fit(Xraw)
    d = {"gp_models": {}, "scalers_X": {}, "scalers_y": {}, "training_stats": {}}
    for b, name in enumerate(OUTPUT_NAMES):
        p = model_inputs(b, 60, 400, 10)
        yraw = (0.5 + b) * p["y"] + 0.1 * b
        sy = StandardScaler().fit(yraw.reshape(-1, 1))
        Xs = sx.transform(Xraw)
        p = dict(p, X=Xs, Z=Xs[np.random.default_rng(b).permutation(400)[:60]].copy(), y=sy.transform(yraw.reshape(-1, 1)).ravel(),
                 ym=0.0, ys=1.0)
        d["gp_models"][name], d["scalers_X"][name], d["scalers_y"][name] = build_model(p), sx, sy
    rows = rng.standard_normal((25, 10)) * (1.0 + np.arange(10)) + np.arange(10)
    return d, rows


def pretrained(d):
    from unmanned_aerial_vehicles_amd import PreTrainedGP
    pt = PreTrainedGP("/nonexistent/model.pkl")
    assert not pt.is_loaded
    assert pt.load_dict(d)
    return pt


def surfaces(pt, rows):
    Xg = np.hstack([rows[:9, :6].T, rows[8:9, :6].T])      # (6, N + 1), N = 9
    return (pt.predict_residual_batch(rows), pt.predict_residual_jacobian_batch(rows, return_std=True),
            pt.predict_residual_cov_batch(rows), (pt.sample_residuals(rows, n_samples=3, random_state=4),),
            pt.linearize_residuals(Xg, rows[:9, 6:].T, 0.02), pt.predict_residual(rows[0, :6], rows[0, 6:]))


def test_pretrained_gp_serves_the_batch(model_dict, tmp_path):
    from unmanned_aerial_vehicles_amd import BatchedSparseGP, PreTrainedGP
    d, rows = model_dict
    pt = pretrained(d)
    assert pt.is_loaded and isinstance(pt._fused()[0], BatchedSparseGP) and len(pt._fused()[1]) == 6
    fused = surfaces(pt, rows)
    loop_pt = pretrained(d)
    loop_pt._fused_bg = False
    loop = surfaces(loop_pt, rows)
    for k, (fa, la) in enumerate(zip(fused, loop)):
        for x, y in zip(fa, la):
            assert np.isfinite(x).all() and x.shape == y.shape
            assert np.array_equal(x, y), f"surface {k}: the batch and the per-model loop differ"
    assert np.max(fused[0][1]) < 1e5 and np.abs(fused[1][1]).max() > 0.0      # served, not the fallback
    # a pickled file round-trips through PreTrainedGP(path)
    path = str(tmp_path / "sparse_models.pkl")
    with open(path, "wb") as f:
        pickle.dump(dict(d, model_name="sparse", creation_time=0.0), f)
    pt2 = PreTrainedGP(path)
    assert pt2.is_loaded and isinstance(pt2._fused()[0], BatchedSparseGP)
    again = surfaces(pt2, rows)
    for fa, la in zip(fused, again):
        for x, y in zip(fa, la):
            assert np.array_equal(x, y), "the pickled file serves other bits"


def test_pretrained_gp_mixed_models_fall_back(model_dict):
    from unmanned_aerial_vehicles_amd import RBF, GaussianProcessRegressor, WhiteKernel
    from unmanned_aerial_vehicles_amd.trainer import OUTPUT_NAMES
    d, rows = model_dict
    name = OUTPUT_NAMES[2]
    sp = d["gp_models"][name]
    Xs = d["scalers_X"][name].transform(np.random.default_rng(3).standard_normal((80, 10)) * (1.0 + np.arange(10)) + np.arange(10))
    exact = GaussianProcessRegressor(kernel=RBF(np.full(10, 2.0)) + WhiteKernel(0.05), alpha=ALPHA, optimizer=None).fit(
        Xs, np.sin(Xs[:, 0]))
    mixed = dict(d, gp_models=dict(d["gp_models"], **{name: exact}))
    pt = pretrained(mixed)
    assert pt._fused() is False
    mean, std = pt.predict_residual_batch(rows)
    ref_mean, ref_std = pretrained(d).predict_residual_batch(rows)
    assert np.isfinite(mean).all() and np.max(std) < 1e5
    keep = [i for i in range(6) if i != 2]
    assert np.array_equal(mean[:, keep], ref_mean[:, keep]) and np.array_equal(std[:, keep], ref_std[:, keep])
    assert d["gp_models"][name] is sp


# ---- 7. GPTrainer.sparsify ------------------------------------------------------------------------------------------------------------
def test_trainer_sparsify(tmp_path):
    from unmanned_aerial_vehicles_amd import BatchedSparseGP, GPTrainer, PreTrainedGP, SparseGP
    from unmanned_aerial_vehicles_amd.trainer import OUTPUT_NAMES
    rng = np.random.default_rng(77)
    X = rng.standard_normal((600, 10))
    W = rng.standard_normal((10, 6))
    y = np.sin(0.5 * X @ W) * (1.0 + np.arange(6)) + 0.05 * rng.standard_normal((600, 6))
    tr = GPTrainer(model_dir=str(tmp_path))
    tr.train_gp_models(X[:150], y[:150], optimizer=None)
    assert len(tr.gp_models) == 6
    tr.sparsify(X, y, inducing=48)
    assert all(isinstance(m, SparseGP) and m.n_rows_ == 600 and m.inducing_.shape == (48, 10) for m in tr.gp_models.values())
    path = tr.save_models("sparse")
    pt = PreTrainedGP(path)
    assert pt.is_loaded and isinstance(pt._fused()[0], BatchedSparseGP)
    assert all(m.n_rows_ == 600 for m in pt.gp_models.values())
    rows = X[:25]
    mean, std = pt.predict_residual_batch(rows)
    assert np.isfinite(mean).all() and np.isfinite(std).all() and np.max(std) < 1e5
    bg = BatchedSparseGP([tr.gp_models[n] for n in OUTPUT_NAMES])
    ms, ss = bg.predict(tr.scalers_X[OUTPUT_NAMES[0]].transform(rows), return_std=True)
    for j, n in enumerate(OUTPUT_NAMES):
        sy = tr.scalers_y[n]
        assert np.array_equal(mean[:, j], sy.inverse_transform(ms[:, j].reshape(-1, 1)).ravel())
        assert np.array_equal(std[:, j], np.abs(ss[:, j] * sy.scale_[0]))
    # GPTrainer.load_models accepts the file
    tr2 = GPTrainer(model_dir=str(tmp_path))
    tr2.load_models(path)
    assert all(isinstance(m, SparseGP) for m in tr2.gp_models.values())


# ---- 8. pickle round trip -------------------------------------------------------------------------------------------------------------
def test_pickle_round_trip():
    ps, models, bg, Xq_all, ref = case(2, 60, 400, 10)
    Xq = Xq_all[:25]
    before = serve(bg, Xq)
    bg2 = pickle.loads(pickle.dumps(bg))
    assert len(bg2.models) == 2 and bg2.models[0] is not models[0]
    after = serve(bg2, Xq)
    for name, x, y in zip(NAMES, before, after):
        assert np.array_equal(x, y), f"{name} changed over the pickle round trip"
    draws = bg.sample_y(Xq, n_samples=3, random_state=2)
    assert draws.shape == (25, 2, 3) and np.array_equal(draws, bg2.sample_y(Xq, n_samples=3, random_state=2))
