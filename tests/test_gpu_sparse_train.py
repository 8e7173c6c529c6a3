"""Training the sparse inducing-point GP on the GPU against tests/golden/sparse_train_ref.npz (NumPy / SciPy,
two independent forms of every gradient): the row pass alone (`gpk_sparse_grad_pass`), the evaluation (`SparseGP.log_bound`,
`gpk_sparse_eval`) and `SparseGP.train`.  Buffers start out as NaN (conftest: GPK_DEBUG_FILL)."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest

from conftest import GOLDEN, relerr
from test_sparse_train_host import load_writer

pytestmark = pytest.mark.gpu

ROUTE_BAR = 1e-12     # routes that differ in summation order only (of the sum of the terms' absolute values)
LIMIT_BAR = 2e-12     # ... at the limits (D = P = 16), as the statistics pass has it
FP64_BAR = 1e-8


@pytest.fixture(scope="module")
def ref():
    d = np.load(os.path.join(GOLDEN, "sparse_train_ref.npz"))
    return {k: d[k] for k in d.files}


@pytest.fixture(scope="module")
def writer():
    return load_writer()


def run_pass(be, X, Yn, Z, ls, sf2, Cfull):
    """gpk_sparse_grad_pass on host arrays; Cfull ((m + P) x m) goes into the padded, zero-filled device layout.  Returns the
    17 sums."""
    import torch
    n, D, m, P = X.shape[0], X.shape[1], Z.shape[0], Yn.shape[1]
    mp = (m + 127) // 128 * 128
    Cm = np.zeros((mp + 128, mp))
    Cm[:m, :m] = Cfull[:m]
    Cm[mp:mp + P, :m] = Cfull[m:]
    dX, dY, dZ, dC = be.upload(X), be.upload(Yn), be.upload(Z), be.upload(Cm)
    sums = torch.full((17,), float("nan"), dtype=torch.float64, device=be.device)
    ls = np.ascontiguousarray(ls, dtype=np.float64)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    with be.lock:
        be.bind_stream()
        be.check(be.lib.gpk_sparse_grad_pass(be.h, p(dX), p(dY), n, p(dZ), m, D, P, ls.ctypes.data_as(C.POINTER(C.c_double)),
                                             float(sf2), p(dC), mp, p(sums)))
        be.sync()
    return sums.cpu().numpy()


def pass_error(got, want, scale, D):
    idx = list(range(D)) + [16]
    return float(np.max(np.abs(got[idx] - want) / scale))


# ---- 1. the row pass alone -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("panel", [256, 0])
def test_row_pass_case_a(ref, panel):
    """panel = 256: three panels, the last with 188 rows."""
    from unmanned_aerial_vehicles_amd.device import Backend
    be = Backend(0).set_options(sparse_panel=panel)
    Yn = (ref["A_Y"] - ref["A_y_mean"]) / ref["A_y_std"]
    runs = [run_pass(be, ref["A_X"], Yn, ref["A_Z"], ref["A_ls"], ref["A_hyper"][0], ref["A_C"]) for _ in range(2)]
    e = pass_error(runs[0], ref["A_pass"], ref["A_pass_abs"], 4)
    print(f"panel {panel}: row pass against the fixture {e:.2e} of the sum of absolute values")
    assert e < ROUTE_BAR
    assert np.array_equal(runs[0][[0, 1, 2, 3, 16]], runs[1][[0, 1, 2, 3, 16]]), "two runs must give identical bits"
    be.lib.gpk_destroy(be.h)


@pytest.mark.parametrize("m,n,D,P", [(1, 17, 3, 2), (128, 17, 16, 16), (5, 1, 4, 1)])
def test_row_pass_at_the_limits(writer, m, n, D, P):
    from unmanned_aerial_vehicles_amd.device import Backend
    rng = np.random.default_rng(842 + m + n)
    X, Z, Yn = rng.standard_normal((n, D)), rng.standard_normal((m, D)), rng.standard_normal((n, P))
    ls = 3.0 * (1.0 + 0.05 * np.arange(D))
    Cr = rng.standard_normal((m + P, m))
    want, scale = writer.pass_sums(X, Yn, Z, ls, 0.9, Cr)
    be = Backend(0)
    e = pass_error(run_pass(be, X, Yn, Z, ls, 0.9, Cr), want, scale, D)
    print(f"m {m} n {n} D {D} P {P}: {e:.2e}")
    assert e < LIMIT_BAR
    be.lib.gpk_destroy(be.h)


def case_a_kernel(ref, variant="free", iso=False):
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, WhiteKernel
    sf2, noise, alpha, jit = ref["A_hyper"]
    ls = float(ref["Aiso_ls"][0]) if iso else ref["A_ls"]
    const = ConstantKernel(sf2, constant_value_bounds="fixed") if variant == "constant fixed" else ConstantKernel(sf2)
    white = WhiteKernel(noise, noise_level_bounds="fixed") if variant == "noise fixed" else WhiteKernel(noise)
    return const * RBF(ls) + white


def case_a_model(ref, kernel):
    from unmanned_aerial_vehicles_amd import SparseGP
    sf2, noise, alpha, jit = ref["A_hyper"]
    return SparseGP(kernel, ref["A_Z"], alpha=float(alpha), jitter_uu=float(jit), y_mean=ref["A_y_mean"], y_std=ref["A_y_std"])


def test_unweighted_sum_from_the_statistics(ref, writer):
    """sums[16] of the pass on C = [2 dL/dG ; dL/dg^T] equals 2 sum dL/dG o G + sum dL/dg o g formed from the exported
    statistics, to 1e-12 of the sum of the absolute values of those terms (only the order of summation differs)."""
    gp = case_a_model(ref, case_a_kernel(ref)).hold(ref["A_X"], ref["A_Y"])
    st = gp.statistics()
    G, g = st["G"], st["g"]
    sf2, noise, alpha, jit = ref["A_hyper"]
    s2, Z, ls, P = noise + alpha, ref["A_Z"], ref["A_ls"], 2
    Kuu = writer.rbf(Z, Z, ls, sf2) + jit * np.eye(len(Z))
    Ki, Si = np.linalg.inv(Kuu), np.linalg.inv(Kuu + G / s2)
    au = Si @ g / s2
    GG, Gg = P / (2 * s2) * (Ki - Si) - au @ au.T / (2 * s2), au / s2
    want = 2 * np.sum(GG * G) + np.sum(Gg * g)
    scale = 2 * np.sum(np.abs(GG * G)) + np.sum(np.abs(Gg * g))
    Yn = (ref["A_Y"] - ref["A_y_mean"]) / ref["A_y_std"]
    got = run_pass(gp._backend(), ref["A_X"], Yn, Z, ls, sf2, np.vstack([2 * GG, Gg.T]))[16]
    print(f"unweighted sum {got:.12e} against the statistics {want:.12e}: {abs(got - want) / scale:.2e} of {scale:.3e}")
    assert abs(got - want) < 1e-12 * scale


# ---- 2. the evaluation -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iso", [False, True], ids=["ard", "isotropic"])
@pytest.mark.parametrize("variant", ["free", "noise fixed", "constant fixed"])
def test_log_bound_case_a(ref, variant, iso):
    kernel = case_a_kernel(ref, variant, iso)
    gp = case_a_model(ref, kernel).hold(ref["A_X"], ref["A_Y"])
    value, grad = gp.log_bound(kernel.theta, eval_gradient=True)
    pre = "Aiso" if iso else "A"
    want = kernel.components().map_gradient(ref[pre + "_grad"], 1 if iso else 4)
    e = (abs(value - float(ref[pre + "_bound"])) / abs(float(ref[pre + "_bound"])), relerr(grad, want))
    print(f"{variant}, {'isotropic' if iso else 'ARD'}: bound {e[0]:.2e} gradient {e[1]:.2e} of its largest component")
    assert grad.shape == kernel.theta.shape and max(e) < FP64_BAR
    assert gp.log_bound(kernel.theta) == value == gp.bound(), "the value alone, and the finalised model's bound"
    assert gp.n_rows_ == 700


def test_case_b_against_the_exact_lml(ref):
    """Z = X: the bound is the exact LML at every theta, so is its gradient, up to jitter_uu."""
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, GaussianProcessRegressor, SparseGP, WhiteKernel
    sf2, noise, alpha, jit = ref["B_hyper"]
    kernel = ConstantKernel(sf2) * RBF(ref["B_ls"]) + WhiteKernel(noise)
    X, y = ref["B_X"], ref["B_Y"][:, 0]
    exact = GaussianProcessRegressor(kernel=kernel, alpha=float(alpha), normalize_y=True, optimizer=None).fit(X, y)
    theta = kernel.theta + 0.05 * np.cos(np.arange(kernel.theta.size))          # not the fitted point
    lml, lgrad = exact.log_marginal_likelihood(theta, eval_gradient=True)
    sp = SparseGP.from_exact(exact, inducing=None, jitter_uu=float(jit)).hold(X, y)
    value, grad = sp.log_bound(theta, eval_gradient=True)
    e = (abs(value - lml) / abs(lml), relerr(grad, lgrad))
    bar = 10.0 * float(ref["B_jitter_diff"])
    print(f"Z = X against the exact GP: bound {e[0]:.2e} gradient {e[1]:.2e} (bar {bar:.1e}: ten times the jitter's effect)")
    assert e[0] < FP64_BAR and e[1] < bar


def test_not_positive_definite(ref, writer):
    from unmanned_aerial_vehicles_amd import RBF, SparseGP, WhiteKernel
    X, Y = ref["A_X"], ref["A_Y"][:, :1]
    ym, ys = ref["A_y_mean"][:1], ref["A_y_std"][:1]
    kernel = RBF(1.0) + WhiteKernel(0.01)
    # two identical rows, no jitter: Kuu = [[1, 1], [1, 1]], the second pivot is exactly zero - at every theta
    gp = SparseGP(kernel, np.stack([X[5], X[5]]), alpha=1e-6, jitter_uu=0.0, y_mean=ym, y_std=ys).hold(X, Y)
    value, grad = gp.log_bound(kernel.theta, eval_gradient=True)
    assert value == -np.inf and grad.shape == (2,) and not grad.any()
    assert gp.log_bound(kernel.theta) == -np.inf
    # two rows 1e-8 apart: exp(-0.5e-16) rounds to one and the same happens at length-scale 1, while at 1e-5 the matrix is
    # well conditioned - the object that has just failed evaluates correctly there
    Z = np.stack([X[5], X[5]])
    Z[1, 0] += 1e-8
    gp = SparseGP(kernel, Z, alpha=1e-6, jitter_uu=0.0, y_mean=ym, y_std=ys).hold(X, Y)
    value, grad = gp.log_bound(kernel.theta, eval_gradient=True)
    assert value == -np.inf and not grad.any()
    with pytest.raises(np.linalg.LinAlgError):
        gp.predict(X[:2])
    good = np.log([1e-5, 0.02])
    value, grad = gp.log_bound(good, eval_gradient=True)
    Yn = (Y - ym) / ys
    want = writer.bound_value(X, Yn, Z, np.full(4, 1e-5), 1.0, 0.02, 1e-6, 0.0)
    g = writer.grad_assembly(X, Yn, Z, np.full(4, 1e-5), 1.0, 0.02, 1e-6, 0.0)[0]
    e = (abs(value - want) / abs(want), relerr(grad, [g[:4].sum(), g[4]]))
    print(f"after the failure, at a good theta: bound {e[0]:.2e} gradient {e[1]:.2e}")
    assert max(e) < FP64_BAR and np.isfinite(gp.predict(X[:2])).all()


def test_log_bound_needs_held_rows(ref):
    kernel = case_a_kernel(ref)
    gp = case_a_model(ref, kernel).partial_fit(ref["A_X"][:50], ref["A_Y"][:50])
    with pytest.raises(RuntimeError, match="hold"):
        gp.log_bound(kernel.theta)
    with pytest.raises(ValueError):
        gp.log_bound(None, eval_gradient=True)
    gp.hold(ref["A_X"][:50], ref["A_Y"][:50]).partial_fit(ref["A_X"][50:60], ref["A_Y"][50:60])
    with pytest.raises(RuntimeError, match="hold"):
        gp.log_bound(kernel.theta)
    assert gp.n_rows_ == 60


# ---- 3. train --------------------------------------------------------------------------------------------------------
def training_model(ref, kernel=None):
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, SparseGP, WhiteKernel
    sf2, ls0, ls1, noise = ref["T_start"]
    jitter, jit = ref["T_hyper"]
    if kernel is None:
        kernel = ConstantKernel(sf2) * RBF([ls0, ls1]) + WhiteKernel(noise)
    return SparseGP(kernel, ref["T_Z"], alpha=float(jitter), jitter_uu=float(jit), y_mean=ref["T_y_mean"], y_std=ref["T_y_std"])


def test_train(ref):
    X, y = ref["T_X"], ref["T_Y"][:, 0]
    gp = training_model(ref)
    before = gp.hold(X, y).log_bound(gp.kernel_.theta)
    assert abs(before - float(ref["T_bound_start"])) < FP64_BAR * abs(float(ref["T_bound_start"]))
    assert gp.train(X, y) is gp
    opt = float(ref["T_bound_opt"])
    print(f"bound {before:.6f} -> {gp.bound_value_:.6f} (SciPy on the NumPy bound: {opt:.6f}); kernel {gp.kernel_}")
    assert gp.bound_value_ > before
    assert gp.bound_value_ >= opt - 1e-6 * abs(opt)
    assert gp.bound() == gp.bound_value_ and gp.n_rows_ == 600
    assert np.array_equal(gp.kernel.theta, np.log(ref["T_start"])), "the kernel passed in is left alone"
    # the model left behind is the one a fresh object builds from the trained kernel
    Xq = np.random.default_rng(843).uniform(-3.0, 3.0, (40, 2))
    mean, std = gp.predict(Xq, return_std=True)
    fresh = training_model(ref, gp.kernel_).fit(X, y)
    fm, fs = fresh.predict(Xq, return_std=True)
    e = (relerr(mean, fm), relerr(std, fs))
    print(f"trained model against a fresh fit with its kernel: mean {e[0]:.2e} std {e[1]:.2e}")
    assert mean.shape == (40,) and max(e) < 1e-12
    # pickle keeps the kernel and the predictions
    gp2 = pickle.loads(pickle.dumps(gp))
    assert np.array_equal(gp2.kernel_.theta, gp.kernel_.theta) and gp2.bound_value_ == gp.bound_value_
    pm, ps = gp2.predict(Xq, return_std=True)
    assert np.array_equal(pm, mean) and np.array_equal(ps, std)
    # ... and the trained model goes on learning
    Xn = np.random.default_rng(844).uniform(-3.0, 3.0, (30, 2))
    yn = np.sin(Xn[:, 0])
    gp.partial_fit(Xn, yn)
    fresh.partial_fit(Xn, yn)
    assert gp.n_rows_ == 630
    assert relerr(gp.predict(Xq), fresh.predict(Xq)) < 1e-12


def test_train_refusals(ref):
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel
    X, y = ref["T_X"], ref["T_Y"][:, 0]
    fixed = ConstantKernel(1.0, constant_value_bounds="fixed") * RBF([1.0, 1.0], length_scale_bounds="fixed")
    with pytest.raises(ValueError, match="no free parameter"):
        training_model(ref, fixed).train(X, y)
    with pytest.raises(ValueError, match="Unknown optimizer"):
        training_model(ref).train(X, y, optimizer="nope")
    with pytest.raises(ValueError):
        training_model(ref).train(X[:, :1], y)


def test_train_with_a_restart(ref):
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, WhiteKernel
    X, y = ref["T_X"][:200], ref["T_Y"][:200, 0]
    sf2, ls0, ls1, noise = ref["T_start"]
    kernel = ConstantKernel(sf2, (1e-2, 1e2)) * RBF([ls0, ls1], (1e-1, 1e1)) + WhiteKernel(noise, (1e-3, 1e1))
    a = training_model(ref, kernel).train(X, y, n_restarts_optimizer=1, random_state=3)
    b = training_model(ref, kernel).train(X, y, n_restarts_optimizer=1, random_state=3)
    single = training_model(ref, kernel).train(X, y)
    assert a.bound_value_ == b.bound_value_ and np.array_equal(a.kernel_.theta, b.kernel_.theta)
    assert a.bound_value_ >= single.bound_value_
    lo, hi = kernel.bounds[:, 0], kernel.bounds[:, 1]
    assert np.all(a.kernel_.theta >= lo) and np.all(a.kernel_.theta <= hi)


# ---- 4. the untrained object is unchanged ----------------------------------------------------------------------------
def test_untrained_object_unchanged(ref):
    d = np.load(os.path.join(GOLDEN, "sparse_ref.npz"))
    gp = case_a_model(ref, case_a_kernel(ref)).fit(ref["A_X"][:400], ref["A_Y"][:400]).partial_fit(ref["A_X"][400:], ref["A_Y"][400:])
    mean, std = gp.predict(d["A_Xq"], return_std=True)
    noise = d["A_hyper"][1]
    want_std = np.sqrt(d["A_var"] + noise)[:, None] * d["A_y_std"][None, :]
    e = (relerr(mean, d["A_mean"]), relerr(std, want_std), abs(gp.bound() - float(d["A_bound"])) / abs(float(d["A_bound"])))
    print(f"fit / partial_fit / predict: mean {e[0]:.2e} std {e[1]:.2e} bound {e[2]:.2e}")
    assert max(e) < FP64_BAR
    assert np.array_equal(gp.kernel_.theta, gp.kernel.theta) and not hasattr(gp, "bound_value_")
