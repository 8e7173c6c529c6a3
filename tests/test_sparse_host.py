"""tests/golden/sparse_ref.npz (the sparse inducing-point GP's fixture, written by tests/golden/make_golden_sparse.py) is
self-consistent - its expectations are recomputed here by the naive dense form Sigma = Kuu + Kuf Kfu / s2, which shares no
intermediate with the assembly that wrote them - and, where Z = X (case B), consistent with the oracle's exact GP.  NumPy /
SciPy only: no GPU."""
import os

import numpy as np
import pytest
from scipy.linalg import cho_solve, cholesky

from conftest import GOLDEN, relerr
from oracle import gp_oracle as O


@pytest.fixture(scope="module")
def ref():
    d = np.load(os.path.join(GOLDEN, "sparse_ref.npz"))
    return {k: d[k] for k in d.files}


def dense_form(X, Yn, Z, Xq, ls, sf2, s2, jit):
    N, m = len(X), len(Z)
    Kuu = O.rbf_gram(Z, ls, sf2, jit)
    Kuf = O.rbf_cross(Z, X, ls, sf2)
    ku = O.rbf_cross(Z, Xq, ls, sf2)
    cS, cU = (cholesky(Kuu + Kuf @ Kuf.T / s2, lower=True), True), (cholesky(Kuu, lower=True), True)
    mean_n = ku.T @ cho_solve(cS, Kuf @ Yn) / s2
    var = sf2 - np.sum(ku * cho_solve(cU, ku), axis=0) + np.sum(ku * cho_solve(cS, ku), axis=0)
    Qff = Kuf.T @ cho_solve(cU, Kuf)
    Lq = cholesky(Qff + s2 * np.eye(N), lower=True)
    a = cho_solve((Lq, True), Yn)
    bound = sum(-0.5 * Yn[:, p] @ a[:, p] - np.sum(np.log(np.diag(Lq))) - 0.5 * N * np.log(2 * np.pi)
                - 0.5 * (N * sf2 - np.trace(Qff)) / s2 for p in range(Yn.shape[1]))
    return mean_n, var, float(bound), Kuf


@pytest.mark.parametrize("case", ["A", "B"])
def test_fixture_is_self_consistent(ref, case):
    X, Y, Xq, ls = ref[case + "_X"], ref[case + "_Y"], ref[case + "_Xq"], ref[case + "_ls"]
    Z = ref["A_Z"] if case == "A" else X
    sf2, noise, alpha, jit = ref[case + "_hyper"]
    ym, ys = ref[case + "_y_mean"], ref[case + "_y_std"]
    Yn = (Y - ym) / ys
    mean_n, var, bound, Kuf = dense_form(X, Yn, Z, Xq, ls, sf2, noise + alpha, jit)
    # the two NumPy forms differ by 5e-11 (mean), 7e-13 (variance / sf2) and 4e-12 (bound) on case A
    assert relerr(ym + ys * mean_n, ref[case + "_mean"]) < 1e-9
    assert np.max(np.abs(var - ref[case + "_var"])) / sf2 < 1e-10
    assert abs(bound - float(ref[case + "_bound"])) < 1e-10 * abs(bound)
    assert np.all(ref[case + "_var"] > 0) and np.all(ref[case + "_var"] <= sf2 * (1 + 1e-12))
    if case == "A":
        assert ref["A_Z"].shape == (130, 4) and X.shape == (700, 4) and Y.shape == (700, 2) and Xq.shape == (40, 4)
        assert relerr(Kuf @ Kuf.T, ref["A_G"]) < 1e-13 and relerr(Kuf @ Yn, ref["A_g"]) < 1e-13
        assert relerr(np.sum(Yn * Yn, axis=0), ref["A_yy"]) < 1e-13
        assert relerr(ref["A_G"], ref["A_G"].T) < 1e-15


def test_case_b_is_the_exact_gp(ref):
    """Z = X: the sparse predictor is the exact GP with noise s2 (up to jitter_uu = 1e-10 sf2) and the bound its LML."""
    X, Y, Xq, ls = ref["B_X"], ref["B_Y"], ref["B_Xq"], ref["B_ls"]
    sf2, noise, alpha, jit = ref["B_hyper"]
    st = O.fit_fixed(X, Y, ls, sf2, noise, alpha, normalize_y=True)
    assert relerr(st.y_mean, ref["B_y_mean"]) < 1e-14 and relerr(st.y_std, ref["B_y_std"]) < 1e-14
    mean, std = O.predict(st, Xq, return_std=True, diag_includes_noise=False)
    lml = O.log_marginal_likelihood(st)
    ys = ref["B_y_std"]
    sp_std = np.sqrt(ref["B_var"]) * ys[0]
    assert relerr(ref["B_exact_mean"], np.asarray(mean).reshape(ref["B_exact_mean"].shape)) < 1e-10
    assert abs(float(ref["B_exact_lml"]) - lml) < 1e-10 * abs(lml)
    # measured: mean 2.2e-10, variance 2.5e-10 of sf2, bound 1.3e-9 (the jitter on Kuu)
    assert relerr(ref["B_mean"], np.asarray(mean).reshape(ref["B_mean"].shape)) < 1e-8
    assert relerr(sp_std, np.asarray(std).reshape(sp_std.shape)) < 1e-8
    assert abs(float(ref["B_bound"]) - lml) < 1e-8 * abs(lml)
