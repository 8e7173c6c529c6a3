"""Writes tests/golden/sparse_fitc_ref.npz: expected results of the FITC sparse GP ("FITC").

NumPy and SciPy only, reproduces its file bit for bit.  The inputs of cases A and B are those of sparse_ref.npz (read here,
not repeated in this file); case C is generated here, seeded.  Every expectation is computed twice and the two must agree
to 1e-8 relative before anything is written; the measured distances are recorded:

* the weighted-statistics form the library uses (include/gpk.h, "FITC"): Wuu = Luu^-1, q_i = |Wuu k_u(x_i)|^2,
  lambda_i = s2 + max(sf2 - q_i, 0), w_i = s2 / lambda_i, G = Kuf diag(w) Kfu, g = Kuf diag(w) Yn, yy = sum w Yn^2, then
  the assembly of gpk_sparse_finalize and the likelihood with -1/2 sum log lambda_i;
* the dense form: Qff + diag(lambda) factorised at N x N, mean = Q*f (Qff + Lambda)^-1 Yn,
  var = sf2 - Q*f (Qff + Lambda)^-1 Qf*, likelihood = log N(Yn | 0, Qff + Lambda).

Case A: N = 700, m = 130, D = 4, P = 2.  Case B: Z = X, N = m = 300, P = 1 - FITC, DTC and the exact GP coincide up to what
jitter_uu on an ill-conditioned Kuu leaves; the distances to the DTC numbers of sparse_ref.npz and to the exact GP are
recorded, not asserted.  Case C: N = 500, m = 40, D = 3, P = 1, the inducing inputs are training rows: for those rows
sf2 - q_i is at jitter level and their weights are 1 to within jitter / s2.  (In exact arithmetic sf2 - q_i = jitter_uu -
O(jitter_uu^2) there, and on this well-conditioned Kuu rounding does not reach it: the script prints how many of these rows
fall below zero - none.  The clip itself is exercised on the GPU with an inverse factor scaled up by 1e-3, whose q_i exceed
sf2 at these rows; the expectation is NumPy's on the same factor.)

    python tests/golden/make_golden_sparse_fitc.py
"""
import os

for _v in ("OPENBLAS_NUM_THREADS", "OMP_NUM_THREADS", "MKL_NUM_THREADS"):      # one BLAS thread: the bits must not depend on how
    os.environ[_v] = "1"                                                     # many the machine, or a busy test run, hands out

import numpy as np  # noqa: E402
from scipy.linalg import cho_solve, cholesky, solve_triangular  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def rbf(A, B, ls, sf2):
    a, b = A / ls, B / ls
    d = a[:, None, :] - b[None, :, :]
    return sf2 * np.exp(-0.5 * np.sum(d * d, axis=2))


def by_weighted_statistics(X, Yn, Z, Xq, ls, sf2, s2, jit):
    N, m = len(X), len(Z)
    Kuf = rbf(Z, X, ls, sf2)
    Luu = cholesky(rbf(Z, Z, ls, sf2) + jit * np.eye(m), lower=True)
    Wuu = solve_triangular(Luu, np.eye(m), lower=True)
    q = np.sum((Wuu @ Kuf) ** 2, axis=0)
    resid = sf2 - q
    lam = s2 + np.maximum(resid, 0.0)
    w = s2 / lam
    G, g, yy = (Kuf * w) @ Kuf.T, (Kuf * w) @ Yn, np.sum(w[:, None] * Yn * Yn, axis=0)
    loglam = float(np.sum(np.log(lam)))
    B = np.eye(m) + Wuu @ G @ Wuu.T / s2
    LB = cholesky(B, lower=True)
    r = Wuu @ g / s2
    c = cho_solve((LB, True), r)
    alpha_u = Wuu.T @ c
    WS = solve_triangular(LB, Wuu, lower=True)
    ku = rbf(Z, Xq, ls, sf2)
    mean_n = ku.T @ alpha_u
    var = sf2 - np.sum((Wuu @ ku) ** 2, axis=0) + np.sum((WS @ ku) ** 2, axis=0)
    lik = sum(-0.5 * N * np.log(2 * np.pi) - 0.5 * loglam - np.sum(np.log(np.diag(LB))) - 0.5 * yy[p] / s2
              + 0.5 * r[:, p] @ c[:, p] for p in range(Yn.shape[1]))
    return dict(G=G, g=g, yy=yy, loglam=loglam, w=w, resid=resid, mean_n=mean_n, var=var, lik=float(lik))


def by_dense_form(X, Yn, Z, Xq, ls, sf2, s2, jit):
    N, m = len(X), len(Z)
    cU = (cholesky(rbf(Z, Z, ls, sf2) + jit * np.eye(m), lower=True), True)
    Kuf = rbf(Z, X, ls, sf2)
    Qff = Kuf.T @ cho_solve(cU, Kuf)
    lam = s2 + np.maximum(sf2 - np.diag(Qff), 0.0)
    Ly = cholesky(Qff + np.diag(lam), lower=True)
    ku = rbf(Z, Xq, ls, sf2)
    Qsf = ku.T @ cho_solve(cU, Kuf)
    mean_n = Qsf @ cho_solve((Ly, True), Yn)
    V = solve_triangular(Ly, Qsf.T, lower=True)
    var = sf2 - np.sum(V * V, axis=0)
    a = cho_solve((Ly, True), Yn)
    lik = sum(-0.5 * Yn[:, p] @ a[:, p] - np.sum(np.log(np.diag(Ly))) - 0.5 * N * np.log(2 * np.pi) for p in range(Yn.shape[1]))
    return dict(mean_n=mean_n, var=var, lik=float(lik))


def dist(a, b):
    """max |a - b| / max |b|"""
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(np.asarray(b))), 1e-300))


def agree(a, b, tol, what):
    err = dist(a, b)
    assert err < tol, (what, err)
    return err


def case(name, X, Y, Z, Xq, ls, hyper, y_mean, y_std, out):
    sf2, noise, alpha, jit = hyper
    s2 = noise + alpha
    Yn = (Y - y_mean) / y_std
    a = by_weighted_statistics(X, Yn, Z, Xq, ls, sf2, s2, jit)
    d = by_dense_form(X, Yn, Z, Xq, ls, sf2, s2, jit)
    e = np.array([agree(a["mean_n"], d["mean_n"], 1e-8, name + " mean"), agree(a["var"] / sf2, d["var"] / sf2, 1e-8, name + " var"),
                  agree(a["lik"], d["lik"], 1e-8, name + " likelihood")])
    print("case %s: the two forms differ by  mean %.1e  var/sf2 %.1e  likelihood %.1e;  weights in [%.3g, %.3g]" % (
        name, e[0], e[1], e[2], a["w"].min(), a["w"].max()))
    assert np.all(np.isfinite(a["w"])) and a["w"].min() > 0.0 and a["w"].max() <= 1.0
    out.update({name + "_g": a["g"], name + "_yy": a["yy"], name + "_loglam": np.array(a["loglam"]), name + "_w": a["w"],
                name + "_mean": y_mean + y_std * a["mean_n"], name + "_var": a["var"], name + "_lik": np.array(a["lik"]),
                name + "_forms": e})
    return a


def main():
    ref = np.load(os.path.join(HERE, "sparse_ref.npz"))
    out = {}
    # ---- case A ----------------------------------------------------------------------------------------------------
    a = case("A", ref["A_X"], ref["A_Y"], ref["A_Z"], ref["A_Xq"], ref["A_ls"], ref["A_hyper"], ref["A_y_mean"], ref["A_y_std"], out)
    out["A_G"] = a["G"]
    print("case A: FITC against DTC         mean %.1e  (std(y) units)" % float(
        np.max(np.abs((out["A_mean"] - ref["A_mean"]) / ref["A_y_std"]))))
    # ---- case B: Z = X (G is 300 x 300 and is not stored) ------------------------------------------------------------
    b = case("B", ref["B_X"], ref["B_Y"], ref["B_X"], ref["B_Xq"], ref["B_ls"], ref["B_hyper"], ref["B_y_mean"], ref["B_y_std"], out)
    sf2 = ref["B_hyper"][0]
    out["B_vs_dtc"] = np.array([dist(out["B_mean"], ref["B_mean"]), dist(b["var"] / sf2, ref["B_var"] / sf2),
                                dist(b["lik"], ref["B_bound"])])
    out["B_vs_exact"] = np.array([dist(out["B_mean"], ref["B_exact_mean"]), dist(b["var"] / sf2, ref["B_exact_var"] / sf2),
                                  dist(b["lik"], ref["B_exact_lml"])])
    print("case B: FITC against DTC         mean %.1e  var/sf2 %.1e  likelihood %.1e" % tuple(out["B_vs_dtc"]))
    print("case B: FITC against exact       mean %.1e  var/sf2 %.1e  likelihood %.1e" % tuple(out["B_vs_exact"]))
    # ---- case C: the inducing inputs are training rows -------------------------------------------------------------
    rng = np.random.default_rng(3106)
    N, m, D, M = 500, 40, 3, 40
    X = rng.standard_normal((N, D))
    Y = (np.sin(X[:, 0]) + 0.5 * np.cos(1.3 * X[:, 1]) + 0.3 * X[:, 2] + 0.1 * rng.standard_normal(N))[:, None]
    idx = np.sort(rng.permutation(N)[:m])
    Z = X[idx].copy()
    Xq = rng.standard_normal((M, D))
    Xq[[2, 11]] = X[[idx[0], 7]]
    ls = 0.8 * (1.0 + 0.1 * np.arange(D))
    hyper = np.array([1.1, 0.04, 1e-6, 1e-8 * 1.1])
    y_mean, y_std = Y.mean(axis=0), Y.std(axis=0)
    c = case("C", X, Y, Z, Xq, ls, hyper, y_mean, y_std, out)
    out["C_G"] = c["G"]
    at_z = c["resid"][idx]
    print("case C: sf2 - q_i at the inducing rows in [%.2e, %.2e], %d of %d below zero (clipped); their weights differ from 1 by "
          "at most %.1e" % (at_z.min(), at_z.max(), int(np.sum(at_z < 0)), m, float(np.max(1.0 - c["w"][idx]))))
    assert np.max(1.0 - c["w"][idx]) < 1e-6
    out.update(C_X=X, C_Y=Y, C_Z=Z, C_idx=idx, C_Xq=Xq, C_ls=ls, C_hyper=hyper, C_y_mean=y_mean, C_y_std=y_std)
    path = os.path.join(HERE, "sparse_fitc_ref.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
