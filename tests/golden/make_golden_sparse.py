"""Writes tests/golden/sparse_ref.npz: inputs and expected results of the sparse inducing-point GP.

NumPy and SciPy only, seeded, reproduces its file bit for bit.  Every expectation is computed twice and the two must agree
before anything is written:

* by the assembly the library uses (include/gpk.h, gpk_sparse_finalize): Luu, Wuu = Luu^-1, B = I + Wuu G Wuu^T / s2, ...
* by the naive dense form: Sigma = Kuu + Kuf Kfu / s2, mean = k_u^T Sigma^-1 Kuf Yn / s2,
  var = sf2 - k_u^T Kuu^-1 k_u + k_u^T Sigma^-1 k_u, and the bound as log N(Yn | 0, Qff + s2 I) - tr(Kff - Qff) / (2 s2)
  with Qff + s2 I factorised at N x N.

Case A: N = 700, m = 130 (a partial tile plus a padded one), D = 4, P = 2.  Case B: Z = X, N = m = 300, D = 6, P = 1, where
the sparse model is the exact GP (up to jitter_uu): its expectations are the exact GP's, computed here as well.

    python tests/golden/make_golden_sparse.py
"""
import os

import numpy as np
from scipy.linalg import cho_solve, cholesky, solve_triangular

HERE = os.path.dirname(os.path.abspath(__file__))


def rbf(A, B, ls, sf2):
    a, b = A / ls, B / ls
    d = a[:, None, :] - b[None, :, :]
    return sf2 * np.exp(-0.5 * np.sum(d * d, axis=2))


def by_assembly(X, Yn, Z, Xq, ls, sf2, s2, jit):
    N, m = len(X), len(Z)
    Kuf = rbf(Z, X, ls, sf2)
    G, g, yy = Kuf @ Kuf.T, Kuf @ Yn, np.sum(Yn * Yn, axis=0)
    Luu = cholesky(rbf(Z, Z, ls, sf2) + jit * np.eye(m), lower=True)
    Wuu = solve_triangular(Luu, np.eye(m), lower=True)
    B = np.eye(m) + Wuu @ G @ Wuu.T / s2
    LB = cholesky(B, lower=True)
    r = Wuu @ g / s2
    c = cho_solve((LB, True), r)
    alpha_u = Wuu.T @ c
    WS = solve_triangular(LB, Wuu, lower=True)
    ku = rbf(Z, Xq, ls, sf2)
    mean_n = ku.T @ alpha_u
    var = sf2 - np.sum((Wuu @ ku) ** 2, axis=0) + np.sum((WS @ ku) ** 2, axis=0)
    bound = sum(-0.5 * N * np.log(2 * np.pi * s2) - np.sum(np.log(np.diag(LB))) - 0.5 * (N * sf2 - s2 * (np.trace(B) - m)) / s2
                - 0.5 * yy[p] / s2 + 0.5 * r[:, p] @ c[:, p] for p in range(Yn.shape[1]))
    return dict(G=G, g=g, yy=yy, mean_n=mean_n, var=var, bound=float(bound))


def by_dense_form(X, Yn, Z, Xq, ls, sf2, s2, jit):
    N, m = len(X), len(Z)
    Kuu = rbf(Z, Z, ls, sf2) + jit * np.eye(m)
    Kuf = rbf(Z, X, ls, sf2)
    Sigma = Kuu + Kuf @ Kuf.T / s2
    ku = rbf(Z, Xq, ls, sf2)
    cS, cU = (cholesky(Sigma, lower=True), True), (cholesky(Kuu, lower=True), True)
    mean_n = ku.T @ cho_solve(cS, Kuf @ Yn) / s2
    var = sf2 - np.sum(ku * cho_solve(cU, ku), axis=0) + np.sum(ku * cho_solve(cS, ku), axis=0)
    Qff = Kuf.T @ cho_solve(cU, Kuf)
    Lq = cholesky(Qff + s2 * np.eye(N), lower=True)
    a = cho_solve((Lq, True), Yn)
    bound = sum(-0.5 * Yn[:, p] @ a[:, p] - np.sum(np.log(np.diag(Lq))) - 0.5 * N * np.log(2 * np.pi)
                - 0.5 * (N * sf2 - np.trace(Qff)) / s2 for p in range(Yn.shape[1]))
    return dict(mean_n=mean_n, var=var, bound=float(bound))


def exact_gp(X, Yn, Xq, ls, sf2, s2):
    N = len(X)
    L = cholesky(rbf(X, X, ls, sf2) + s2 * np.eye(N), lower=True)
    alpha = cho_solve((L, True), Yn)
    ks = rbf(X, Xq, ls, sf2)
    V = solve_triangular(L, ks, lower=True)
    lml = sum(-0.5 * Yn[:, p] @ alpha[:, p] - np.sum(np.log(np.diag(L))) - 0.5 * N * np.log(2 * np.pi)
              for p in range(Yn.shape[1]))
    return ks.T @ alpha, sf2 - np.sum(V * V, axis=0), float(lml)


def targets(X, P, rng):
    Y = np.stack([np.sin(X[:, 0] + 0.5 * p) + 0.5 * np.cos(1.3 * X[:, 1] - 0.2 * p) + 0.3 * X[:, 2] * (p + 1) for p in range(P)],
                 axis=1)
    return 2.0 + 1.5 * Y + 0.1 * rng.standard_normal(Y.shape)


def agree(a, b, tol, what):
    err = float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(np.asarray(b))), 1e-300))
    assert err < tol, (what, err)
    return err


def main():
    out = {}
    # ---- case A ----------------------------------------------------------------------------------------------------
    rng = np.random.default_rng(830)
    N, m, D, P, M = 700, 130, 4, 2, 40
    X = rng.standard_normal((N, D))
    Y = targets(X, P, rng)
    Z = X[np.sort(rng.permutation(N)[:m])].copy()
    Xq = rng.standard_normal((M, D))
    Xq[[3, 17, 31]] = X[[5, 250, 699]]
    ls = 1.0 * (1.0 + 0.1 * np.arange(D))
    sf2, noise, alpha = 1.3, 0.0099, 1e-4
    s2, jit = noise + alpha, 1e-8 * sf2
    y_mean, y_std = Y.mean(axis=0), Y.std(axis=0)
    Yn = (Y - y_mean) / y_std
    a, d = by_assembly(X, Yn, Z, Xq, ls, sf2, s2, jit), by_dense_form(X, Yn, Z, Xq, ls, sf2, s2, jit)
    print("case A: the two forms differ by  mean %.1e  var/sf2 %.1e  bound %.1e" % (
        agree(a["mean_n"], d["mean_n"], 1e-8, "A mean"), agree(a["var"] / sf2, d["var"] / sf2, 1e-8, "A var"),
        agree(a["bound"], d["bound"], 1e-9, "A bound")))
    out.update(A_X=X, A_Y=Y, A_Z=Z, A_Xq=Xq, A_ls=ls, A_hyper=np.array([sf2, noise, alpha, jit]), A_y_mean=y_mean,
               A_y_std=y_std, A_G=a["G"], A_g=a["g"], A_yy=a["yy"], A_mean=y_mean + y_std * a["mean_n"], A_var=a["var"],
               A_bound=np.array(a["bound"]))
    # ---- case B: Z = X ---------------------------------------------------------------------------------------------
    rng = np.random.default_rng(831)
    N, D, P, M = 300, 6, 1, 40
    X = rng.standard_normal((N, D))
    Y = targets(X, P, rng)
    Xq = rng.standard_normal((M, D))
    Xq[[0, 9]] = X[[1, 77]]
    ls = 1.0 * (1.0 + 0.1 * np.arange(D))
    sf2, noise, alpha = 1.0, 0.05 - 1e-10, 1e-10
    s2, jit = noise + alpha, 1e-10 * sf2
    y_mean, y_std = Y.mean(axis=0), Y.std(axis=0)
    Yn = (Y - y_mean) / y_std
    a, d = by_assembly(X, Yn, X, Xq, ls, sf2, s2, jit), by_dense_form(X, Yn, X, Xq, ls, sf2, s2, jit)
    e_mean, e_var, e_lml = exact_gp(X, Yn, Xq, ls, sf2, s2)
    print("case B: the two forms differ by  mean %.1e  var/sf2 %.1e  bound %.1e" % (
        agree(a["mean_n"], d["mean_n"], 1e-8, "B mean"), agree(a["var"] / sf2, d["var"] / sf2, 1e-8, "B var"),
        agree(a["bound"], d["bound"], 1e-9, "B bound")))
    print("case B: sparse against exact     mean %.1e  var/sf2 %.1e  bound %.1e" % (
        agree(a["mean_n"], e_mean, 1e-8, "B mean exact"), agree(a["var"] / sf2, e_var / sf2, 1e-8, "B var exact"),
        agree(a["bound"], e_lml, 1e-8, "B lml exact")))
    out.update(B_X=X, B_Y=Y, B_Xq=Xq, B_ls=ls, B_hyper=np.array([sf2, noise, alpha, jit]), B_y_mean=y_mean, B_y_std=y_std,
               B_mean=y_mean + y_std * a["mean_n"], B_var=a["var"], B_bound=np.array(a["bound"]),
               B_exact_mean=y_mean + y_std * e_mean, B_exact_var=e_var, B_exact_lml=np.array(e_lml))
    path = os.path.join(HERE, "sparse_ref.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
