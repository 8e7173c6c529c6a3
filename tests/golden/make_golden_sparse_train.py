"""Writes tests/golden/sparse_train_ref.npz: the gradient of the sparse GP's collapsed bound and a training case.

NumPy and SciPy only, seeded, reproduces its file bit for bit.  Every gradient is computed twice,

* by the assembly form the library uses (include/gpk.h, gpk_sparse_eval): the partial derivatives of the bound with respect to
  the statistics G, g and to Kuu, then one pass over the rows with Q^T = F C, F = [Kfu | Yn], C = [2 dL/dG ; dL/dg^T];
* by the dense N x N form: dL/dQff = (a a^T - P C^-1) / 2 + P / (2 s2) I with C = Qff + s2 I, a = C^-1 Yn, chained through
  Qff = Kfu Kuu^-1 Kuf,

and the file is written only if the two agree to 1e-9 of the largest component and the central differences of the bound to
1e-6.  The measured agreements are stored.  The gradient is [d/dlog ls_0 .., d/dlog noise, d/dlog sf2]; jitter (the regressor's
alpha, part of s2 = noise + jitter) and jitter_uu (absolute, on the diagonal of Kuu) do not depend on the hyper-parameters.

Cases A and B reuse the inputs of tests/golden/sparse_ref.npz (copied into the new file).

    python tests/golden/make_golden_sparse_train.py
"""
import os

import numpy as np
from scipy.linalg import cho_solve, cholesky, solve_triangular
from scipy.optimize import minimize

HERE = os.path.dirname(os.path.abspath(__file__))


def rbf(A, B, ls, sf2):
    a, b = A / ls, B / ls
    d = a[:, None, :] - b[None, :, :]
    return sf2 * np.exp(-0.5 * np.sum(d * d, axis=2))


def sqdiff(A, B, ls):
    """((a_nd - b_id) / ls_d)^2 as (n, i, d), by differences of the divided coordinates"""
    a, b = A / ls, B / ls
    d = a[:, None, :] - b[None, :, :]
    return d * d


def bound_value(X, Yn, Z, ls, sf2, noise, jitter, jit):
    """The collapsed bound by the assembly of gpk_sparse_finalize."""
    N, m, P = len(X), len(Z), Yn.shape[1]
    s2 = noise + jitter
    Kuf = rbf(Z, X, ls, sf2)
    G, g, yy = Kuf @ Kuf.T, Kuf @ Yn, np.sum(Yn * Yn, axis=0)
    Luu = cholesky(rbf(Z, Z, ls, sf2) + jit * np.eye(m), lower=True)
    Wuu = solve_triangular(Luu, np.eye(m), lower=True)
    B = np.eye(m) + Wuu @ G @ Wuu.T / s2
    LB = cholesky(B, lower=True)
    r = Wuu @ g / s2
    c = cho_solve((LB, True), r)
    return float(sum(-0.5 * N * np.log(2 * np.pi * s2) - np.sum(np.log(np.diag(LB))) - 0.5 * (N * sf2 - s2 * (np.trace(B) - m)) / s2
                     - 0.5 * yy[p] / s2 + 0.5 * r[:, p] @ c[:, p] for p in range(P)))


def partials(X, Yn, Z, ls, sf2, noise, jitter, jit):
    """alpha_u and the partial derivatives of the bound with respect to g, G and Kuu (the issue's Gamma_g, Gamma_G, Gamma_K)."""
    m, P = len(Z), Yn.shape[1]
    s2 = noise + jitter
    Kuf = rbf(Z, X, ls, sf2)
    G, g = Kuf @ Kuf.T, Kuf @ Yn
    Kuu = rbf(Z, Z, ls, sf2) + jit * np.eye(m)
    Ki = cho_solve((cholesky(Kuu, lower=True), True), np.eye(m))
    Si = cho_solve((cholesky(Kuu + G / s2, lower=True), True), np.eye(m))
    au = Si @ g / s2
    Gg = au / s2
    GG = P / (2 * s2) * (Ki - Si) - au @ au.T / (2 * s2)
    GK = P / 2 * (Ki - Si) - P / (2 * s2) * (Ki @ G @ Ki) - 0.5 * au @ au.T
    return dict(Kuf=Kuf, G=G, g=g, Ki=Ki, Si=Si, au=au, Gg=Gg, GG=GG, GK=GK)


def pass_sums(X, Yn, Z, ls, sf2, Cm):
    """The row pass: sums[d] = sum_ni Q_ni Kfu_ni ((x_nd - z_id) / ls_d)^2 with Q = [Kfu | Yn] Cm, the unweighted sum
    sum Q o Kfu, and the sums of the absolute values of the same terms."""
    Kfu = rbf(X, Z, ls, sf2)
    Q = np.hstack([Kfu, Yn]) @ Cm
    T = Q * Kfu
    W = T[:, :, None] * sqdiff(X, Z, ls)
    return (np.concatenate([W.sum(axis=(0, 1)), [T.sum()]]), np.concatenate([np.abs(W).sum(axis=(0, 1)), [np.abs(T).sum()]]))


def coef_matrix(pt):
    return np.vstack([2.0 * pt["GG"], pt["Gg"].T])


def grad_assembly(X, Yn, Z, ls, sf2, noise, jitter, jit):
    N, m, P = len(X), len(Z), Yn.shape[1]
    s2 = noise + jitter
    pt = partials(X, Yn, Z, ls, sf2, noise, jitter, jit)
    G, g, au, Ki, Si, GK = pt["G"], pt["g"], pt["au"], pt["Ki"], pt["Si"], pt["GK"]
    sums, _ = pass_sums(X, Yn, Z, ls, sf2, coef_matrix(pt))
    Kuu0 = rbf(Z, Z, ls, sf2)
    g_ls = sums[:-1] + np.einsum("ij,ij,ijd->d", GK, Kuu0, sqdiff(Z, Z, ls))
    g_sf2 = 2 * np.sum(pt["GG"] * G) + np.sum(pt["Gg"] * g) + np.sum(GK * Kuu0) - P * N * sf2 / (2 * s2)
    yy = np.sum(Yn * Yn)
    g_noise = noise * (P * (-N / (2 * s2) + N * sf2 / (2 * s2 ** 2) - np.trace(Ki @ G) / (2 * s2 ** 2) + np.trace(Si @ G) / (2 * s2 ** 2))
                       + yy / (2 * s2 ** 2) - np.sum(au * g) / s2 ** 2 + np.trace(au.T @ G @ au) / (2 * s2 ** 2))
    unweighted_from_stats = 2 * np.sum(pt["GG"] * G) + np.sum(pt["Gg"] * g)
    return np.concatenate([g_ls, [g_noise, g_sf2]]), sums[-1], unweighted_from_stats


def grad_dense(X, Yn, Z, ls, sf2, noise, jitter, jit):
    N, m, P = len(X), len(Z), Yn.shape[1]
    s2 = noise + jitter
    Kfu = rbf(X, Z, ls, sf2)
    Kuu0 = rbf(Z, Z, ls, sf2)
    cU = (cholesky(Kuu0 + jit * np.eye(m), lower=True), True)
    A = cho_solve(cU, Kfu.T)                     # Kuu^-1 Kuf
    Qff = Kfu @ A
    cC = (cholesky(Qff + s2 * np.eye(N), lower=True), True)
    Ci = cho_solve(cC, np.eye(N))
    a = Ci @ Yn
    M = 0.5 * (a @ a.T - P * Ci) + P / (2 * s2) * np.eye(N)
    dKfu = 2.0 * M @ A.T
    dKuu = -A @ M @ A.T
    g_ls = np.einsum("ni,ni,nid->d", dKfu, Kfu, sqdiff(X, Z, ls)) + np.einsum("ij,ij,ijd->d", dKuu, Kuu0, sqdiff(Z, Z, ls))
    g_sf2 = np.sum(dKfu * Kfu) + np.sum(dKuu * Kuu0) - P * N * sf2 / (2 * s2)
    g_noise = noise * (0.5 * np.trace(a @ a.T - P * Ci) + P / (2 * s2 ** 2) * (N * sf2 - np.trace(Qff)))
    return np.concatenate([g_ls, [g_noise, g_sf2]])


def grad_central(X, Yn, Z, ls, sf2, noise, jitter, jit, h=1e-4):
    t0 = np.log(np.concatenate([ls, [noise, sf2]]))
    D = len(ls)
    out = np.empty_like(t0)
    for k in range(len(t0)):
        v = []
        for s in (1.0, -1.0):
            t = t0.copy()
            t[k] += s * h
            e = np.exp(t)
            v.append(bound_value(X, Yn, Z, e[:D], e[D + 1], e[D], jitter, jit))
        out[k] = (v[0] - v[1]) / (2 * h)
    return out


def exact_lml_grad(X, Yn, ls, sf2, noise, jitter):
    N, P = len(X), Yn.shape[1]
    K0 = rbf(X, X, ls, sf2)
    Ci = cho_solve((cholesky(K0 + (noise + jitter) * np.eye(N), lower=True), True), np.eye(N))
    a = Ci @ Yn
    M = 0.5 * (a @ a.T - P * Ci)
    return np.concatenate([np.einsum("ij,ij,ijd->d", M, K0, sqdiff(X, X, ls)), [noise * np.trace(M), np.sum(M * K0)]])


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(np.asarray(b))))


def checked_gradient(name, X, Yn, Z, ls, sf2, noise, jitter, jit):
    ga, unw, unw_stats = grad_assembly(X, Yn, Z, ls, sf2, noise, jitter, jit)
    gd = grad_dense(X, Yn, Z, ls, sf2, noise, jitter, jit)
    gc = grad_central(X, Yn, Z, ls, sf2, noise, jitter, jit)
    e_forms, e_fd = rel(ga, gd), rel(gc, ga)
    print("%s: assembly against dense form %.1e, central differences %.1e, unweighted sum %.1e" % (
        name, e_forms, e_fd, abs(unw - unw_stats) / abs(unw_stats)))
    assert e_forms < 1e-9, (name, "the two forms", e_forms)
    assert e_fd < 1e-6, (name, "central differences", e_fd)
    return ga, e_forms, e_fd


def main():
    src = np.load(os.path.join(HERE, "sparse_ref.npz"))
    out = {}
    # ---- case A (ARD) and its isotropic variant --------------------------------------------------------------------
    X, Y, Z, ls = src["A_X"], src["A_Y"], src["A_Z"], src["A_ls"]
    sf2, noise, alpha, jit = src["A_hyper"]
    ym, ys = src["A_y_mean"], src["A_y_std"]
    Yn = (Y - ym) / ys
    ga, ef, ed = checked_gradient("case A", X, Yn, Z, ls, sf2, noise, alpha, jit)
    out.update(A_X=X, A_Y=Y, A_Z=Z, A_ls=ls, A_hyper=src["A_hyper"], A_y_mean=ym, A_y_std=ys,
               A_bound=np.array(bound_value(X, Yn, Z, ls, sf2, noise, alpha, jit)), A_grad=ga, A_agree=np.array([ef, ed]))
    assert abs(float(out["A_bound"]) - float(src["A_bound"])) < 1e-12 * abs(float(src["A_bound"]))
    iso = 1.0
    gi, ef, ed = checked_gradient("case A, isotropic", X, Yn, Z, np.full(X.shape[1], iso), sf2, noise, alpha, jit)
    out.update(Aiso_ls=np.array([iso]), Aiso_bound=np.array(bound_value(X, Yn, Z, np.full(X.shape[1], iso), sf2, noise, alpha, jit)),
               Aiso_grad=np.concatenate([[gi[:X.shape[1]].sum()], gi[X.shape[1]:]]), Aiso_agree=np.array([ef, ed]))
    # the row pass alone, on a random coefficient matrix
    rng = np.random.default_rng(840)
    Cr = rng.standard_normal((len(Z) + Yn.shape[1], len(Z)))
    sums, asums = pass_sums(X, Yn, Z, ls, sf2, Cr)
    out.update(A_C=Cr, A_pass=sums, A_pass_abs=asums)
    # ---- case B: Z = X, the bound is the exact LML (up to jitter_uu) -----------------------------------------------------
    X, Y, ls = src["B_X"], src["B_Y"], src["B_ls"]
    sf2, noise, alpha, jit = src["B_hyper"]
    ym, ys = src["B_y_mean"], src["B_y_std"]
    Yn = (Y - ym) / ys
    gb, ef, ed = checked_gradient("case B", X, Yn, X, ls, sf2, noise, alpha, jit)
    ge = exact_lml_grad(X, Yn, ls, sf2, noise, alpha)
    jd = rel(gb, ge)
    print("case B: sparse gradient against the exact LML gradient %.1e (the jitter on Kuu)" % jd)
    assert jd < 1e-6
    out.update(B_X=X, B_Y=Y, B_ls=ls, B_hyper=src["B_hyper"], B_y_mean=ym, B_y_std=ys, B_grad=gb, B_exact_grad=ge,
               B_agree=np.array([ef, ed]), B_jitter_diff=np.array(jd))
    # ---- the training case: targets drawn from a known kernel, the start a factor 3 off in every parameter ------------------
    rng = np.random.default_rng(841)
    N, D, m = 600, 2, 64
    X = rng.uniform(-3.0, 3.0, (N, D))
    ls_true, sf2_true, noise_true = np.array([0.5, 0.9]), 1.4, 0.05
    Lk = cholesky(rbf(X, X, ls_true, sf2_true) + 1e-10 * np.eye(N), lower=True)
    Y = (Lk @ rng.standard_normal(N) + np.sqrt(noise_true) * rng.standard_normal(N))[:, None]
    Z = X[np.sort(rng.permutation(N)[:m])].copy()
    ym, ys = Y.mean(axis=0), Y.std(axis=0)
    Yn = (Y - ym) / ys
    jitter, jit = 1e-10, 1e-4
    ls0, sf20, noise0 = ls_true * 3.0, sf2_true / ys[0] ** 2 / 3.0, noise_true / ys[0] ** 2 * 3.0
    lo, hi = np.log(1e-5), np.log(1e5)

    def obj(t):
        e = np.exp(t)               # theta in the kernel's layout: [sf2, ls_0, ls_1, noise]
        try:
            b = bound_value(X, Yn, Z, e[1:3], e[0], e[3], jitter, jit)
            g, _, _ = grad_assembly(X, Yn, Z, e[1:3], e[0], e[3], jitter, jit)
        except np.linalg.LinAlgError:
            return np.inf, np.zeros_like(t)
        return -b, -np.array([g[3], g[0], g[1], g[2]])

    t0 = np.log(np.array([sf20, ls0[0], ls0[1], noise0]))
    checked_gradient("training case, start", X, Yn, Z, ls0, sf20, noise0, jitter, jit)
    res = minimize(obj, t0, method="L-BFGS-B", jac=True, bounds=[(lo, hi)] * 4)
    print("training case: bound %.6f -> %.6f in %d evaluations, theta %s" % (-obj(t0)[0], -res.fun, res.nfev, np.exp(res.x)))
    assert -res.fun > -obj(t0)[0]
    out.update(T_X=X, T_Y=Y, T_Z=Z, T_y_mean=ym, T_y_std=ys, T_start=np.array([sf20, ls0[0], ls0[1], noise0]),
               T_hyper=np.array([jitter, jit]), T_bound_start=np.array(-obj(t0)[0]), T_bound_opt=np.array(-res.fun),
               T_theta_opt=res.x)
    path = os.path.join(HERE, "sparse_train_ref.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
