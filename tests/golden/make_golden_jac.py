"""Regenerate tests/golden/jac_ref.npz: input gradients of scikit-learn's posterior mean and variance at fixed
hyper-parameters (optimizer=None) on the committed flight data (csv_170501.npz).  Needs scikit-learn only.

    python tests/golden/make_golden_jac.py [out.npz]

scikit-learn has no gradient call, so the closed forms of the RBF kernel are evaluated in NumPy fp64 from scikit-learn's OWN
fitted attributes (X_train_, alpha_, L_, _y_train_std, kernel_), c = K^-1 k* by two solve_triangular calls with L_:

    u_jd            = (x_jd - x*_d) / ls_d^2
    d mean_p / dx*_d =  y_std[p] sum_j k(x*, x_j) u_jd alpha_jp
    d var_p  / dx*_d = -2 y_std[p]^2 sum_j k(x*, x_j) u_jd c_j           (k without the WhiteKernel term)

Cases (prefix_*): ka1 - RBF(0.5) + White(0.1), alpha 1e-4, normalize_y, D = 10, P = 6 on the 64 Xq10 queries; one - the same
kernel, one 1-D target, normalize_y=False; ard - C(2.0) * RBF(linspace(0.4, 1.3, 10)) + White(0.05), 2-D target with one
column; train - the ka1 model on 8 training rows + 17 queries (variances at the noise level); pkg - the package GP's
conventions: C(1.5) * RBF(0.8) + White(0.02), alpha 0, no normalisation, k** = sf2 WITHOUT the noise, variance floored at
1e-10 (one variance and one gradient row per query).  Each case stores mean / var (scikit-learn's predict), dmean / dvar (the
closed forms) and two cross-checks of the closed forms, relative to the largest entry, as *_chk = [dmean, dvar] against the same
formulas through an explicit inverse of L_, and *_fd = [dmean, dvar] against a fourth-order central difference (h = 1e-3) of
scikit-learn's own predict(return_std=True)."""
import os
import sys

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"        # one BLAS thread: the same bits on every run

import numpy as np  # noqa: E402
from scipy.linalg import solve_triangular  # noqa: E402
from sklearn.gaussian_process import GaussianProcessRegressor  # noqa: E402
from sklearn.gaussian_process.kernels import RBF, ConstantKernel, WhiteKernel  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
FD_H = 1e-3


def rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def closed_form(g, ls, sf2, Xq, explicit_inverse=False):
    """(dmean (M, P, D), dvar_n (M, D) in normalised-target units) from scikit-learn's fitted attributes."""
    X = g.X_train_
    ls = np.broadcast_to(np.asarray(ls, dtype=np.float64), (X.shape[1],))
    alpha = g.alpha_.reshape(len(X), -1)
    ystd = np.asarray(g._y_train_std, dtype=np.float64).reshape(-1)
    diff = X[None, :, :] - Xq[:, None, :]                                      # (M, N, D): x_j - x*
    k = sf2 * np.exp(-0.5 * np.sum((diff / ls) ** 2, axis=2))                  # (M, N)
    u = diff / ls ** 2
    dmean = np.einsum("mj,mjd,jp->mpd", k, u, alpha) * ystd[None, :, None]
    if explicit_inverse:
        Li = solve_triangular(g.L_, np.eye(len(X)), lower=True)
        c = Li.T @ (Li @ k.T)
    else:
        c = solve_triangular(g.L_.T, solve_triangular(g.L_, k.T, lower=True), lower=False)     # (N, M)
    dvar = -2.0 * np.einsum("mj,mjd,jm->md", k, u, c)
    return dmean, dvar


def finite_difference(g, Xq, var_of):
    """Fourth-order central differences of predict(return_std=True): (dmean (M, P, D), dvar (M, P, D))."""
    M, D = Xq.shape
    c = np.array([1.0, -8.0, 8.0, -1.0]) / (12.0 * FD_H)
    dm = dv = None
    for d in range(D):
        acc_m = acc_v = 0.0
        for w, s in zip(c, (-2, -1, 1, 2)):
            Xs = Xq.copy()
            Xs[:, d] += s * FD_H
            mean, std = g.predict(Xs, return_std=True)
            acc_m = acc_m + w * mean.reshape(M, -1)
            acc_v = acc_v + w * var_of(std.reshape(M, -1))
        if dm is None:
            dm = np.zeros((M, acc_m.shape[1], D))
            dv = np.zeros((M, acc_v.shape[1], D))
        dm[:, :, d], dv[:, :, d] = acc_m, acc_v
    return dm, dv


def case(out, name, g, ls, sf2, noise, Xq, pkg=False):
    mean, std = g.predict(Xq, return_std=True)
    ystd2 = np.asarray(g._y_train_std, dtype=np.float64).reshape(-1) ** 2
    dmean, dvar_n = closed_form(g, ls, sf2, Xq)
    dmean2, dvar_n2 = closed_form(g, ls, sf2, Xq, explicit_inverse=True)
    if pkg:
        # package conventions: k** = sf2 (scikit-learn's diag carries the noise: take it off), floor 1e-10, one row per query
        var = np.maximum(std.reshape(len(Xq), -1)[:, 0] ** 2 - noise, 1e-10)
        dvar = dvar_n
        fdm, fdv = finite_difference(g, Xq, lambda s: s ** 2)
        fdv = fdv[:, 0, :]
    else:
        var = std ** 2
        dvar = dvar_n[:, None, :] * ystd2[None, :, None]
        fdm, fdv = finite_difference(g, Xq, lambda s: s ** 2)
    if dmean.shape[1] == 1:       # predict's squeezing for one target
        dmean, dmean2, fdm = dmean[:, 0], dmean2[:, 0], fdm[:, 0]
        if not pkg:
            dvar, fdv = dvar[:, 0], fdv[:, 0]
    chk_v = dvar_n2 if pkg else (dvar_n2[:, None, :] * ystd2[None, :, None]).reshape(dvar.shape)
    out[name + "_mean"], out[name + "_var"] = mean, var
    out[name + "_dmean"], out[name + "_dvar"] = dmean, dvar
    out[name + "_chk"] = np.array([rel(dmean2, dmean), rel(chk_v, dvar)])
    out[name + "_fd"] = np.array([rel(fdm, dmean), rel(fdv, dvar)])


def main(path):
    d = np.load(os.path.join(HERE, "csv_170501.npz"))
    X, Y, Xq = d["X10"], d["Y6"], d["Xq10"]
    out = {}
    k1 = RBF(0.5) + WhiteKernel(0.1)
    g = GaussianProcessRegressor(kernel=k1, alpha=1e-4, normalize_y=True, optimizer=None).fit(X, Y)
    case(out, "ka1", g, 0.5, 1.0, 0.1, Xq)
    Xt = np.vstack([X[d["q_train_idx"][:8]], Xq[:17]])
    out["train_Xq"] = Xt
    case(out, "train", g, 0.5, 1.0, 0.1, Xt)

    g = GaussianProcessRegressor(kernel=k1, alpha=1e-4, normalize_y=False, optimizer=None).fit(X, Y[:, 0])
    case(out, "one", g, 0.5, 1.0, 0.1, Xq)

    ls = np.linspace(0.4, 1.3, X.shape[1])
    k3 = ConstantKernel(2.0) * RBF(ls) + WhiteKernel(0.05)
    g = GaussianProcessRegressor(kernel=k3, alpha=1e-5, normalize_y=True, optimizer=None).fit(X, Y[:, [2]])
    out["ard_ls"] = ls
    case(out, "ard", g, ls, 2.0, 0.05, Xq)

    out["pkg_hyper"] = np.array([0.8, 1.5, 0.02])          # length_scale, signal_variance, noise_variance
    k4 = ConstantKernel(1.5) * RBF(0.8) + WhiteKernel(0.02)
    g = GaussianProcessRegressor(kernel=k4, alpha=0.0, normalize_y=False, optimizer=None).fit(X, Y)
    case(out, "pkg", g, 0.8, 1.5, 0.02, Xq, pkg=True)
    np.savez_compressed(path, **out)
    return out


if __name__ == "__main__":
    out = main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "jac_ref.npz"))
    for k, v in out.items():
        print(k, v.shape, v.ravel()[:3])
