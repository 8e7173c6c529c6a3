"""Writes tests/golden/sparse_serve_ref.npz: the sparse GP's mean Jacobian, variance gradient and joint covariance at the
query rows of tests/golden/sparse_ref.npz ("serving: gradients and covariance").

NumPy and SciPy only, seeded (nothing is drawn: the inputs are read from sparse_ref.npz, not copied), reproduces its file
bit for bit (one BLAS thread, a fixed time stamp on the archive's members).  With k = k_u(x), u_jd = (z_jd - x_d) / ls_d^2 every result is computed twice,

* by the assembly form the library uses (include/gpk.h, gpk_sparse_predict_grad / gpk_sparse_predict_cov): the inverse
  factors Wuu = Luu^-1 and WSigma = LB^-1 Wuu of gpk_sparse_finalize,
      dmean[m, p, d] = y_std[p] sum_j k_mj u_jd alpha_u[j, p]
      dvar[m, d]     = -2 sum_j k_mj u_jd (c0 - c1)_jm,   c0 = Wuu^T (Wuu k),  c1 = WSigma^T (WSigma k)
      cov            = K(Xq, Xq) + noise I - V0^T V0 + V1^T V1,   V0 = Wuu K*^T,  V1 = WSigma K*^T;
* by the dense form: Sigma = Kuu + Kuf Kfu / s2, alpha_u = Sigma^-1 Kuf Yn / s2, c0 = Kuu^-1 k and c1 = Sigma^-1 k by
  Cholesky solves instead of inverse factors,

and the file is written only if the two agree to 1e-8 of each array's largest component; the achieved agreement is stored
beside each result (`*_agree`).  Central differences (h = 1e-5) of the mean and the variance are printed as a further check
and gated at 1e-6.  dmean is un-normalised (M, P, D); dvar (M, D) and cov (M, M) are in normalised-target units (output p
carries y_std[p]^2), cov with the WhiteKernel level on its diagonal.  Case B (Z = X) also stores the exact GP's three results.

    python tests/golden/make_golden_sparse_serve.py
"""
import io
import os
import sys
import zipfile

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"        # one BLAS thread: the same bits on every run

import numpy as np  # noqa: E402
from scipy.linalg import cho_solve, cholesky, solve_triangular  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_sparse import rbf  # noqa: E402

FORMS_GATE, FD_GATE, FD_STEP = 1e-8, 1e-6, 1e-5


def u_terms(Z, Xq, ls):
    """u[m, j, d] = (z_jd - x_md) / ls_d^2, the difference taken in length-scale units first"""
    return ((Z / ls)[None, :, :] - (Xq / ls)[:, None, :]) / ls


def grads(ku, U, alpha_u, cdiff, y_std):
    """ku (m, M), U (M, m, D), alpha_u (m, P), cdiff = c0 - c1 (m, M)"""
    dmean = np.einsum("jm,mjd,jp->mpd", ku, U, alpha_u) * y_std[None, :, None]
    dvar = -2.0 * np.einsum("jm,mjd,jm->md", ku, U, cdiff)
    return dmean, dvar


def by_assembly(X, Yn, Z, Xq, ls, sf2, noise, s2, jit, y_std):
    m = len(Z)
    Kuf = rbf(Z, X, ls, sf2)
    G, g = Kuf @ Kuf.T, Kuf @ Yn
    Luu = cholesky(rbf(Z, Z, ls, sf2) + jit * np.eye(m), lower=True)
    Wuu = solve_triangular(Luu, np.eye(m), lower=True)
    LB = cholesky(np.eye(m) + Wuu @ G @ Wuu.T / s2, lower=True)
    alpha_u = Wuu.T @ cho_solve((LB, True), Wuu @ g / s2)
    WS = solve_triangular(LB, Wuu, lower=True)
    ku = rbf(Z, Xq, ls, sf2)
    V0, V1 = Wuu @ ku, WS @ ku
    dmean, dvar = grads(ku, u_terms(Z, Xq, ls), alpha_u, Wuu.T @ V0 - WS.T @ V1, y_std)
    cov = rbf(Xq, Xq, ls, sf2) + noise * np.eye(len(Xq)) - V0.T @ V0 + V1.T @ V1
    return dmean, dvar, cov


def by_dense_form(X, Yn, Z, Xq, ls, sf2, noise, s2, jit, y_std):
    m = len(Z)
    Kuu = rbf(Z, Z, ls, sf2) + jit * np.eye(m)
    Kuf = rbf(Z, X, ls, sf2)
    cS, cU = (cholesky(Kuu + Kuf @ Kuf.T / s2, lower=True), True), (cholesky(Kuu, lower=True), True)
    ku = rbf(Z, Xq, ls, sf2)
    alpha_u = cho_solve(cS, Kuf @ Yn) / s2
    c0, c1 = cho_solve(cU, ku), cho_solve(cS, ku)
    dmean, dvar = grads(ku, u_terms(Z, Xq, ls), alpha_u, c0 - c1, y_std)
    cov = rbf(Xq, Xq, ls, sf2) + noise * np.eye(len(Xq)) - ku.T @ c0 + ku.T @ c1
    return dmean, dvar, cov


def mean_var(X, Yn, Z, Xq, ls, sf2, s2, jit, y_std):
    """un-normalised mean (M, P) and normalised latent variance (M,), dense form: what the central differences differentiate"""
    m = len(Z)
    Kuu = rbf(Z, Z, ls, sf2) + jit * np.eye(m)
    Kuf = rbf(Z, X, ls, sf2)
    cS, cU = (cholesky(Kuu + Kuf @ Kuf.T / s2, lower=True), True), (cholesky(Kuu, lower=True), True)
    ku = rbf(Z, Xq, ls, sf2)
    mean = (ku.T @ cho_solve(cS, Kuf @ Yn) / s2) * y_std
    var = sf2 - np.sum(ku * cho_solve(cU, ku), axis=0) + np.sum(ku * cho_solve(cS, ku), axis=0)
    return mean, var


def exact_gp(X, Yn, Xq, ls, sf2, noise, s2, y_std):
    N = len(X)
    L = cholesky(rbf(X, X, ls, sf2) + s2 * np.eye(N), lower=True)
    alpha = cho_solve((L, True), Yn)
    ks = rbf(X, Xq, ls, sf2)
    V = solve_triangular(L, ks, lower=True)
    dmean, dvar = grads(ks, u_terms(X, Xq, ls), alpha, cho_solve((L, True), ks), y_std)
    return dmean, dvar, rbf(Xq, Xq, ls, sf2) + noise * np.eye(len(Xq)) - V.T @ V


def rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def case(name, src, Z, out):
    X, Y, Xq, ls = src[name + "_X"], src[name + "_Y"], src[name + "_Xq"], src[name + "_ls"]
    sf2, noise, alpha, jit = src[name + "_hyper"]
    y_mean, y_std = src[name + "_y_mean"], src[name + "_y_std"]
    Yn = (Y - y_mean) / y_std
    s2 = noise + alpha
    a = by_assembly(X, Yn, Z, Xq, ls, sf2, noise, s2, jit, y_std)
    d = by_dense_form(X, Yn, Z, Xq, ls, sf2, noise, s2, jit, y_std)
    agree = [rel(x, y) for x, y in zip(a, d)]
    print("case %s: the two forms differ by  dmean %.1e  dvar %.1e  cov %.1e" % (name, *agree))
    assert max(agree) < FORMS_GATE, (name, agree)
    # central differences of the dense form's mean and variance
    M, D = Xq.shape
    fd_m, fd_v = np.empty_like(a[0]), np.empty_like(a[1])
    for dd in range(D):
        step = np.zeros(D)
        step[dd] = FD_STEP
        mp_, vp_ = mean_var(X, Yn, Z, Xq + step, ls, sf2, s2, jit, y_std)
        mm_, vm_ = mean_var(X, Yn, Z, Xq - step, ls, sf2, s2, jit, y_std)
        fd_m[:, :, dd] = (mp_ - mm_) / (2 * FD_STEP)
        fd_v[:, dd] = (vp_ - vm_) / (2 * FD_STEP)
    e_fd = rel(fd_m, a[0]), rel(fd_v, a[1])
    print("case %s: central differences (h = %g)  dmean %.1e  dvar %.1e;  smallest eigenvalue of cov %.1e" % (
        name, FD_STEP, *e_fd, np.linalg.eigvalsh(a[2]).min()))
    assert max(e_fd) < FD_GATE, (name, e_fd)
    out.update({name + "_dmean": a[0], name + "_dvar": a[1], name + "_cov": a[2], name + "_dmean_agree": np.array(agree[0]),
                name + "_dvar_agree": np.array(agree[1]), name + "_cov_agree": np.array(agree[2])})
    return X, Yn, Xq, ls, sf2, noise, s2, y_std, a


def save_npz(path, arrays):
    """np.savez with a fixed time stamp on every member: the same arrays give the same file, byte for byte"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


def main():
    src = np.load(os.path.join(HERE, "sparse_ref.npz"))
    out = {}
    case("A", src, src["A_Z"], out)
    X, Yn, Xq, ls, sf2, noise, s2, y_std, a = case("B", src, src["B_X"], out)
    e = exact_gp(X, Yn, Xq, ls, sf2, noise, s2, y_std)
    ex = [rel(x, y) for x, y in zip(a, e)]
    print("case B: sparse against exact     dmean %.1e  dvar %.1e  cov %.1e" % tuple(ex))
    assert max(ex) < FORMS_GATE, ex
    out.update(B_exact_dmean=e[0], B_exact_dvar=e[1], B_exact_cov=e[2], B_exact_agree=np.array(ex))
    path = os.path.join(HERE, "sparse_serve_ref.npz")
    save_npz(path, out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
