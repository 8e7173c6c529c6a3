"""Regenerate tests/golden/hess_ref.npz: input Hessians of the posterior mean at fixed hyper-parameters on the committed flight
data (csv_170501.npz) and on the sparse case of sparse_ref.npz.  Needs NumPy, SciPy and scikit-learn only; one BLAS thread and a
fixed time stamp on the archive's members, so the same inputs give the same file, byte for byte.

    python tests/golden/make_golden_hess.py [out.npz]

scikit-learn has no derivative call, so the closed form of the RBF kernel is evaluated in NumPy fp64 from scikit-learn's OWN
fitted attributes (X_train_, alpha_, _y_train_std), with q = x* / ls, r_j = x_j / ls, delta_j = q - r_j and
k_j = sf2 exp(-|delta_j|^2 / 2) (no WhiteKernel term):

    T_p[d][e] = sum_j k_j alpha_jp delta_jd delta_je,      S_p = sum_j k_j alpha_jp
    hess[m][p][d][e] = y_std[p] / (ls_d ls_e) (T_p[d][e] - [d = e] S_p)

The upper triangle is computed and mirrored: every stored D x D block is symmetric bit for bit.

Cases (prefix_*), kernels and data exactly as make_golden_jac.py has them: ka1 - RBF(0.5) + White(0.1), alpha 1e-4, normalize_y,
D = 10, P = 6, the 64 Xq10 queries; train - the ka1 model on 8 training rows + 17 queries; one - the same kernel, one 1-D target,
normalize_y=False (the first 32 queries); ard - C(2.0) * RBF(linspace(0.4, 1.3, 10)) + White(0.05), 2-D target with one column
(32 queries); pkg - the package GP's conventions, C(1.5) * RBF(0.8) + White(0.02), alpha 0, no normalisation (16 queries).
axis - the recipe `csv` of make_golden_axis_jac.py: six scalar ARD models on the scaled inputs behind one input scaler and six
target scalers, the first 25 of its query rows; axis_hess_scaled (M, 6, D, D) is d2 mu_b / dz dz on the scaled inputs, axis_hess
the same in RAW units, sy_b.scale_ / (sx.scale_[d] sx.scale_[e]) times it (the yaw-rate column's scale is ~1e-21, so its raw
entries dwarf all others: a test compares both).  sparse - case A of sparse_ref.npz with its first 64 inducing rows: the Titsias
posterior in dense NumPy, alpha_u = Sigma^-1 Kuf Yn / s2 with Sigma = Kuu + Kuf Kfu / s2 as make_golden_sparse_serve.py forms it,
the Hessian that of the exact form over (Z, alpha_u).

Each case stores *_Xq (the query rows), *_hess, and two cross-checks relative to the largest entry: *_chk against the same
formula in np.longdouble, *_fd against a fourth-order central difference (h = 1e-3) of the closed-form Jacobian
dmean[m][p][d] = y_std[p] sum_j k_j alpha_jp (x_jd - x*_d) / ls_d^2 (for axis both on the scaled inputs)."""
import io
import os
import sys
import zipfile

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"        # one BLAS thread: the same bits on every run

import numpy as np  # noqa: E402
from scipy.linalg import cho_solve, cholesky  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
FD_H = 1e-3


def rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def hessian(X, alpha, ls, sf2, ystd, Xq, dtype=np.float64):
    """(M, P, D, D) from the model arrays: X (N, D), alpha (N, P), ls scalar or (D,), y_std (P,)."""
    X, alpha, Xq = (np.asarray(a, dtype=dtype) for a in (X, alpha, Xq))
    D = X.shape[1]
    ls = np.broadcast_to(np.asarray(ls, dtype=dtype), (D,))
    ystd = np.asarray(ystd, dtype=dtype).reshape(-1)
    delta = (Xq / ls)[:, None, :] - (X / ls)[None, :, :]                       # (M, N, D): q - r_j
    k = dtype(sf2) * np.exp(dtype(-0.5) * np.sum(delta * delta, axis=2))        # (M, N)
    w = k[:, :, None] * alpha.reshape(len(X), -1)[None, :, :]                   # (M, N, P)
    M, P = len(Xq), w.shape[2]
    H = np.zeros((M, P, D, D), dtype=dtype)
    S = np.sum(w, axis=1)                                                       # (M, P)
    for d in range(D):
        wd = w * delta[:, :, d, None]
        for e in range(d, D):
            t = np.sum(wd * delta[:, :, e, None], axis=1)
            if d == e:
                t = t - S
            H[:, :, d, e] = H[:, :, e, d] = ystd[None, :] / (ls[d] * ls[e]) * t
    return H


def jacobian(X, alpha, ls, sf2, ystd, Xq):
    """(M, P, D): the closed form of make_golden_jac.py."""
    D = X.shape[1]
    ls = np.broadcast_to(np.asarray(ls, dtype=np.float64), (D,))
    diff = X[None, :, :] - Xq[:, None, :]
    k = sf2 * np.exp(-0.5 * np.sum((diff / ls) ** 2, axis=2))
    return np.einsum("mj,mjd,jp->mpd", k, diff / ls ** 2, alpha.reshape(len(X), -1)) * np.reshape(ystd, (1, -1, 1))


def fd_hessian(X, alpha, ls, sf2, ystd, Xq):
    """Fourth-order central differences of the Jacobian: H[m, p, d, e] = d dmean[m, p, d] / dx_e."""
    M, D = Xq.shape
    out = None
    for e in range(D):
        acc = 0.0
        for w, s in zip((1.0, -8.0, 8.0, -1.0), (-2, -1, 1, 2)):
            Xs = Xq.copy()
            Xs[:, e] += s * FD_H
            acc = acc + w * jacobian(X, alpha, ls, sf2, ystd, Xs)
        if out is None:
            out = np.zeros(acc.shape + (D,))
        out[..., e] = acc / (12.0 * FD_H)
    return out


def model_case(out, name, X, alpha, ls, sf2, ystd, Xq, squeeze=False):
    H = hessian(X, alpha, ls, sf2, ystd, Xq)
    assert np.array_equal(H, H.swapaxes(-1, -2))
    Hl = hessian(X, alpha, ls, sf2, ystd, Xq, dtype=np.longdouble)
    chk = float(np.max(np.abs(Hl - H.astype(np.longdouble))) / np.max(np.abs(Hl)))
    fd = rel(fd_hessian(X, alpha, ls, sf2, ystd, Xq), H)
    out[name + "_Xq"], out[name + "_hess"] = Xq, (H[:, 0] if squeeze else H)
    out[name + "_chk"], out[name + "_fd"] = np.array(chk), np.array(fd)
    print(f"{name}: hess {out[name + '_hess'].shape}  chk {chk:.1e}  fd {fd:.1e}")
    return H


def sk_case(out, name, g, ls, sf2, Xq, squeeze=False):
    ystd = np.asarray(g._y_train_std, dtype=np.float64).reshape(-1)
    return model_case(out, name, g.X_train_, g.alpha_.reshape(len(g.X_train_), -1), ls, sf2, ystd, Xq, squeeze)


def case_axis(out, d):
    """make_golden_axis_jac.py's case `csv`."""
    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, WhiteKernel
    from sklearn.preprocessing import StandardScaler
    X, Y = d["X10"], d["Y6"]
    D, B = X.shape[1], Y.shape[1]
    Xq = np.vstack([d["Xq10"], X[d["q_train_idx"][:8]]])[:25]
    sx = StandardScaler().fit(X)
    Xs, Z = sx.transform(X), sx.transform(Xq)
    Hs, chk, fd, lss, noises, sym, sys_ = [], [], [], [], [], [], []
    for b in range(B):
        sy = StandardScaler().fit(Y[:, [b]])
        ls, noise = np.roll(np.linspace(0.6, 3.0, D), b), 0.02 * (b + 1)
        kern = ConstantKernel(1.0, constant_value_bounds="fixed") * RBF(ls) + WhiteKernel(noise)
        g = GaussianProcessRegressor(kernel=kern, alpha=1e-6, normalize_y=False, optimizer=None)
        g.fit(Xs, sy.transform(Y[:, [b]]).ravel())
        one = {}
        Hs.append(sk_case(one, f"axis[{b}]", g, ls, 1.0, Z)[:, 0])
        chk.append(one[f"axis[{b}]_chk"])
        fd.append(one[f"axis[{b}]_fd"])
        lss.append(ls)
        noises.append(noise)
        sym.append(float(sy.mean_[0]))
        sys_.append(float(sy.scale_[0]))
    Hs = np.stack(Hs, axis=1)                                                   # (M, B, D, D), scaled inputs, model units
    scale = np.array(sys_)[None, :, None, None] / (sx.scale_[:, None] * sx.scale_[None, :])[None, None]
    out["axis_Xq"], out["axis_hess_scaled"], out["axis_hess"] = Xq, Hs, scale * Hs
    assert np.array_equal(out["axis_hess"], out["axis_hess"].swapaxes(-1, -2))
    out["axis_chk"], out["axis_fd"] = np.array(max(chk)), np.array(max(fd))
    out["axis_sx_mean"], out["axis_sx_scale"] = sx.mean_, sx.scale_
    out["axis_sy_mean"], out["axis_sy_scale"] = np.array(sym), np.array(sys_)
    out["axis_ls"], out["axis_noise"] = np.stack(lss), np.array(noises)


def case_sparse(out):
    sys.path.insert(0, HERE)
    from make_golden_sparse import rbf
    src = np.load(os.path.join(HERE, "sparse_ref.npz"))
    X, Y, Xq, ls = src["A_X"], src["A_Y"], src["A_Xq"], src["A_ls"]
    Z = src["A_Z"][:64]
    sf2, noise, alpha, jit = (float(v) for v in src["A_hyper"])
    y_mean, y_std = src["A_y_mean"], src["A_y_std"]
    Yn = (Y - y_mean) / y_std
    s2 = noise + alpha
    Kuu = rbf(Z, Z, ls, sf2) + jit * np.eye(len(Z))
    Kuf = rbf(Z, X, ls, sf2)
    alpha_u = cho_solve((cholesky(Kuu + Kuf @ Kuf.T / s2, lower=True), True), Kuf @ Yn) / s2
    model_case(out, "sparse", Z, alpha_u, ls, sf2, y_std, Xq)
    out["sparse_Z"] = Z
    out["sparse_mean"] = (rbf(Xq, Z, ls, sf2) @ alpha_u) * y_std + y_mean
    out["sparse_dmean"] = jacobian(Z, alpha_u, ls, sf2, y_std, Xq)


def save_npz(path, arrays):
    """np.savez_compressed with a fixed time stamp on every member: the same arrays give the same file, byte for byte"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def main(path):
    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, WhiteKernel
    d = np.load(os.path.join(HERE, "csv_170501.npz"))
    X, Y, Xq = d["X10"], d["Y6"], d["Xq10"]
    out = {}
    k1 = RBF(0.5) + WhiteKernel(0.1)
    g = GaussianProcessRegressor(kernel=k1, alpha=1e-4, normalize_y=True, optimizer=None).fit(X, Y)
    sk_case(out, "ka1", g, 0.5, 1.0, Xq)
    sk_case(out, "train", g, 0.5, 1.0, np.vstack([X[d["q_train_idx"][:8]], Xq[:17]]))

    g = GaussianProcessRegressor(kernel=k1, alpha=1e-4, normalize_y=False, optimizer=None).fit(X, Y[:, 0])
    sk_case(out, "one", g, 0.5, 1.0, Xq[:32], squeeze=True)

    ls = np.linspace(0.4, 1.3, X.shape[1])
    k3 = ConstantKernel(2.0) * RBF(ls) + WhiteKernel(0.05)
    g = GaussianProcessRegressor(kernel=k3, alpha=1e-5, normalize_y=True, optimizer=None).fit(X, Y[:, [2]])
    out["ard_ls"] = ls
    sk_case(out, "ard", g, ls, 2.0, Xq[:32], squeeze=True)

    out["pkg_hyper"] = np.array([0.8, 1.5, 0.02])          # length_scale, signal_variance, noise_variance
    k4 = ConstantKernel(1.5) * RBF(0.8) + WhiteKernel(0.02)
    g = GaussianProcessRegressor(kernel=k4, alpha=0.0, normalize_y=False, optimizer=None).fit(X, Y)
    sk_case(out, "pkg", g, 0.8, 1.5, Xq[:16])

    case_axis(out, d)
    case_sparse(out)
    save_npz(path, out)
    print(path, os.path.getsize(path), "bytes")
    return out


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "hess_ref.npz"))
